"""The stream-power fluvial model of tests/fluvial_ref.py (the one nz_fluvial_erosion follows) on the CPU: a hand-worked
tile, the tie order, the exact accumulation as the fixed point of the drainage step, the bounds on the heights, no pits at
the defaults, the options' identities, and the hosts' side of the feature."""
import ctypes
import os
import re

import numpy as np
import pytest

import fluvial_ref as F
from conftest import ROOT
from test_hydraulic_ref import relief

f32 = np.float32
ENTRIES = ("nz_fluvial_erosion_work_floats", "nz_fluvial_erosion", "nz_fluvial_erosion_rw", "nz_fluvial_erosion_batch")


def sines(res, seed=0):
    """A multi-octave sine relief tilted towards one corner: positive heights, no -0, no flats."""
    z, x = np.meshgrid(np.arange(res, dtype=np.float64), np.arange(res, dtype=np.float64), indexing="ij")
    h = 2.0 + 0.004 * (x + 0.7 * z)
    for o in range(4):
        f = 2.0 ** o * 2.0 * np.pi / res
        h += 0.5 ** o * 0.3 * np.sin(f * x * 1.3 + 0.9 * o + seed) * np.cos(f * z * 1.1 + 0.4 * o)
    return h.astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- known answer ------------------------------------------------------------------------------------------------------
def test_hand_worked_5x5():
    """Border 0, interior rows z = 1, 2, 3: (4 2 4), (8 6 8), (16 12 16); erodibility 1/4, uplift 1/8, dt 1, rain 1.
    Iteration 1.  Column x = 1 drains W (4, 8, 16 down to 0; for z = 1 the S neighbour ties at slope 4 and W, the earlier k,
    stays), column x = 3 drains E.  (2,1) drains S (slope 2), (2,2) drains S (6 - 2 = 4 beats SW (6 - 4) * 0.7071), (2,3)
    drains N (12 beats S 6 and NW 12 * 0.7071).  So A' is 1 everywhere except (2,1) = 1 + A(2,2) = 2 and the border cells
    (0,z), (4,z), (2,0), (2,4) that each take one interior cell: 2.  e = 1/4 * sqrt(A') * S, below the half drop everywhere:
    h' = h - e + 1/8."""
    h = np.zeros((5, 5), f32)
    h[1, 1:4] = [4, 2, 4]
    h[2, 1:4] = [8, 6, 8]
    h[3, 1:4] = [16, 12, 16]
    prm = dict(erodibility=0.25, uplift=0.125, dt=1.0, rain=1.0)
    n = F.NONE
    r, S, drop = F.receivers(h)
    assert r.tolist() == [[n, n, n, n, n], [n, 0, 2, 1, n], [n, 0, 2, 1, n], [n, 0, 3, 1, n], [n, n, n, n, n]]
    assert S.tolist() == [[0, 0, 0, 0, 0], [0, 4, 2, 4, 0], [0, 8, 4, 8, 0], [0, 16, 12, 16, 0], [0, 0, 0, 0, 0]]
    assert np.array_equal(drop, S)  # every receiver here is axial
    root2 = np.sqrt(f32(2.0))
    h1, A1 = F.run(h, 1, **prm)
    assert A1.tolist() == [[1, 1, 2, 1, 1], [2, 1, 2, 1, 2], [2, 1, 1, 1, 2], [2, 1, 1, 1, 2], [1, 1, 2, 1, 1]]
    c21 = (f32(2.0) - (f32(0.25) * root2) * f32(2.0)) + f32(0.125)  # 1.4178932
    want1 = np.zeros((5, 5), f32)
    want1[1, 1:4] = [3.125, c21, 3.125]
    want1[2, 1:4] = [6.125, 5.125, 6.125]
    want1[3, 1:4] = [12.125, 9.125, 12.125]
    assert np.array_equal(bits(h1), bits(want1))
    assert abs(float(c21) - 1.4178932) < 1e-7
    # Iteration 2: the same receivers.  (2,0) now takes A1(2,1) = 2: 3.  (2,1): slope c21 to the border, A' = 1 + A1(2,2) = 2.
    # (2,2): slope 5.125 - c21, A' = 1.  The columns x = 1, 3: e = 1/4 * h1
    h2, A2 = F.run(h, 2, **prm)
    assert A2.tolist() == [[1, 1, 3, 1, 1], [2, 1, 2, 1, 2], [2, 1, 1, 1, 2], [2, 1, 1, 1, 2], [1, 1, 2, 1, 1]]
    want2 = np.zeros((5, 5), f32)
    want2[1, 1:4] = [2.46875, (c21 - (f32(0.25) * root2) * c21) + f32(0.125), 2.46875]
    want2[2, 1:4] = [4.71875, (f32(5.125) - f32(0.25) * (f32(5.125) - c21)) + f32(0.125), 4.71875]
    want2[3, 1:4] = [9.21875, 6.96875, 9.21875]
    assert np.array_equal(bits(h2), bits(want2))
    assert abs(float(want2[1, 2]) - 1.0415922) < 1e-6 and abs(float(want2[2, 2]) - 4.323223) < 1e-6


# ---- tie order ---------------------------------------------------------------------------------------------------------
def test_a_tie_keeps_the_earlier_neighbour():
    def centre(**nb):
        h = np.full((5, 5), f32(4.0))
        for k, v in nb.items():
            dx, dz = F.NEIGHBOURS[int(k[1:])]
            h[2 + dz, 2 + dx] = v
        r, S, drop = F.receivers(h)
        return int(r[2, 2]), float(S[2, 2]), float(drop[2, 2])
    assert centre(k0=3.0, k1=3.0) == (0, 1.0, 1.0)          # W and E: W
    assert centre(k1=3.0, k3=3.0) == (1, 1.0, 1.0)          # E and N: E
    assert centre(k2=3.0, k3=3.0)[0] == 2                    # S and N: S
    assert centre(k5=3.0, k6=3.0)[0] == 5                    # two diagonals: SE before NW
    r, S, drop = centre(k4=3.0, k3=3.0)                      # the same drop on a diagonal and on an axis: the axis
    assert (r, S, drop) == (3, 1.0, 1.0)
    r, S, drop = centre(k4=2.0)                              # a diagonal alone: slope = drop * 0.70710678f
    assert r == 4 and drop == 2.0 and f32(S) == f32(2.0) * F.DIAG and bits(F.DIAG) == 0x3F3504F3
    assert centre()[0] == F.NONE                             # a flat has no receiver


# ---- exact accumulation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [64, 97])
def test_the_drainage_converges_to_the_exact_accumulation(res):
    h = sines(res, seed=res)
    assert not np.signbit(h).any()
    A = F.rain_plane(h.shape, 1.0)
    r, _, _ = F.receivers(h)
    fixed = None
    for it in range(4 * res):  # the reference alone reaches its fixed point within the count the test allows
        nxt = F.drainage(A, r, F.rain_plane(h.shape, 1.0))
        if np.array_equal(nxt, A):
            fixed = it
            break
        A = nxt
    assert fixed is not None and fixed > 8, fixed
    got_h, got_A = F.run(h, fixed + 3, erodibility=0.0, uplift=0.0)
    assert np.array_equal(bits(got_h), bits(h))
    assert np.array_equal(got_A, A)
    assert np.array_equal(got_A.astype(np.float64), F.exact_accumulation(h))
    assert got_A[r == F.NONE].astype(np.float64).sum() == res * res


# ---- bounds ------------------------------------------------------------------------------------------------------------
def test_heights_stay_within_the_stated_bounds():
    h0 = relief(64)
    rng = np.random.default_rng(3)
    um = (rng.random(h0.shape, dtype=f32) * f32(2.0)).astype(f32)
    for maps in (None, um):
        h, A = h0.copy(), None
        lo = h0.min()
        for it in range(1, 61):
            h, A = F.run(h, 1, upliftMap=maps, drainageIn=A)
            assert h.min() >= lo, it
            top = it * 1.0 * 0.002 * (1.0 if maps is None else float(um.max()))
            slack = it * float(np.spacing(f32(np.abs(h0).max() + top)))
            assert float((h.astype(np.float64) - h0).max()) <= top + slack, it
        assert np.isfinite(h).all() and (A >= 1).all()


# ---- pits --------------------------------------------------------------------------------------------------------------
def test_no_pits_are_left_at_the_defaults():
    h0 = relief(128)
    assert F.pits(h0) > 0
    h, A = F.run(h0, 600)
    assert np.isfinite(h).all()
    assert F.pits(h) == 0


# ---- options -----------------------------------------------------------------------------------------------------------
def test_the_options_and_their_identities():
    h0 = relief(48)
    its = 12
    base_h, base_A = F.run(h0, its)
    ones, zeros = np.ones(h0.shape, f32), np.zeros(h0.shape, f32)
    for opt in (dict(rainMap=ones), dict(hardness=zeros), dict(upliftMap=ones), dict(rainMap=ones, hardness=zeros, upliftMap=ones),
                dict(drainageIn=F.rain_plane(h0.shape, 1.0))):
        h, A = F.run(h0, its, **opt)
        assert np.array_equal(bits(h), bits(base_h)) and np.array_equal(bits(A), bits(base_A)), list(opt)
    # nothing can be eroded: every cell that is no outlet rises by du per iteration, one add each
    h, A = F.run(h0, its, hardness=ones)
    want = h0.copy()
    for _ in range(its):
        want = np.where(F.outlets(h0), h0, want + f32(1.0) * f32(0.002)).astype(f32)
    assert np.array_equal(bits(h), bits(want))
    # the sea: low cells are outlets and keep their height; the others still erode
    sea = float(np.median(h0))
    h, A = F.run(h0, its, seaLevel=sea)
    low = h0 <= f32(sea)
    assert low.any() and not low.all()
    assert np.array_equal(bits(h[low]), bits(h0[low])) and not np.array_equal(h[~low], h0[~low])
    assert (F.receivers(h0, sea)[0][low] == F.NONE).all()
    # a rain map scales the drainage; a rain of 2 everywhere doubles the integers
    h, A = F.run(h0, its, erodibility=0.0, uplift=0.0, rainMap=ones * f32(2.0))
    assert np.array_equal(A, F.run(h0, its, erodibility=0.0, uplift=0.0)[1] * f32(2.0))
    # no iteration: the heights stay and the drainage is the start state
    for opt, start in ((dict(), F.rain_plane(h0.shape, 1.0)), (dict(rainMap=h0), F.rain_plane(h0.shape, 1.0, h0)),
                       (dict(drainageIn=base_A), base_A)):
        h, A = F.run(h0, 0, **opt)
        assert np.array_equal(bits(h), bits(h0)) and np.array_equal(bits(A), bits(start))


# ---- the hosts ---------------------------------------------------------------------------------------------------------
def test_the_hosts_carry_the_stage(nj):
    N = nj._native
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert N.lib.nz_fluvial_erosion_work_floats(64, 3) == 3 * 64 * 64 * 3 and N.lib.nz_fluvial_erosion_work_floats(0, 1) == 0
    # nz_fluvial_desc field by field against the binding and the C# struct
    hdr = open(os.path.join(ROOT, "include", "noize_hip.h")).read()
    body = re.search(r"typedef struct nz_fluvial_desc \{(.*?)\} nz_fluvial_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].replace("float *", "").split(",")]
    assert names == ["iterations", "erodibility", "uplift", "dt", "rain", "seaLevel", "rainMap", "hardness", "upliftMap", "drainageIn"]
    assert [f[0] for f in N.FluvialDesc._fields_] == names
    assert ctypes.sizeof(N.FluvialDesc) == 24 + 4 * ctypes.sizeof(ctypes.c_void_p)
    cs = open(os.path.join(ROOT, "host-cs", "Runtime.cs")).read()
    cs_body = re.search(r"public struct NzFluvialDesc\s*\{(.*?)\}", cs, re.S).group(1)
    assert [n.strip() for d in re.findall(r"public\s+\w+\s+([^;]+);", cs_body) for n in d.split(",")] == names
    # the stage: the model's defaults, and it chains in a pipeline
    st = nj.FluvialErosionStage(None)
    assert (st.iterations, st.erodibility, st.uplift, st.dt, st.rain) == (200, 0.05, 0.002, 1.0, 1.0)
    assert f32(st.seaLevel) == f32(F.SEA_OFF) and F.DEFAULTS["seaLevel"] == st.seaLevel
    assert (st.rainMap, st.hardness, st.upliftMap, st.drainageIn) == (None, None, None, None)
    assert st.drainage is None  # no payload yet: like the other hosts' null
    pipe = nj.BasePipeline([nj.NoiseStage(None, nj.FractalNoise.Simplex, 0.4, 1.0, 8, 2.0, 0.0, 300), st], "fluvial")
    assert isinstance(st, nj.PipelineStage) and pipe is not None
    for src, pat in (("noize_job_amd/host/noize_pipeline.hpp", r"class FluvialErosionStage\s*:\s*public PipelineStage"),
                     ("host-cs/Stages/Stages.cs", r"class FluvialErosionStage\s*:\s*PipelineStage")):
        assert re.search(pat, open(os.path.join(ROOT, src)).read()), src
