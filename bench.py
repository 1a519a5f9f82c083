#!/usr/bin/env python3
"""bench.py -- the BASELINE.json metric on MI355X.

A step = one pass of the metric pipeline (simplex fBm 13 oct -> Gauss5 x17 -> FlowMap x5 -> value
erosion x5) over one device-resident grid; nothing crosses PCIe inside the timed region.
  N = 1 : the 4096^2 tile BASELINE.json's metric is quoted on.
  N > 1 : one process per GPU (torch.distributed, backend nccl = RCCL); BASELINE config 5's 16384^2 grid,
          row-stripe sharded over the N ranks (16384 / N rows each) -> "scaling": "strong" (the same grid at
          every N; the N = 1 line carries the whole grid on one GPU as `grid_16384`, the denominator).  The
          ranks exchange the ghost rows every stencil launch consumes with their neighbour ranks over RCCL
          (--halo exchange, the default at N > 1: P2P batches on the process group's stream, overlapped with
          the launch's interior rows); `comm` says what RCCL ran and what the exchanges cost.  --halo
          recompute: every rank recomputes its 49 ghost rows per side from the closed-form noise instead (no
          data-path communication); it is reported beside the headline in `grid_16384`.
  `python bench.py --gpus N` without a launcher starts its own: N ranks through torch.distributed.run, before
  this process touches the GPU, and relays rank 0's line.
A plain run does what the headline needs and no more: set-up, warm-up, the K timed steps, --dump-outputs, the line.
Rank 0 prints ONE JSON line:
  * `stages`  : per stage, launch time from HIP events recorded on the kernels' stream inside the timed steps, and
                -- from the counter summary profiles/*_counters.json that belongs to THESE kernel sources -- the
                fraction of the fp32 VALU issue rate and of the HBM peak the kernel reaches; `bound` = the larger.
  * `roofline`: the kernel with the largest share of the step under the bound that limits it (frac <= 1).
  * `pipeline_hbm`: the 400 B/cell algorithmic-equivalent figure of SURVEY.md 8(d) (exceeds the HBM peak by design:
                filter / flow iterations are fused on chip, so it is not a roofline).
With --full, beside these, every measurement and check that runs outside the timed steps:
  * `cold_ms` and `literal_command`: one step from an idle chip, and the command taken literally (no preheat).
  * `cpu_baseline`: the CPU oracle (reference-shaped restatement of the Burst jobs) timed on this box's host cores,
                and `verified`: the device plane of the last timed step compared with the oracle's plane, bit for bit
                (sharded runs: the rows every rank owns against the oracle's rows of the monolithic grid).
  * `float_modes`, `in_place_entries`, `two_tiles_in_flight`: the other float modes, flush form and tile concurrency.
  * `grid_16384`: BASELINE config 5's grid split over the N ranks (N = 1: the whole grid on one GPU) -- the strong-
                scaling quantity the >= 6x target is defined on -- with ghost rows recomputed and, at N > 1, exchanged.
"""
import argparse
import gc
import glob
import hashlib
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# peaks: /opt/skills/guides/MI355X_MICROARCH.md (HBM3E 8 TB/s spec; 256 CU x 4 SIMD x 2.4 GHz, a wave64 fp32 VALU
# instruction occupies its SIMD for 2 cycles = 32 lanes/clk)
HBM_PEAK_GBS = 8000.0
N_SIMD, CLK_HZ, VALU_CYCLES_PER_INST = 1024, 2.4e9, 2.0
VALU_PEAK_TOPS = N_SIMD * 32 * CLK_HZ / 1e12   # 78.64 T lane-ops/s (non-FMA fp32 ops)

# algorithmic bytes per cell: fused minimum, one read + one write per plane per application
G_IT, F_IT, E_IT = 17, 5, 5
BYTES = {"noise": 4.0, "gauss": 8.0 * G_IT, "flow": 24.0 + 44.0 * (F_IT - 1) + 20.0, "erosion": 8.0 * E_IT}
STAGES = ["noise", "gauss", "flow", "erosion"]
# kernel of each stage as rocprofv3 names it (prefixes; the first that the counter summary holds)
KERNEL_PREFIX = {"noise": ("fractal_simplex_tab_kernel",), "gauss": ("conv_chain_kernel<5", "conv_reg_kernel<5"),
                 "flow": ("flow_stream_kernel", "flow_fused_kernel"), "erosion": ("erosion_reg_kernel",)}
# algorithmic fp32 lane-operations per cell (no FMA contraction anywhere, so a multiply-add is two): fBm 13
# octaves x 82 (the table form's octave-cell in the ISA: skew, two floors, unskew, two mod289, the table offsets, three corner
# falloffs and dots, 0.5 + 65 n, the amplitude; "~85" until round 5 folded rectify); one 5-tap application = 2 passes x (5 mul + 4 add); one flow iteration ~40 + velocity / normalise ~15; one
# value-erosion application = 2 min.  useful_valu_frac = this x cells / (SQ_INSTS_VALU x 64): what the halo recompute,
# selects, moves and address arithmetic leave of the instructions executed
ALGO_LANE_OPS = {"noise": 13 * 82.0, "gauss": G_IT * 18.0, "flow": F_IT * 40.0 + 15.0, "erosion": E_IT * 2.0}
# the same in lane-INSTRUCTIONS of the tolerance forms (an FMA is one): the fBm octave with its polynomial tail contracted
# (64 per octave-cell in the ISA), a 5-tap application as 2 x (1 mul + 4 fma), a flow iteration with v_rcp_f32 for the division
ALGO_LANE_OPS_MODE = {"strict": ALGO_LANE_OPS,
                      "fast": dict(ALGO_LANE_OPS, noise=13 * 64.0, gauss=G_IT * 10.0),
                      "relaxed": dict(ALGO_LANE_OPS, noise=13 * 64.0, gauss=G_IT * 10.0, flow=F_IT * 30.0 + 8.0)}
FLOAT_MODES = {"strict": 0, "fast": 1, "relaxed": 2}

CPU_PASSES = 11         # ~10 s of host work on the GPU box's 32 cores (0.9-1.0 s per 4096^2 pass)
PREHEAT_MIN_STEPS = 50  # untimed passes before the timed region, warm-up included (clock settling)
MAX_MARKED_STEPS = 200  # per-stage markers are kept for the last steps only (the handle ring holds 4096)
DUMP_MAX_BYTES = 48 << 20  # --dump-outputs: a larger plane is written as a fixed, seeded sample of its rows
DUMP_SEED = 20240917


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # the GPU's clocks keep ramping for some tens of ms of continuous work (0.96 ms/step over 5 steps,
    # 0.89 over 20, 0.85 over 100 and beyond, tools/probe_host_enqueue.py): the defaults time steady state
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--res", type=int, default=4096, help="tile resolution at N=1")
    ap.add_argument("--stripe-rows", type=int, default=0,
                    help="rows per rank at N>1 (0: --grid / N, strong scaling; a fixed count gives weak scaling)")
    ap.add_argument("--cols", type=int, default=16384, help="grid columns at N>1")
    ap.add_argument("--grid", type=int, default=16384,
                    help="--full: side of the strong-scaling grid reported as grid_16384 at every N (0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, every measurement and check outside the timed steps: the cold step and the "
                         "literal command, the CPU baseline and the oracle comparison, the other float modes, the in-place "
                         "and two-tile forms, the --grid strong-scaling grid (a plain run: the headline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="--full without the CPU baseline and the comparisons with the oracle")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the informational measurements after the timed steps")
    ap.add_argument("--sharded", action="store_true", help="run the row-stripe path even with one rank (rehearsal)")
    ap.add_argument("--halo", choices=("recompute", "exchange", "exchange_once"), default=None,
                    help="N>1 (default exchange): ghost rows exchanged with the neighbour ranks over RCCL before every "
                         "launch, or recomputed from the closed-form noise (no data-path communication; the default "
                         "of the one-rank rehearsals)")
    ap.add_argument("--self-launch", action="store_true",
                    help="go through the launcher even with one rank (what --gpus N > 1 does when no launcher set "
                         "WORLD_SIZE): the ranks are children started with torch.distributed.run")
    ap.add_argument("--as-rank", type=int, nargs=2, metavar=("R", "P"), default=None,
                    help="one-process rehearsal of rank R of a P-rank job: --halo recompute, or (native schedule) --halo "
                         "exchange / exchange_once with the neighbour ranks played by the rank itself through RCCL")
    ap.add_argument("--overlap", type=int, choices=(0, 1, 2), default=0,
                    help="native exchange schedule: 0 = RCCL transfers on the compute stream between the launches; 1 = a launch's "
                         "interior rows while its ghost rows travel, border rows after; 2 = border rows first, the NEXT "
                         "launch's exchange travels while the interior runs")
    ap.add_argument("--marked-steps", type=int, default=200,
                    help="sharded runs: stage markers (five event records per step) in the last this-many timed steps only")
    ap.add_argument("--impl", choices=("native", "python"), default="native",
                    help="sharded runs: `native` = the stripe schedule and the RCCL exchange behind the C ABI "
                         "(nz_sharded_pipeline: one call per step, ncclSend / ncclRecv on the library's communicator "
                         "stream); `python` = the same schedule in noize_job_amd/sharded.py over torch.distributed P2P")
    ap.add_argument("--flush", choices=("swap", "copy"), default="swap",
                    help="N=1: the tile is a READ / WRITE plane pair and TileHelpers.SWAP_RWTILE is a pointer swap "
                         "(nz_*_rw entries), or one plane with the in-place entries and their flush copies")
    ap.add_argument("--cpu-res", type=int, default=0, help="tile side of the CPU baseline (0 = --res)")
    ap.add_argument("--float-mode", choices=tuple(FLOAT_MODES), default="strict",
                    help="nz_ctx_set_float_mode of the timed steps: strict (the reference's operation sequence, bit-equal to the "
                         "oracle: the headline), fast (fBm tail and tap sums FMA-contracted, every stage within 1e-5 of strict), "
                         "relaxed (fast + the flow iterations).  The other modes are timed beside the headline in `float_modes`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the height plane the last timed step left (what a caller of the timed "
                         "path receives) as DIR/height.npy (float32, rows x cols) and the global index of each of its rows as "
                         "DIR/height_rows.npy (float64); a plane over %d MiB is written as a fixed, seeded sample of its rows"
                         % (DUMP_MAX_BYTES >> 20))
    return ap.parse_args()


def dump_rows(grid_rows, cols):
    """The global rows --dump-outputs writes for a grid_rows x cols plane: all of them, or a fixed, seeded sample (sorted) that
    fits DUMP_MAX_BYTES.  The same arguments give the same rows on every run and every build."""
    import numpy as np
    k = min(grid_rows, max(1, DUMP_MAX_BYTES // (cols * 4)))
    if k == grid_rows:
        return np.arange(grid_rows)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(grid_rows, k, replace=False))


def write_dump(np, out_dir, rows, height):
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "height.npy"), np.ascontiguousarray(height, dtype=np.float32))
    np.save(os.path.join(out_dir, "height_rows.npy"), np.asarray(rows, dtype=np.float64))


# ---- counter summaries ---------------------------------------------------------------------------------------------
def kernel_sources_sha():
    """sha256 over the kernel sources: a counter summary is only used for a run of the very same kernels."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "noize_job_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".cpp", ".hpp")) or name == "Makefile":
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def load_counters(res, flush, mode="strict"):
    """Newest profiles/*_counters.json (tools/fold_counters.py) taken with these kernel sources, this flush mode and this float mode:
    per kernel SQ_INSTS_VALU and HBM bytes (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes) per launch.  A summary of
    another tile size is used scaled by the cell count and says so.  None if nothing matches."""
    sha = kernel_sources_sha()
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_counters.json"))):
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        c = d.get("config", {}) if isinstance(d, dict) else {}
        if not isinstance(c, dict) or "kernels" not in d:  # another tool's summary (e.g. *_config4_counters.json)
            continue
        if (c.get("kernel_sources_sha") == sha and c.get("flush") == flush and not c.get("sharded")
                and c.get("float_mode", "strict") == mode):
            best = (path, d)
    if best is None:
        return None
    path, d = best
    scale = float(res * res) / float(d["config"]["res"] ** 2)
    return {"file": os.path.relpath(path, ROOT), "commit": d["config"].get("commit"), "kernels": d["kernels"],
            "scale": scale, "res": d["config"]["res"]}


def counters_for(cnt, stage):
    if cnt is None:
        return None
    for prefix in KERNEL_PREFIX[stage]:
        for name, e in cnt["kernels"].items():
            if name.startswith(prefix):
                return name, e
    return None


# ---- informational measurements --------------------------------------------------------------------------------------
def make_stages(nj, ctx, p):
    return [nj.NoiseStage(ctx, nj.FractalNoise.Simplex, p.hurst, p.startingAmplitude, p.octaves, p.stepdown,
                          p.detuneRate, p.noiseSize),
            nj.KernelFilterStage(ctx, nj.KernelFilterType.Gauss5_S1, G_IT),
            nj.FlowMapStage(ctx, F_IT, p.normMin, p.normMax), nj.ErosionStage(ctx, E_IT)]


def two_tiles(nj, ctx, stages, gd, res, p, swap, steps=100):
    """Informational, outside the timed steps: two INDEPENDENT tiles, each with its own context (HIP stream), pipelines
    issued alternately.  The fp32-bound and the HBM-bound kernels of different tiles overlap; `value` above is the
    single tile BASELINE.json names."""
    ctx2 = nj.Context(ctx.device)
    cells = res * res
    stages2 = make_stages(nj, ctx2, p)
    gd2 = nj.GeneratorData("bench2", ctx2.alloc(cells), res, res, 0, write=ctx2.alloc(cells) if swap else None)
    h0 = nj.JobHandle()

    def both():
        for a, b in zip(stages, stages2):
            a.Schedule(nj.PipelineWorkItem(gd), h0)
            b.Schedule(nj.PipelineWorkItem(gd2), h0)
    for _ in range(20):
        both()
    ctx.synchronize(); ctx2.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        both()
    ctx.synchronize(); ctx2.synchronize()
    dt = (time.perf_counter() - t0) / (2 * steps)
    for st in stages2:
        st.OnDestroy()
    gd2.data.Dispose()
    if gd2.write is not None:
        gd2.write.Dispose()
    ctx2.close()
    return {"streams": 2, "ms_per_tile": round(dt * 1e3, 4), "Mcells/s": round(cells / dt / 1e6, 1),
            "note": "two independent %d^2 tiles on two HIP streams, not the headline value" % res}


def in_place_entries(nj, ctx, res, p, steps=60):
    """Informational: the strictly drop-in form -- ONE plane, the in-place stage entries, results land in `data` as in
    the reference (their flush copies stand for TileHelpers.SWAP_RWTILE) -- what `--flush copy` times as its headline."""
    cells = res * res
    stages = make_stages(nj, ctx, p)
    gd = nj.GeneratorData("inplace", ctx.alloc(cells), res, 0, 0)
    pipe = nj.BasePipeline(stages, "in-place")

    def one():
        pipe.Schedule(gd)
        pipe.pipelineRunning = False
    for _ in range(20):
        one()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / steps
    pipe.Destroy()
    gd.data.Dispose()
    return {"ms_per_step": round(dt * 1e3, 4), "Mcells/s": round(cells / dt / 1e6, 1),
            "note": "one plane, in-place entries with their flush copies (bench.py --flush copy): results land in "
                    "`data` exactly as in the reference"}


class TimedComm:
    """Wraps a halo-exchange object: stream markers around every exchange, so the time the compute stream spends
    waiting for ghost rows is known per step."""

    def __init__(self, comm, ctx):
        self.comm, self.ctx, self.spans = comm, ctx, []
        self.overlap = getattr(comm, "overlap", False)
        self.enabled = True  # markers only while set (the handle ring holds 4096 markers)

    def exchange(self, planes, plan, up_rows, down_rows):
        if not self.enabled:
            return self.comm.exchange(planes, plan, up_rows, down_rows)
        a = self.ctx.record()
        self.comm.exchange(planes, plan, up_rows, down_rows)
        self.spans.append((a, self.ctx.record()))

    def begin(self, planes, plan, up_rows, down_rows):  # asynchronous: only the stream's wait in finish() is charged
        return self.comm.begin(planes, plan, up_rows, down_rows)

    def finish(self, reqs):
        if not self.enabled:
            return self.comm.finish(reqs)
        a = self.ctx.record()
        self.comm.finish(reqs)
        self.spans.append((a, self.ctx.record()))

    def total_ms(self):
        t = sum(self.ctx.elapsed_ms(a, b) for a, b in self.spans)
        self.spans = []
        return t


def make_native_comm(sh, torch, dist, ctx, rank, world):
    """nz_comm for this rank: rank 0 draws the ncclUniqueId (nz_comm_unique_id), torch.distributed carries its 128 bytes to
    the other ranks (out-of-band plumbing), every rank joins with nz_comm_init."""
    uid = [sh.NativeComm.unique_id() if rank == 0 else None]
    if world > 1:
        dist.broadcast_object_list(uid, src=0)
    return sh.NativeComm(ctx, uid[0], rank, world)


def strong_grid(nj, sh, torch, dist, ctx, grid, rank, world, impl="native", ncomm=None, steps=20, warm=5, verify=True,
                strict=True):
    """BASELINE config 5's grid (grid^2) split into `world` row stripes, one per rank: the quantity the >= 6x target is
    defined on, measured at EVERY N (N = 1: the whole grid on one GPU).  Ghost rows recomputed from the closed-form
    noise (no communication) and, at N > 1, exchanged with the neighbour ranks over RCCL before every launch, with the
    time the compute stream spends in the exchanges split out.  Barrier + synchronize on both sides, max over ranks."""
    import numpy as np
    out = {}
    ops = sh.HipStripeOps(ctx)
    oracle_cache = {}
    # native: "exchange" = the transfers on the compute stream between the launches (overlap 0, the default);
    # "exchange_interior_first" / "exchange_border_first" = the two overlapped schedules (overlap 1 / 2).
    # python: "exchange" = overlapped P2P batches, "exchange_blocking" = the exchange completes first
    if world <= 1:
        modes = ("recompute",)
    elif impl == "native":
        modes = ("recompute", "exchange", "exchange_interior_first", "exchange_border_first", "exchange_once")
    else:
        modes = ("recompute", "exchange", "exchange_blocking", "exchange_once")
    for label in modes:
        gc.collect()  # (main() holds the collector off; a pass by hand before every warm-up)
        mode = "exchange" if label.startswith("exchange_") and label != "exchange_once" else label
        p = sh.PipelineParams(gaussIterations=G_IT, flowIterations=F_IT, erosionIterations=E_IT, haloMode=mode)

        def fence():
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
        host_s = 0.0
        if impl == "native":
            g = sh.ShardedGrid(ctx, ncomm if world > 1 else None, grid, grid, p, stripes=world,
                               overlap={"exchange_interior_first": 1, "exchange_border_first": 2}.get(label, 0))
            for _ in range(warm):
                g.run()
            fence()
            g.set_timing(mode != "recompute" and world > 1)
            t0 = time.perf_counter()
            for _ in range(steps):
                h0 = time.perf_counter()
                g.run()
                host_s += time.perf_counter() - h0
            fence()
            dt = time.perf_counter() - t0
            ex_ms = g.exchange_ms() / steps if (mode != "recompute" and world > 1) else 0.0
            # the rows every rank owns after the last timed pass against the CPU oracle (outside the timed region)
            ver = verify_sharded(np, torch, dist, g, p, grid, grid, world, oracle_cache, strict) if verify else None
            g.close()
        else:
            halo = sh.halo_rows_needed(ops, p)
            plan = sh.StripePlan(rank, world, grid, grid, halo, neighbours_own_halo=mode != "recompute")
            bufs = (torch.zeros(plan.rows, grid, dtype=torch.float32, device="cuda"),
                    torch.zeros(plan.rows, grid, dtype=torch.float32, device="cuda"),
                    torch.zeros(sh.FLOW_PLANES, plan.rows, grid, dtype=torch.float32, device="cuda"),
                    torch.zeros(sh.FLOW_PLANES, plan.rows, grid, dtype=torch.float32, device="cuda"))
            # "exchange": the launch that needs the ghost rows runs its interior while they travel (RCCL P2P on the process
            # group's stream), its border rows after; "exchange_blocking": the exchange completes first
            comm = sh.NoComm() if mode == "recompute" else TimedComm(sh.TorchComm(dist, overlap=label != "exchange_blocking"), ctx)
            for _ in range(warm):
                sh.run_pipeline(ops, comm, plan, p, bufs)
            fence()
            if isinstance(comm, TimedComm):
                comm.total_ms()
            t0 = time.perf_counter()
            for _ in range(steps):
                h0 = time.perf_counter()
                sh.run_pipeline(ops, comm, plan, p, bufs)
                host_s += time.perf_counter() - h0
            fence()
            dt = time.perf_counter() - t0
            ex_ms = comm.total_ms() / steps if isinstance(comm, TimedComm) else 0.0
            ver = None  # (the Python schedule is verified by tests/test_gpu_fullsize.py)
            del bufs
            torch.cuda.empty_cache()
        host_ms = host_s / steps * 1e3
        if world > 1:
            t = torch.tensor([dt, ex_ms, host_ms], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt, ex_ms, host_ms = float(t[0].item()), float(t[1].item()), float(t[2].item())
        e = {"ms_per_step": round(dt / steps * 1e3, 4), "Mcells/s": round(grid * grid / (dt / steps) / 1e6, 1),
             "host_enqueue_ms_per_step": round(host_ms, 4)}
        if mode != "recompute":
            e["exchange_ms_per_step"] = round(ex_ms, 4)
        if ver is not None:
            e.update(ver)
        out[label] = e
    out["grid"] = "%dx%d as %d row stripes of %d rows" % (grid, grid, world, grid // world)
    out["steps"] = steps
    out["impl"] = impl
    checked = [out[k]["verified"] for k in modes if isinstance(out.get(k), dict) and "verified" in out[k]]
    out["verified"] = all(checked) if checked else None
    out["note"] = ("strong scaling: the same %d^2 grid at every N; speed-up at N GPUs = this figure at N / this figure "
                   "at N = 1.  `verified`: after the timed passes of every schedule each rank compares the rows it owns with "
                   "the CPU oracle's rows of the monolithic grid%s" % (grid, " (bit for bit)" if strict else " (1e-5 rel / 1e-6 abs)"))
    return out


def oracle_rows(p, grid_rows, cols, g0, g1, threads=0):
    """Rows [g0, g1) of the monolithic grid_rows x cols pipeline from the CPU oracle (the checker), computed on a window
    widened by more than the stage list's dependency radius (2 rows per 5-tap application, 2 per flow iteration, 1 per
    erosion application upwards): the clamps at the window's own ends cannot reach the rows kept, the clamps at the grid's
    real border are the window's.  1 / N of the whole-grid oracle pass per rank."""
    import oracle as O
    O.lib()
    if threads > 0:
        O.set_threads(threads)
    margin = 4 * p.gaussIterations + 2 * p.flowIterations + p.erosionIterations + 8  # generous for every 3..9-tap filter
    a, b = max(0, g0 - margin), min(grid_rows, g1 + margin)
    w = O.pipeline(b - a, cols, p.noiseType, p.hurst, p.startingAmplitude, p.stepdown, p.detuneRate, p.octaves, p.xpos,
                   p.zpos + a, p.noiseSize, p.filter, p.gaussIterations, p.flowIterations, p.normMin, p.normMax,
                   p.erosionIterations)
    return w[g0 - a:g1 - a]


def verify_sharded(np, torch, dist, grid_obj, p, grid_rows, cols, world, cache, strict):
    """The rows this rank owns after the last pass against the oracle's (bit for bit in strict mode), every rank for itself,
    the verdicts combined (min over ranks).  -> {"verified", "rows_checked", "oracle_s"}.  `cache` keeps a rank's oracle rows
    between the schedules of one grid."""
    t0 = time.perf_counter()
    ok, rows_checked, worst = True, 0, 0.0
    for i in range(grid_obj.local_stripes):
        g0, got = grid_obj.owned_rows(i)
        key = (grid_rows, cols, g0, g0 + got.shape[0])
        if key not in cache:
            cache[key] = oracle_rows(p, grid_rows, cols, g0, g0 + got.shape[0], threads=max(1, (os.cpu_count() or 1) // max(1, world)))
        want = cache[key]
        same = bool(np.array_equal(got, want))
        if not same:
            worst = max(worst, float(np.abs(got - want).max()))
        ok = ok and (same if strict else bool(np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 1e-6)))
        rows_checked += got.shape[0]
    if world > 1:
        t = torch.tensor([1.0 if ok else 0.0, -float(rows_checked), -worst], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        ok, worst = bool(t[0].item() > 0.5), -float(t[2].item())
        tr = torch.tensor([float(rows_checked)], dtype=torch.float64, device="cuda")
        dist.all_reduce(tr, op=dist.ReduceOp.SUM)
        rows_checked = int(tr[0].item())
    r = {"verified": ok, "rows_checked": rows_checked, "oracle_and_compare_s": round(time.perf_counter() - t0, 2)}
    if not ok:
        r["max_abs_diff"] = worst
    return r


def cpu_baseline(res):
    import oracle as O
    O.lib()
    times, plane = [], None
    for _ in range(CPU_PASSES):
        t0 = time.perf_counter()
        plane = O.pipeline(res, res, O.SIMPLEX, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700, O.GAUSS5_S1, G_IT, F_IT, 0.0, 0.005,
                           E_IT)
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[len(times) // 2]
    flags = "?"
    try:
        with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
            mk = f.read()
        flags = " ".join(mk.split("CFLAGS  ?=")[1].split("LDFLAGS")[0].replace("\\\n", " ").split())
    except (OSError, IndexError):
        pass
    return {"value": round(res * res / dt / 1e6, 2), "unit": "Mcells/s", "cores": O.get_threads(), "kind": "port",
            "sample": "median of %d passes of the full metric pipeline on a %dx%d tile (%.2f s per pass); oracle/"
                      "noize_oracle.c built with gcc %s; OpenMP `parallel for` over rows per pass (schedule(dynamic,1) "
                      "for the fBm rows, static for the stencil passes), the reference's serial flush copy after every "
                      "read-write pass" % (CPU_PASSES, res, res, dt, flags)}, plane


def stage_planes(res):
    """The oracle's plane after every stage of the metric pipeline (the checker's intermediates; ~ one CPU pass)."""
    import oracle as O
    noise = O.fractal(O.SIMPLEX, res, res, 0.4, 1.0, 2.0, 0.0, 13, 0, 0, 1700)
    gauss = O.kernel_filter(noise, O.GAUSS5_S1, G_IT)
    flow = O.flowmap(gauss, F_IT, 0.0, 0.005)
    return {"noise": noise, "gauss": gauss, "flow": flow, "erosion": O.erosion_min(flow, E_IT)}


def stages_within_tolerance(np, nj, ctx, p, res, want):
    """Every stage of the metric pipeline in the context's float mode, EACH FED THE ORACLE'S INPUT PLANE, against the oracle's
    output plane: the per-stage contract of BASELINE.json (1e-5 relative, 1e-6 absolute floor), as tests/test_gpu_fast.py
    checks it.  -> (all inside, {stage: {"max_rel", "max_abs", "cells_outside"}})."""
    cells = res * res
    inputs = {"noise": None, "gauss": want["noise"], "flow": want["gauss"], "erosion": want["flow"]}
    detail, ok = {}, True
    for name, st in zip(STAGES, make_stages(nj, ctx, p)):
        t = ctx.alloc(cells) if inputs[name] is None else ctx.from_host(inputs[name])
        w = ctx.alloc(cells)
        gd = nj.GeneratorData("check-" + name, t, res, 0, 0, write=w)
        st.ReceiveHandledInput(nj.PipelineWorkItem(gd), nj.JobHandle())
        st.jobHandle.Complete()
        got = gd.data.ToArray((res, res))
        st.OnDestroy()
        t.Dispose()
        w.Dispose()
        d = np.abs(got.astype(np.float64) - want[name])
        bad = int((d > 1e-5 * np.abs(want[name]) + 1e-6).sum())
        detail[name] = {"max_rel": float((d / np.maximum(np.abs(want[name]), 0.1)).max()), "max_abs": float(d.max()),
                        "cells_outside": bad}
        ok = ok and bad == 0
    return ok, detail


def self_launch(argv, gpus):
    """`python bench.py --gpus N` as the driver runs N = 1, with no launcher around it: start the N ranks as children
    (python -m torch.distributed.run, rendezvous on 127.0.0.1) BEFORE this process has touched the GPU -- a process that
    has initialised HIP must never exec or be replaced -- relay their stdout (rank 0's one JSON line) and exit with the
    launcher's code."""
    import socket
    import subprocess
    import tempfile
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL between processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "4")
    rc, last = 1, None
    for attempt in range(3):
        with socket.socket() as sk:  # a free port for the rendezvous
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + \
              [a for a in argv if a != "--self-launch"]
        print("bench.py: no launcher (WORLD_SIZE unset): starting %d rank(s): %s" % (gpus, " ".join(cmd)), file=sys.stderr)
        with tempfile.TemporaryFile("w+") as err:
            child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=err, text=True)
            last = None
            for line in child.stdout:
                if line.startswith("{"):
                    last = line
                else:
                    sys.stderr.write(line)
            rc = child.wait()
            err.seek(0)
            text = err.read()
        sys.stderr.write(text)
        # the port was free when it was probed and taken when the launcher's store bound it (another process of the box, a
        # socket of an earlier run still closing): nothing has touched a GPU yet, take another port
        if rc and last is None and "EADDRINUSE" in text and attempt < 2:
            print("bench.py: port %d was taken before the rendezvous bound it; trying another" % port, file=sys.stderr)
            continue
        break
    if last is not None:
        sys.stdout.write(last)
        sys.stdout.flush()
    raise SystemExit(rc if rc else (0 if last is not None else 1))


def main():
    args = parse()
    if args.dump_outputs and args.impl == "python" and (args.gpus > 1 or args.sharded or args.as_rank is not None):
        raise SystemExit("--dump-outputs: the sharded runs dump the native schedule's planes only (--impl native)")
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.self_launch):
        self_launch(sys.argv[1:], args.gpus)
    import numpy as np
    import torch
    import torch.distributed as dist

    import noize_job_amd as nj
    from noize_job_amd import sharded as sh

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.halo is None:
        args.halo = "exchange" if world > 1 else "recompute"
    # a plain run times the headline and nothing else; --full adds the checks against the oracle and the informational
    # measurements, which --no-cpu-baseline / --no-extras narrow
    checks = args.full and not args.no_cpu_baseline
    extras = args.full and not args.no_extras
    # stdout carries the ONE JSON line only: whatever libraries print while they initialise (RCCL's version
    # banner under NCCL_DEBUG=VERSION) is sent to stderr
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    ndev = torch.cuda.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs an MI355X: no HIP device is visible")
    local_rank %= ndev  # a launcher that narrows HIP_VISIBLE_DEVICES per rank leaves one device, index 0
    torch.cuda.set_device(local_rank)
    sharded = world > 1 or args.sharded or args.as_rank is not None
    if args.as_rank is not None and (world != 1 or (args.halo != "recompute" and args.impl != "native")):
        raise SystemExit("--as-rank is a single-process rehearsal: --halo recompute, or the native schedule with the "
                         "neighbour ranks played by the rank itself")
    if sharded:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    ctx = nj.Context(local_rank, stream=stream.cuda_stream)
    ctx.float_mode = FLOAT_MODES[args.float_mode]

    p = sh.PipelineParams(gaussIterations=G_IT, flowIterations=F_IT, erosionIterations=E_IT, haloMode=args.halo)
    marks = []  # per step: handles at stage boundaries
    cold_ms = None

    if not sharded:
        res = args.res
        cells = res * res
        data = torch.empty(cells, dtype=torch.float32, device="cuda")
        tile = ctx.wrap(data.data_ptr(), cells)
        swap = args.flush == "swap"
        data_w = torch.empty(cells, dtype=torch.float32, device="cuda") if swap else None
        stages = make_stages(nj, ctx, p)
        pipe = nj.BasePipeline(stages, "metric")
        gd = nj.GeneratorData("bench", tile, res, 0, 0, write=ctx.wrap(data_w.data_ptr(), cells) if swap else None)

        pipe.Schedule(gd)  # one untimed pass: buffers, code objects
        pipe.pipelineRunning = False

        prev_end = [None]  # the last marked step's final handle, while nothing else has been enqueued since

        def step(record):
            if record:
                # the step's first marker IS the previous step's last one (the stage handles are the only events a
                # marked step records: each costs the stream ~3 us, tools/probe_event_cost.py)
                hs = [prev_end[0] if prev_end[0] is not None else ctx.record()]
                for st in stages:  # same chain BasePipeline.Schedule builds, with a marker between stages
                    st.Schedule(nj.PipelineWorkItem(gd), hs[-1])
                    hs.append(st.jobHandle)
                marks.append(hs)
                prev_end[0] = hs[-1]
            else:
                prev_end[0] = None
                pipe.Schedule(gd)
                pipe.pipelineRunning = False

        workload = "%dx%d tile: simplex-13oct(h0.4,size1700) -> Gauss5_S1 x%d -> FlowMap x%d (norm 0/0.005) -> " \
                   "ValueErosion x%d" % (res, res, G_IT, F_IT, E_IT)
        parallelism = "single tile"
        flush_note = ("READ/WRITE plane pair, SWAP_RWTILE = pointer swap (nz_*_rw entries)" if swap else
                      "one plane, in-place entries with flush copies")
    else:
        swap, flush_note = False, "stripe entries (explicit src / dst planes)"
        ops = sh.HipStripeOps(ctx)
        halo = sh.halo_rows_needed(ops, p)
        prank, pworld = args.as_rank if args.as_rank is not None else (rank, world)
        strong = args.stripe_rows <= 0  # the same --grid rows at every N, split over the ranks
        stripe_rows = args.stripe_rows if not strong else max(1, (args.grid or 16384) // pworld)
        plan = sh.StripePlan(prank, pworld, stripe_rows * pworld, args.cols, halo,
                             neighbours_own_halo=args.halo != "recompute")
        cells = plan.nown * world * plan.cols  # every rank owns stripe_rows rows
        host_s = [0.0]  # host time spent enqueueing the timed steps
        ncomm = grid = comm = None
        if args.impl == "native":
            # the schedule and the exchange behind the C ABI: one nz_sharded_pipeline call per step
            if world > 1 or args.halo != "recompute":
                ncomm = make_native_comm(sh, torch, dist, ctx, rank, world)
            grid = sh.ShardedGrid(ctx, ncomm, plan.grows, plan.cols, p, stripes=pworld, overlap=args.overlap, as_rank=args.as_rank)

            def step(record):
                h0 = time.perf_counter()
                if record:  # stream markers where the stages begin (exchanges of a stage are charged to it)
                    marks.append(grid.run(marks=True)[1])
                else:
                    grid.run()
                host_s[0] += time.perf_counter() - h0
        else:
            bufs = (torch.zeros(plan.rows, plan.cols, dtype=torch.float32, device="cuda"),
                    torch.zeros(plan.rows, plan.cols, dtype=torch.float32, device="cuda"),
                    torch.zeros(sh.FLOW_PLANES, plan.rows, plan.cols, dtype=torch.float32, device="cuda"),
                    torch.zeros(sh.FLOW_PLANES, plan.rows, plan.cols, dtype=torch.float32, device="cuda"))
            # the exchanges are asynchronous (P2P batches on the process group's stream, the launch's interior rows run
            # meanwhile); TimedComm brackets the compute stream's wait for them with stream markers
            comm = sh.NoComm() if args.halo == "recompute" else TimedComm(sh.TorchComm(dist), ctx)

            def step(record):
                h0 = time.perf_counter()
                if record:  # stream markers where the stages begin (exchanges of a stage are charged to it)
                    hs = {}
                    sh.run_pipeline(ops, comm, plan, p, bufs, on_stage=lambda name: hs.__setitem__(name, ctx.record()))
                    marks.append([hs[n] for n in ("noise", "gauss", "flow", "erosion", "end")])
                else:
                    sh.run_pipeline(ops, comm, plan, p, bufs)
                host_s[0] += time.perf_counter() - h0

        how = {"exchange": "ghost rows exchanged over RCCL before every launch",
               "exchange_once": "%d ghost rows per side of the source plane exchanged once over RCCL" % halo,
               "recompute": "%d ghost rows per side recomputed from the closed-form noise, no data-path "
                            "communication" % halo}[args.halo]
        workload = "%dx%d grid as %d row stripes of %dx%d (%s): simplex-13oct -> Gauss5_S1 x%d " \
                   "-> FlowMap x%d -> ValueErosion x%d" % (plan.grows, plan.cols, pworld, stripe_rows, plan.cols,
                                                            how, G_IT, F_IT, E_IT)
        parallelism = "row-stripe dp%d" % world
        if args.as_rank is not None:
            parallelism = "rehearsal of rank %d of %d on one GPU" % (prank, pworld)

    def fence():
        if sharded:
            dist.barrier()
        torch.cuda.synchronize()

    if args.full and not sharded:
        # first-tile latency: what a tile server sees for a request that finds the chip idle (code objects loaded and
        # buffers allocated by one untimed pass, then half a second of idleness for the clocks to fall back)
        step(False)
        fence()
        time.sleep(0.5)
        t0 = time.perf_counter()
        step(False)
        fence()
        cold_ms = (time.perf_counter() - t0) * 1e3

    # The chip's clocks need some tens of ms of continuous work to settle (see --steps above).  A caller that asks
    # for a short run still gets the steady-state rate: the GPU is kept busy with untimed passes first, so that
    # warm-up + preheat cover at least PREHEAT_MIN_STEPS passes.  The K timed steps are exactly the K asked for.
    # The host of this bench is CPython: its cyclic collector starts a full pass at a fixed allocation count -- with the
    # default steps, inside the 60th marked step's filter stage -- and that pass takes 34-67 ms with torch's heap loaded.  The
    # host enqueues ~25 us per step and is 38 ms of GPU work ahead at that point: on a slow host the GPU ran dry for up to
    # 30 ms, one step in 200 (tools/trace_outliers.sh, NZ_BENCH_HOST_TIMES=1).  A host's pauses are not
    # the library's throughput: the collector is held off while steps are timed (from before the warm-up: a collection is
    # 35 ms of idle GPU, and the clocks it lets fall take a few steps to come back).
    gc.collect()
    gc.disable()
    preheat = max(0, PREHEAT_MIN_STEPS - args.warmup)
    literal = None
    if args.full and preheat > 0:
        # The command exactly as given -- W warm-ups, then K timed steps, from a chip that has been idle for half a second,
        # no preheat: reported as `literal_command` beside the steady-state headline (whose `warmup_effective` says what ran)
        fence()
        time.sleep(0.5)
        for _ in range(args.warmup):
            step(False)
        fence()
        tl = time.perf_counter()
        for _ in range(args.steps):
            step(False)
        fence()
        literal = (time.perf_counter() - tl) / args.steps
        if sharded:
            tlit = torch.tensor([literal], dtype=torch.float64, device="cuda")
            dist.all_reduce(tlit, op=dist.ReduceOp.MAX)
            literal = float(tlit[0].item())
    for _ in range(preheat):
        step(False)
    for _ in range(args.warmup):
        step(False)
    fence()
    if sharded and isinstance(comm, TimedComm):
        comm.total_ms()  # forget the warm-up's exchanges
    if sharded:
        host_s[0] = 0.0
    timed_exchanges = sharded and args.halo != "recompute" and (grid is not None or isinstance(comm, TimedComm))
    t0 = time.perf_counter()
    host_t = [t0]  # when the host had enqueued each timed step
    ex_steps = min(args.steps, 64)  # exchanges are bracketed with markers in the last steps only
    for i in range(args.steps):
        if timed_exchanges and args.steps - i == ex_steps:
            if grid is not None:
                grid.set_timing(True)
            else:
                comm.enabled = True
        elif timed_exchanges and i == 0 and grid is None:
            comm.enabled = False
        step(args.steps - i <= (MAX_MARKED_STEPS if not sharded else min(MAX_MARKED_STEPS, args.marked_steps)))
        host_t.append(time.perf_counter())
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        # outside the timed region: the plane the last timed step left, before anything else runs on it
        if not sharded:
            rows = dump_rows(res, res)
            last = np.empty(cells, np.float32)
            nj._native.check(nj._native.lib.nz_tile_download(ctx._h, gd.data.ptr, last.ctypes.data, cells, 0, None),
                             "download")
            fence()
            write_dump(np, args.dump_outputs, rows, last.reshape(res, res)[rows])
        else:
            # every rank's share of the sampled rows, gathered on rank 0 in global row order
            rows = dump_rows(plan.grows, plan.cols)
            mine = []
            for i in range(grid.local_stripes):
                g0, got = grid.owned_rows(i)
                sel = rows[(rows >= g0) & (rows < g0 + got.shape[0])]
                mine.append((sel, got[sel - g0]))
            parts = [None] * world
            if world > 1:
                dist.all_gather_object(parts, mine)
            else:
                parts = [mine]
            if rank == 0:
                got_rows = np.concatenate([r for part in parts for r, _ in part])
                height = np.concatenate([h for part in parts for _, h in part], axis=0)
                order = np.argsort(got_rows, kind="stable")
                write_dump(np, args.dump_outputs, got_rows[order], height[order])
    # (the collector stays off for the informational measurements below, which collect by hand before their own warm-ups)
    if os.environ.get("NZ_BENCH_HOST_TIMES"):
        iv = [(host_t[k + 1] - host_t[k]) * 1e3 for k in range(len(host_t) - 1)]
        top = sorted(range(len(iv)), key=lambda k: -iv[k])[:4]
        print("host enqueue per timed step: median %.3f ms; longest %s; all %d steps enqueued after %.2f ms of the %.2f ms they took"
              % (sorted(iv)[len(iv) // 2], [(k, round(iv[k], 3)) for k in top], len(iv), (host_t[-1] - t0) * 1e3, dt * 1e3),
              file=sys.stderr)
    exchange_ms = host_enqueue_ms = host_idle_ms = None
    if sharded:
        if args.full:
            # the host's own cost of enqueueing a step, measured where the queue cannot push back: eight steps on an idle
            # stream, each call timed on its own (the timed steps above run against a full queue)
            probe = []
            for _ in range(8):
                h0 = time.perf_counter()
                step(False)
                probe.append(time.perf_counter() - h0)
            fence()
            host_idle_ms = sorted(probe)[len(probe) // 2] * 1e3
        ex = 0.0
        if timed_exchanges:
            ex = (grid.exchange_ms() if grid is not None else comm.total_ms()) / ex_steps
        t = torch.tensor([dt, ex, host_s[0] / args.steps * 1e3], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, exchange_ms, host_enqueue_ms = float(t[0].item()), float(t[1].item()), float(t[2].item())

    rank_reports = None
    if sharded:
        # what every rank's communicator says about itself (nz_comm_rank / nz_comm_world = ncclCommUserRank / ncclCommCount of the
        # library's own communicator), its HIP device and the rows it owns: gathered so that the line shows N distinct devices
        mine = {"rank": rank, "device": torch.cuda.current_device(), "device_name": torch.cuda.get_device_name(),
                "pci_bus": getattr(torch.cuda.get_device_properties(torch.cuda.current_device()), "pci_bus_id", None),
                "native_comm": None if ncomm is None else {"rank": sh.N.lib.nz_comm_rank(ncomm._h), "world": sh.N.lib.nz_comm_world(ncomm._h)},
                "owned_rows": [plan.g0, plan.g0 + plan.nown]}
        rank_reports = [None] * world
        dist.all_gather_object(rank_reports, mine)

    out = None
    out_lock = threading.Lock()
    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = cells / (dt / args.steps) / 1e6
        total_bytes = sum(BYTES.values())
        out = {"metric": "Mcells/s 4096^2 simplex13oct->Gauss5x17->FlowMap->Erosion; %HBM roofline @1/8GPU",
               "value": round(value, 1), "unit": "Mcells/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "warmup_effective": preheat + args.warmup,
               "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
               "scaling": "strong" if (not sharded or strong) else "weak", "vs_baseline": None, "dtype": "f32",
               "data": "synthetic",
               "config": {"workload": workload, "cells": cells, "parallelism": parallelism, "preheat_steps": preheat,
                          "algorithmic_bytes_per_cell": total_bytes, "flush": flush_note},
               "pipeline_hbm": {"achieved": round(total_bytes * cells / (dt / args.steps) / 1e9 / world, 1),
                                "peak": HBM_PEAK_GBS, "unit": "GB/s per GPU",
                                "frac": round(total_bytes * cells / (dt / args.steps) / 1e9 / world / HBM_PEAK_GBS, 4),
                                "note": "algorithmic-equivalent bytes (SURVEY.md 8d: 400 B/cell, one plane round trip per "
                                        "filter / flow / erosion application) over the step time.  NOT a roofline: the "
                                        "applications are fused on chip, the HBM traffic actually moved is `stages.*."
                                        "hbm_bytes_per_launch`, so this figure may exceed the peak"}}
        out["config"]["float_mode"] = args.float_mode
        if literal is not None:
            out["literal_command"] = {
                "ms_per_step": round(literal * 1e3, 4), "Mcells/s": round(cells / literal / 1e6, 1),
                "note": "--warmup %d --steps %d taken literally: %d warm-up steps from an idle chip (0.5 s), then the %d timed "
                        "steps, no preheat.  `value` is the steady state: %d untimed steps (warmup_effective) precede its %d timed "
                        "ones, because the chip's clocks need some tens of ms of continuous work to settle" %
                        (args.warmup, args.steps, args.warmup, args.steps, preheat + args.warmup, args.steps)}
        if sharded:
            try:
                rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:  # noqa: BLE001
                rccl = None
            if grid is not None:
                n_ex, sent = grid.traffic()
                impl_note = {"impl": "native: nz_sharded_pipeline (one C-ABI call per step; ncclGroupStart / ncclSend / ncclRecv "
                                     "/ ncclGroupEnd with rank +- 1, " +
                                     {0: "on the compute stream between the launch that produced the rows and the launch "
                                         "that reads them",
                                      1: "on the library's communicator stream with event hand-offs; interior rows enqueued "
                                         "before the wait, border rows after",
                                      2: "on the library's communicator stream with event hand-offs; border rows first, the "
                                         "next launch's exchange travels while the interior rows run"}[args.overlap] + ")",
                             "exchanges_per_step": n_ex, "bytes_sent_per_step": sent,
                             "data_path_rccl": ("librccl %d opened by libnoize_hip.so" % sh.rccl_version()) if ncomm is not None else None}
            else:
                impl_note = {"impl": "python: noize_job_amd/sharded.py over torch.distributed batch_isend_irecv"}
            out["comm"] = {"backend": dist.get_backend(), "world": dist.get_world_size(), "rccl_version": rccl,
                           "halo": args.halo, "overlapped": (args.overlap != 0) if grid is not None else bool(getattr(comm, "overlap", False)),
                           "exchange_ms_per_step": None if exchange_ms is None else round(exchange_ms, 4),
                           "host_enqueue_ms_per_step": None if host_enqueue_ms is None else round(host_enqueue_ms, 4),
                           "host_enqueue_ms_idle_queue": None if host_idle_ms is None else round(host_idle_ms, 4),
                           "overlap_mode": args.overlap if grid is not None else None,
                           **impl_note,
                           "ranks_on_device": "one process per GPU (LOCAL_RANK -> device), %d device(s) visible to rank 0" % ndev,
                           "note": "exchange_ms_per_step = time the compute stream waits for ghost rows (HIP events around "
                                   "every wait, max over ranks); 0 ghost-row traffic with --halo recompute; "
                                   "host_enqueue_ms_per_step = host time inside the step's enqueue calls during the timed steps "
                                   "(max over ranks; includes the time the full command queue pushes back); "
                                   "host_enqueue_ms_idle_queue = the same call on an idle stream (--full; median of 8, rank 0): the "
                                   "host's own cost -- the step is host-bound if THIS approaches ms_per_step"}
            out["comm"]["ranks"] = rank_reports
            out["config"]["strong_scaling"] = (
                "the same %dx%d grid at every N; denominator = `grid_%d`.recompute of the N = 1 line of bench.py --full (the "
                "whole grid on one GPU)" % (plan.grows, plan.cols, plan.grows)) if strong else None
        else:
            out["config"]["strong_scaling"] = ("this N = 1 line is the 4096^2 metric tile; the N > 1 lines run the %d^2 grid "
                                               "split over the ranks, whose one-GPU figure is `grid_%d` (bench.py --full)" %
                                               (args.grid, args.grid)) if args.grid else None
        if cold_ms is not None:
            out["cold_ms"] = round(cold_ms, 4)
            out["config"]["cold_ms_note"] = "one step from an idle chip (0.5 s after the previous one), host-timed"
    def analyse(marks, mode, ms_step):
        """Per-stage launch times from the stage-boundary markers of `marks`, priced with the counter summary that belongs to
        these kernel sources in float mode `mode`: {"stages", "roofline", "counters_source", "step_valu"}."""
        res_ = {}
        flow_cap = nj._native.lib.nz_flow_fused_max_iterations()
        flow_launches = len(sh.split_iterations(F_IT, flow_cap))
        # the tile API ends a one-launch flow stage with a copy back into the caller's plane; stripes ping-pong
        pingpong = sharded or swap  # explicit src / dst: no copy back, no even-launch-count rule
        mctx = ctx
        ero_cap = nj._native.lib.nz_erosion_max_fused_iterations()
        n_gauss = len(sh.split_iterations(G_IT, nj._native.lib.nz_kernel_filter_max_fused(2)))
        if n_gauss & 1 and not pingpong:  # the tile API keeps the launch count even (result back in `src`)
            n_gauss += 1
        # the tile entries run these fused launches as ONE grid with tile-level dependencies (conv_chain_kernel) unless
        # NZ_CONV_CHAIN=0; the stripe entries launch them one by one
        gauss_chained = (not sharded and os.environ.get("NZ_CONV_CHAIN", "1") != "0" and 3 <= n_gauss <= 8)
        if gauss_chained:
            stage_note = {"gauss": "%d fused launches (%s applications) as one chained grid" %
                                   (n_gauss, "+".join(str(t) for t in sh.split_iterations(G_IT, nj._native.lib.nz_kernel_filter_max_fused(2))))}
            n_gauss = 1
        else:
            stage_note = {}
        launches = {"noise": 1, "gauss": n_gauss, "flow": flow_launches,
                    "erosion": len(sh.split_iterations(E_IT, ero_cap)) if pingpong else 2}
        rcells = cells // world  # rank 0's own cells: the stage figures are per GPU
        per_step = {n: [] for n in STAGES}
        for hs in marks:
            for i, n in enumerate(STAGES):
                per_step[n].append(mctx.elapsed_ms(hs[i], hs[i + 1]))
        stage_ms = {n: sum(per_step[n]) / len(marks) for n in STAGES}
        kernel_ms = dict(stage_ms)
        # `ms` is the mean over the marked steps (what the roofline is priced with); the spread says whether a mean is a
        # few slow steps or all of them
        stages_out = {n: {"ms": round(stage_ms[n], 4), "launches": launches[n],
                          "ms_min_median_max": [round(x, 4) for x in (min(per_step[n]), sorted(per_step[n])[len(marks) // 2],
                                                                     max(per_step[n]))],
                          "slowest_marked_step": max(range(len(marks)), key=lambda k, n=n: per_step[n][k])} for n in STAGES}
        for n, note in stage_note.items():
            stages_out[n]["note"] = note
        # The in-place tile API's one-launch flow stage ends with a plane copy back into the caller's buffer (and the
        # in-place erosion with none: two launches): time that copy on its own so the flow KERNEL's time is known (--full;
        # a plain run leaves the copy inside the flow stage's time and says so with copy_back_ms = None)
        if not pingpong and flow_launches == 1 and not args.full:
            stages_out["flow"]["copy_back_ms"] = None
        elif not pingpong and flow_launches == 1:
            scratch = ctx.alloc(rcells)
            hc0 = ctx.record()
            for _ in range(20):
                ctx.call("nz_flush_write_slice", scratch.ptr, tile.ptr, rcells)
            hc1 = ctx.record()
            hc1.Complete()
            copy_ms = ctx.elapsed_ms(hc0, hc1) / 20
            scratch.Dispose()
            stages_out["flow"]["copy_back_ms"] = round(copy_ms, 4)
            kernel_ms["flow"] = stage_ms["flow"] - copy_ms
        # Counter summary of these very kernels (same source hash, same flush mode), if one is committed: VALU
        # instructions and HBM bytes per launch.  Launch times are this run's; the counters are not re-measured here
        # (rocprofv3 --pmc cannot run inside the timed region) and `counters_source` says where they come from.
        cnt = None if sharded else load_counters(res, args.flush, mode)
        valu_floor_ms = 0.0
        for n in STAGES:
            s = stages_out[n]
            launch_ms = kernel_ms[n] / launches[n]
            s["avg_launch_ms"] = round(launch_ms, 4)
            gbs = BYTES[n] * rcells / (stage_ms[n] * 1e-3) / 1e9
            s["algorithmic_equivalent_GB/s"] = round(gbs, 1)
            hit = counters_for(cnt, n)
            if hit is None:
                s.update({"kernel": KERNEL_PREFIX[n][0], "valu_issue_frac": None, "hbm_traffic_frac": None, "bound": None,
                          "useful_valu_frac": None})
                continue
            name, e = hit
            insts = e["SQ_INSTS_VALU"] * cnt["scale"]
            hbm = e["hbm_bytes_per_launch"] * cnt["scale"]
            valu_frac = insts * VALU_CYCLES_PER_INST / (N_SIMD * CLK_HZ) / (launch_ms * 1e-3)
            hbm_frac = hbm / (launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
            valu_floor_ms += launches[n] * insts * VALU_CYCLES_PER_INST / (N_SIMD * CLK_HZ) * 1e3
            s["useful_valu_frac"] = round(ALGO_LANE_OPS_MODE[mode][n] * rcells / (launches[n] * insts * 64.0), 4)
            s.update({"kernel": name, "valu_insts_per_launch": round(insts), "hbm_bytes_per_launch": round(hbm),
                      "valu_issue_frac": round(valu_frac, 4), "hbm_traffic_frac": round(hbm_frac, 4),
                      "bound": "valu-fp32" if valu_frac >= hbm_frac else "hbm"})
        res_["stages"] = stages_out
        dom = max(STAGES, key=lambda n: kernel_ms[n])
        s = stages_out[dom]
        if s.get("bound") == "hbm":
            ach = s["hbm_bytes_per_launch"] / (s["avg_launch_ms"] * 1e-3) / 1e9
            res_["roofline"] = {"kernel": s["kernel"], "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                               "traffic": s["hbm_bytes_per_launch"]}
        elif s.get("bound") == "valu-fp32":
            ach = s["valu_insts_per_launch"] * 64 / (s["avg_launch_ms"] * 1e-3) / 1e12
            # `achieved` counts EXECUTED instructions; `algorithmic` the lane-operations of SURVEY.md 8(d) only
            # (ALGO_LANE_OPS x the cells one launch produces), over the same launch time and the same peak
            alg = ALGO_LANE_OPS_MODE[mode][dom] * rcells / launches[dom] / (s["avg_launch_ms"] * 1e-3) / 1e12
            res_["roofline"] = {"kernel": s["kernel"], "bound": "valu-fp32", "achieved": round(ach, 2),
                               "peak": round(VALU_PEAK_TOPS, 2), "unit": "Tlane-op/s",
                               "frac": round(ach / VALU_PEAK_TOPS, 4), "traffic": s["hbm_bytes_per_launch"],
                               "hbm_traffic_frac": s["hbm_traffic_frac"],
                               "algorithmic": {"achieved": round(alg, 2), "frac": round(alg / VALU_PEAK_TOPS, 4),
                                               "lane_ops_per_cell": ALGO_LANE_OPS_MODE[mode][dom]}}
        else:  # no counter summary of these kernels: the only figure this run can form itself
            ach = BYTES[dom] * rcells / launches[dom] / (s["avg_launch_ms"] * 1e-3) / 1e9
            res_["roofline"] = {"kernel": s["kernel"], "bound": "unknown", "achieved": None, "peak": HBM_PEAK_GBS,
                               "unit": "GB/s", "frac": None, "traffic": None,
                               "algorithmic_equivalent_GB/s": round(ach, 1)}
        res_["roofline"].update({
            "stage": dom, "share_of_step": round(kernel_ms[dom] / sum(stage_ms.values()), 4),
            "launches_per_step": launches[dom], "avg_launch_ms": s["avg_launch_ms"],
            "note": "the kernel with the largest share of the step, under the larger of its two fractions: VALU issue "
                    "(SQ_INSTS_VALU x 2 cycles / (1024 SIMDs x 2.4 GHz x launch time)) and HBM traffic (FETCH_SIZE x2 + "
                    "WRITE_SIZE bytes / launch time / 8 TB/s); launch time from this run's HIP events, counters from "
                    "`counters_source`"})
        if cnt is not None:
            res_["counters_source"] = {"file": cnt["file"], "commit": cnt["commit"],
                                      "kernel_sources_sha": kernel_sources_sha(),
                                      "scaled_from_res": cnt["res"] if cnt["scale"] != 1.0 else None,
                                      "collected": "rocprofv3 --kernel-trace --pmc, one pass per counter group "
                                                   "(tools/collect_profiles.sh), folded by tools/fold_counters.py"}
            res_["step_valu"] = {"floor_ms": round(valu_floor_ms, 4), "frac": round(valu_floor_ms / ms_step, 4),
                                "note": "sum over the step's launches of SQ_INSTS_VALU x 2 cycles / (1024 SIMDs x 2.4 GHz)"
                                        ": the time the step's VALU instructions need at full issue rate, over "
                                        "ms_per_step"}
        else:
            res_["counters_source"] = None
        return res_

    if rank == 0 and marks:
        out.update(analyse(marks, args.float_mode, ms_per_step))
    if rank == 0 and checks and not sharded:
        cres = args.cpu_res or res
        out["cpu_baseline"], plane = cpu_baseline(cres)
        if cres == res:
            # the device plane the last timed step left behind against the oracle's (outside the timed region)
            got = np.empty(cells, np.float32)
            src = gd.data
            nj._native.check(nj._native.lib.nz_tile_download(ctx._h, src.ptr, got.ctypes.data, cells, 0, None), "download")
            fence()
            if os.environ.get("NZ_BENCH_FLIP_CELL"):   # debug hook (tests/test_gpu_bench.py): a wrong run must fail
                got[cells // 2] += np.float32(1.0)
                out["debug_flipped_cell"] = cells // 2
            same = bool(np.array_equal(got.reshape(res, res), plane))
            out["verified"] = same
            if not same:
                bad = ~(np.abs(got.reshape(res, res) - plane) <= 1e-5 * np.abs(plane) + 1e-6)
                out.setdefault("verified_detail", {}).update({
                    "cells_outside_1e-5_rel": int(bad.sum()),
                    "max_abs_diff": float(np.abs(got.reshape(res, res) - plane).max())})
        else:
            out["verified"] = None
    plane_oracle = plane if (rank == 0 and checks and not sharded and (args.cpu_res or res) == res) else None
    if sharded and grid is not None and checks:
        # every rank: the rows it owns after the last timed pass against the CPU oracle's rows of the monolithic grid
        if args.as_rank is not None and args.halo != "recompute":
            ver = {"verified": None, "note": "rehearsal with exchanged ghost rows: the neighbour ranks are played by the rank "
                                             "itself, so the rows that arrive are not the grid's -- timing only (--halo recompute "
                                             "rehearsals are verified)"}
        else:
            ver = verify_sharded(np, torch, dist, grid, p, plan.grows, plan.cols, world, {}, args.float_mode == "strict")
        if rank == 0:
            out["verified"] = ver.pop("verified")
            out["verified_detail"] = ver
    if rank == 0 and not sharded and extras:
        # the other float modes beside the headline: the same step on the same planes, 100 timed steps after 30 untimed ones,
        # then 40 marked steps for the stage times; the plane each mode leaves is compared with the oracle's
        modes_out = {}
        want_stages = stage_planes(res) if plane_oracle is not None else None
        for mode in FLOAT_MODES:
            gc.collect()
            ctx.float_mode = FLOAT_MODES[mode]
            for _ in range(30):
                step(False)
            fence()
            t1 = time.perf_counter()
            for _ in range(100):
                step(False)
            fence()
            dtm = (time.perf_counter() - t1) / 100
            del marks[:]
            prev_end[0] = None
            for _ in range(40):
                step(True)
            fence()
            e = {"ms_per_step": round(dtm * 1e3, 4), "Mcells/s": round(cells / dtm / 1e6, 1)}
            a = analyse(list(marks), mode, dtm * 1e3)
            e["stages_ms"] = {n: a["stages"][n]["ms"] for n in STAGES}
            e["valu_issue_frac"] = {n: a["stages"][n].get("valu_issue_frac") for n in STAGES}
            e["roofline"] = {k: a["roofline"].get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac")}
            e["counters_source"] = a["counters_source"]["file"] if a.get("counters_source") else None
            if plane_oracle is not None:
                got = np.empty(cells, np.float32)
                nj._native.check(nj._native.lib.nz_tile_download(ctx._h, gd.data.ptr, got.ctypes.data, cells, 0, None), "download")
                fence()
                got = got.reshape(res, res)
                d = np.abs(got - plane_oracle)
                e["end_to_end_vs_oracle"] = {"bit_equal": bool(np.array_equal(got, plane_oracle)), "max_abs": float(d.max()),
                                             "cells_within_1e-5_rel_1e-6_abs": round(float(np.mean(d <= 1e-5 * np.abs(plane_oracle) + 1e-6)), 6)}
                # the per-stage contract, each stage fed the oracle's input plane (strict: bit-equal, so inside by definition)
                e["stages_within_1e-5"], e["stages_vs_oracle"] = stages_within_tolerance(np, nj, ctx, p, res, want_stages)
            modes_out[mode] = e
        del marks[:]
        ctx.float_mode = FLOAT_MODES[args.float_mode]
        modes_out["note"] = (
            "nz_ctx_set_float_mode.  strict = the reference's operation sequence, bit-equal to the oracle (the headline unless "
            "--float-mode says otherwise).  fast = the fBm octave's polynomial tail and the tap sums FMA-contracted: EVERY STAGE within "
            "1e-5 rel / 1e-6 abs of strict for the same input plane (tests/test_gpu_fast.py, 4096^2: fBm 9e-7, Gauss5 x17 4.5e-7, "
            "flow and erosion run their strict forms).  relaxed = fast + v_rcp_f32 / FMA / v_sqrt_f32 in the flow iterations: the "
            "flow stage leaves the band in ~1e-4 of its cells.  END TO END no tolerance mode stays inside 1e-5: the flow map "
            "differentiates the filtered heights (neighbours 1e-3 apart, each known to 6e-8), so one ulp in its input plane moves "
            "its output by ~1e-4 relative -- as between any two FloatMode.Fast builds of the reference")
        out["float_modes"] = modes_out
    if rank == 0 and extras and not sharded:
        # informational, outside the timed steps; never allowed to cost the JSON line: an exception is recorded, and
        # should one of them ever block, a watchdog prints the line without them and ends the process
        printed = []

        def bail():
            with out_lock:
                if printed:
                    return
                printed.append(1)
                line = dict(out)
                line["extras"] = "skipped: an informational measurement did not return within 240 s"
                os.write(real_stdout, (json.dumps(line) + "\n").encode())
                os._exit(3)   # the line is out, but a measurement hung: never a clean exit
        watchdog = threading.Timer(240.0, bail)
        watchdog.daemon = True
        watchdog.start()
        for key, fn in (("in_place_entries", lambda: in_place_entries(nj, ctx, res, p) if swap else None),
                        ("two_tiles_in_flight", lambda: two_tiles(nj, ctx, stages, gd, res, p, swap))):
            try:
                gc.collect()
                r = fn()
            except Exception as e:  # noqa: BLE001
                r = {"error": "%s: %s" % (type(e).__name__, e)}
            with out_lock:
                if r is not None:
                    out[key] = r
        watchdog.cancel()
    # BASELINE config 5's grid at this N (every rank takes part)
    if extras and args.grid > 0 and args.as_rank is None and args.grid % world == 0:
        if not sharded:  # N = 1 without a process group: the whole grid as one stripe
            g = None
            try:
                g = strong_grid(nj, sh, torch, None, ctx, args.grid, 0, 1, impl=args.impl, verify=checks,
                                strict=args.float_mode == "strict")
            except Exception as e:  # noqa: BLE001  (e.g. not enough free memory next to other processes)
                g = {"error": "%s: %s" % (type(e).__name__, e)}
            out["grid_%d" % args.grid] = g
        else:
            if args.impl == "native" and ncomm is None and world > 1:
                ncomm = make_native_comm(sh, torch, dist, ctx, rank, world)
            g = strong_grid(nj, sh, torch, dist, ctx, args.grid, rank, world, impl=args.impl, ncomm=ncomm,
                            verify=checks, strict=args.float_mode == "strict")
            if rank == 0:
                out["grid_%d" % args.grid] = g
    if sharded:
        if grid is not None:
            grid.close()
        if ncomm is not None:
            ncomm.close()
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    os.close(real_stdout)
    if out is not None:
        with out_lock:
            print(json.dumps(out), flush=True)
        failed = failed_checks(out)
        if failed:
            print("bench.py: the line is printed, but these checks against the oracle FAILED: %s" % ", ".join(failed),
                  file=sys.stderr, flush=True)
            sys.exit(4)


def failed_checks(out):
    """Every verdict the line carries that says a computed plane is not the oracle's: `verified` (headline and grid, any
    schedule), strict end to end not bit-equal, strict / fast per-stage contract broken.  (relaxed is reported only: its
    flow stage is documented to leave the band.)"""
    bad = []

    def walk(d, path):
        for k, v in d.items():
            if k == "verified" and v is False:
                bad.append("/".join(path + [k]))
            elif isinstance(v, dict):
                walk(v, path + [k])
    walk(out, [])
    fm = out.get("float_modes") or {}
    for mode in ("strict", "fast"):
        e = fm.get(mode) or {}
        if e.get("stages_within_1e-5") is False:
            bad.append("float_modes/%s/stages_within_1e-5" % mode)
    if (fm.get("strict") or {}).get("end_to_end_vs_oracle", {}).get("bit_equal") is False and out.get("debug_flipped_cell") is None:
        bad.append("float_modes/strict/end_to_end_vs_oracle/bit_equal")
    return bad


if __name__ == "__main__":
    main()
