"""The case lists of tests/test_gpu_sweep_terrain.py, on the CPU: the seeded sweep of the four older families is pinned --
describe(c), the generator's name and the bytes of the case heights of sweep_cases(seed), seeds 0 to 7, hashed when the
drainage family joined the sweep, so that a later family cannot move a draw of that stream -- and the drainage sweep draws
from a stream of its own, covers both forms, the rain map of either sign and the sea, and stays finite in the model."""
import hashlib

import numpy as np
import pytest

import test_gpu_sweep_terrain as S

SWEEP_DIGESTS = {0: "1cae3b852e1f9b05", 1: "2979c0a0c1167aff", 2: "c1578698fbc95578", 3: "e42a2b334f888cad",
                 4: "1b21e4b882dad922", 5: "26002a34ab9cc3ec", 6: "26ccd8815b5b78d6", 7: "43fd507dbaf585a1"}


def digest(cases):
    m = hashlib.sha256()
    for c in cases:
        m.update(S.describe(c).encode())
        m.update(c["name"].encode())
        m.update(np.ascontiguousarray(c["hh"]).tobytes())
        for name in sorted(c.get("maps", {})):
            m.update(np.ascontiguousarray(c["maps"][name]).tobytes())
    return m.hexdigest()[:16]


@pytest.mark.parametrize("seed", range(8))
def test_the_seeded_sweep_of_the_older_families_is_pinned(seed):
    cases = S.sweep_cases(seed)
    print("%d: %r" % (seed, digest(cases)))
    assert len(cases) == 5 and all(c["family"] in S.FAMILIES[:4] for c in cases)
    assert digest(cases) == SWEEP_DIGESTS[seed], [S.describe(c) for c in cases]


def test_the_drainage_sweep_is_finite_inside_its_budget_and_covers_its_options():
    """check() of the GPU sweep refuses a model that is not finite; "cells of the longest flow path" + 1 passes is what it
    allows the kernel, so the budget of every case has to hold that."""
    cases = [c for seed in range(8) for c in S.drainage_sweep_cases(seed)]
    assert len(cases) == 40 and all(c["family"] == "drainage" and c["hh"].shape[-1] in S.SWEEP_SIZES for c in cases)
    for c in cases:
        A, height = S.model(c)
        assert np.isfinite(A).all() and int(height.max()) + 1 <= c["budget"], S.describe(c)
    seen = {(c["form"], bool(c["on"]), c["signed"], c["sea"] == S.OFF) for c in cases}
    assert seen == {(f, m, s, o) for f in ("inplace", "batch") for m in (False, True) for s in (False, True) for o in (False, True)
                    if m or not s}
    assert {c["rain"] for c in cases} == {0.0, 0.3, 0.75, 1.0, 2.5}
    # batches of even and of odd sizes: at an odd size tile k starts 4 * k bytes off the vector alignment
    assert {c["hh"].shape[-1] % 2 for c in cases if c["form"] == "batch" and len(c["hh"]) >= 3} == {0, 1}
    assert len({S.describe(c) + c["name"] for c in cases}) == 40
