"""The `hydraulic` stripe operation of noize_job_amd.sharded on the CPU reference driver (test infrastructure, in the
pattern of tests/oracle_stripe_ops.py): n iterations of hydraulic_ex_ref.step on the rows of the stripe's buffer that the
call may read -- the owned rows and `ghost` rows per iteration on each side, cut at the global border -- of which the owned
rows are kept.  step() clamps (and opens the border) at the edge of the plane it is handed, so a cut that is not the global
border is wrong there, and the error travels 3 rows per iteration: with ghost = 3 it stops short of the owned rows, with
ghost = 2 (the negative control) it reaches them.  Buffers are torch CPU float32 tensors."""
import numpy as np

import hydraulic_ex_ref as X
from noize_job_amd.sharded import HYDRAULIC_SCALARS

f32 = np.float32
STEP_NAMES = HYDRAULIC_SCALARS[1:]  # step() takes no initialWater


class HydraulicStripeOps:
    def __init__(self, ghost=3):
        self.ghost = ghost

    def hydraulic(self, h_in, h_out, S_in, S_out, work, plan, prm, n, first, last, rainMap=None, hardness=None, wear=None,
                  deposits=None):
        # the rows the call reads: inside the buffer and inside the global grid
        v0 = max(0, -plan.grow0, plan.own0 - self.ghost * n)
        v1 = min(plan.rows, plan.grows - plan.grow0, plan.own1 + self.ghost * n)
        own = slice(plan.own0 - v0, plan.own1 - v0)
        rows = slice(plan.own0, plan.own1)
        cut = lambda t: None if t is None else t.numpy()[v0:v1].copy()  # noqa: E731
        b = cut(h_in)
        if first:
            d = np.full(b.shape, f32(prm["initialWater"]), f32)
            s = np.zeros(b.shape, f32)
            flux = tuple(np.zeros(b.shape, f32) for _ in range(4))
        else:
            d, s = cut(S_in[0]), cut(S_in[1])
            flux = tuple(cut(S_in[i]) for i in range(2, 6))
        # the masks live on the owned rows only; the rows around them are scratch of this call
        w, dep = np.zeros(b.shape, f32), np.zeros(b.shape, f32)
        if not first:
            if wear is not None:
                w[own] = wear.numpy()[rows]
            if deposits is not None:
                dep[own] = deposits.numpy()[rows]
        scalars = [prm[k] for k in STEP_NAMES]
        for _ in range(n):
            b, d, s, flux, w, dep = X.step(b, d, s, flux, w, dep, *scalars, border=prm["border"], rainMap=cut(rainMap),
                                           hardness=cut(hardness))
        if last:
            h_out.numpy()[rows] = (b + s).astype(f32)[own]
            S_out[0].numpy()[rows] = d[own]
            dep = (dep + s).astype(f32)
        else:
            h_out.numpy()[rows] = b[own]
            for i, a in enumerate((d, s) + tuple(flux)):
                S_out[i].numpy()[rows] = a[own]
        if wear is not None:
            wear.numpy()[rows] = w[own]
        if deposits is not None:
            deposits.numpy()[rows] = dep[own]
