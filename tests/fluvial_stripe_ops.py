"""The `fluvial` stripe operation of noize_job_amd.sharded on the numpy reference (test infrastructure, in the pattern of
tests/hydraulic_stripe_ops.py): n iterations of fluvial_ref.run on the rows of the stripe's buffer that the call may read --
the owned rows and `ghost` rows per iteration on each side, cut at the global border -- of which the owned rows are kept.
run() makes the edge of the plane it is handed a border of outlets, so a cut that is not the global border is wrong there,
and the error travels 2 rows per iteration: a receiver looks at the heights 1 row away and the drainage is gathered along
the receivers 1 row away.  With ghost = 2 it stops short of the owned rows, with ghost = 1 (the negative control) it reaches
them.  Buffers are torch CPU float32 tensors."""
import fluvial_ref as F
from noize_job_amd.sharded import FLUVIAL_SCALARS


class FluvialStripeOps:
    def __init__(self, ghost=2):
        self.ghost = ghost

    def fluvial(self, h_in, h_out, d_in, d_out, work, plan, prm, n, rainMap=None, hardness=None, upliftMap=None):
        # the rows the call reads: inside the buffer and inside the global grid
        v0 = max(0, -plan.grow0, plan.own0 - self.ghost * n)
        v1 = min(plan.rows, plan.grows - plan.grow0, plan.own1 + self.ghost * n)
        own = slice(plan.own0 - v0, plan.own1 - v0)
        rows = slice(plan.own0, plan.own1)
        cols = slice(0, plan.cols)
        cut = lambda t: None if t is None else t.numpy()[v0:v1, cols].copy()  # noqa: E731
        h, a = F.run(cut(h_in), n, rainMap=cut(rainMap), hardness=cut(hardness), upliftMap=cut(upliftMap),
                     drainageIn=cut(d_in), **{k: prm[k] for k in FLUVIAL_SCALARS})
        h_out.numpy()[rows, cols] = h[own]
        d_out.numpy()[rows, cols] = a[own]
