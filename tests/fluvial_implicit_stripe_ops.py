"""The `fluvial_implicit` and `fluvial_implicit_finalise` stripe operations of noize_job_amd.sharded on the numpy reference
(test infrastructure, in the pattern of tests/drainage_stripe_ops.py, whose drainage operations it inherits: the chain runs
the drainage area first).  A round with `first` takes fluvial_implicit_ref.coefficients on the rows held within 1 of the
owned ones -- the outlets are those of the global grid, so a cut is no border -- and keeps them for the later rounds, as
nz_implicit_fluvial_stripe_round keeps its receiver bytes and coefficients in `work`; one round is at most maxPasses Jacobi
steps (fluvial_implicit_ref.step) on the owned rows against one ghost row of h' on each side, which is frozen: the heights
as they stand in a round with `first`, the exchanged `out` afterwards.  `changed` is 1 with `first`, 1 when any step of the
round changed a bit, 0 when the round's first step found the stripe at rest.  Buffers are torch CPU tensors."""
import numpy as np

import fluvial_implicit_ref as R
from drainage_stripe_ops import DrainageStripeOps, same

f32 = np.float32


class FluvialImplicitStripeOps(DrainageStripeOps):
    def __init__(self):
        super().__init__()
        self.coefficients = {}  # per work buffer: (has, q, b, f) of the rows _held(plan, 1)
        self.solve_steps = []   # Jacobi steps of every round of a solve that ran

    def fluvial_implicit(self, h, a, out, work, plan, prm, first, proceed, changed, hardness=None, upliftMap=None):
        if proceed is not None and int(proceed[0]) == 0:
            changed[0] = 0
            return
        cols = slice(0, plan.cols)
        v0, v1 = self._held(plan, 1)
        own = slice(plan.own0 - v0, plan.own1 - v0)
        if first:
            H = h.numpy()[v0:v1, cols].copy()
            part = lambda t: None if t is None else t.numpy()[v0:v1, cols]  # noqa: E731
            # the first and last row held are outlets to the reference: nobody asks for a ghost row's receiver, and an
            # owned row is the first or last one held only when it is the global border.  A and the maps are looked at
            # where a cell has a receiver: on owned rows only
            has, q, b, f = R.coefficients(H, a.numpy()[v0:v1, cols], erodibility=prm["erodibility"], uplift=prm["uplift"],
                                          dt=prm["dt"], seaLevel=prm["seaLevel"], hardness=part(hardness),
                                          upliftMap=part(upliftMap))
            frozen = np.ones(H.shape, bool)
            frozen[own] = False
            assert not has[frozen].any()
            b = np.where(frozen, H, b)  # the frozen rows: the heights as they stand
            self.coefficients[work.data_ptr()] = (has, q, b, f)
        has, q, b, f = self.coefficients[work.data_ptr()]
        hn = b.copy() if first else out.numpy()[v0:v1, cols].copy()
        steps = 0
        for _ in range(prm["maxPasses"]):
            nxt = R.step(hn, has, q, b, f)  # a cell without a receiver, every frozen one among them, keeps its value
            if same(nxt, hn):
                break
            hn, steps = nxt, steps + 1
        self.solve_steps.append(steps)
        out.numpy()[plan.own0:plan.own1, cols] = hn[own]
        changed[0] = 1 if first or steps > 0 else 0

    def fluvial_implicit_finalise(self, h, out, plan, converged):
        if int(converged[0]) == 0:
            out.numpy()[plan.own0:plan.own1, :plan.cols] = h.numpy()[plan.own0:plan.own1, :plan.cols]
