"""The `drainage` and `drainage_finalise` stripe operations of noize_job_amd.sharded on the numpy reference (test
infrastructure, in the pattern of tests/fill_stripe_ops.py).  A round with `first` takes fluvial_ref.receivers on the rows
held within 2 of the owned ones -- the outlets are those of the global grid, so a cut is no border -- and keeps them for
the later rounds, as nz_drainage_stripe_round keeps its donor bytes in `work`; one round is at most maxPasses Jacobi passes of
fluvial_ref.drainage on the owned rows and one ghost row of A on each side, cut at the global border; the ghost rows are
frozen: put back after every pass.  `changed` is 1 with `first`, 1 when any pass of the round changed a value, 0 when the
round's first pass found the stripe at rest.  Buffers are torch CPU tensors (float32 planes, int32 words)."""
import numpy as np

import fluvial_ref as F

f32 = np.float32


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


class DrainageStripeOps:
    def __init__(self):
        self.receivers = {}  # per work buffer: the receiver codes of the rows _held(plan, 1)
        self.steps = []      # Jacobi steps of every round that ran, for the tests that look at budgets

    @staticmethod
    def _held(plan, ghost):
        """The buffer rows within `ghost` of the owned ones, cut at the global border."""
        return max(0, -plan.grow0, plan.own0 - ghost), min(plan.rows, plan.grows - plan.grow0, plan.own1 + ghost)

    @staticmethod
    def _rain(plan, prm, rainMap, v0, v1):
        rm = None if rainMap is None else rainMap.numpy()[v0:v1, :plan.cols]
        return F.rain_plane((v1 - v0, plan.cols), prm["rain"], rm)

    def drainage(self, h, a, work, plan, prm, first, proceed, changed, rainMap=None):
        if proceed is not None and int(proceed[0]) == 0:
            changed[0] = 0
            return
        cols = slice(0, plan.cols)
        v0, v1 = self._held(plan, 1)
        if first:
            u0, u1 = self._held(plan, 2)
            H = h.numpy()[u0:u1, cols].copy()
            # the first and last row held are outlets to F.receivers: at radius 2 nobody asks for their receiver, and a
            # row at radius 1 or 0 is the first or last one held only when it is the global border
            self.receivers[work.data_ptr()] = F.receivers(H, prm["seaLevel"])[0][v0 - u0:v1 - u0].copy()
        r = self.receivers[work.data_ptr()]
        rc = self._rain(plan, prm, rainMap, v0, v1)
        own = slice(plan.own0 - v0, plan.own1 - v0)
        frozen = np.ones(rc.shape, bool)
        frozen[own] = False
        A = rc.copy() if first else a.numpy()[v0:v1, cols].copy()
        steps = 0
        for _ in range(prm["maxPasses"]):
            nxt = F.drainage(A, r, rc)
            nxt[frozen] = A[frozen]
            if same(nxt, A):
                break
            A, steps = nxt, steps + 1
        self.steps.append(steps)
        a.numpy()[plan.own0:plan.own1, cols] = A[own]
        changed[0] = 1 if first or steps > 0 else 0

    def drainage_finalise(self, a, plan, prm, converged, rainMap=None):
        if int(converged[0]) == 0:
            a.numpy()[plan.own0:plan.own1, :plan.cols] = self._rain(plan, prm, rainMap, plan.own0, plan.own1)
