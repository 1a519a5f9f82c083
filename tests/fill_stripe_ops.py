"""The `fill` and `fill_finalise` stripe operations of noize_job_amd.sharded on the numpy reference (test infrastructure, in
the pattern of tests/fluvial_stripe_ops.py): one round is at most maxPasses Jacobi passes of fill_ref.step on the owned
rows and `ghost` rows of W on each side, cut at the global border; the ghost rows are frozen -- put back after every pass --
and the outlets are those of the global grid, so a cut is no border.  Buffers are torch CPU tensors (float32 planes, int32
words)."""
import numpy as np

import fill_ref as L

f32 = np.float32


class FillStripeOps:
    def __init__(self, ghost=1):
        self.ghost = ghost

    def fill(self, h, w, work, plan, prm, first, proceed, changed):
        if proceed is not None and int(proceed[0]) == 0:
            changed[0] = 0
            return
        v0 = max(0, -plan.grow0, plan.own0 - self.ghost)
        v1 = min(plan.rows, plan.grows - plan.grow0, plan.own1 + self.ghost)
        own = slice(plan.own0 - v0, plan.own1 - v0)
        cols = slice(0, plan.cols)
        H = h.numpy()[v0:v1, cols].copy()
        out = H <= f32(prm["seaLevel"])  # the outlets of the global grid
        out[:, 0] = out[:, -1] = True
        g = np.arange(v0, v1) + plan.grow0
        out[(g == 0) | (g == plan.grows - 1), :] = True
        frozen = np.ones(H.shape, bool)
        frozen[own] = False
        W = np.where(out, H, L.INF).astype(f32) if first else w.numpy()[v0:v1, cols].copy()
        entry = W[own].copy()
        eps = f32(prm["epsilon"])
        for _ in range(prm["maxPasses"]):
            nxt = L.step(W, H, out, eps)
            nxt[frozen] = W[frozen]
            if L.same(nxt, W):
                break
            W = nxt
        w.numpy()[plan.own0:plan.own1, cols] = W[own]
        changed[0] = 1 if first or not L.same(W[own], entry) else 0

    def fill_finalise(self, h, w, depth, plan, converged):
        rows, cols = slice(plan.own0, plan.own1), slice(0, plan.cols)
        if int(converged[0]) != 0:
            hv, wv = h.numpy()[rows, cols].copy(), w.numpy()[rows, cols]
            h.numpy()[rows, cols] = wv
            if depth is not None:
                depth.numpy()[rows, cols] = wv - hv
        elif depth is not None:
            depth.numpy()[rows, cols] = f32(0.0)
