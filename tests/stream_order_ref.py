"""The stream-order model of nz_stream_order (include/noize_hip.h) in plain numpy: Strahler order and river links over the
receiver tree of fluvial_ref.receivers, gathered downstream.  Planes are rows x cols arrays indexed [z, x], c = z * cols + x.

    ch(c)    = drainage is None ? True : drainage[c] >= threshold      (one float32 comparison: a NaN is no channel)
    D(c)     = the existing neighbours k of c with r(k) == c and ch(k)
    order[c] = 0 without ch(c);  1 when D(c) is empty;  otherwise m + (n >= 2), m = max order[D(c)], n = #{d: order[d] == m}
    link[c]  = -1 without ch(c);  c when |D(c)| != 1;  otherwise link[d] of the one donor

A receiver is strictly lower than its donor, so the graph is a forest, a cell's value is a fixed function of its donors'
final values and every schedule of updates ends in the same bytes:

    walk(h, seaLevel, drainage, threshold) -> (order, link, chain)  the model as a walk, cells highest first (stable sort): a
                                                            cell's donors have their final values already; chain = cells
                                                            of the longest chain of channel donors (0: no channel cell)
    jacobi(h, ...) -> (order, link, steps)                  every cell from its donors' values of the step before, from the
                                                            start state ch ? 1 : 0 and ch ? c : -1, until a step changes nothing
    tiled(h, ..., tile, sweeps) -> (order, link, passes)    Jacobi inside the kernel's tiles: 64 x 16 tiles against frozen rings, at
                                                            most `sweeps` sweeps per tile and pass"""
import numpy as np

from fluvial_ref import NEIGHBOURS, OPPOSITE, SEA_OFF, _window, receivers

f32 = np.float32


def channel(shape, drainage=None, threshold=0.0):
    """ch, the channel predicate, as a plane of bools."""
    if drainage is None:
        return np.ones(shape, bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(drainage, f32).reshape(shape) >= f32(threshold)


def donor_bits(h, seaLevel=SEA_OFF, drainage=None, threshold=0.0):
    """(ch, bits): bit k of bits[c] is set when neighbour k of c exists, drains into c and is a channel cell."""
    h = np.ascontiguousarray(h, f32)
    r = receivers(h, seaLevel)[0]
    ch = channel(h.shape, drainage, threshold)
    bits = np.zeros(h.shape, np.uint8)
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        c, n = _window(h.shape, dx, dz)
        bits[c] |= (((r[n] == OPPOSITE[k]) & ch[n]).astype(np.uint8) << k).astype(np.uint8)
    return ch, bits


def start(ch):
    """The start state, and the "nothing" of all or nothing."""
    own = np.arange(ch.size, dtype=np.int32).reshape(ch.shape)
    return ch.astype(np.uint8), np.where(ch, own, np.int32(-1)).astype(np.int32)


def step(order, link, ch, bits):
    """One Jacobi step: every cell from its donors' values."""
    own = np.arange(ch.size, dtype=np.int32).reshape(ch.shape)
    m = np.zeros(ch.shape, np.int64)
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        c, n = _window(ch.shape, dx, dz)
        m[c] = np.maximum(m[c], np.where((bits[c] >> k) & 1, order[n], 0))
    cnt = np.zeros(ch.shape, np.int64)
    one = np.full(ch.shape, -1, np.int32)  # the link of the donor with the highest k: THE donor where there is one
    for k, (dx, dz) in enumerate(NEIGHBOURS):
        c, n = _window(ch.shape, dx, dz)
        is_d = ((bits[c] >> k) & 1).astype(bool)
        cnt[c] += is_d & (order[n] == m[c])
        one[c] = np.where(is_d, link[n], one[c])
    donors = np.unpackbits(bits.reshape(-1, 1), axis=1).sum(axis=1).reshape(ch.shape)
    no = np.where(donors == 0, 1, m + (cnt >= 2))
    nl = np.where(donors == 1, one, own)
    return np.where(ch, no, 0).astype(np.uint8), np.where(ch, nl, np.int32(-1)).astype(np.int32)


def walk(h, seaLevel=SEA_OFF, drainage=None, threshold=0.0):
    h = np.ascontiguousarray(h, f32)
    rows, cols = h.shape
    ch, bits = donor_bits(h, seaLevel, drainage, threshold)
    chl, bl = ch.reshape(-1).tolist(), bits.reshape(-1).tolist()
    off = [dz * cols + dx for dx, dz in NEIGHBOURS]
    order, link, height = [0] * h.size, [-1] * h.size, [0] * h.size
    for c in np.argsort(-h.reshape(-1).astype(np.float64), kind="stable").tolist():
        if not chl[c]:
            continue
        ds = [c + off[k] for k in range(8) if bl[c] >> k & 1]  # strictly higher: they have their final values already
        if not ds:
            order[c], link[c], height[c] = 1, c, 1
            continue
        m = max(order[d] for d in ds)
        n = sum(1 for d in ds if order[d] == m)
        order[c] = m + (1 if n >= 2 else 0)
        link[c] = link[ds[0]] if len(ds) == 1 else c
        height[c] = 1 + max(height[d] for d in ds)
    return (np.array(order, np.uint8).reshape(h.shape), np.array(link, np.int32).reshape(h.shape), max(height))


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b)


def jacobi(h, seaLevel=SEA_OFF, drainage=None, threshold=0.0):
    ch, bits = donor_bits(h, seaLevel, drainage, threshold)
    order, link = start(ch)
    steps = 0
    while True:
        no, nl = step(order, link, ch, bits)
        if same(no, order) and same(nl, link):
            return order, link, steps
        order, link, steps = no, nl, steps + 1


def tiled(h, seaLevel=SEA_OFF, drainage=None, threshold=0.0, tile=(64, 16), sweeps=None):
    ch, bits = donor_bits(h, seaLevel, drainage, threshold)
    order, link = start(ch)
    rows, cols = order.shape
    tx, tz = tile
    passes = 0
    while True:
        no_plane, nl_plane = order.copy(), link.copy()
        for z0 in range(0, rows, tz):
            for x0 in range(0, cols, tx):
                own = (slice(z0, min(z0 + tz, rows)), slice(x0, min(x0 + tx, cols)))
                # the state of the pass before everywhere, of which only the own cells are updated: the ring is frozen
                o, l = order.copy(), link.copy()
                s = 0
                while sweeps is None or s < sweeps:
                    no, nl = step(o, l, ch, bits)
                    if same(no[own], o[own]) and same(nl[own], l[own]):
                        break
                    o[own], l[own] = no[own], nl[own]
                    s += 1
                no_plane[own], nl_plane[own] = o[own], l[own]
        if same(no_plane, order) and same(nl_plane, link):
            return order, link, passes
        order, link, passes = no_plane, nl_plane, passes + 1


def channel_of(h, heads=((1, 1),)):
    """The channel plane of drainage_ref.serpentine and of two_heads as a `drainage` for threshold 0.5: 1 on the flow
    paths from the heads (z, x) to the outlet, 0 elsewhere -- on the walls, which drain into the channel like any slope
    and are no river, and on the two cells the steepest descent cuts off at every turn."""
    h = np.asarray(h, f32)
    r = receivers(h)[0]
    ch = np.zeros(h.shape, f32)
    for z, x in heads:
        while True:
            ch[z, x] = 1
            if r[z, x] >= len(NEIGHBOURS):
                break
            dx, dz = NEIGHBOURS[r[z, x]]
            z, x = z + dz, x + dx
    return ch


def two_heads(res=160):
    """drainage_ref.serpentine with a second head that joins the first at the top: the wall cell beside the first
    connector, (z, x) = (2, res - 3), comes down to 10 above the connector.  That is above everything around it, so nothing
    new drains into it, and its steepest descent is the cardinal one to (3, res - 3) -- 10.5 against 10.75 * DIAG to
    (3, res - 4) -- which is where the connector drains as well, across the corner.  Row 1 and the connector stay one
    reach of order 1, the new head is a reach of its own, and from (3, res - 3) on the channel has order 2: it has to
    travel the whole rest of the chain.  channel_of(h, ((1, 1), (2, res - 3))) is its channel plane."""
    from drainage_ref import serpentine
    h = serpentine(res)
    h[2, res - 3] = h[2, res - 2] + f32(10.0)
    return h
