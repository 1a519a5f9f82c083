"""tests/slab.py must fail when it should: the guard check over a numpy stand-in for the device context (no GPU, no oracle)."""
import numpy as np
import pytest

from slab import CANARY, Slab, canary, is_canary

f32 = np.float32


class HostTile:
    """DeviceTile's surface over host memory: `ptr` is a real address inside one of the context's arrays."""

    def __init__(self, ctx, length, ptr, dtype):
        self.ctx, self.Length, self.ptr, self.dtype = ctx, int(length), int(ptr), np.dtype(dtype)

    def _bytes(self):
        return self.ctx.view(self.ptr, self.Length * self.dtype.itemsize)

    def CopyFrom(self, host):
        host = np.ascontiguousarray(host, self.dtype).reshape(-1)
        assert host.size == self.Length
        self._bytes()[:] = host.view(np.uint8)
        return self

    def ToArray(self, shape=None):
        out = self._bytes().copy().view(self.dtype)
        return out.reshape(shape) if shape is not None else out

    def Dispose(self):
        self.ptr = 0


class HostContext:
    """alloc / wrap of noize_job_amd.Context over numpy arrays; `skew` moves the allocations off 16 bytes."""

    def __init__(self, skew=0):
        self.arrays, self.skew = [], skew

    def alloc(self, length, dtype=f32):
        raw = np.zeros(int(length) * np.dtype(dtype).itemsize + 64, np.uint8)
        start = (-raw.ctypes.data) % 16 + self.skew
        self.arrays.append(raw)
        return HostTile(self, length, raw.ctypes.data + start, dtype)

    def wrap(self, ptr, length, dtype=f32):
        return HostTile(self, length, ptr, dtype)

    def view(self, ptr, nbytes):
        for raw in self.arrays:
            off = ptr - raw.ctypes.data
            if 0 <= off and off + nbytes <= raw.size:
                return raw[off:off + nbytes]
        raise AssertionError("address outside every allocation")

    def poke(self, ptr, value, dtype=f32):
        """What a wrong kernel does: one store at a raw address."""
        self.view(ptr, np.dtype(dtype).itemsize)[:] = np.array([value], dtype).view(np.uint8)


def two_planes(skew=0, guard=32):
    ctx = HostContext(skew)
    s = Slab(ctx, guard)
    a = s.carve(10, 1, fill=np.arange(10, dtype=f32), name="src")
    b = s.carve(7, 3, name="tmp")
    s.upload()
    return ctx, s, a, b


def test_silent_when_only_the_planes_are_written():
    ctx, s, a, b = two_planes()
    assert np.array_equal(a.ToArray(), np.arange(10, dtype=f32))
    assert is_canary(b.ToArray()).all()                     # a plane without a fill starts as canary words
    s.check()
    a.CopyFrom(np.full(10, np.nan, f32))
    b.CopyFrom(np.arange(7, dtype=f32))
    ctx.poke(a.ptr, 1.0)
    ctx.poke(b.ptr + 4 * 6, -2.0)
    s.check()
    assert s.damage() is None


@pytest.mark.parametrize("skew", [0, 4, 8, 12])
def test_addresses_have_the_requested_phase(skew):
    ctx = HostContext(skew)                                  # whatever the allocator's own alignment is
    s = Slab(ctx, 16)
    tiles = [(s.carve(5 + p, p), 4 * p) for p in range(4)]
    tiles += [(s.carve(9, 0, dtype=np.uint16, byte_phase=bp), bp) for bp in (0, 2, 6, 14)]
    tiles += [(s.carve(13, 0, dtype=np.uint8, byte_phase=bp), bp) for bp in (0, 1, 2, 3)]
    tiles += [(s.carve(3, 2, dtype=np.uint32), 8)]
    s.upload()
    for t, want in tiles:
        assert t.ptr % 16 == want, (t.ptr % 16, want)
    s.check()
    with pytest.raises(AssertionError):
        Slab(ctx, 16).carve(4, 0, dtype=np.uint16, byte_phase=3)  # a 16-bit stream cannot sit on an odd byte
    with pytest.raises(AssertionError):
        s.carve(4, 0)                                        # the slab was uploaded: it is uploaded once


def test_carvings_never_overlap_and_keep_their_guards():
    ctx = HostContext()
    guard = 24
    s = Slab(ctx, guard)
    rng = np.random.default_rng(0)
    tiles = []
    for k in range(40):
        dt = [f32, np.uint16, np.uint8, np.uint32][k % 4]
        size = np.dtype(dt).itemsize
        bp = int(rng.integers(0, 16 // size)) * size
        tiles.append(s.carve(int(rng.integers(1, 300)), 0, dtype=dt, byte_phase=bp))
    s.upload()
    spans = sorted((t.ptr, t.ptr + t.Length * t.dtype.itemsize) for t in tiles)
    lo, hi = s._origin, s._origin + s._total
    assert spans[0][0] - lo >= 4 * guard and hi - spans[-1][1] >= 4 * guard
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert b0 - a1 >= 4 * guard, "two planes closer than the guard"
    ctx.view(lo, hi - lo)                                    # the whole layout lies inside the one allocation
    assert len(ctx.arrays) == 1


def test_a_store_one_element_after_a_plane_is_reported():
    ctx, s, a, b = two_planes()
    ctx.poke(a.ptr + 4 * 10, 0.0)
    assert s.damage().startswith("1 floats after `src`"), s.damage()
    with pytest.raises(AssertionError, match="1 floats after `src`"):
        s.check()
    ctx, s, a, b = two_planes()
    ctx.poke(b.ptr + 4 * (7 + 2), 5.0)                       # the third float behind the last plane
    with pytest.raises(AssertionError, match="3 floats after `tmp`"):
        s.check()


def test_a_store_one_element_before_a_plane_is_reported():
    ctx, s, a, b = two_planes()
    ctx.poke(a.ptr - 4, 0.0)
    with pytest.raises(AssertionError, match="1 floats before `src`"):
        s.check()
    ctx, s, a, b = two_planes()
    ctx.poke(b.ptr - 8, 1.5)
    with pytest.raises(AssertionError, match="2 floats before `tmp`"):
        s.check()


def test_a_different_nan_in_the_guard_is_reported():
    ctx, s, a, b = two_planes()
    assert np.isnan(canary(1)[0]) and canary(1).view(np.uint32)[0] == CANARY
    ctx.poke(a.ptr + 4 * 10, np.float32(np.nan))             # the default quiet NaN, 0x7FC00000: not the canary's payload
    with pytest.raises(AssertionError, match="0x7FC00000"):
        s.check()
    ctx, s, a, b = two_planes()
    ctx.poke(a.ptr - 4, CANARY, np.uint32)                   # the canary itself changes nothing
    s.check()


def test_a_store_into_the_gap_between_two_planes_is_reported():
    ctx, s, a, b = two_planes(guard=32)
    gap0, gap1 = a.ptr + 4 * 10, b.ptr
    assert gap1 - gap0 >= 4 * 32
    mid = (gap0 + (gap1 - gap0) // 2) // 4 * 4
    ctx.poke(mid, 3.0)
    msg = s.damage()
    assert msg is not None and ("after `src`" in msg or "before `tmp`" in msg), msg
    with pytest.raises(AssertionError, match="slab guard damaged"):
        s.check()


def test_byte_and_halfword_stores_next_to_narrow_planes_are_reported():
    ctx = HostContext()
    s = Slab(ctx, 16)
    idx = s.carve(9, 0, dtype=np.uint16, byte_phase=6, name="indices")
    tex = s.carve(10, 0, dtype=np.uint8, byte_phase=3, name="texture")
    s.upload()
    s.check()
    ctx.poke(idx.ptr + 2 * 9, 7, np.uint16)
    with pytest.raises(AssertionError, match="1 halfwords after `indices`"):
        s.check()
    ctx.poke(idx.ptr + 2 * 9, canary(2, np.uint16)[(idx.ptr + 18) % 4 // 2], np.uint16)
    s.check()
    ctx.poke(tex.ptr - 1, 0, np.uint8)
    with pytest.raises(AssertionError, match="1 bytes before `texture`"):
        s.check()
