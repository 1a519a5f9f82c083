"""Planes carved out of one guarded device allocation.

Every plane a test hands to the library is normally its own nz_tile_alloc allocation: 256-byte aligned, exactly n floats
long, with the allocator's slack behind it.  A `Slab` lays the planes of one call out inside ONE allocation instead, each at
a chosen phase of the 16-byte vector alignment, with a guard band on both sides, and fills everything that is not a plane's
initial content with the canary word 0x7FC0BEEF -- a quiet NaN with a payload no kernel produces.  After the call `check()`
requires the canary's bit pattern in every byte outside the planes: a store past an end is seen (a NaN store too: the payload
differs), a load from a guard that a kernel uses poisons its result, and a wrong kernel damages a guard instead of leaving
the allocation.

    slab = Slab(ctx, guard=max(2 * pitch, 1024))
    src = slab.carve(n, phase=1, fill=plane, name="src")
    tmp = slab.carve(n, phase=3, name="tmp")          # no fill: the plane starts as canary words
    slab.upload()                                       # one upload; src.ptr / tmp.ptr are valid from here on
    ctx.call(..., src.ptr, tmp.ptr, ...).Complete()
    got = src.ToArray(shape); slab.check()

The context is anything with `alloc(n, dtype=)` -> tile (`ptr`, `CopyFrom`, `ToArray`, `Dispose`) and `wrap(ptr, n, dtype=)`:
noize_job_amd.Context, or the numpy stand-in of tests/test_slab.py.  No GPU import here."""
import numpy as np

CANARY = 0x7FC0BEEF
_CANARY_BYTES = np.frombuffer(np.array([CANARY], "<u4").tobytes(), np.uint8)
_UNITS = {"float32": "floats", "uint32": "words", "int32": "words", "uint16": "halfwords", "uint8": "bytes"}


def canary(n, dtype=np.float32):
    """n elements of `dtype` whose bytes are the canary pattern (for a region that starts on a word boundary)."""
    dtype = np.dtype(dtype)
    words = np.full((n * dtype.itemsize + 3) // 4, CANARY, np.uint32)
    return words.view(np.uint8)[:n * dtype.itemsize].view(dtype).copy()


def is_canary(a):
    """True where the float32 / uint32 cells of `a` still hold the canary word."""
    return np.ascontiguousarray(a).view(np.uint32) == np.uint32(CANARY)


class _Region:
    __slots__ = ("name", "start", "nbytes", "dtype", "length", "tile")


class Slab:
    def __init__(self, ctx, guard):
        self.ctx = ctx
        self.guard_bytes = 4 * int(guard)
        assert self.guard_bytes >= 16, "a guard shorter than one vector checks nothing"
        self.regions = []
        self._fills = []
        self._cursor = 0     # end of the last region, in bytes from the 16-byte aligned origin
        self._dev = None
        self._origin = None  # device address of byte 0 of the layout (16-byte aligned)
        self._total = 0

    # ---- layout -----------------------------------------------------------------------------------------------------------
    def carve(self, n_elems, phase, dtype=np.float32, fill=None, name=None, byte_phase=None):
        """A plane of n_elems elements whose address is 4 * phase past a 16-byte boundary (byte_phase: that many bytes
        instead, a multiple of the element size -- the 2-byte steps of a 16-bit stream, the byte steps of a texture).
        `fill`: initial content (array of n_elems, or a scalar); None leaves the canary in it.  Returns a non-owning tile
        whose `ptr` is set by upload()."""
        assert self._dev is None, "carve before upload(): the slab is uploaded once"
        dtype = np.dtype(dtype)
        off = 4 * int(phase) if byte_phase is None else int(byte_phase)
        assert 0 <= off < 16 and off % dtype.itemsize == 0, (phase, byte_phase, dtype)
        r = _Region()
        r.name = name or "plane%d" % len(self.regions)
        r.start = -(-(self._cursor + self.guard_bytes) // 16) * 16 + off
        r.length, r.dtype, r.nbytes = int(n_elems), dtype, int(n_elems) * dtype.itemsize
        r.tile = self.ctx.wrap(0, r.length, dtype=dtype)
        self._cursor = r.start + r.nbytes
        self.regions.append(r)
        if fill is not None:
            host = np.empty(r.length, dtype)
            host[:] = np.asarray(fill, dtype).reshape(-1) if np.ndim(fill) else dtype.type(fill)
            self._fills.append((r, host))
        return r.tile

    def upload(self):
        """Allocate the slab, fill it (canary everywhere, the planes' initial content inside them) with ONE upload and
        give every carved tile its address."""
        assert self._dev is None
        self._total = -(-(self._cursor + self.guard_bytes) // 16) * 16
        self._dev = self.ctx.alloc(self._total // 4 + 4, dtype=np.uint32)  # 16 spare bytes: the origin is rounded up
        shift = -self._dev.ptr % 16
        assert shift % 4 == 0
        self._origin = self._dev.ptr + shift
        host = np.full(self._total // 4 + 4, CANARY, np.uint32)
        body = host.view(np.uint8)[shift:shift + self._total]
        for r, a in self._fills:
            body[r.start:r.start + r.nbytes] = a.view(np.uint8)
        self._dev.CopyFrom(host)
        for r in self.regions:
            r.tile.ptr = self._origin + r.start
            assert r.tile.ptr % r.dtype.itemsize == 0
        return self

    def region(self, tile):
        for r in self.regions:
            if r.tile is tile:
                return r
        raise KeyError("not a tile of this slab")

    # ---- the check --------------------------------------------------------------------------------------------------------
    def damage(self):
        """None if every byte outside the carved planes still holds the canary, otherwise a description of the first
        damaged byte relative to the nearest plane."""
        assert self._dev is not None, "upload() first"
        shift = self._origin - self._dev.ptr
        raw = np.ascontiguousarray(self._dev.ToArray()).view(np.uint8)
        body = raw[shift:shift + self._total]
        want = np.tile(_CANARY_BYTES, self._total // 4)
        free = np.ones(self._total, bool)
        for r in self.regions:
            free[r.start:r.start + r.nbytes] = False
        edge = np.ones(raw.size, bool)          # the spare bytes either side of the layout are guard as well
        edge[shift:shift + self._total] = False
        bad = np.flatnonzero(free & (body != want))
        if not bad.size:
            stray = np.flatnonzero(edge & (raw != np.tile(_CANARY_BYTES, raw.size // 4)))
            return "byte %d of the slab's own margin was overwritten" % int(stray[0]) if stray.size else None
        first = int(bad[0])
        # nearest plane: the one whose end is closest before, or whose start is closest after
        best = None
        for r in self.regions:
            if r.start + r.nbytes <= first:
                d, side = first - (r.start + r.nbytes), "after"
            else:
                d, side = r.start - 1 - first, "before"
            if r.start <= first < r.start + r.nbytes:
                continue
            if best is None or d < best[0]:
                best = (d, side, r)
        word = body[first // 4 * 4:first // 4 * 4 + 4].view("<u4")[0]
        if best is None:
            return "guard byte %d damaged (word 0x%08X); no plane carved" % (first, word)
        d, side, r = best
        return "%d %s %s `%s`: guard word reads 0x%08X, not the canary 0x%08X (%d damaged bytes in all)" % (
            d // r.dtype.itemsize + 1, _UNITS.get(r.dtype.name, "elements"), side, r.name, word, CANARY, bad.size)

    def check(self):
        msg = self.damage()
        assert msg is None, "slab guard damaged: " + msg

    def Dispose(self):
        if self._dev is not None:
            self._dev.Dispose()
            self._dev = None
        for r in self.regions:
            r.tile.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.Dispose()
