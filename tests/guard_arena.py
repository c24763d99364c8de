"""One allocation cut into guarded regions: the memory a test hands to the C ABI (include/acimg.h: "the CALLER owns every
buffer") with a band of canary bytes before and after every region.  Everything a guarded call can reach lies inside the
arena, so a kernel that writes past a workspace slab or an output extent lands in memory the test owns: `check()` reports
it (which region, which side, the first touched offset) instead of the write going unnoticed in an allocator's slack - or
faulting.  Works on CPU tensors too (tests/test_guard_arena_cpu.py)."""
import torch

ALIGN = 256
GUARD_MIN = 64 * 1024
GUARD_MAX = 4 * 1024 * 1024
CANARY = 0xA5


def guard_bytes(nbytes):
    """guard band of a region of `nbytes`: max(64 KiB, min(nbytes, 4 MiB)), rounded up to the region alignment"""
    g = max(GUARD_MIN, min(int(nbytes), GUARD_MAX))
    return -(-g // ALIGN) * ALIGN


def arena_bytes(sizes):
    """capacity that holds regions of these sizes, whatever the base address's alignment"""
    return ALIGN + sum(2 * guard_bytes(n) + int(n) + ALIGN for n in sizes)


class Region(object):
    """`nbytes` bytes at offset `off` of the arena; bands [off - before, off) and [off + nbytes, off + nbytes + after)"""

    def __init__(self, arena, name, off, nbytes, before, after):
        self.arena, self.name, self.off, self.nbytes, self.before, self.after = arena, name, off, nbytes, before, after

    @property
    def u8(self):
        return self.arena.buf[self.off:self.off + self.nbytes]

    @property
    def ptr(self):
        return self.arena.buf.data_ptr() + self.off

    def fill(self, byte):
        self.u8.fill_(int(byte))
        return self

    def view(self, dtype, *shape):
        """the region's leading bytes as a tensor of `shape` (the shape must fit; the rest stays addressable via .u8)"""
        n = 1
        for s in shape:
            n *= int(s)
        nb = n * torch.empty((), dtype=dtype).element_size()
        assert nb <= self.nbytes, (self.name, nb, self.nbytes)
        return self.u8[:nb].view(dtype).view(*shape)


class GuardArena(object):
    def __init__(self, device, capacity, canary=CANARY):
        self.canary = int(canary)
        self.buf = torch.full((int(capacity),), self.canary, dtype=torch.uint8, device=device)
        self.regions = []
        self._end = 0                                    # first byte not yet owned by a region or one of its bands

    @classmethod
    def for_sizes(cls, device, sizes, canary=CANARY):
        return cls(device, arena_bytes(sizes), canary)

    def region(self, nbytes, fill=None, name=None):
        """a 256-byte-aligned region of `nbytes` (0 allowed) pre-filled with the byte `fill` (None: left as canary)"""
        nbytes = int(nbytes)
        g = guard_bytes(nbytes)
        base = self.buf.data_ptr()
        off = self._end + g
        off += (-(base + off)) % ALIGN                   # align the ADDRESS, not the offset
        if off + nbytes + g > self.buf.numel():
            raise ValueError("guard arena too small: region %r of %d bytes needs %d, capacity %d"
                             % (name, nbytes, off + nbytes + g, self.buf.numel()))
        r = Region(self, name if name is not None else "region%d" % len(self.regions), off, nbytes, off - self._end, g)
        self._end = off + nbytes + g
        self.regions.append(r)
        if fill is not None and nbytes:
            r.fill(fill)
        return r

    def _bands(self):
        for r in self.regions:
            yield r, "before", r.off - r.before, r.off
            yield r, "after", r.off + r.nbytes, r.off + r.nbytes + r.after

    def touched(self):
        """[(region name, side, offset)] of every damaged band; offset = first touched byte relative to the region's
        start (negative in the band before it, >= nbytes in the band after it).  One device -> host transfer when clean."""
        bands = list(self._bands())
        if not bands:
            return []
        flags = torch.stack([self.buf[lo:hi].ne(self.canary).any() for _, _, lo, hi in bands]).cpu()
        out = []
        for bad, (r, side, lo, hi) in zip(flags.tolist(), bands):
            if bad:
                first = int(self.buf[lo:hi].ne(self.canary).nonzero()[0])
                out.append((r.name, side, lo + first - r.off))
        return out

    def check(self, what=""):
        bad = self.touched()
        assert not bad, "%sguard band touched: %s" % (
            what + ": " if what else "",
            "; ".join("region %r, band %s it, first at offset %d" % b for b in bad))

    def restore(self):
        """repaint every band (after a reported overrun, so that later checks speak about later calls)"""
        for _, _, lo, hi in self._bands():
            self.buf[lo:hi].fill_(self.canary)
