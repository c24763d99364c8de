"""The guard arena of the caller-memory tests (tests/guard_arena.py) on CPU tensors: it must see a single planted byte in
either band of any region and say which region it was - a checker that cannot fail would make every guarded GPU case
vacuous."""
import pytest
import torch

from guard_arena import ALIGN, CANARY, GUARD_MAX, GUARD_MIN, GuardArena, arena_bytes, guard_bytes

SIZES = (1000, 0, 70000, 4096, 16)


def _arena():
    a = GuardArena.for_sizes("cpu", SIZES)
    regs = [a.region(n, fill=0x7B if i % 2 else 0xFF, name="r%d" % i) for i, n in enumerate(SIZES)]
    return a, regs


def test_guard_size_rule():
    assert guard_bytes(0) == GUARD_MIN and guard_bytes(1000) == GUARD_MIN
    assert guard_bytes(70000) == -(-70000 // ALIGN) * ALIGN
    assert guard_bytes(1 << 30) == GUARD_MAX
    assert arena_bytes([0]) >= 2 * GUARD_MIN


def test_regions_are_aligned_disjoint_and_filled():
    a, regs = _arena()
    a.check()
    end = 0
    for i, (r, n) in enumerate(zip(regs, SIZES)):
        assert r.ptr % ALIGN == 0 and r.nbytes == n and r.u8.numel() == n
        assert r.before >= guard_bytes(n) and r.after == guard_bytes(n)
        assert r.off - r.before == end                       # bands and regions tile the arena without holes
        end = r.off + r.nbytes + r.after
        if n:
            assert bool((r.u8 == (0x7B if i % 2 else 0xFF)).all())
    assert end <= a.buf.numel()
    # a zero-length region still has an address and both bands
    z = regs[1]
    assert z.nbytes == 0 and z.u8.numel() == 0 and z.view(torch.float32, 0).numel() == 0
    # typed views alias the arena
    v = regs[3].view(torch.float32, 8, 128)
    v.fill_(2.0)
    assert bool((regs[3].u8.view(torch.float32) == 2.0).all())
    a.check()
    with pytest.raises(AssertionError):
        regs[4].view(torch.float32, 5)                        # 20 bytes do not fit 16
    with pytest.raises(ValueError):
        a.region(GUARD_MAX, name="too much")


@pytest.mark.parametrize("which", range(len(SIZES)))
@pytest.mark.parametrize("side", ["before", "after"])
@pytest.mark.parametrize("edge", ["near", "far"])
def test_planted_byte_is_found_and_attributed(which, side, edge):
    a, regs = _arena()
    r = regs[which]
    if side == "before":
        rel = -1 if edge == "near" else -r.before
    else:
        rel = r.nbytes if edge == "near" else r.nbytes + r.after - 1
    assert a.buf[r.off + rel] == CANARY
    a.buf[r.off + rel] = CANARY ^ 1                            # one byte, one bit
    assert a.touched() == [(r.name, side, rel)]
    with pytest.raises(AssertionError) as e:
        a.check("planted")
    msg = str(e.value)
    assert "planted" in msg and repr(r.name) in msg and "band %s it" % side in msg and "offset %d" % rel in msg
    for other in regs:
        if other is not r:
            assert repr(other.name) not in msg
    a.restore()
    a.check()


def test_writes_inside_a_region_are_not_reported():
    a, regs = _arena()
    for r in regs:
        if r.nbytes:
            r.u8[0] = 1
            r.u8[-1] = 2
    a.check()


def test_first_touched_offset_of_a_run():
    a, regs = _arena()
    r = regs[2]
    a.buf[r.off + r.nbytes + 40: r.off + r.nbytes + 90] = 0
    a.buf[r.off - 7: r.off] = 0
    assert a.touched() == [(r.name, "before", -7), (r.name, "after", r.nbytes + 40)]
