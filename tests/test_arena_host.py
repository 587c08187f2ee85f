"""The guard-band arena (tests/_arena.py) on CPU tensors: the proof that the
checker behind tests/test_gpu_bounds.py can fail.  Needs no GPU."""
import struct

import pytest
import torch

from _arena import HEAD, MIN_GUARD, POISON, TAIL, Arena, Violation


def small_arena():
    a = Arena(1 << 20)
    tok = a.take("tokens", 3 * 128 * 256, "bf16", align=16, skew=16, guard=8 * 128 * 256)
    dl = a.take("doclens", 3 * 4, "doclens", align=4, skew=4, fill=128)
    q = a.take("Q", 32 * 256, "bf16", align=16, skew=16)
    bits = a.take("allow", 4, "bitmap", align=4, skew=4)
    sc = a.take("scores", 5 * 4, "scores", align=4, skew=4)
    out = a.take("out", 2 * 10 * 4, "out", align=4, skew=4, writable=True)
    tok.view(torch.bfloat16).fill_(0.25)
    dl.view(torch.int32).copy_(torch.tensor([0, 1, 128], dtype=torch.int32))
    q.view(torch.bfloat16).fill_(0.5)
    bits.view(torch.int32).fill_(5)
    sc.view(torch.float32).fill_(1.0)
    return a


def test_alignment_and_skew_are_what_was_asked():
    a = small_arena()
    assert a.address("tokens") % 256 == 16 and a.address("Q") % 256 == 16       # 16-B aligned, no better
    for name in ("doclens", "allow", "scores", "out"):
        assert a.address(name) % 16 == 4, name                                  # 4-B aligned, no better
    b = Arena(1 << 16)
    assert b.take("x", 100, "f32", align=256, skew=0).data_ptr() % 256 == 0
    assert b.take("y", 100, "f32", align=64, skew=64).data_ptr() % 256 == 64
    for bad in (dict(align=16, skew=4), dict(align=16, skew=256), dict(align=48, skew=0)):
        with pytest.raises(ValueError):
            b.take("z", 16, "f32", **bad)
    with pytest.raises(ValueError):
        b.take("x", 16, "f32")                      # a name taken twice
    with pytest.raises(ValueError):
        b.take("w", 16, "doclens")                  # no fill value
    with pytest.raises(MemoryError):
        b.take("big", 1 << 16, "f32")


def test_views_have_exact_extents_and_guards():
    a = small_arena()
    assert a.view("tokens").numel() == 3 * 128 * 256 and a.view("doclens").numel() == 12
    assert a.size == HEAD + (1 << 20) + TAIL
    for r in a.regions:
        assert r.glo >= MIN_GUARD and r.ghi >= MIN_GUARD, r
        if r.name == "tokens":
            assert r.glo >= 8 * 128 * 256 and r.ghi >= 8 * 128 * 256      # a whole stray doc group lands in it
        assert r.off - r.glo >= HEAD and r.off + r.nbytes + r.ghi <= a.size - TAIL
    spans = sorted((r.off - r.glo, r.off + r.nbytes + r.ghi) for r in a.regions)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))            # no two reservations overlap


def test_guard_values_win_when_read():
    a = small_arena()
    raw = a.buf

    def around(name, dtype, count):
        r = a._region(name)
        n = count * torch.empty((), dtype=dtype).element_size()
        return raw[r.off - n: r.off].view(dtype), raw[r.off + r.nbytes: r.off + r.nbytes + n].view(dtype)

    for side in around("tokens", torch.bfloat16, 8 * 128 * 128):
        assert (side == 100.0).all()
    for side in around("doclens", torch.int32, 64):
        assert (side == 128).all()
    for side in around("allow", torch.int32, 64):
        assert (side == -1).all()
    for side in around("scores", torch.float32, 64):
        assert torch.isposinf(side).all()
    for side in around("out", torch.uint8, 4096):
        assert (side == POISON).all()
    assert a.untouched("out")
    assert struct.unpack("<f", bytes(around("scores", torch.uint8, 4)[1].tolist()))[0] == float("inf")


def test_untouched_arena_verifies():
    a = small_arena()
    a.snapshot()
    a.view("out").fill_(0)            # a call may write its outputs
    assert a.check() == []
    a.verify()
    assert not a.untouched("out")
    a.wipe("out")
    assert a.untouched("out")


def test_verify_needs_a_snapshot():
    a = small_arena()
    with pytest.raises(RuntimeError):
        a.verify()
    a.snapshot()
    a.take("late", 16, "f32")
    with pytest.raises(RuntimeError):
        a.verify()


@pytest.mark.parametrize("name", ["tokens", "doclens", "Q", "allow", "scores", "out"])
def test_planted_guard_bytes_are_reported(name):
    a = small_arena()
    a.snapshot()
    r = a._region(name)
    for side, pos, rel in [("guard before", r.off - r.glo, -r.glo), ("guard before", r.off - 1, -1),
                           ("guard after", r.off + r.nbytes, r.nbytes),
                           ("guard after", r.off + r.nbytes + r.ghi - 1, r.nbytes + r.ghi - 1)]:
        old = int(a.buf[pos])
        a.buf[pos] = old ^ 1
        assert a.check() == [Violation(name, side, rel, rel, 1)]
        with pytest.raises(AssertionError, match=f"{name}: {side} changed, 1 byte"):
            a.verify()
        a.buf[pos] = old
    assert a.check() == []


@pytest.mark.parametrize("name", ["tokens", "doclens", "Q", "allow", "scores"])
def test_planted_input_bytes_are_reported(name):
    a = small_arena()
    a.snapshot()
    r = a._region(name)
    a.buf[r.off] ^= 1
    a.buf[r.off + r.nbytes - 1] ^= 1
    assert a.check() == [Violation(name, "buffer", 0, r.nbytes - 1, 2 if r.nbytes > 1 else 1)]
    with pytest.raises(AssertionError, match=rf"{name}: buffer changed, 2 byte\(s\), first at \+0, last at \+{r.nbytes - 1}"):
        a.verify()


def test_arena_head_and_tail_are_guards():
    a = small_arena()
    a.snapshot()
    a.buf[0] ^= 1
    a.buf[a.size - 1] ^= 1
    assert a.check() == [Violation("<arena>", "guard before", -HEAD, -HEAD, 1),
                         Violation("<arena>", "guard after", TAIL - 1, TAIL - 1, 1)]


def test_release_drops_later_buffers():
    a = small_arena()
    m = a.mark()
    a.take("ws", 1000, "out", writable=True).fill_(7)
    a.release(m)
    assert [r.name for r in a.regions][-1] == "out"
    ws = a.take("ws", 1000, "out", writable=True)
    assert a.untouched("ws") and ws.numel() == 1000
    a.snapshot()
    a.verify()


def test_frozen_output_is_checked_as_an_input():
    a = small_arena()
    a.view("out").fill_(3)
    a.snapshot()
    a.view("out")[5] = 4              # still writable: not compared
    assert a.check() == []
    a.freeze("out")
    with pytest.raises(RuntimeError):
        a.verify()                    # freezing asks for a new snapshot
    a.snapshot()
    a.view("out")[5] = 9
    assert a.check() == [Violation("out", "buffer", 5, 5, 1)]
