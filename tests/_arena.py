"""Guard-band arena: every buffer of one call inside ONE uint8 allocation.

``Arena.take`` reserves ``[guard][buffer][guard]`` and returns the buffer as a
uint8 view with exactly the bytes asked for, at a chosen address phase.  The
guards are filled with a value that WINS if a kernel reads it (a huge score,
a full-length doc, an allowed bit), writable buffers and their guards with the
byte 0xA5, so that ``snapshot()`` before a call and ``verify()`` after it show

  - every write outside a buffer (a guard changed),
  - every write into an input (a read-only buffer changed),
  - every slot of an output the call left unwritten (still 0xA5),

and a comparison of the call's results with the same operation on clones of
the inputs shows every guard value that reached a result.  The arena's own
head and tail (1 MiB each) keep a small overrun inside the allocation, where it
fails an assertion instead of faulting.  Works on CPU tensors too
(tests/test_arena_host.py).
"""
from __future__ import annotations

import struct
from typing import List, NamedTuple, Optional, Tuple

import torch

HEAD = TAIL = 1 << 20          # the arena's own guards
MIN_GUARD = 4096               # smallest guard on either side of a buffer
PHASE = 256                    # buffers are placed relative to 256-B boundaries
COPY_MAX = 64 << 20            # read-only buffers up to this size are compared byte for byte
POISON = 0xA5                  # writable buffers, their guards, head, tail and gaps

# guard fill per kind: the little-endian bytes of one element ("doclens" and
# "ids" take theirs from take(..., fill=))
_FILL = {
    "bf16": struct.pack("<H", 0x42C8),          # 100.0 (not NaN: fmaxf drops a NaN and would hide the read)
    "e4m3": b"\x7e",                            # 448, the largest e4m3
    "e8m0": b"\x8a",                            # 2^11
    "f32": struct.pack("<f", 100.0),
    "bitmap": b"\xff\xff\xff\xff",              # every doc allowed
    "scores": struct.pack("<f", float("inf")),  # beats every score of a selection
    "out": bytes([POISON]),
}
_FILL_ARG = ("doclens", "ids")                  # int32 kinds whose winning value depends on the case


class Region(NamedTuple):
    name: str
    off: int          # buffer offset in the arena
    nbytes: int
    glo: int          # guard bytes before / after
    ghi: int
    writable: bool


class Violation(NamedTuple):
    name: str
    side: str         # "guard before" | "buffer" | "guard after"
    first: int        # changed byte offsets relative to the buffer's first byte
    last: int         # (negative in the guard before, >= nbytes in the guard after)
    count: int

    def __str__(self):
        return (f"{self.name}: {self.side} changed, {self.count} byte(s), "
                f"first at {self.first:+d}, last at {self.last:+d} from the buffer's start")


def _round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, capacity: int, device="cpu"):
        """``capacity``: bytes available to ``take`` (buffers, guards, padding)."""
        self.size = HEAD + int(capacity) + TAIL
        self.buf = torch.empty((self.size,), dtype=torch.uint8, device=device)
        self.buf.fill_(POISON)
        self.base = self.buf.data_ptr()
        self.cursor = HEAD
        self.regions: List[Region] = []
        self._snap: Optional[list] = None

    # ------------------------------------------------------------------ layout
    def _pattern(self, kind: str, fill) -> bytes:
        if kind in _FILL_ARG:
            if fill is None:
                raise ValueError(f"kind {kind!r} needs fill= (the int32 a stray read would see)")
            return struct.pack("<i", int(fill))
        if kind not in _FILL:
            raise ValueError(f"unknown kind {kind!r}")
        return _FILL[kind]

    def _fill(self, a: int, b: int, pattern: bytes) -> None:
        if b <= a:
            return
        if len(pattern) == 1:
            self.buf[a:b].fill_(pattern[0])
            return
        assert (b - a) % len(pattern) == 0
        unit = torch.tensor(list(pattern), dtype=torch.uint8)
        step = 16 << 20
        rep = unit.repeat(min(b - a, step) // len(pattern)).to(self.buf.device)
        for s in range(a, b, step):
            e = min(b, s + step)
            self.buf[s:e] = rep[: e - s]

    def take(self, name: str, nbytes: int, kind: str, align: int = 16, skew: int = 0, writable: bool = False,
             guard: int = MIN_GUARD, fill=None) -> torch.Tensor:
        """Reserve ``nbytes`` and return them as a uint8 view.

        The buffer starts ``skew`` bytes past a 256-B boundary (``skew`` a
        multiple of ``align`` below 256): skew=16, align=16 gives an address
        that is 16-B aligned and no better; skew=4, align=4 one that is 4-B
        aligned and no better.  ``guard``: least bytes on either side (at
        least 4 KiB).  Read-only buffers come back filled with ``kind``'s guard
        value too: the caller writes the real contents before ``snapshot()``.
        """
        nbytes = int(nbytes)
        if nbytes < 0 or align < 1 or skew % align or not 0 <= skew < PHASE or PHASE % align:
            raise ValueError(f"bad reservation {name!r}: nbytes {nbytes}, align {align}, skew {skew}")
        if any(r.name == name for r in self.regions):
            raise ValueError(f"buffer {name!r} taken twice")
        pattern = bytes([POISON]) if writable else self._pattern(kind, fill)
        glo = _round_up(max(int(guard), MIN_GUARD), 16)
        addr = _round_up(self.base + self.cursor + glo, PHASE) + skew
        off = addr - self.base
        glo = off - self.cursor                       # the padding up to the phase belongs to the guard
        lead = glo % len(pattern)                     # keep the pattern in step with the buffer's elements
        ghi = _round_up(max(int(guard), MIN_GUARD), 16)
        end = off + nbytes + ghi
        if end > self.size - TAIL:
            raise MemoryError(f"arena full at {name!r}: {end - HEAD} of {self.size - HEAD - TAIL} bytes")
        self._fill(self.cursor, self.cursor + lead, bytes([pattern[0]]))
        self._fill(self.cursor + lead, off, pattern)
        body = nbytes - nbytes % len(pattern)
        self._fill(off, off + body, pattern)
        self._fill(off + body, off + nbytes, bytes([pattern[0]]))
        self._fill(off + nbytes, end, pattern)
        self.regions.append(Region(name, off, nbytes, glo, ghi, bool(writable)))
        self.cursor = end
        self._snap = None
        return self.buf[off: off + nbytes]

    def view(self, name: str) -> torch.Tensor:
        r = self._region(name)
        return self.buf[r.off: r.off + r.nbytes]

    def address(self, name: str) -> int:
        return self.base + self._region(name).off

    def _region(self, name: str) -> Region:
        for r in self.regions:
            if r.name == name:
                return r
        raise KeyError(name)

    def wipe(self, name: str) -> None:
        """Refill a writable buffer with 0xA5 (between two calls on one arena)."""
        r = self._region(name)
        assert r.writable, name
        self.buf[r.off: r.off + r.nbytes].fill_(POISON)

    def freeze(self, name: str) -> None:
        """From now on a writable buffer is an input: what a call produced there
        (a filter's id list, a quantized query) must survive the calls that read it."""
        i = self.regions.index(self._region(name))
        self.regions[i] = self.regions[i]._replace(writable=False)
        self._snap = None

    def untouched(self, name: str) -> bool:
        """True when every byte of a writable buffer is still 0xA5."""
        r = self._region(name)
        return bool((self.buf[r.off: r.off + r.nbytes] == POISON).all())

    def mark(self) -> Tuple[int, int]:
        """A point to ``release`` to: buffers taken later are per-test (a long-lived arena)."""
        return self.cursor, len(self.regions)

    def release(self, mark: Tuple[int, int]) -> None:
        cursor, count = mark
        self.buf[cursor: self.cursor].fill_(POISON)
        self.cursor = cursor
        del self.regions[count:]
        self._snap = None

    # ------------------------------------------------------------------ checking
    def _spans(self):
        """(name, side, start, end, offset of the buffer) of everything compared."""
        yield "<arena>", "guard before", 0, HEAD, HEAD
        for r in self.regions:
            yield r.name, "guard before", r.off - r.glo, r.off, r.off
            if not r.writable and r.nbytes <= COPY_MAX:
                yield r.name, "buffer", r.off, r.off + r.nbytes, r.off
            yield r.name, "guard after", r.off + r.nbytes, r.off + r.nbytes + r.ghi, r.off
        yield "<arena>", "guard after", self.size - TAIL, self.size, self.size - TAIL

    def snapshot(self) -> None:
        """Copy every guard and every read-only buffer of at most 64 MiB."""
        self._snap = [(n, s, a, b, o, self.buf[a:b].clone()) for n, s, a, b, o in self._spans()]

    def check(self) -> List[Violation]:
        """Everything that differs from the snapshot (an empty list: nothing)."""
        if self._snap is None:
            raise RuntimeError("verify() without a snapshot() after the last take()")
        bad = []
        for name, side, a, b, o, copy in self._snap:
            now = self.buf[a:b]
            if torch.equal(now, copy):
                continue
            idx = (now != copy).nonzero().flatten()
            bad.append(Violation(name, side, int(idx[0]) + a - o, int(idx[-1]) + a - o, int(idx.numel())))
        return bad

    def verify(self) -> None:
        bad = self.check()
        assert not bad, "out-of-bounds write or modified input:\n  " + "\n  ".join(str(v) for v in bad)
