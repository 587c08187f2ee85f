"""Sparse full-size index layouts whose few real docs lie astride byte offsets
2^31 and 2^32 of the token arrays (test infrastructure; numpy only).

A kernel that forms a token address as ``int * stride``, or keeps an offset in
32 bits, is right for the first 2 or 4 GiB of an index and silently reads
another doc beyond it.  A full-size index need not be dense to show that: here
the W docs of an exact-arithmetic corpus (tests/_exact.py) sit in three
contiguous runs of about W / 3 docs --

    low    docs [0, W / 3)                  (at doc 0 on purpose: an address that
                                             wraps mod 2^32 from doc d32 + j lands
                                             on real doc j, not on filler)
    mid    centred on d31 = 2^31 / docbytes
    high   centred on d32 = 2^32 / docbytes

-- of an index of n_total = d32 + W docs, and every other doc is FILLER:
doclens = 0 and every token element 2.0 (bf16 0x4000; e4m3 byte 0x40 with scale
byte 127; faithful hi = 2.0, lo = 0).  Filler is a defined value, so any read
of it changes a score by an exactly known amount.  docbytes = ld * 256 for bf16
tokens and the faithful hi / lo arrays, ld * 128 for MXFP8 token bytes.

The corpus is an ``ExactCorpus`` whose plan is amended before planting: a few
docs with drawn lengths become empty, 1-token and full docs, so that each side
of each boundary can hold one of each (the base plan has one empty doc).  The
assignment of corpus docs to positions is a permutation fixed by the seed that
puts, on each side of each boundary, an empty doc, a 1-token doc, a full doc
and a doc whose length is no multiple of 16.

``expected_rows(lq)`` is the exact score matrix of the big index (-inf for every
filler doc); ``wrapped_twin()`` the scores a kernel with a wrapped address
would give.  A doc below its boundary has the same offset under the mask, so
the twin differs from the index only in the docs at or past a boundary
(``Layout.wrapped``).
"""
import numpy as np

import _exact as ex

LDS = (128, 256, 512, 1024)
SIZE = {128: (600, 65), 256: (300, 65), 512: (200, 40), 1024: (200, 40)}      # ld -> (docs W, queries)
FILLER = 2 * ex.ONE                                                           # 2.0 in units of 2^-16
RUNS = ("low", "mid", "high")
EXTRA = 5                                                                     # amended docs per required length
SEED = 3             # of the assignment: the first seed at which the twin condition holds for all 12 layouts
                     # (seeds 0-2 leave a wrapped doc whose 5-token score under query 0 equals its twin's)


SCORE_LQS = (ex.LQ, 5)                                                        # the query lengths the GPU file scores


def score_batches(kind, ld):
    """One B inside every dispatch branch of the scans (the B of
    test_gpu_exact_scores._sweep_batches, whose docstring lists the branches)."""
    if kind == "fp32":
        return (1, 2, 7, 33) if ld == 128 else (1, 14, 21)
    if ld != 128:
        return (1, 2, 8, 9) if kind == "bf16" else (2, 8, 9)
    return (1, 2, 4, 8, 16, 32, 40) if kind == "bf16" else (1, 4, 8, 16, 24, 32, 48, 64)


def docbytes(kind, ld):
    return ld * (128 if kind == "mxfp8" else 256)


class _Corpus(ex.ExactCorpus):
    """ExactCorpus with EXTRA more empty, 1-token and full docs (the amended
    docs are taken from those whose length was drawn, so every special length
    of the base plan stays)."""

    def _plan(self, rng):
        super()._plan(rng)
        special = set(ex.special_doclens(self.ld))
        free = [i for i in range(self.N) if int(self.doclens[i]) not in special]
        pick = rng.choice(np.array(free), 3 * EXTRA, replace=False)
        for j, i in enumerate(pick):
            L = (0, 1, self.ld)[j % 3]
            self.doclens[i] = L
            if L == 0:
                self.slots[i] = -1
            elif L == 1:
                self.slots[i] = -1
                self.slots[i, 0] = 0
            # L = ld: the planted slots of the shorter doc stay valid


class Layout:
    def __init__(self, kind, ld, seed=SEED):
        W, B = SIZE[ld]
        self.kind, self.ld, self.W, self.B = kind, ld, W, B
        self.docbytes = docbytes(kind, ld)
        self.d31, self.d32 = (1 << 31) // self.docbytes, (1 << 32) // self.docbytes
        self.n_total = self.d32 + W
        a = W // 3
        self.sizes = (a, a, W - 2 * a)
        self.starts = (0, self.d31 - a // 2, self.d32 - self.sizes[2] // 2)
        # position p in [0, W) -> global doc
        self.pos_doc = np.concatenate([s + np.arange(m) for s, m in zip(self.starts, self.sizes)]).astype(np.int64)
        self.pos_run = np.repeat(np.arange(3), self.sizes)
        self.c = c = _Corpus(kind, ld, W, B, seed=1)
        self._assign(np.random.default_rng([seed, ld, ex.KINDS.index(kind), 77]))
        self.doclens = np.zeros(self.n_total, np.int32)
        self.doclens[self.doc_of] = c.doclens
        self.corpus_at = np.full(self.n_total, -1, np.int64)                 # global doc -> corpus doc, -1 filler
        self.corpus_at[self.doc_of] = np.arange(W)
        bound = np.array([0, self.d31, self.d32])[self.run_of]
        self.wrapped = np.flatnonzero((self.run_of > 0) & (self.doc_of >= bound))   # corpus docs at / past a boundary
        self._rows = {}

    # ------------------------------------------------------------------ assignment
    def sides(self):
        """The four sides: positions of the mid / high run below, and at or past, their boundary."""
        out = {}
        for r, bnd in ((1, self.d31), (2, self.d32)):
            p = np.flatnonzero(self.pos_run == r)
            out[(RUNS[r], "below")] = p[self.pos_doc[p] < bnd]
            out[(RUNS[r], "past")] = p[self.pos_doc[p] >= bnd]
        return out

    def classes(self):
        dl = self.c.doclens
        return {"empty": np.flatnonzero(dl == 0), "one": np.flatnonzero(dl == 1),
                "full": np.flatnonzero(dl == self.ld), "ragged": np.flatnonzero((dl % 16 != 0) & (dl > 1))}

    def _assign(self, rng):
        """doc_of[i]: the global doc of corpus doc i.  One doc of each class is
        dealt to a random position of each side first; the rest is a random
        permutation of what is left."""
        W = self.W
        pos_of = np.full(W, -1, np.int64)
        used_pos, used_doc = set(), set()
        for cls, docs in self.classes().items():
            docs = [int(d) for d in rng.permutation(docs) if int(d) not in used_doc]
            for side, ps in self.sides().items():
                d = docs.pop()
                p = int(rng.choice([int(x) for x in ps if int(x) not in used_pos]))
                pos_of[d] = p
                used_pos.add(p)
                used_doc.add(d)
        rest_doc = np.array([d for d in range(W) if d not in used_doc])
        rest_pos = np.array([p for p in range(W) if p not in used_pos])
        pos_of[rest_doc] = rng.permutation(rest_pos)
        assert sorted(pos_of.tolist()) == list(range(W))
        self.pos_of = pos_of
        self.doc_of = self.pos_doc[pos_of]
        self.run_of = self.pos_run[pos_of]

    # ------------------------------------------------------------------ expected values
    def expected_rows(self, lq=ex.LQ):
        """float32 [B, n_total]: -inf, and ref[b, lq - 1, i] at the position of corpus doc i."""
        if lq not in self._rows:
            rows = np.full((self.B, self.n_total), -np.inf, np.float32)
            rows[:, self.doc_of] = self.c.ref[:, lq - 1].astype(np.float32)
            rows.setflags(write=False)
            self._rows[lq] = rows
        return self._rows[lq]

    def place(self, doc):
        """Words on where global doc ``doc`` lies: its run and its distance to the run's boundary."""
        if not 0 <= doc < self.n_total:
            return "outside the index"
        i = int(self.corpus_at[doc])
        if i < 0:
            return f"filler, byte offset {doc * self.docbytes:#x}"
        r = int(self.run_of[i])
        if r == 0:
            return "low run"
        d = doc - (self.d31, self.d32)[r - 1]
        return f"{RUNS[r]} run, {abs(d)} docs {'below' if d < 0 else 'at or past'} byte offset 2^{30 + r}"

    def wrapped_source(self):
        """For each doc of ``wrapped``: the global doc whose tokens a wrapped
        address reads (byte offset & 0x7fffffff in the mid run, & 0xffffffff in
        the high run)."""
        off = self.doc_of[self.wrapped] * self.docbytes
        mask = np.where(self.run_of[self.wrapped] == 1, 0x7FFFFFFF, 0xFFFFFFFF)
        src = (off & mask) // self.docbytes
        assert ((off & mask) % self.docbytes == 0).all() and (src != self.doc_of[self.wrapped]).all()
        return src

    def wrapped_twin(self):
        """-> (docs, scores): ``docs`` the corpus docs at or past a boundary
        (``wrapped``), ``scores`` float64 [B, 32, len(docs)] of the index a
        kernel with a 32-bit address would see: their tokens replaced by those
        at the wrapped offset (a low-run doc, or filler), doclens unchanged."""
        c = self.c
        src = self.corpus_at[self.wrapped_source()]
        real = src >= 0
        dhi = np.full((len(src), self.ld, ex.DIM), FILLER, np.int32)
        dlo = np.zeros_like(dhi)
        dhi[real], dlo[real] = c.dhi[src[real]], c.dlo[src[real]]
        dl = c.doclens[self.wrapped]
        return self.wrapped, ex.prefix_scores(c.row_max(dhi=dhi, dlo=dlo, doclens=dl), dl)


_layouts = {}


def layout(kind, ld):
    """One Layout (and its corpus) per (kind, ld) and process."""
    if (kind, ld) not in _layouts:
        _layouts[(kind, ld)] = Layout(kind, ld)
    return _layouts[(kind, ld)]
