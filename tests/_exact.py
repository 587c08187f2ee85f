"""Exact-arithmetic corpora in which every row, residual and scale byte matters
(test infrastructure), and their independent integer reference.

tests/_grid.py's codebook corpus pins ids, order and ties at 1M docs, but a doc
there repeats a few codes, its residual is zero and every scale byte is the
same.  Here every value is a dyadic rational with few bits, so the kernels'
fp32 results must EQUAL the reference bit for bit in any accumulation order,
and the inputs are built so that a wrong row, token, residual term or scale
byte changes a score:

  values   each token has 16 non-zero dims, 8 at random positions of each
           64-dim half (a half is never empty, so its scale byte is its own);
           doc values +-k/16 with k in [5, 16], query values +-k/16 with k in
           [5, 8].  (k >= 5: at a binade edge a negative residual would round
           bf16 off the grid.)
  bf16     those grid values.
  fp32     grid + j/4096, j in [-3, 3], on every non-zero value: hi = bf16(x)
           is the grid value and lo = j/4096 exactly (about 10 % of all
           elements have lo != 0); every term of lo.qhi + hi.qlo + hi.qhi is a
           multiple of 2^-16 and every partial sum stays below 2^6, so fp32 in
           any order is exact.  Every query token has qlo.qhi != 0.
  mxfp8    no residual; each 64-dim half of each token times 2^e, e from
           {0, -1, -2} for docs and {0, -1} for queries: scale bytes differ
           between the halves of a token, between neighbouring tokens and
           between query tokens, and quantisation stays lossless (at most 4
           significant bits, a half's smallest non-zero >= max / 16).  Products
           are multiples of 2^-11, |dot| <= 16.

  rows     doc i with doclens[i] = L > 0 holds P = ld / 128 planted rows (one
           for 128-slot docs; long-document corpora have fewer docs than slots,
           so one planted row per doc could not reach every slot): planted row
           m at slot slots[i, m] is a copy of query token (qb[i], qj[i, m]) and
           is the UNIQUE arg-max of that token over the doc's scoring rows
           (checked; other rows that reach it are re-drawn).  Every padding row
           (t >= L) holds planted token 0 doubled: any read of padding raises
           the score of query qb[i].  qb favours low query indices, so a batch
           of 1, 2 or 4 queries still owns a large share of the planted rows.
           (tests/_padding.py overwrites the padding of an encoded corpus
           with NaN / Inf encodings instead: the reference below reads the
           scoring rows only, so it stays what it is.)
  doclens  0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128 and, for ld >
           128, 129, ld - 129, ld - 128, ld - 1, ld; the rest drawn so that
           every residue mod 16 and every planted slot in [0, ld) occurs (the
           constructor raises when N is too small for that).

Reference: integers, the values times 2^16.  ``row_max`` gives the per-token
row maxima M[b, j, n] of the three-term sum (hi + lo).qhi + hi.qlo (lo.qlo is
not part of cbv2_score_f32; lo = 0 for the other kinds) under doclens; the
score of any lq is the prefix sum over j, so one table serves an lq sweep.  The
dot products are integer sums below 2^40: ``row_max`` forms them either in
int64 (``pure_int``; the CPU tests pin the two against each other) or, for the
GPU-sized corpora, as integer-valued float64 in BLAS -- exact, every partial
sum being an integer below 2^53 -- and everything after the dot (max, prefix
sums) is int64.  An empty doc scores -inf.
"""
import numpy as np

DIM = 128
LQ = 32
HALF_NNZ = 8
ONE = 1 << 16                       # fixed point: value = integer / 2^16
NEG = -(1 << 50)                    # row max of an empty doc (32 of them still fit int64)
KINDS = ("bf16", "mxfp8", "fp32")
SPECIAL = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)


def special_doclens(ld):
    v = list(SPECIAL)
    if ld > 128:
        v += [129, ld - 129, ld - 128, ld - 1, ld]
    return sorted({x for x in v if 0 <= x <= ld})


def _grid(rng, n, klo, khi):
    """n tokens of signed grid steps k (value k/16): 8 non-zeros per 64-dim half -> int64 [n, 128]."""
    pos = np.argsort(rng.random((n, 2, 64)), axis=2)[:, :, :HALF_NNZ]
    k = rng.integers(klo, khi + 1, size=pos.shape) * rng.choice(np.array([-1, 1]), size=pos.shape)
    out = np.zeros((n, 2, 64), np.int64)
    np.put_along_axis(out, pos, k, axis=2)
    return out.reshape(n, DIM)


def _tokens(rng, kind, n, khi, exps, need_cross=False):
    """-> (hi, lo) int64 [n, 128] in units of 2^-16."""
    hi = _grid(rng, n, 5, khi) * (ONE // 16)
    lo = np.zeros_like(hi)
    if kind == "mxfp8":
        e = rng.choice(np.asarray(exps), size=(n, 2))
        hi = hi // np.repeat(1 << (-e), 64, axis=1)          # exact: k * 4096 / 2^-e
    elif kind == "fp32":
        lo = np.where(hi != 0, rng.integers(-3, 4, size=hi.shape) * (ONE // 4096), 0)
        if need_cross:                                        # every query token: qlo.qhi != 0
            while True:
                bad = np.nonzero((hi * lo).sum(axis=1) == 0)[0]
                if len(bad) == 0:
                    break
                lo[bad] = np.where(hi[bad] != 0, rng.integers(-3, 4, size=(len(bad), DIM)) * (ONE // 4096), 0)
    return hi, lo


def scale_exp(x_int):
    """The MXFP8 quantizer's exponent per 64-value half (scale byte - 127) of
    integer values [..., 128] in units of 2^-16: the smallest e with
    max|x| <= 448 * 2^e (0 for an all-zero half)."""
    m = np.abs(np.asarray(x_int)).reshape(*np.shape(x_int)[:-1], 2, 64).max(axis=-1) / ONE
    f, p = np.frexp(m)
    return np.where(m > 0, np.where(f <= 0.875, p - 9, p - 8), 0).astype(np.int64)


def rescale(x_int, e_from, e_to):
    """Values whose halves were quantized with exponents e_from, read back with e_to."""
    x = np.asarray(x_int, np.int64).reshape(*np.shape(x_int)[:-1], 2, 64)
    sh = (np.asarray(e_to) - np.asarray(e_from))[..., None]
    num = x * (1 << np.maximum(sh, 0))
    den = 1 << np.maximum(-sh, 0)
    assert not (num % den).any(), "rescaled value leaves the 2^-16 grid"
    return (num // den).reshape(np.shape(x_int))


def row_max(qhi, qlo, dhi, dlo, doclens, pure_int=False, skip_row=None, budget=1 << 24):
    """M[t, n] = max over rows r < doclens[n] (r != skip_row[n]) of
    (dhi + dlo)[n, r].qhi[t] + dhi[n, r].qlo[t], int64 [T, N] in units of 2^-32;
    NEG where no row scores.  qhi / qlo [T, 128], dhi / dlo [N, ld, 128]."""
    T, (N, ld, _) = qhi.shape[0], dhi.shape
    three = bool(np.any(qlo)) or bool(np.any(dlo))
    valid = np.arange(ld)[None, :] < np.asarray(doclens)[:, None]
    if skip_row is not None:
        valid = valid & (np.arange(ld)[None, :] != np.asarray(skip_row)[:, None])
    dt = np.int64 if pure_int else np.float64
    qh, ql = qhi.astype(dt), qlo.astype(dt)
    out = np.empty((T, N), np.int64)
    step = max(1, budget // (T * ld))
    for a in range(0, N, step):
        h = dhi[a:a + step].reshape(-1, DIM).astype(dt)
        if three:
            d = qh @ (h + dlo[a:a + step].reshape(-1, DIM).astype(dt)).T + ql @ h.T
        else:
            d = qh @ h.T
        d = d.astype(np.int64).reshape(T, -1, ld)
        out[:, a:a + step] = np.where(valid[None, a:a + step], d, NEG).max(axis=2)
    return out


def prefix_scores(M, doclens):
    """Row maxima int64 [B, 32, N] -> float64 [B, 32, N]: [:, lq - 1] is the
    score of the first lq query tokens; -inf for an empty doc."""
    s = np.cumsum(M, axis=1).astype(np.float64) / float(1 << 32)
    s[:, :, np.asarray(doclens) == 0] = -np.inf
    return s


class ExactCorpus:
    def __init__(self, kind, ld, N, B, seed=0, plant=True, pad=True, pure_int=False):
        assert kind in KINDS and ld % 128 == 0
        self.kind, self.ld, self.N, self.B = kind, ld, N, B
        self.P = ld // 128
        rng = np.random.default_rng([seed, ld, KINDS.index(kind)])
        self.qhi, self.qlo = (x.reshape(B, LQ, DIM) for x in
                              _tokens(rng, kind, B * LQ, 8, (0, -1), need_cross=True))
        self._plan(rng)
        dhi, dlo = _tokens(rng, kind, N * ld, 16, (0, -1, -2))
        self.dhi, self.dlo = dhi.reshape(N, ld, DIM), dlo.reshape(N, ld, DIM)
        self._doc_rng = lambda n: _tokens(rng, kind, n, 16, (0, -1, -2))
        if plant:
            self._plant()
            self._make_unique()
        if pad:
            self._pad()
        self.dhi, self.dlo = self.dhi.astype(np.int32), self.dlo.astype(np.int32)
        self.M = self.row_max(pure_int=pure_int)                    # [B, 32, N]
        self.ref = prefix_scores(self.M, self.doclens)              # float64 [B, 32, N]
        fin = np.isfinite(self.ref)
        assert np.array_equal(self.ref.astype(np.float32).astype(np.float64), self.ref)   # fp32 holds every score
        assert np.abs(self.ref[fin]).max() < 64

    # ------------------------------------------------------------------ layout
    def _plan(self, rng):
        ld, N, B, P = self.ld, self.N, self.B, self.P
        spec = special_doclens(ld)
        if N < len(spec):
            raise ValueError(f"N = {N} cannot hold the {len(spec)} required doc lengths")
        doclens = np.empty(N, np.int32)
        slots = np.full((N, P), -1, np.int64)
        cov = np.zeros(ld, bool)
        need_res = set(range(16))
        for i in range(N):
            if i < len(spec):
                L = spec[i]
            else:
                unc = np.nonzero(~cov)[0]
                lo = int(unc[-1]) + 1 if len(unc) else 1
                L = int(rng.integers(lo, ld + 1))
                if need_res:
                    c = lo + (min(need_res) - lo) % 16
                    L = c if c <= ld else L
            need_res.discard(L % 16)
            doclens[i] = L
            m = min(P, L)
            take = np.nonzero(~cov[:L])[0][::-1][:m]                # the highest uncovered slots first
            if len(take) < m:
                rest = np.setdiff1d(np.arange(L), take)
                take = np.concatenate([take, rng.choice(rest, m - len(take), replace=False)])
            cov[take] = True
            slots[i, :m] = take
        if not cov.all() or need_res:
            raise ValueError(f"N = {N} is too small to cover every slot of ld = {ld} and every length mod 16")
        perm = rng.permutation(N)                                   # the required lengths anywhere in the corpus
        self.doclens, self.slots = doclens[perm], slots[perm]
        share = (1, 2, 4, 16, B)
        self.qb = np.array([rng.integers(min(share[i % 5], B)) for i in range(N)], np.int64)
        cnt = np.zeros(B, np.int64)
        self.qj = np.empty((N, P), np.int64)
        for i in range(N):
            self.qj[i] = (cnt[self.qb[i]] + np.arange(P)) % LQ
            cnt[self.qb[i]] += P

    def _plant(self):
        i, m = np.nonzero(self.slots >= 0)
        self.dhi[i, self.slots[i, m]] = self.qhi[self.qb[i], self.qj[i, m]]
        self.dlo[i, self.slots[i, m]] = self.qlo[self.qb[i], self.qj[i, m]]

    def _pad(self):
        pad = np.arange(self.ld)[None, :] >= self.doclens[:, None]
        i, t = np.nonzero(pad)
        self.dhi[i, t] = 2 * self.qhi[self.qb[i], self.qj[i, 0]]
        self.dlo[i, t] = 2 * self.qlo[self.qb[i], self.qj[i, 0]]

    def _make_unique(self):
        """Re-draw every scoring row that reaches a planted row's dot product with its token."""
        N, ld, P = self.N, self.ld, self.P
        qh = self.qhi[self.qb[:, None], self.qj].astype(np.float64)        # [N, P, 128]
        ql = self.qlo[self.qb[:, None], self.qj].astype(np.float64)
        t = np.arange(ld)
        for _ in range(200):
            h, l = self.dhi.astype(np.float64), self.dlo.astype(np.float64)
            d = np.matmul(h + l, qh.transpose(0, 2, 1)) + np.matmul(h, ql.transpose(0, 2, 1))   # [N, ld, P]
            own = np.take_along_axis(d, np.maximum(self.slots, 0)[:, None, :], axis=1)          # [N, 1, P]
            other = (t[None, :, None] < self.doclens[:, None, None]) & (t[None, :, None] != self.slots[:, None, :]) \
                & (self.slots[:, None, :] >= 0)
            bad = (other & (d >= own)).any(axis=2)                                           # [N, ld]
            planted = np.zeros((N, ld), bool)
            i, m = np.nonzero(self.slots >= 0)
            planted[i, self.slots[i, m]] = True
            if (bad & planted).any():
                raise ValueError("two planted tokens of one doc collide; try another seed")
            if not bad.any():
                return
            i, r = np.nonzero(bad)
            self.dhi[i, r], self.dlo[i, r] = self._doc_rng(len(i))
        raise ValueError("planted rows did not become unique")

    # ------------------------------------------------------------------ reference
    def row_max(self, qhi=None, qlo=None, dhi=None, dlo=None, doclens=None, pure_int=False, skip_row=None):
        qhi = self.qhi if qhi is None else qhi
        qlo = self.qlo if qlo is None else qlo
        B = qhi.shape[0]
        M = row_max(qhi.reshape(-1, DIM), qlo.reshape(-1, DIM), self.dhi if dhi is None else dhi,
                    self.dlo if dlo is None else dlo, self.doclens if doclens is None else doclens,
                    pure_int=pure_int, skip_row=skip_row)
        return M.reshape(B, LQ, -1)

    def scores(self, lq=LQ, B=None):
        """float32 [B, N]: the exact scores of the first lq tokens of the first B queries."""
        return self.ref[: self.B if B is None else B, lq - 1].astype(np.float32)

    # ------------------------------------------------------------------ inputs
    def docs_f32(self):
        return ((self.dhi.astype(np.int64) + self.dlo) / float(ONE)).astype(np.float32)

    def queries_f32(self):
        return ((self.qhi + self.qlo) / float(ONE)).astype(np.float32)


_corpora = {}


def cached_corpus(kind, ld, N, B, seed=0):
    """ExactCorpus(kind, ld, N, B, seed), built once per process (a pool takes
    4-5 s) and shared by the test files of a session: read-only."""
    key = (kind, ld, N, B, seed)
    if key not in _corpora:
        _corpora[key] = ExactCorpus(kind, ld, N, B, seed=seed)
    return _corpora[key]


def difference_message(c, kind, ld, what, B, lq, got, want, docs=None, corpus_at=None, place=None):
    """The failure message of a bit comparison: names the first differing
    (query, doc), its length, its planted slots and both bit patterns.  ``got``
    / ``want`` float32 [B, cols]; ``docs`` int [B, cols]: the doc of each
    column (default: the column); ``corpus_at``: doc -> doc of corpus ``c`` or
    -1 (default: the docs are c's own); ``place(doc)``: words on where the doc
    lies."""
    g = np.ascontiguousarray(got, np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(g != w)
    b, col = (int(x) for x in bad[0])
    col_docs = bad[:, 1] if docs is None else np.asarray(docs)[bad[:, 0], bad[:, 1]]
    d = int(col_docs[0])
    if corpus_at is None:
        inside = col_docs[(col_docs >= 0) & (col_docs < c.N)]
        cd = d if 0 <= d < c.N else -1
    else:
        inside = col_docs[(col_docs >= 0) & (col_docs < len(corpus_at))]
        inside = corpus_at[inside][corpus_at[inside] >= 0]
        cd = int(corpus_at[d]) if 0 <= d < len(corpus_at) else -1
    where = f"doc {d}"
    if cd >= 0:
        where += (f" (doclens {int(c.doclens[cd])}, planted slots {c.slots[cd].tolist()} = tokens "
                  f"{c.qj[cd].tolist()} of query {int(c.qb[cd])})")
    if place is not None:
        where += f" [{place(d)}]"
    return (f"{what}: {kind} ld={ld} B={B} lq={lq}: {len(bad)} of {g.size} scores differ from the exact "
            f"reference; first at query {b}, {where}: got 0x{int(g[b, col]):08x} "
            f"({float(got[b, col])!r}), want 0x{int(w[b, col]):08x} ({float(want[b, col])!r}); "
            f"queries {sorted(set(bad[:, 0].tolist()))[:12]}, doclens % 16 of the differing docs "
            f"{sorted(set((c.doclens[inside] % 16).tolist()))}, doclens {sorted(set(c.doclens[inside].tolist()))[:12]}")
