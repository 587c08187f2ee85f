"""CPU: the exact corpora of tests/_exact.py and their integer reference.

tests/test_gpu_exact_scores.py compares every scan, rescoring and rerank
dispatch with ``ExactCorpus.ref`` bit for bit.  That is worth what the
reference is worth, so here
  (a) the reference is checked against independent evaluations: the oracle's
      maxsim on the bf16 values and on the dequantized MXFP8 values, a float64
      three-term evaluation of the faithful score, pure int64 dot products, and
      fp32 evaluations under random permutations of the dims and of the rows
      (every accumulation order gives the same bits);
  (b) the inputs are what the generator's docstring says: the oracle's split
      returns the constructed hi / lo, MXFP8 quantisation is lossless and its
      scale bytes vary inside a token, between tokens and between queries, the
      required doc lengths and every planted slot occur;
  (c) the reference separates the mutants: a kernel that drops a row, reads the
      first padding row, miscounts the query tokens, loses a residual term,
      takes a neighbouring scale byte or skips a 16-dim slice changes a score
      of every doc or query it touches.  (Built with plant=False or pad=False
      the generator leaves those rows random, and the row and padding mutants
      below fail.)
"""
import functools

import numpy as np
import pytest

import _exact as ex
from oracle import oracle as orc

LD, N, B = 128, 176, 33


@functools.lru_cache(maxsize=None)
def corpus(kind):
    return ex.ExactCorpus(kind, LD, N, B, seed=5)


def _changed(a, b):
    """Score tables differ (-inf == -inf is no change)."""
    return ~((a == b) | (np.isneginf(a) & np.isneginf(b)))


def _three_term(c, dtype, dperm=None, rperm=None):
    """(hi + lo).qhi + hi.qlo, max over the scoring rows, summed over the 32
    query tokens, evaluated in ``dtype`` with the dims / rows permuted."""
    dperm = np.arange(ex.DIM) if dperm is None else dperm
    rperm = np.arange(c.ld) if rperm is None else rperm
    hi = (c.dhi[:, rperm][:, :, dperm] / ex.ONE).astype(dtype)
    lo = (c.dlo[:, rperm][:, :, dperm] / ex.ONE).astype(dtype)
    qh = (c.qhi[:, :, dperm] / ex.ONE).astype(dtype).reshape(-1, ex.DIM)
    ql = (c.qlo[:, :, dperm] / ex.ONE).astype(dtype).reshape(-1, ex.DIM)
    valid = (rperm[None, :] < c.doclens[:, None])
    hi, lo = hi.reshape(-1, ex.DIM), lo.reshape(-1, ex.DIM)
    d = lo @ qh.T + hi @ ql.T + hi @ qh.T                                  # [N * ld, B * 32]
    assert d.dtype == dtype
    m = np.where(valid[:, :, None], d.reshape(c.N, c.ld, -1), dtype(-np.inf)).max(axis=1)
    return np.ascontiguousarray(m.reshape(c.N, c.B, ex.LQ).sum(axis=2, dtype=dtype).T)


# ---------------------------------------------------------------------------- (a) the reference is exact
@pytest.mark.parametrize("kind", ex.KINDS)
def test_reference_equals_independent_evaluations(kind):
    c = corpus(kind)
    want = c.ref[:, ex.LQ - 1]
    assert np.isneginf(want[:, c.doclens == 0]).all() and np.isfinite(want[:, c.doclens > 0]).all()
    # pure int64 dot products (the table itself came through integer-valued float64)
    assert np.array_equal(c.row_max(qhi=c.qhi[:3], qlo=c.qlo[:3], pure_int=True), c.M[:3])
    # float64 three-term evaluation (lo = 0 for bf16 / mxfp8: the plain dot product)
    assert np.array_equal(_three_term(c, np.float64), want)
    # fp32 under permutations of the dims and of the rows: any order gives the same bits
    rng = np.random.default_rng(11)
    for _ in range(3):
        got = _three_term(c, np.float32, rng.permutation(ex.DIM), rng.permutation(c.ld))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    # one table serves the lq sweep: a prefix of the query is a shorter query
    Q, X = c.queries_f32(), c.docs_f32()
    if kind != "fp32":
        assert np.array_equal(orc.maxsim(Q, X, c.doclens), want)
        for lq in (1, 17, 31):
            assert np.array_equal(orc.maxsim(Q[:2, :lq], X, c.doclens), c.scores(lq, 2).astype(np.float64))
    else:
        hi, lo, _ = orc.split_f32(X)
        assert np.array_equal(hi * ex.ONE, c.dhi) and np.array_equal(lo * ex.ONE, c.dlo)
        qh, ql, _ = orc.split_f32(Q)
        assert np.array_equal(qh * ex.ONE, c.qhi) and np.array_equal(ql * ex.ONE, c.qlo)
        assert 0.08 < (c.dlo[np.arange(LD)[None, :] < c.doclens[:, None]] != 0).mean() < 0.13
        assert ((c.qhi * c.qlo).sum(axis=2) != 0).all()
        # the full product differs from the three-term sum only by lo.qlo, below 2^-16 per 32 tokens
        full = orc.maxsim(Q, X, c.doclens)
        fin = np.isfinite(want)
        assert np.abs(full[fin] - want[fin]).max() < 2.0 ** -16


def test_bf16_values_are_bf16():
    c = corpus("bf16")
    for x in (c.docs_f32(), c.queries_f32()):
        assert np.array_equal(orc.bf16_round(x), x)
    assert not c.dlo.any() and not c.qlo.any()


def test_mxfp8_is_lossless_and_its_scale_bytes_vary():
    c = corpus("mxfp8")
    X, Q = c.docs_f32(), c.queries_f32()
    sub = np.r_[0:40, np.nonzero(c.doclens < 8)[0]]                        # the quantizer restatement is slow
    for x, xi in ((X[sub], c.dhi[sub]), (Q, c.qhi)):
        assert np.array_equal(orc.bf16_round(x), x)
        q, sc = orc.mxfp8_quantize(x)
        assert np.array_equal(orc.mxfp8_dequant(q, sc), x.astype(np.float64))
        assert np.array_equal(sc.astype(np.int64) - 127, ex.scale_exp(xi))
    q, sc = orc.mxfp8_quantize(X[sub])
    qq, qs = orc.mxfp8_quantize(Q)
    deq = orc.mxfp8_dequant(q, sc)
    assert np.array_equal(orc.maxsim(orc.mxfp8_dequant(qq, qs), deq, c.doclens[sub]), c.ref[:, ex.LQ - 1][:, sub])
    e = ex.scale_exp(c.dhi)                                                # [N, ld, 2]
    scoring = np.arange(LD)[None, :] < c.doclens[:, None]
    assert len(np.unique(e[scoring])) >= 3
    assert (e[..., 0] != e[..., 1])[scoring].mean() >= 0.25
    nxt = (e[:, 1:] != e[:, :-1]).any(axis=2)
    assert nxt[scoring[:, 1:]].mean() >= 0.25                              # neighbouring tokens
    eq = ex.scale_exp(c.qhi)
    assert len(np.unique(eq)) >= 2 and (eq[..., 0] != eq[..., 1]).mean() >= 0.25
    assert (eq[:, 1:] != eq[:, :-1]).any(axis=2).mean() >= 0.25
    fin = c.M > ex.NEG
    assert np.abs(c.M[fin]).max() <= 16 << 32 and not (c.M[fin] % (1 << 21)).any()   # |dot| <= 16, multiples of 2^-11


# ---------------------------------------------------------------------------- (b) the layout
@pytest.mark.parametrize("ld,n", [(128, 176), (256, 176), (512, 160), (1024, 160)])
def test_required_lengths_slots_planted_and_padding_rows(ld, n):
    c = ex.ExactCorpus("bf16", ld, n, 4, seed=2)
    d = ex.ExactCorpus("bf16", ld, n, 4, seed=2)
    assert np.array_equal(c.dhi, d.dhi) and np.array_equal(c.doclens, d.doclens) and np.array_equal(c.M, d.M)
    assert set(ex.special_doclens(ld)) <= set(c.doclens.tolist())
    assert {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128} <= set(ex.special_doclens(ld))
    if ld > 128:
        assert {129, ld - 129, ld - 128, ld - 1, ld} <= set(ex.special_doclens(ld))
    assert set((c.doclens % 16).tolist()) == set(range(16))
    assert set(c.slots[c.slots >= 0].tolist()) == set(range(ld))
    assert c.P == ld // 128
    for i in range(n):
        L = int(c.doclens[i])
        s = c.slots[i][c.slots[i] >= 0]
        assert len(s) == min(c.P, L) and len(set(s.tolist())) == len(s) and (s < L).all()
        for m, t in enumerate(s):
            assert np.array_equal(c.dhi[i, t], c.qhi[c.qb[i], c.qj[i, m]])
        assert (c.dhi[i, L:] == 2 * c.qhi[c.qb[i], c.qj[i, 0]]).all()
    for small in (1, 2, 4):                                                # small batches own planted rows too
        assert (c.qb < small).mean() >= 0.2
    with pytest.raises(ValueError):
        ex.ExactCorpus("bf16", ld, 40, 4, seed=2)


# ---------------------------------------------------------------------------- (c) the mutants
@pytest.mark.parametrize("kind", ex.KINDS)
def test_row_padding_and_query_token_mutants_change_scores(kind):
    c = corpus(kind)
    i = np.arange(c.N)
    own = c.M[c.qb[:, None], c.qj, i[:, None]]                             # [N, P] the planted tokens' maxima
    # drop row t, for every t: the doc planted at t loses its token's maximum
    seen = set()
    for m in range(c.P):
        has = c.slots[:, m] >= 0
        Mm = c.row_max(skip_row=c.slots[:, m])
        assert (Mm[c.qb, c.qj[:, m], i] < own[:, m])[has].all()
        assert _changed(ex.prefix_scores(Mm, c.doclens), c.ref)[c.qb, ex.LQ - 1, i][has].all()
        seen |= set(c.slots[has, m].tolist())
    assert seen == set(range(c.ld))
    # read the first padding row: query qb[i]'s score of doc i goes up (an empty doc stops being -inf)
    short = c.doclens < c.ld
    Mp = c.row_max(doclens=np.minimum(c.doclens + 1, c.ld))
    assert (Mp[c.qb, c.qj[:, 0], i] > own[:, 0])[short & (c.doclens > 0)].all()
    sp = ex.prefix_scores(Mp, np.minimum(c.doclens + 1, c.ld))
    assert (sp[c.qb, ex.LQ - 1, i] > c.ref[c.qb, ex.LQ - 1, i])[short].all() and short.sum() >= c.N // 2
    # drop query token lq - 1 / include token lq: every token moves a score of its query
    full = c.doclens > 0
    assert (c.M[:, :, full] != 0).any(axis=2).all()
    for lq in range(1, ex.LQ):
        assert _changed(c.ref[:, lq - 1], c.ref[:, lq]).any(axis=1).all()
        if lq > 1:
            assert _changed(c.ref[:, lq - 1], c.ref[:, lq - 2]).any(axis=1).all()


def test_residual_mutants_change_scores():
    c = corpus("fp32")
    full = c.doclens > 0
    no_lo = ex.prefix_scores(c.row_max(dlo=np.zeros_like(c.dlo)), c.doclens)
    assert _changed(no_lo, c.ref)[:, ex.LQ - 1].any(axis=0)[full].all()     # every doc
    i = np.nonzero(full)[0]
    assert _changed(no_lo, c.ref)[c.qb[i], :, i].any(axis=1).all()          # ... through its planted query, at some lq
    no_qlo = ex.prefix_scores(c.row_max(qlo=np.zeros_like(c.qlo)), c.doclens)
    assert _changed(no_qlo, c.ref)[:, ex.LQ - 1].any(axis=1).all()          # every query
    assert _changed(no_qlo, c.ref)[:, 0].any(axis=1).all()                  # ... already at lq = 1


def test_scale_byte_mutants_change_scores():
    c = corpus("mxfp8")
    scoring = np.arange(LD)[None, :] < c.doclens[:, None]
    e = ex.scale_exp(c.dhi)                                                # [N, ld, 2]
    last = c.ref[:, ex.LQ - 1]

    def docs_with(e_read):
        s = ex.prefix_scores(c.row_max(dhi=ex.rescale(c.dhi, e, e_read)), c.doclens)[:, ex.LQ - 1]
        touched = ((e_read != e).any(axis=2) & scoring).any(axis=1)
        return _changed(s, last).any(axis=0), touched

    # a token's two scale bytes swapped
    changed, touched = docs_with(e[..., ::-1])
    assert changed[touched].all() and touched.sum() >= 0.75 * (c.doclens > 0).sum()
    # the previous token's scale bytes (row 0 reads the previous doc's last row)
    changed, touched = docs_with(np.roll(e.reshape(-1, 2), 1, axis=0).reshape(e.shape))
    assert changed[touched].all() and touched.sum() >= 0.75 * (c.doclens > 0).sum()
    # the previous query token's scale bytes
    eq = ex.scale_exp(c.qhi)
    eq_read = np.roll(eq, 1, axis=1)
    s = ex.prefix_scores(c.row_max(qhi=ex.rescale(c.qhi, eq, eq_read)), c.doclens)[:, ex.LQ - 1]
    assert (eq_read != eq).any(axis=(1, 2)).all() and _changed(s, last).any(axis=1).all()


@pytest.mark.parametrize("kind", ex.KINDS)
def test_dropped_dim_slice_changes_scores(kind):
    c = corpus(kind)
    nb = 8
    for s in range(ex.DIM // 16):
        qh, ql = c.qhi[:nb].copy(), c.qlo[:nb].copy()
        qh[:, :, 16 * s:16 * s + 16] = 0
        ql[:, :, 16 * s:16 * s + 16] = 0
        Ms = c.row_max(qhi=qh, qlo=ql)
        uses = (c.qhi[:nb, :, 16 * s:16 * s + 16] != 0).any(axis=2)        # [nb, 32]
        assert uses.sum() >= nb * ex.LQ // 2
        assert (Ms != c.M[:nb]).any(axis=2)[uses].all()
        # and the docs planted with such a token lose exactly that slice of |q|^2
        i = np.nonzero((c.qb < nb) & (c.doclens > 0))[0]
        u = uses[c.qb[i], c.qj[i, 0]]
        assert (Ms[c.qb[i], c.qj[i, 0], i] < c.M[c.qb[i], c.qj[i, 0], i])[u].all()
