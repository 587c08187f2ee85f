"""GPU: adversarial tests of the faithful search's band certificate.

The fp32-faithful search is exact only because |T - F| <= beta(q) for every
doc (include/colbert_mi355x.h under cbv2_search_f32), so the bands T >= lb -
beta and T >= T_k - 2 beta hold the faithful top-k.  On random unit vectors
|T - F| / beta is 0.03 and any threshold passes; here the corpora come from
tests/_adversarial.py, where |T - F| / beta reaches 0.82 .. 0.88: per query
the bf16 top-10 are ten anti-aligned decoys and the faithful top-10 are ten
aligned hidden docs 1.35 .. 1.50 beta below T_k and 0.525 .. 0.64 beta below
lb.  A search returns the hidden docs only if its band reaches as far down as
documented: half of beta, T_k - beta, or a beta without its E term lose them.

Every test runs _adversarial.check_preconditions on the CPU first, with E and
M from the index's own bounds, so none can go vacuous.  The expectation is
always the oracle's top-k SELECTION of the GPU's own cbv2_score_f32 matrix
(bit for bit) plus "the ids are exactly the hidden docs".
"""
import os
import re
import threading

import numpy as np
import pytest
import torch

import _adversarial as adv
from _parity import assert_selection_exact
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.distributed import NativeExchange, loopback_comms
from hybrid_rag_colbertv2_amd.hybrid import OneTripRetriever, rrf_fuse
from hybrid_rag_colbertv2_amd.index import ColbertIndex, merge_topk
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K = 10
N = 600
BMAX = 12
# the handle's defaults (csrc/colbert_mi355x.hip, struct cbv2_index)
DEFAULTS = {_lib.OPT_BAND_LOWER_BOUND: 1, _lib.OPT_BAND_REUSE: 1, _lib.OPT_P1_COLLECT_FUSED: 1, _lib.OPT_BAND_FUSED: 0,
            _lib.OPT_RESCORE_SPLIT: 1, _lib.OPT_BAND_DOC_MAJOR: 0, _lib.OPT_RESCORE_GRID: 0,
            _lib.OPT_BAND_BLOCK_SKIP: 1, _lib.OPT_TOPK_BMAX: 1, _lib.OPT_FOLD_KEYS: 1}

# split_query_kernel rounds up three times: each token's ||q|| and ||q - qhi||
# by kBoundUp, and the sum of the tokens' terms by kBoundUp again, so its beta is
# oracle.band_beta(Q, E, M) * kBoundUp^2 up to fp32 rounding.  Per token: 8
# serial adds + 4 shuffle adds of squares, a square root, 5 multiplies / adds;
# then <= 8 serial + 2 pairwise adds and the last multiply: fewer than 40
# roundings of 2^-24 each, < 2^-18 in all.
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hybrid-rag-colbertv2_amd", "csrc",
                   "colbert_mi355x.hip")
KBOUNDUP = 1.0 + 1.0 / 1024.0
BETA_UP = KBOUNDUP ** 2 * (1 + 2.0 ** -18)
# a threshold lb - beta or T_k - 2 beta is one or two fp32 operations on values
# below 32 (lq <= 32 unit tokens): each rounds by at most ulp(32) / 2 = 1.9e-6
THR_EPS = 4e-6


def test_kboundup_is_what_the_band_size_window_assumes():
    src = open(HIP).read()
    assert re.search(r"constexpr float kBoundUp = 1\.0f \+ 1\.0f / 1024\.0f;", src)
    assert re.search(r"const float nq = sqrtf\(xx\) \* kBoundUp, eq = sqrtf\(rr\) \* kBoundUp;", src)
    assert re.search(r"beta\[b\] = \(\(a\[0\] \+ a\[1\]\) \+ \(a\[2\] \+ a\[3\]\)\) \* kBoundUp;", src)


def _sub(case, B):
    """The first B queries of a case (the other queries' planted docs are fillers to them)."""
    return adv.Case(case.docs, case.doclens, case.Q[:B], case.decoys[:B], case.hidden[:B], case.K, case.groups)


class Corpus:
    def __init__(self, dev, lq):
        self.case = adv.adversarial_case(1000 + lq, N=N, B=BMAX, lq=lq, K=K)
        c = self.case
        self.ix = ColbertIndex.faithful_f32(torch.from_numpy(c.docs).to(dev), torch.from_numpy(c.doclens).to(dev),
                                            id_base=7)
        self.pre = adv.check_preconditions(c, K, bounds=self.ix.bounds)
        self.Q = torch.from_numpy(c.Q).to(dev)


_corpora = {}


@pytest.fixture(scope="module")
def corpus(dev):
    def get(lq):
        if lq not in _corpora:
            _corpora[lq] = Corpus(dev, lq)
        return _corpora[lq]
    yield get
    _corpora.clear()


def _check(ix, Qb, F, hidden, k, band_min=None, id_base=0, search=None):
    """search (default ix.search) == the selection of the GPU's own faithful
    score matrix F, its ids exactly the hidden docs, the band path taken."""
    s, i = (search or (lambda: ix.search(Qb, k)))()
    ids = i.cpu().numpy()
    assert_selection_exact(ids, s.cpu().numpy(), F, k, id_base=id_base)
    for b in range(len(ids)):
        assert set(ids[b].tolist()) == set((hidden[b] + id_base).tolist()), (b, ids[b], hidden[b] + id_base)
    band = ix.last_band.cpu().numpy()
    if band_min is not None:
        assert (band >= band_min).all(), band            # never -1: the band path ran, not the fallback
    return band


SWEEP = [("lower_bound", _lib.OPT_BAND_LOWER_BOUND, (0, 1)), ("reuse", _lib.OPT_BAND_REUSE, (0, 1)),
         ("p1_collect_fused", _lib.OPT_P1_COLLECT_FUSED, (0, 1)), ("band_fused", _lib.OPT_BAND_FUSED, (0, 1)),
         ("rescore_split", _lib.OPT_RESCORE_SPLIT, (0, 1)), ("doc_major", _lib.OPT_BAND_DOC_MAJOR, (0, 1, 2, 3, 4)),
         ("rescore_grid", _lib.OPT_RESCORE_GRID, (7,))]


@pytest.mark.parametrize("B", [1, 3, 12])
@pytest.mark.parametrize("lq", [32, 7])
def test_every_band_path_finds_the_hidden_docs(dev, corpus, lq, B):
    """Each handle option that changes how the band is thresholded, collected
    or rescored, one at a time from the defaults: the two-pass band (lb -
    beta) and the one-pass band (T_k - 2 beta), phase-1 reuse, the fused
    phase-1 + collect, the fused collect + rescore, both rescoring kernels,
    the doc-major modes (B = 12) and a forced rescoring grid; and the full-scan
    fallback (cap = k: status -1)."""
    c = corpus(lq)
    ix, Qb = c.ix, c.Q[:B].contiguous()
    hidden = c.case.hidden[:B]
    F = ix.score(Qb).cpu().numpy()
    # the GPU's faithful scores are the oracle's F within fp32 accumulation, far inside (c)'s 0.10 beta
    fin = np.isfinite(c.pre["F"][:B])
    assert np.abs(F[fin] - c.pre["F"][:B][fin]).max() < 1e-4
    # the inequality itself in the device's arithmetic: the bf16 scan's T within beta of the faithful F
    # for every doc, and within 0.8 .. 1 of it for the planted ones
    T = ColbertIndex(ix.tokens, ix.doclens).score(Qb.bfloat16()).cpu().numpy()
    dev_TF = np.zeros(F.shape)
    dev_TF[fin] = np.abs(T[fin].astype(np.float64) - F[fin])
    ratio = dev_TF.max(axis=1) / c.pre["beta"][:B]
    assert (ratio >= 0.8).all() and (ratio <= 1.0).all(), ratio
    bands = {}
    for name, opt, values in SWEEP:
        if name == "doc_major" and B <= 8:
            continue
        for v in values:
            ix.set_option(opt, v)
            try:
                bands[(name, v)] = _check(ix, Qb, F, hidden, K, band_min=2 * K, id_base=7)
            finally:
                ix.set_option(opt, DEFAULTS[opt])
    # every band here is the 10 decoys + the 10 hidden docs, the fillers far below
    assert all((b == 2 * K).all() for b in bands.values()), bands
    _check(ix, Qb, F, hidden, K, id_base=7, search=lambda: ix._search_f32(Qb, B, lq, K, cap=K))
    assert (ix.last_band.cpu().numpy() == -1).all()


# --------------------------------------------------------------------------- block keys (n > 65,536)
N_BIG = 65_536 + 3 * 64 + 37      # not a multiple of the 64-doc block
STRIDE = N_BIG // N


def _big_index(dev, case, dense):
    """N_BIG docs: random unit fillers generated on the device (ragged with
    empty docs, or all 128 tokens when ``dense``), the case's planted docs at
    id * STRIDE + 5.  -> (index, the planted docs' ids in the case)."""
    g = torch.Generator(device=dev).manual_seed(11 + int(dense))
    x = torch.empty((N_BIG, 128, 128), dtype=torch.float32, device=dev)
    for a in range(0, N_BIG, 8192):
        t = torch.randn((min(8192, N_BIG - a), 128, 128), generator=g, device=dev)
        x[a:a + 8192] = t / t.norm(dim=-1, keepdim=True)
    if dense:
        dl = torch.full((N_BIG,), 128, dtype=torch.int32, device=dev)
    else:
        dl = torch.randint(1, 129, (N_BIG,), generator=g, device=dev, dtype=torch.int32)
        dl[::97] = 0
    small = adv.planted_ids(case)
    big = torch.from_numpy(small * STRIDE + 5).to(dev)
    x[big] = torch.from_numpy(case.docs[small]).to(dev)
    dl[big] = 128
    ix = ColbertIndex.faithful_f32(x, dl, id_base=3)
    del x
    torch.cuda.empty_cache()
    return ix, small


def _big_preconditions(dev, ix, case, small, B):
    """(a)-(d) on the planted docs by the CPU oracle with the index's bounds;
    (e) -- every filler below T_k - 2 beta -- on the GPU's own bf16 score
    matrix.  -> the faithful score matrix of the first B queries."""
    sub = _sub(case, B)
    pre = adv.check_preconditions(sub, K, bounds=ix.bounds, docs_subset=small)
    Q = torch.from_numpy(sub.Q).to(dev)
    T = ColbertIndex(ix.tokens, ix.doclens).score(Q.bfloat16()).cpu().numpy()
    filler = np.ones(N_BIG, bool)
    filler[small * STRIDE + 5] = False
    assert (T[:, filler].max(axis=1) < pre["Tk"] - 2 * pre["beta"]).all()
    np.testing.assert_allclose(T[:, small * STRIDE + 5], pre["T"], atol=1e-4, rtol=0)
    return Q, ix.score(Q).cpu().numpy()


@pytest.fixture(scope="module")
def big(dev, corpus):
    case = corpus(32).case
    ix, small = _big_index(dev, case, dense=False)
    yield ix, case, small
    del ix
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1, 12])
def test_block_keys_keep_the_hidden_docs(dev, big, B):
    """Past 65,536 docs the block-max top-k leaves 64-doc block keys and the
    band collect skips the blocks whose key is below uthr0 = T_k - 2 beta
    (block_skip), with and without the block-max top-k itself: the hidden
    docs' blocks hold nothing but fillers far below, so a uthr0 taken too high
    skips them."""
    ix, case, small = big
    assert not ix.dense_docs
    Q, F = _big_preconditions(dev, ix, case, small, B)
    hidden = case.hidden[:B] * STRIDE + 5
    for skip in (0, 1):
        for bmax in (0, 1):
            for lower in (1, 0):
                ix.set_option(_lib.OPT_BAND_BLOCK_SKIP, skip)
                ix.set_option(_lib.OPT_TOPK_BMAX, bmax)
                ix.set_option(_lib.OPT_BAND_LOWER_BOUND, lower)
                try:
                    band = _check(ix, Q, F, hidden, K, band_min=2 * K, id_base=3)
                finally:
                    for o in (_lib.OPT_BAND_BLOCK_SKIP, _lib.OPT_TOPK_BMAX, _lib.OPT_BAND_LOWER_BOUND):
                        ix.set_option(o, DEFAULTS[o])
                assert (band == 2 * K).all(), (skip, bmax, lower, band)


def test_folded_block_keys_keep_the_hidden_docs(dev, corpus):
    """The dense-doc variant (every doc 128 tokens), B <= 4: the 4 x 1 scan folds
    the block keys in by atomic max (fold_keys) or a separate pass computes them."""
    case = corpus(32).case
    ix, small = _big_index(dev, case, dense=True)
    assert ix.dense_docs
    for B in (1, 4):
        Q, F = _big_preconditions(dev, ix, case, small, B)
        hidden = case.hidden[:B] * STRIDE + 5
        for fold in (0, 1, 1):                     # twice in a row: the keys are zeroed per call
            ix.set_option(_lib.OPT_FOLD_KEYS, fold)
            try:
                band = _check(ix, Q, F, hidden, K, band_min=2 * K, id_base=3)
            finally:
                ix.set_option(_lib.OPT_FOLD_KEYS, DEFAULTS[_lib.OPT_FOLD_KEYS])
            assert (band == 2 * K).all(), (B, fold, band)
    del ix
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------- band size pins beta
def _graded_corpus(seed, n, B, lq):
    """n docs of lq tokens: doc j copies the tokens of query (j mod B), each
    moved by sigma_j times a random unit vector and renormalised, sigma_j
    graded so that T falls about evenly from lq to lq - 0.4 (three to five
    betas, past both bands' thresholds): n / (0.4 B) docs per unit of T and
    query, so every 5 % of beta holds about ten docs."""
    rng = np.random.default_rng(seed)
    Q = adv.rand_unit(rng, B, lq, 128)
    docs = np.zeros((n, 128, 128), np.float32)
    sigma = np.sqrt(2 * rng.uniform(0.0, 0.4, n) / lq).astype(np.float32)
    x = Q[np.arange(n) % B] + sigma[:, None, None] * adv.rand_unit(rng, n, lq, 128)
    docs[:, :lq] = x / np.linalg.norm(x, axis=-1, keepdims=True)
    return docs, np.full(n, lq, np.int32), Q


@pytest.mark.parametrize("B,lq", [(3, 32), (12, 20)])
def test_band_size_pins_beta_from_both_sides(dev, B, lq):
    """The band size is the only view of the kernel's beta.  With T the plain
    bf16 index's score matrix, lb the least of the GPU's faithful scores at T's
    top-k and beta_o = oracle.band_beta(Q, *ix.bounds):

        count(T >= lb - beta_o)  <=  last_band  <=  count(T >= lb - beta_o u)

    with u = kBoundUp^2 (1 + 2^-18), the kernel's documented round-ups (BETA_UP
    above), and the same for the one-pass band T_k - 2 beta.  The thresholds
    move by THR_EPS for their own fp32 rounding.  The corpus is dense near the
    thresholds, so the counts at 0.95 beta_o and 1.05 beta_o fall outside the
    window: a beta 5 % off fails.

    Measured on an MI355X: the search's scan is bit-identical to the plain
    bf16 index's scores as far as this shows (no widening needed); the window
    [lo, hi] holds 0 .. 4 docs (band sizes 211 .. 1447) and last_band == hi in
    every row -- the kernel's beta is beta_o kBoundUp^2 -- while -5 % / +5 % of
    beta move the count by 7 .. 81 docs below lo / 3 .. 74 above hi."""
    n, k = 2000 * B if B <= 3 else 1000 * B, K
    docs, doclens, Qn = _graded_corpus(77 + B, n, B, lq)
    ix = ColbertIndex.faithful_f32(torch.from_numpy(docs).to(dev), torch.from_numpy(doclens).to(dev))
    Q = torch.from_numpy(Qn).to(dev)
    T = ColbertIndex(ix.tokens, ix.doclens).score(Q.bfloat16()).cpu().numpy().astype(np.float64)
    F = ix.score(Q).cpu().numpy().astype(np.float64)
    beta_o = orc.band_beta(Qn, *ix.bounds)
    Ts, Ti = orc.topk(T, k)
    lb = np.array([F[b, Ti[b]].min() for b in range(B)])
    Tk = Ts[:, -1]

    def count(base, width):
        return np.array([(T[b] >= base[b] - width[b]).sum() for b in range(B)])

    for lower, base, mult in ((1, lb, 1.0), (0, Tk, 2.0)):
        ix.set_option(_lib.OPT_BAND_LOWER_BOUND, lower)
        try:
            s, i = ix.search(Q, k)
        finally:
            ix.set_option(_lib.OPT_BAND_LOWER_BOUND, 1)
        band = ix.last_band.cpu().numpy()
        assert_selection_exact(i.cpu().numpy(), s.cpu().numpy(), F.astype(np.float32), k)
        lo = count(base, mult * beta_o - THR_EPS)
        hi = count(base, mult * beta_o * BETA_UP + THR_EPS)
        near = count(base, mult * beta_o * BETA_UP + 1e-5) - count(base, mult * beta_o - 1e-5)
        print(f"lower_bound={lower} band={band} lo={lo} hi={hi} within 1e-5 of the window={near} "
              f"-5%={count(base, 0.95 * mult * beta_o)} +5%={count(base, 1.05 * mult * beta_o)}")
        assert (band > 0).all() and (lo <= band).all() and (band <= hi).all(), (lower, lo, band, hi)
        # the window discriminates: 5 % of beta either way leaves it
        assert (count(base, 0.95 * mult * beta_o) < lo).all()
        assert (count(base, 1.05 * mult * beta_o) > hi).all()


# --------------------------------------------------------------------------- caller-supplied / exchanged bounds
def _run_ranks(G, fn):
    out, errs = [None] * G, []

    def body(r):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                out[r] = fn(r)
            s.synchronize()
        except BaseException as e:  # noqa: BLE001 - re-raised on the main thread
            errs.append((r, e))

    ts = [threading.Thread(target=body, args=(r,)) for r in range(G)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "a rank thread hung"
    if errs:
        raise errs[0][1]
    return out


@pytest.mark.parametrize("B", [1, 5, 12])
def test_global_lower_bounds_keep_the_hidden_docs(dev, B):
    """Two shards, each with 10 decoys and 10 hidden docs per query.  The
    global bound -- the k-th largest of the gathered faithful scores of both
    shards' bf16 top-k (decoys all) -- is higher than either shard's own, so
    each shard's band lb_global - beta is at its narrowest; the merged top-10
    are hidden docs of both shards, equal to the unsharded search bit for bit:
    through search(lb_reduce=) with the k-th of the gathered lists, and through
    the in-ABI exchange at G = 2 on the loopback communicator."""
    case = adv.adversarial_case(2000 + B, N=N, B=B, lq=32, K=K, groups=2)
    n = N // 2
    docs, doclens = torch.from_numpy(case.docs).to(dev), torch.from_numpy(case.doclens).to(dev)
    Q = torch.from_numpy(case.Q).to(dev)
    full = ColbertIndex.faithful_f32(docs, doclens)
    shards = [ColbertIndex.faithful_f32(docs[a:a + n].contiguous(), doclens[a:a + n].contiguous(), id_base=a)
              for a in (0, n)]
    for g, sh in enumerate(shards):                   # each shard alone is a full adversarial case
        adv.check_preconditions(case.shard(g), K, bounds=sh.bounds)
    fs, fi = full.search(Q, K)
    assert (full.last_band >= 2 * K).all()
    assert_selection_exact(fi.cpu().numpy(), fs.cpu().numpy(), full.score(Q).cpu().numpy(), K)
    for b in range(B):
        got = set(fi[b].tolist())
        assert got <= set(case.hidden[b].tolist())
        assert got & set(case.hidden[b, :K].tolist()) and got & set(case.hidden[b, K:].tolist())   # of both shards

    fks = []

    def own(fk):
        fks.append(fk.clone())
        return fk.min(dim=1).values
    for sh in shards:
        sh.search(Q, K, lb_reduce=own)
    glob = torch.cat(fks, dim=1).topk(K, dim=1).values[:, K - 1]
    assert (glob > torch.stack([f.min(dim=1).values for f in fks]).max(dim=0).values).all()
    lists = []
    for sh in shards:
        lists.append(sh.search(Q, K, lb_reduce=lambda fk: glob))
        assert (sh.last_band >= K).all(), sh.last_band       # the band path, not the fallback
    ms, mi = merge_topk(torch.stack([x[0] for x in lists]), torch.stack([x[1] for x in lists]), K)
    assert torch.equal(mi, fi) and torch.equal(ms, fs)

    comms = loopback_comms(2)
    nxs = [NativeExchange(shards[r], comm=comms[r]) for r in range(2)]
    outs = _run_ranks(2, lambda r: [x.cpu() for x in nxs[r].search(Q, K)[:2]])
    torch.cuda.synchronize()
    for r, (s, i) in enumerate(outs):
        assert torch.equal(i, fi.cpu()) and torch.equal(s, fs.cpu()), f"rank {r} differs from the unsharded search"
    del nxs


# --------------------------------------------------------------------------- one-trip retrieve
@pytest.mark.parametrize("B", [1, 5])
def test_one_trip_retrieve_finds_the_hidden_docs(dev, corpus, B):
    """cbv2_retrieve_begin / _finish with an empty stage-1 list: the fused
    candidates are the faithful search's top-k, so the final top-k are the
    hidden docs, equal to search + RRF + rerank called one by one."""
    c = corpus(32)
    ix, Qb = c.ix, c.Q[:B].contiguous()
    one = OneTripRetriever(ix, colbert_k=K, fused=K, final_k=K)
    got = [x.cpu() for x in one(Qb, None)]
    _, ids = ix.search(Qb, K)
    cand = rrf_fuse(np.zeros((B, 0), np.int32), ids.cpu().numpy(), rrf_k=60, C=K)
    want = [x.cpu() for x in ix.rerank(Qb, torch.from_numpy(cand).to(dev), K)]
    for g, w, name in zip(got, want, ("scores", "ids", "positions")):
        assert torch.equal(g, w), name
    for b in range(B):
        assert set(got[1][b].tolist()) == set((c.case.hidden[b] + 7).tolist())
    goth = one(Qb, None, host=True)
    for g, w in zip(goth, want):
        assert np.array_equal(g, w.numpy())


# --------------------------------------------------------------------------- outlier norms
@pytest.mark.parametrize("B", [2, 12])
def test_outlier_norms_search_equals_own_scores(dev, B):
    """Token norms over 2^-6 .. 2^6 and one outlier row (norm 96) that sets M:
    beta is loose (E and M are corpus maxima), bands are wide or overflow the
    cap -- whatever status the rows report, the search equals the selection of
    its own faithful score matrix, which matches the float64 oracle within
    2^-15 M sum_i ||q_i||."""
    g = torch.Generator().manual_seed(40 + B)
    n, k = 3000, K
    docs = torch.randn(n, 128, 128, generator=g)
    docs = docs / docs.norm(dim=-1, keepdim=True) * torch.exp2(12 * torch.rand(n, 128, 1, generator=g) - 6)
    docs[7, 3] = docs[7, 3] / docs[7, 3].norm() * 96.0
    doclens = torch.randint(0, 129, (n,), generator=g, dtype=torch.int32)
    doclens[7] = 128
    Q = torch.randn(B, 32, 128, generator=g)
    Q = Q / Q.norm(dim=-1, keepdim=True) * torch.exp2(4 * torch.rand(B, 32, 1, generator=g) - 2)
    ix = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev), id_base=2)
    assert 95.9 < ix.bounds[1] < 96.2
    F = ix.score(Q.to(dev)).cpu().numpy()
    exact = orc.maxsim(Q.numpy(), docs.numpy(), doclens.numpy())
    fin = np.isfinite(exact)
    # per query token and doc row the faithful product drops lo . qlo (<= 2^-18 ||q|| ||d||), rounds lo to bf16
    # (<= 2^-18 again) and accumulates in fp32 (128 terms, <= 2^-17 ||q|| ||d||): 2^-15 ||q|| M covers them
    tol = 2.0 ** -15 * ix.bounds[1] * Q.norm(dim=-1).sum(dim=1).numpy()
    assert (np.abs(F[fin] - exact[fin]) <= np.broadcast_to(tol[:, None], F.shape)[fin]).all()
    assert np.array_equal(np.isneginf(F), np.isneginf(exact))
    for lower in (1, 0):
        ix.set_option(_lib.OPT_BAND_LOWER_BOUND, lower)
        s, i = ix.search(Q.to(dev), k)
        print("outlier norms: lower_bound", lower, "status", ix.last_band.cpu().numpy())
        assert_selection_exact(i.cpu().numpy(), s.cpu().numpy(), F, k, id_base=2)
