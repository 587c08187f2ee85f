"""GPU: the band of the filtered faithful search (cbv2_search_filtered_f32,
CBV2_OPT_FILTER_BAND) -- the bf16 subset scan of hi, the band over the compact
row, its rescoring and select, the device-side recomputation of overflowing
rows -- against the pair path (one faithful score per (query, allowed doc)),
which it must equal bit for bit, and against the float64 oracle.

``last_band`` in [k, m] under FILTER_BAND_ON is the assertion that shows the
band ran (the pair path reports -1 everywhere).  The helpers make_case,
filter_ref, check_search and _bits are those of tests/test_gpu_filter.py.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _adversarial as adv
from _arena import Arena
from _parity import assert_ranking_consistent
from conftest import GOLDEN
from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig, _lib
from hybrid_rag_colbertv2_amd.bm25 import HostBM25
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore, DualIndexer, HybridRetriever
from hybrid_rag_colbertv2_amd.index import BAND_CAP, ColbertIndex, _stream_ptr, pack_allow
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ATOL32 = 1e-4
ON, OFF = _lib.FILTER_BAND_ON, _lib.FILTER_BAND_OFF


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def rand_unit(g, *shape):
    x = torch.randn(*shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def make_case(seed, N, B, lq, density, ld=128, empties=True):
    """Random unit tokens (fp32), ragged doclens with some empty docs, and an
    allowed set of max(1, round(density * N)) docs holding at least one empty doc."""
    g = torch.Generator().manual_seed(seed)
    docs = rand_unit(g, N, ld, 128)
    doclens = torch.randint(1, ld + 1, (N,), generator=g, dtype=torch.int32)
    Q = rand_unit(g, B, lq, 128)
    rng = np.random.default_rng(seed)
    m = max(1, int(round(density * N)))
    E = np.sort(rng.choice(N, m, replace=False))
    if not empties:
        return docs, doclens, Q, E
    doclens[torch.from_numpy(rng.choice(N, max(1, N // 50), replace=False))] = 0
    if m >= 3:
        doclens[int(E[m // 2])] = 0          # an allowed empty doc
        doclens[int(E[0])] = 128 if ld == 128 else ld
    return docs, doclens, Q, E


def filter_ref(cols, E, k, id_base):
    """The oracle's top-k of the allowed columns -> (scores [B, k], global ids [B, k])."""
    rs, ri = orc.topk(cols, k)
    ids = np.where(ri >= 0, id_base + E[np.clip(ri, 0, None)] if len(E) else -1, -1)
    return rs, ids


def check_search(ix, Qd, flt, E, k, ref_cols, tol, scorer="maxsim"):
    """ids and score bits equal the selection on the library's own unfiltered
    matrix; scores within tol of the float64 oracle; the ranking consistent.
    Returns (scores, ids, last_band) as numpy."""
    s, i = ix.search(Qd, k, scorer=scorer, filter=flt)
    band = ix.last_band.cpu().numpy()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    M = ix.score(Qd, scorer=scorer).cpu().numpy()
    rs, rid = filter_ref(M[:, E], E, k, ix.id_base)
    assert np.array_equal(i, rid), "ids differ from the selection on the library's own unfiltered scores"
    assert np.array_equal(_bits(s), _bits(rs)), "score bits differ from the unfiltered scorer's"
    pos = np.where(i >= 0, np.searchsorted(E, np.clip(i - ix.id_base, 0, None)), -1)
    for b in range(i.shape[0]):
        live = pos[b] >= 0
        want = np.asarray(ref_cols, np.float64)[b, pos[b][live]]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(s[b][live]), fin)
        np.testing.assert_allclose(s[b][live][fin], want[fin], atol=tol, rtol=0)
        assert np.isneginf(s[b][~live]).all()
    assert_ranking_consistent(pos, ref_cols, tol)
    return s, i, band


def faithful(dev, docs, doclens, id_base=0):
    ix = ColbertIndex.faithful_f32(torch.as_tensor(docs).to(dev), torch.as_tensor(doclens).to(dev), id_base=id_base)
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_SUBSET)
    return ix


def run(ix, Qd, k, flt, band, cap=BAND_CAP):
    """One filtered search under CBV2_OPT_FILTER_BAND = band -> (score bits, ids, status)."""
    ix.set_option(_lib.OPT_FILTER_BAND, band)
    s, i = ix._search_filtered(Qd, k, "maxsim", flt, cap=cap)
    st = ix.last_band.cpu().numpy()
    return _bits(s.cpu().numpy()), i.cpu().numpy(), st


def assert_same(a, b):
    assert np.array_equal(a[1], b[1]), "ids differ between the band and the pair path"
    assert np.array_equal(a[0], b[0]), "score bits differ between the band and the pair path"


# ------------------------------------------------------------------ bit identity
CASES = [(300, 1, 32, 20, 0.5), (300, 2, 7, 20, 0.5), (1000, 3, 32, 10, 0.3), (777, 9, 32, 50, 0.2),
         (1000, 17, 20, 100, 0.5), (2500, 40, 1, 100, 0.9), (129, 33, 32, 128, 1.0), (129, 5, 32, 129, 1.0),
         (300, 5, 32, 50, 0.1)]


@pytest.mark.parametrize("N,B,lq,k,density", CASES)
def test_band_equals_pair_path(dev, N, B, lq, k, density):
    docs, doclens, Q, E = make_case(N + B + 2, N, B, lq, density)
    ix = faithful(dev, docs, doclens, id_base=1000 if N == 777 else 0)
    flt = ix.filter(ids=E + ix.id_base)
    m, Qd = len(E), Q.to(dev)
    assert flt.count == m
    ix.set_option(_lib.OPT_FILTER_BAND, ON)
    ref = orc.maxsim(Q.numpy(), docs[E].numpy(), doclens[E].numpy())
    s, i, band = check_search(ix, Qd, flt, E, k, ref, ATOL32)
    print("band sizes", (N, B, lq, k, m), band.tolist())
    if k < m:
        assert ((band >= k) & (band <= m)).all(), band       # the band ran and was certified
    else:
        assert (band == -1).all(), band                      # nothing to bound: the pair path
    off = run(ix, Qd, k, flt, OFF)
    assert (off[2] == -1).all(), off[2]
    assert_same((_bits(s), i), off)
    if k >= m >= 3:          # the allowed empty doc keeps its id, after every finite score
        assert all(ix.id_base + int(E[m // 2]) in row for row in i)


def test_all_empty_topk(dev):
    """Fewer than k allowed docs have tokens: lb = -inf, the band is the whole list."""
    N, B, k = 400, 3, 10
    docs, doclens, Q, E = make_case(11, N, B, 32, 0.25, empties=False)
    doclens[torch.from_numpy(E[5:])] = 0
    ix = faithful(dev, docs, doclens)
    flt, Qd, m = ix.filter(ids=E), Q.to(dev), len(E)
    off = run(ix, Qd, k, flt, OFF)
    on = run(ix, Qd, k, flt, ON)
    assert_same(on, off)
    assert (on[2] == m).all(), on[2]
    assert np.isneginf(on[0].view(np.float32)[:, 5:]).all() and (on[1][:, 5:] >= 0).all()
    small = run(ix, Qd, k, flt, ON, cap=2 * k)            # m > cap: every row overflows
    assert_same(small, off)
    assert (small[2] == -1).all(), small[2]


@pytest.mark.parametrize("B", [1, 40])
def test_whole_list_band_past_the_lds_list(dev, B):
    """The 2500-doc shape with fewer than k allowed docs holding tokens: lb =
    -inf, so the band is all m = 2250 allowed docs -- one collect workgroup per
    row (m < 8192) meets more than its 2048-entry LDS list holds and appends the
    rest to the global list directly.  Every allowed doc must come out once."""
    N, lq, k = 2500, 1, 100
    docs, doclens, Q, E = make_case(71 + B, N, B, lq, 0.9, empties=False)
    m = len(E)
    assert m == 2250 > 2048
    live = E[np.random.default_rng(B).choice(m, 60, replace=False)]      # 60 < k docs keep their tokens
    doclens[torch.from_numpy(E)] = 0
    doclens[torch.from_numpy(live)] = 128
    ix = faithful(dev, docs, doclens)
    flt, Qd = ix.filter(ids=E), Q.to(dev)
    off = run(ix, Qd, k, flt, OFF)
    on = run(ix, Qd, k, flt, ON)
    assert (on[2] == m).all(), on[2]                      # no hit lost, none counted twice
    assert_same(on, off)
    assert all(set(row[:60].tolist()) == set(live.tolist()) for row in on[1])
    assert np.isneginf(on[0].view(np.float32)[:, 60:]).all()
    assert all(np.array_equal(row[60:], np.setdiff1d(E, live)[:k - 60]) for row in on[1])   # empty docs: id ascending
    for cap in (2100, 2 * k):                             # m > cap: every row overflows; cap 2100 > the LDS list
        small = run(ix, Qd, k, flt, ON, cap=cap)
        assert (small[2] == -1).all(), (cap, small[2])
        assert_same(small, off)


@pytest.mark.parametrize("B", [1, 40])
def test_whole_list_band_with_finite_scores(dev, B):
    """The same m = 2250 > 2048 with every allowed doc scoring: one DISALLOWED
    doc of norm 1000 raises the index's norm bound, so beta exceeds the whole
    score range and the band {T >= lb - beta} is the whole list with a finite
    lb.  The exact top-k then depends on docs the collect put past its LDS list."""
    N, lq, k = 2500, 1, 100
    docs, doclens, Q, E = make_case(81 + B, N, B, lq, 0.9, empties=False)
    m = len(E)
    big = int(np.setdiff1d(np.arange(N), E)[0])
    docs[big] *= 1000.0
    doclens[big] = 128
    ix = faithful(dev, docs, doclens)
    assert ix.bounds[1] > 900.0
    flt, Qd = ix.filter(ids=E), Q.to(dev)
    ref = orc.maxsim(Q.numpy(), docs[E].numpy(), doclens[E].numpy())
    ix.set_option(_lib.OPT_FILTER_BAND, ON)
    s, i, band = check_search(ix, Qd, flt, E, k, ref, ATOL32)
    assert (band == m).all(), band
    assert_same((_bits(s), i), run(ix, Qd, k, flt, OFF))
    small = run(ix, Qd, k, flt, ON, cap=2100)
    assert (small[2] == -1).all(), small[2]
    assert_same(small, (_bits(s), i))


def test_ties_inside_the_band(dev):
    """30 copies of one doc at scattered allowed ids; k = 10 falls inside the group."""
    N, B, lq, k = 500, 3, 32, 10
    docs, doclens, Q, E = make_case(21, N, B, lq, 0.5, empties=False)
    rng = np.random.default_rng(21)
    group = np.sort(rng.choice(E, 30, replace=False))
    docs[int(group[0]), :lq] = Q[0]                       # query 0's best doc by far
    doclens[int(group[0])] = 128
    docs[torch.from_numpy(group)] = docs[int(group[0])].clone()
    doclens[torch.from_numpy(group)] = 128
    ix = faithful(dev, docs, doclens)
    flt, Qd = ix.filter(ids=E), Q.to(dev)
    on, off = run(ix, Qd, k, flt, ON), run(ix, Qd, k, flt, OFF)
    assert_same(on, off)
    assert np.array_equal(on[1][0], group[:k]), (on[1][0], group[:k])     # ids ascending within the tie
    assert len(set(on[0][0].tolist())) == 1
    assert 30 <= on[2][0] <= len(E), on[2]                                # the whole group is in row 0's band


# ------------------------------------------------------------------ overflow
@pytest.mark.parametrize("B", [9, 1])
def test_every_row_overflows(dev, B):
    N, lq, k, density = 1000, 32, 50, 0.3
    docs, doclens, Q, E = make_case(N + B + 3, N, B, lq, density)
    ix = faithful(dev, docs, doclens)
    flt, Qd = ix.filter(ids=E), Q.to(dev)
    off = run(ix, Qd, k, flt, OFF)
    on = run(ix, Qd, k, flt, ON, cap=k)
    assert (on[2] == -1).all(), on[2]
    assert_same(on, off)
    wide = run(ix, Qd, k, flt, ON)
    assert ((wide[2] > k) & (wide[2] <= len(E))).all(), wide[2]          # (so cap = k did overflow)
    assert_same(wide, off)


def mixed_case(seed=5, N=600, lq=32, k=5):
    """Query 0 equals a doc that has k - 1 near copies (its band: those k docs);
    query 1 is random (a band of every doc within beta of its k-th score)."""
    g = torch.Generator().manual_seed(seed)
    docs = rand_unit(g, N, 128, 128)
    doclens = torch.full((N,), 128, dtype=torch.int32)
    rng = np.random.default_rng(seed)
    E = np.sort(rng.choice(N, N // 2, replace=False))
    planted = E[rng.choice(len(E), k, replace=False)]
    base = rand_unit(g, lq, 128)
    for j, d in enumerate(planted):
        x = base + 0.002 * j * torch.randn(lq, 128, generator=g)
        docs[int(d), :lq] = x / x.norm(dim=-1, keepdim=True)
    Q = torch.stack([docs[int(planted[0]), :lq], rand_unit(g, lq, 128)])
    return docs, doclens, Q, E, planted


def band_bounds(S, T, beta, k, eps=1e-3):
    """Per row: (fewest, most) docs the band {T >= lb - beta} can hold, lb the
    least S among the top-k by T, every comparison moved by eps either way."""
    lo, hi = [], []
    for b in range(len(S)):
        order = np.argsort(-T[b], kind="stable")
        assert T[b, order[k - 1]] - T[b, order[k]] > eps, "the bf16 top-k must be unambiguous"
        lb = S[b, order[:k]].min()
        lo.append(int((T[b] >= lb - beta[b] + eps).sum()))
        hi.append(int((T[b] >= lb - beta[b] - eps).sum()))
    return np.array(lo), np.array(hi)


def test_mixed_overflow(dev):
    k = 5
    docs, doclens, Q, E, planted = mixed_case(k=k)
    ix = faithful(dev, docs, doclens)
    flt, Qd = ix.filter(ids=E), Q.to(dev)
    # on the CPU: which row overflows.  S: the library's faithful scores; T: the
    # bf16 scan in float64; beta from the index's own bounds (the kernel rounds it up by < 0.3 %)
    S = ix.score(Qd).cpu().numpy()[:, E].astype(np.float64)
    hi_, _, _ = orc.split_f32(docs[E].numpy(), doclens[E].numpy())
    T = orc.maxsim(orc.bf16_round(Q.numpy()), hi_, doclens[E].numpy())
    beta = orc.band_beta(Q.numpy(), *ix.bounds)
    lo, _ = band_bounds(S, T, beta, k)
    _, hi = band_bounds(S, T, beta * 1.003, k)
    print("band size bounds per row", lo.tolist(), hi.tolist())
    assert hi[0] == k and lo[1] >= k + 3, (lo, hi)
    cap = k + 1
    off = run(ix, Qd, k, flt, OFF)
    on = run(ix, Qd, k, flt, ON, cap=cap)
    assert on[2][0] == k and on[2][1] == -1, on[2]        # only the overflowing row reports -1
    assert_same(on, off)
    assert set(on[1][0].tolist()) == set(planted.tolist())
    rs, rid = filter_ref(ix.score(Qd).cpu().numpy()[:, E], E, k, 0)
    assert np.array_equal(on[1], rid) and np.array_equal(on[0], _bits(rs))


# ------------------------------------------------------------------ the certificate under a filter
K = 10


def _f64_scores(case, ids):
    hi, lo, _ = orc.split_f32(case.docs[ids], case.doclens[ids])
    T = orc.maxsim(orc.bf16_round(case.Q), hi, case.doclens[ids])
    F = orc.maxsim(case.Q, hi.astype(np.float64) + lo.astype(np.float64), case.doclens[ids])
    return T, F


@pytest.mark.parametrize("B,lq", [(1, 32), (4, 7), (12, 32)])
def test_certificate_under_a_filter(dev, B, lq):
    """Aligned residuals (tests/_adversarial.py): the bf16 top-K of the allowed
    docs is the decoys, the faithful top-K the hidden docs, 0.5 .. 0.7 beta
    below lb in T: only a band as wide as the certificate says finds them."""
    seed = 2000 + lq + B
    case = adv.adversarial_case(seed, N=600, B=B, lq=lq, K=K)
    ix = faithful(dev, case.docs, case.doclens)
    Qd = torch.from_numpy(case.Q).to(dev)
    rng = np.random.default_rng(seed)
    planted = adv.planted_ids(case)
    fillers = np.setdiff1d(np.arange(600), planted)
    half = rng.choice(fillers, len(fillers) // 2, replace=False)
    for drop_decoys in (False, True):
        allowed = np.union1d(planted, half)
        if drop_decoys:       # a random half of each query's decoys leaves the filter
            gone = np.concatenate([rng.choice(case.decoys[b], K // 2, replace=False) for b in range(B)])
            allowed = np.setdiff1d(allowed, gone)
        # preconditions, float64, on the allowed docs only
        T, F = _f64_scores(case, allowed)
        beta = orc.band_beta(case.Q, *ix.bounds)
        pos = {int(d): p for p, d in enumerate(allowed)}
        for b in range(B):
            hid = np.array([pos[int(d)] for d in case.hidden[b]])
            top_t = set(np.argsort(-T[b], kind="stable")[:K].tolist())
            top_f = np.argsort(-F[b], kind="stable")[:K]
            if not drop_decoys:
                assert top_t == {pos[int(d)] for d in case.decoys[b]}, "the bf16 top-K must be the decoys"
            else:   # the K / 2 decoys kept lead the bf16 ranking; at most K / 2 hidden docs fill it up
                kept = {pos[int(d)] for d in case.decoys[b] if int(d) in pos}
                assert len(kept) == K - K // 2 and kept <= top_t, "the bf16 top-K must hold every decoy kept"
                assert len(top_t & set(hid.tolist())) <= K // 2
            assert set(top_f.tolist()) == set(hid.tolist()), "the faithful top-K must be the hidden docs"
            other = np.ones(len(allowed), bool)
            other[hid] = False
            assert F[b, hid].min() - F[b, other].max() >= 0.10 * beta[b], "the hidden docs' lead"
        if not drop_decoys:   # and the module's own windows, on the subset
            adv.check_preconditions(case, K, bounds=ix.bounds, docs_subset=allowed)
        flt = ix.filter(ids=allowed)
        on, off = run(ix, Qd, K, flt, ON), run(ix, Qd, K, flt, OFF)
        assert_same(on, off)
        Fg = ix.score(Qd).cpu().numpy()[:, allowed]
        rs, rid = filter_ref(Fg, allowed, K, 0)
        assert np.array_equal(on[1], rid) and np.array_equal(on[0], _bits(rs))
        for b in range(B):
            assert set(on[1][b].tolist()) == set(case.hidden[b].tolist()), (drop_decoys, b)
        assert (on[2] >= (K + K // 2 if drop_decoys else 2 * K)).all(), on[2]   # the decoys kept + the hidden docs


# ------------------------------------------------------------------ poison
@pytest.mark.parametrize("B", [1, 5, 20])
def test_poisoned_padding_and_disallowed_docs_never_score(dev, B):
    """Huge values in the padding rows and in EVERY disallowed doc, hi and residual alike."""
    N, k = 400, 30
    docs, doclens, Q, E = make_case(60 + B, N, B, 32, 0.3)
    poisoned = docs.clone()
    poisoned[torch.arange(128)[None, :] >= doclens[:, None].long()] = 100.0 + 2.0 ** -10   # hi 100, residual 2^-10
    off = np.ones(N, bool)
    off[E] = False
    poisoned[torch.from_numpy(off)] = 100.0 + 2.0 ** -10
    out = []
    for d in (docs, poisoned):
        ix = faithful(dev, d, doclens)
        if d is poisoned:
            assert float(ix.residual.float().abs().max()) > 0 and float(ix.tokens.float().max()) == 100.0
        out.append(run(ix, Q.to(dev), k, ix.filter(ids=E), ON))
        assert ((out[-1][2] >= k) & (out[-1][2] <= len(E))).all()
    # (the poisoned index has other bounds, so another beta and band size: the results may not move)
    assert_same(out[0], out[1])


# ------------------------------------------------------------------ graph replay
def _call(ix, flt, q, B, lq, k, cap, ws, outs):
    _lib.check(_lib.lib().cbv2_search_filtered_f32(ix._h, flt._h, q.data_ptr(), B, lq, k, cap, ws.data_ptr(),
                                                   ws.numel(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                   outs[2].data_ptr(), _stream_ptr(ix.device)))


def test_capture_and_replay(dev):
    """cbv2_search_filtered_f32 captured once, replayed three times over a
    poisoned workspace and poisoned outputs, an eager call on the same
    workspace between the replays."""
    N, B, lq, k, cap = 1000, 9, 32, 50, BAND_CAP
    docs, doclens, Q, E = make_case(31, N, 2 * B, lq, 0.3)
    ix = faithful(dev, docs, doclens)
    ix.set_option(_lib.OPT_FILTER_BAND, ON)
    flt = ix.filter(ids=E)                                # waits for the device: before the capture
    Qs = Q.to(dev)
    need = int(_lib.lib().cbv2_search_filtered_f32_workspace_size(ix._h, flt._h, B, lq, k, cap))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def new_outs():
        return (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev),
                torch.empty((B,), dtype=torch.int32, device=dev))

    qs = torch.empty_like(Qs[:B])
    eager = {}
    for j in (1, 0):
        qs.copy_(Qs[j * B:(j + 1) * B])
        eager[j] = new_outs()
        _call(ix, flt, qs, B, lq, k, cap, ws, eager[j])
    torch.cuda.synchronize()
    assert all(((e[2] >= k) & (e[2] <= len(E))).all() for e in eager.values())
    outs, scratch = new_outs(), new_outs()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    try:
        with torch.cuda.graph(g, stream=side):
            _call(ix, flt, qs, B, lq, k, cap, ws, outs)
        for n, j in enumerate((0, 1, 0)):
            ws.fill_(0xA5)
            outs[0].fill_(float("nan"))
            outs[1].fill_(-7)
            outs[2].fill_(-7)
            qs.copy_(Qs[j * B:(j + 1) * B])
            g.replay()
            torch.cuda.synchronize()
            for got, want in zip(outs, eager[j]):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, j)
            other = Qs[(1 - j) * B:(2 - j) * B].contiguous()           # an eager call between the replays
            _call(ix, flt, other, B, lq, k, cap, ws, scratch)
            torch.cuda.synchronize()
            for got, want in zip(scratch, eager[1 - j]):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, j, "eager")
    finally:
        try:
            g.reset()
        except Exception:
            pass


# ------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("B", [1, 9])
def test_guard_bands(dev, B):
    """Workspace of exactly cbv2_search_filtered_f32_workspace_size bytes, exact
    outputs, the filter's buffer and Q inside one arena: no write outside a
    buffer, no input written, every output slot written, and the results those
    of the same call on separate allocations (no guard value was read)."""
    N, lq, k, cap = 1000, 32, 50, BAND_CAP
    docs, doclens, Q, E = make_case(41 + B, N, B, lq, 0.3)
    ix = faithful(dev, docs, doclens)
    ix.set_option(_lib.OPT_FILTER_BAND, ON)
    want = run(ix, Q.to(dev), k, ix.filter(ids=E), ON)
    L = _lib.lib()
    A = Arena(64 << 20, dev)
    words = pack_allow(E, N).to(dev)
    A.take("allow", words.numel() * 4, "bitmap", align=4, skew=4).copy_(words.view(torch.uint8))
    fbytes = int(L.cbv2_filter_bytes(N))
    A.take("fbuf", fbytes, "out", align=16, skew=16, writable=True)
    h = ctypes.c_void_p()
    _lib.check(L.cbv2_filter_create(ix._h, A.address("allow"), A.address("fbuf"), fbytes, _stream_ptr(dev),
                                    ctypes.byref(h)))
    try:
        assert int(L.cbv2_filter_count(h)) == len(E)
        A.freeze("fbuf")                                   # the handle borrows it: read-only from here on
        A.take("Q", B * lq * 128 * 4, "f32", align=16, skew=16).copy_(Q.contiguous().view(-1).view(torch.uint8).to(dev))
        need = int(L.cbv2_search_filtered_f32_workspace_size(ix._h, h, B, lq, k, cap))
        A.take("ws", need, "out", align=16, skew=16, writable=True)
        for name, n in (("out_s", B * k * 4), ("out_i", B * k * 4), ("status", B * 4)):
            A.take(name, n, "out", align=4, skew=4, writable=True)

        def call(ws_bytes):
            return L.cbv2_search_filtered_f32(ix._h, h, A.address("Q"), B, lq, k, cap, A.address("ws"), ws_bytes,
                                              A.address("out_s"), A.address("out_i"), A.address("status"),
                                              _stream_ptr(dev))
        A.snapshot()
        assert call(need - 1) == _lib.ERR_EINVAL           # one byte short: refused, nothing launched
        torch.cuda.synchronize()
        A.verify()
        assert all(A.untouched(nm) for nm in ("ws", "out_s", "out_i", "status"))
        _lib.check(call(need))
        torch.cuda.synchronize()
        A.verify()
        got_s = A.view("out_s").view(torch.int32).view(B, k).cpu().numpy()
        got_i = A.view("out_i").view(torch.int32).view(B, k).cpu().numpy()
        got_st = A.view("status").view(torch.int32).cpu().numpy()
        assert np.array_equal(got_s, want[0]) and np.array_equal(got_i, want[1]) and np.array_equal(got_st, want[2])
        assert ((got_st >= k) & (got_st <= len(E))).all(), got_st
    finally:
        torch.cuda.synchronize()
        L.cbv2_filter_destroy(h)


# ------------------------------------------------------------------ validation on a device
def test_argument_checks(dev):
    docs, doclens, Q, E = make_case(7, 300, 2, 32, 0.5)
    ix = faithful(dev, docs, doclens)
    flt, Qd, L = ix.filter(ids=E), Q.to(dev), _lib.lib()
    with pytest.raises(ValueError):
        ix.set_option(_lib.OPT_FILTER_BAND, 3)
    ix.set_option(_lib.OPT_FILTER_BAND, ON)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=dev)
    outs = (torch.empty((2, 20), dtype=torch.float32, device=dev), torch.empty((2, 20), dtype=torch.int32, device=dev),
            torch.empty((2,), dtype=torch.int32, device=dev))
    for cap in (19, BAND_CAP + 1):                        # cap outside [k, 16384] while the band is used
        with pytest.raises(ValueError, match="cap must be"):
            _call(ix, flt, Qd, 2, 32, 20, cap, ws, outs)
    other = faithful(dev, docs[:299], doclens[:299])
    with pytest.raises(ValueError, match="another index"):
        _call(other, flt, Qd, 2, 32, 20, BAND_CAP, ws, outs)
    plain = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))      # no residual: CBV2_ESTATE
    pflt = plain.filter(ids=E)
    rc = L.cbv2_search_filtered_f32(plain._h, pflt._h, Qd.data_ptr(), 2, 32, 20, BAND_CAP,
                                    ws.data_ptr(), ws.numel(), outs[0].data_ptr(), outs[1].data_ptr(),
                                    outs[2].data_ptr(), _stream_ptr(dev))
    assert rc == _lib.ERR_ESTATE
    # m == 0: padding only, status 0
    none = ix.filter(mask=np.zeros(300, bool))
    _call(ix, none, Qd, 2, 32, 20, BAND_CAP, ws, outs)
    assert (outs[1] == -1).all() and torch.isneginf(outs[0]).all() and (outs[2] == 0).all()
    # the automatic rule and the dense filter path return the same bits
    on = run(ix, Qd, 20, flt, ON)
    auto = run(ix, Qd, 20, flt, _lib.FILTER_BAND_AUTO)
    assert_same(auto, on)
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_DENSE)
    dense = run(ix, Qd, 20, flt, ON)
    assert_same(dense, on)
    assert (dense[2] == -1).all()
    # cbv2_search_filtered on the same index takes the same routine: same bits
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_SUBSET)
    need = int(L.cbv2_search_filtered_workspace_size(ix._h, flt._h, 2, 32, 20, _lib.SCORER_MAXSIM))
    assert 0 < need <= ws.numel()
    _lib.check(L.cbv2_search_filtered(ix._h, flt._h, _lib.SCORER_MAXSIM, Qd.data_ptr(), _lib.DTYPE_F32, 2, 32, 20,
                                      ws.data_ptr(), need, outs[0].data_ptr(), outs[1].data_ptr(), _stream_ptr(dev)))
    assert np.array_equal(outs[1].cpu().numpy(), on[1]) and np.array_equal(_bits(outs[0].cpu().numpy()), on[0])


# ------------------------------------------------------------------ surface
TOY = json.load(open(os.path.join(GOLDEN, "toy_c1.json")))


def test_retriever_and_hybrid_surface(dev, tmp_path):
    """JinaColBERTRetriever.search(allowed_ids=) and HybridRetriever.retrieve(allowed_ids=)
    on the default (fp32-faithful) index: the same dicts with the band on and off."""
    cfg = RAGConfig(colbert_index_path=str(tmp_path / "colbert"), bm25_index_path=str(tmp_path / "bm25"))
    assert cfg.index_dtype == "fp32"
    ind = DualIndexer(cfg, encoder=FakeEncoder(**TOY["encoder"]))
    r = ind.colbert_retriever
    r.index(TOY["corpus"])
    assert r.corpus_embeddings.faithful
    store = ChunkStore([{"chunk_id": c["id"], "text": t, "document_id": c["document_id"],
                         "heading_path": c["heading_path"], "has_images": c["has_images"],
                         "metadata": json.loads(c["metadata"]) if c["metadata"] else {}}
                        for c, t in zip(TOY["chunks"], TOY["corpus"])])
    ind.bm25_retriever = HostBM25()
    ind.bm25_retriever.index(ind.bm25_retriever.tokenize(TOY["corpus"]))
    hyb = HybridRetriever(cfg, ind, store, verbose=False)
    ix = r.corpus_embeddings
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_SUBSET)
    S = list(range(0, len(TOY["corpus"]), 2)) + [1]       # 26 of the 50 chunks
    flt = r.make_filter(S)
    got = {}
    for band in (ON, OFF):
        ix.set_option(_lib.OPT_FILTER_BAND, band)
        rows = []
        for q in TOY["queries"]:
            rows.append(r.search(q, k=5, allowed_ids=S))
            st = ix.last_band.cpu().numpy()
            assert ((st >= 5) & (st <= len(S))).all() if band == ON else (st == -1).all(), (band, st)
            rows.append(r.search(q, k=5, allowed_ids=flt))
            rows.append(hyb.retrieve(q, allowed_ids=flt))
            assert all(x["document_id"] in S for x in rows[-2]) and all(x["chunk_id"] in S for x in rows[-1])
        got[band] = rows
    assert got[ON] == got[OFF]
