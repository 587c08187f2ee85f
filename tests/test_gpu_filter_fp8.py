"""GPU: filtered search on MXFP8 indexes -- the subset path (the MXFP8 scans
with the id-list indirection: scan_f8_subset, launch_f8_stream_ragged).

Reference, as in tests/test_gpu_filter.py: for allowed local ids E (ascending)
  1. ids and score BITS equal the oracle's top-k of the allowed columns of the
     library's own unfiltered matrix, ``orc.topk(ix.score(Q)[:, E], k)`` mapped
     to ``id_base + E[pos]`` (score descending, then id ascending; an allowed
     empty doc scores -inf, keeps its id and ranks last; slots past min(k, m)
     hold -inf / -1);
  2. the scores are within the project's MXFP8 tolerance ATOL8 = 2e-3 of the
     float64 oracle on the dequantized values;
  3. ``assert_ranking_consistent`` on the allowed columns;
and the subset, the automatic and the dense path return the same bits.  Every
test that forces the subset path also checks that it was taken: the workspace
under FILTER_SUBSET holds no [B][n] block.
"""
import ctypes
import gc
import json
import os

import numpy as np
import pytest
import torch

from _parity import assert_ranking_consistent
from conftest import GOLDEN
from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig, _lib
from hybrid_rag_colbertv2_amd.bm25 import HostBM25
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore, DualIndexer, HybridRetriever
from hybrid_rag_colbertv2_amd.index import ColbertIndex, quantize_mxfp8
from hybrid_rag_colbertv2_amd.retriever import JinaColBERTRetriever
from oracle import oracle as orc
from test_gpu_bounds import N_SMALL, Shard      # the guard-band shard and its per-call buffers (tests/_arena.py)

pytestmark = pytest.mark.gpu
ATOL8 = 2e-3
SUBSET, DENSE, AUTO = _lib.FILTER_SUBSET, _lib.FILTER_DENSE, _lib.FILTER_AUTO
MAXSIM = _lib.SCORER_MAXSIM


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _out(s, i):
    return _bits(s.cpu().numpy()), i.cpu().numpy()


def rand_unit(g, *shape):
    x = torch.randn(*shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def make_case(seed, N, B, lq, density):
    """tests/test_gpu_filter.py's make_case: random unit tokens, ragged doclens
    with some empty docs, max(1, round(density * N)) allowed docs, an empty doc
    (m >= 3) among them."""
    g = torch.Generator().manual_seed(seed)
    docs = rand_unit(g, N, 128, 128)
    doclens = torch.randint(1, 129, (N,), generator=g, dtype=torch.int32)
    Q = rand_unit(g, B, lq, 128)
    rng = np.random.default_rng(seed)
    m = max(1, int(round(density * N)))
    E = np.sort(rng.choice(N, m, replace=False))
    doclens[torch.from_numpy(rng.choice(N, max(1, N // 50), replace=False))] = 0
    if m >= 3:
        doclens[int(E[m // 2])] = 0          # an allowed empty doc
        doclens[int(E[0])] = 128
    return docs, doclens, Q, E


def dequant_ref(ix, Qd, doclens, E=None):
    """The float64 oracle on the dequantized index and queries: [B, len(E)] (every doc without E)."""
    qq, qs = quantize_mxfp8(Qd)
    tok, sc = ix.tokens.cpu().numpy(), ix.scales.cpu().numpy()
    dl = doclens.numpy()
    if E is not None:
        tok, sc, dl = tok[E], sc[E], dl[E]
    return orc.maxsim(orc.mxfp8_dequant(qq.cpu().numpy(), qs.cpu().numpy()), orc.mxfp8_dequant(tok, sc), dl)


def ws_sizes(ix, flt, B, lq, k, batch=False):
    """(bytes under FILTER_SUBSET, bytes under FILTER_DENSE); leaves the option at SUBSET."""
    L = _lib.lib()
    fn = L.cbv2_search_filtered_batch_workspace_size if batch else L.cbv2_search_filtered_workspace_size
    out = []
    for path in (DENSE, SUBSET):
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        out.append(int(fn(ix._h, flt._h, B, lq, k, MAXSIM)))
    return out[1], out[0]


def assert_subset_taken(ix, flt, B, lq, k, batch=False):
    sub, dense = ws_sizes(ix, flt, B, lq, k, batch)
    assert sub + 4 * B * ix.n <= dense, f"MXFP8 subset path not taken: workspace {sub} (subset) vs {dense} (dense)"


def check_search(ix, Qd, flt, E, k, ref_cols):
    """The three checks of the module docstring; returns (scores, ids) as numpy."""
    s, i = ix.search(Qd, k, filter=flt)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    M = ix.score(Qd).cpu().numpy()
    rs, ri = orc.topk(M[:, E], k)
    rid = np.where(ri >= 0, ix.id_base + E[np.clip(ri, 0, None)], -1)
    assert np.array_equal(i, rid), "ids differ from the selection on the library's own unfiltered scores"
    assert np.array_equal(_bits(s), _bits(rs)), "score bits differ from the unfiltered scorer's"
    pos = np.where(i >= 0, np.searchsorted(E, np.clip(i - ix.id_base, 0, None)), -1)
    for b in range(i.shape[0]):
        live = pos[b] >= 0
        want = np.asarray(ref_cols, np.float64)[b, pos[b][live]]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(s[b][live]), fin)
        err = np.abs(s[b][live][fin] - want[fin]).max() if fin.any() else 0.0
        print(f"row {b}: max |score - oracle| = {err:.3e} (bound {ATOL8:.0e})")
        np.testing.assert_allclose(s[b][live][fin], want[fin], atol=ATOL8, rtol=0)
        assert np.isneginf(s[b][~live]).all()
    assert_ranking_consistent(pos, ref_cols, ATOL8)
    return s, i


# ------------------------------------------------------------------ a. subset path, one filter
# (N, B, lq, k, density): every dispatch shape of scan_f8_subset and the edges of the 4-doc group
CASES = [
    (300, 1, 32, 20, 0.5),         # the streaming scan
    (300, 2, 32, 20, 0.1),         # the streaming scan, both query slots
    (1000, 3, 32, 10, 0.3),        # 4 waves x 1 query
    (1000, 5, 32, 30, 0.5),        # 4 x 2 (padded query slots)
    (1000, 8, 32, 30, 0.5),        # 4 x 2
    (1000, 16, 20, 100, 0.5),      # 4 x 4
    (777, 17, 32, 50, 0.2),        # 4 x 8; id_base = 1000
    (2500, 40, 1, 100, 0.05),      # 8 x 8, lq = 1
    (600, 65, 32, 10, 0.25),       # two query groups of 8 x 8
    (129, 33, 32, 200, 1.0),       # k > m; m no multiple of the 4-doc group
    (5000, 4, 32, 1, 0.001),       # m = 5
    (300, 5, 32, 5, 1 / 300),      # m = 1
    (300, 9, 32, 5, 2 / 300),      # m = 2
    (300, 9, 32, 5, 3 / 300),      # m = 3
]


@pytest.mark.parametrize("N,B,lq,k,density", CASES)
def test_subset_mxfp8(dev, N, B, lq, k, density):
    docs, doclens, Q, E = make_case(N + B, N, B, lq, density)
    ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev), id_base=1000 if N == 777 else 0)
    Qd = Q.bfloat16().to(dev)
    flt = ix.filter(ids=E + ix.id_base)
    assert flt.count == len(E)
    assert_subset_taken(ix, flt, B, lq, k)           # (leaves FILTER_SUBSET set)
    ref = dequant_ref(ix, Qd, doclens, E)
    s, i = check_search(ix, Qd, flt, E, k, ref)
    if k > len(E):
        assert (i[:, len(E):] == -1).all() and np.isneginf(s[:, len(E):]).all()
    if len(E) >= 3 and k >= len(E):                  # the allowed empty doc keeps its id, after every finite score
        empty = ix.id_base + int(E[len(E) // 2])
        assert all(empty in row for row in i) and np.isneginf(s[:, len(E) - 1]).all()
        assert all(np.isneginf(s[b, list(i[b]).index(empty)]) for b in range(B))
    for path in (AUTO, DENSE):                       # the automatic choice and the dense path: same bits
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        s0, i0 = ix.search(Qd, k, filter=flt)
        assert np.array_equal(i0.cpu().numpy(), i) and np.array_equal(_bits(s0.cpu().numpy()), _bits(s)), path


# ------------------------------------------------------------------ b. the feature is there
def test_subset_workspace_has_no_dense_block(dev):
    """Under FILTER_SUBSET the workspace of an MXFP8 filtered search (one filter,
    and three per-query filters) is smaller than the dense path's by the whole
    [B][n] score block: the subset path exists for MXFP8."""
    N, B, lq, k = 1000, 5, 32, 10
    docs, doclens, Q, _ = make_case(1, N, B, lq, 0.1)
    ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev))
    rng = np.random.default_rng(2)
    flts = [ix.filter(ids=np.sort(rng.choice(N, 100, replace=False))) for _ in range(3)]
    assert all(f.count == 100 for f in flts)
    sub, dense = ws_sizes(ix, flts[0], B, lq, k)
    assert sub + 4 * B * N <= dense, (sub, dense)
    fb = ix.filter_batch([flts[0], flts[1], flts[2], flts[0], flts[1]])
    sub, dense = ws_sizes(ix, fb, B, lq, k, batch=True)
    assert sub + 4 * B * N <= dense, (sub, dense)


# ------------------------------------------------------------------ c. poison
@pytest.fixture(scope="module")
def poison_case(dev):
    """Per B: the clean MXFP8 arrays and a copy whose padding rows and disallowed
    docs hold e4m3 0x7E (448) under scale bytes 0xFE."""
    cache = {}

    def get(B):
        if B not in cache:
            N = 400
            docs, doclens, Q, E = make_case(50 + B, N, B, 32, 0.3)
            clean = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev))
            tok, sc = clean.tokens.clone(), clean.scales.clone()
            bad = torch.arange(128)[None, :] >= doclens[:, None].long()       # [N, 128] padding rows
            off = np.ones(N, bool)
            off[E] = False
            bad[torch.from_numpy(off)] = True                                  # every row of a disallowed doc
            bad = bad.to(dev)
            tok[bad] = 0x7E
            sc[bad] = 0xFE
            cache[B] = (clean.tokens, clean.scales, tok, sc, doclens.to(dev), Q.bfloat16().to(dev), E)
        return cache[B]

    yield get
    cache.clear()


@pytest.mark.parametrize("B", [1, 2, 5, 20])
@pytest.mark.parametrize("path", [SUBSET, DENSE])
def test_poisoned_padding_and_disallowed_docs_never_score(dev, poison_case, B, path):
    """Huge values in the padding rows and in EVERY disallowed doc change no bit."""
    k = 30
    tok, sc, ptok, psc, doclens, Qd, E = poison_case(B)
    out = []
    for t, s_ in ((tok, sc), (ptok, psc)):
        ix = ColbertIndex(t, doclens, scales=s_)
        flt = ix.filter(ids=E)
        if path == SUBSET:
            assert_subset_taken(ix, flt, B, 32, k)
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        out.append(_out(*ix.search(Qd, k, filter=flt)))
    assert np.isfinite(out[0][0].view(np.float32)[:, :10]).all()
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])


# ------------------------------------------------------------------ d. per-query filters
def ragged_sets(layout, N, doclens):
    """-> (allowed sets of the 4 rows, (a, b): row b takes row a's DocFilter)."""
    rng = np.random.default_rng(N)
    empty = np.flatnonzero(doclens.numpy() == 0)
    if layout == "edges":          # m_b = 0, a full row, one doc with k above it, the full row's handle again
        return [np.zeros(0, np.int64), np.arange(N), np.array([N - 1]), np.arange(N)], (1, 3)
    mid = np.sort(rng.choice(np.arange(empty[0] + 1, empty[-1]), 90, replace=False))
    ends = np.concatenate([empty[:1], mid[(mid > empty[0]) & (mid < empty[-1])], empty[-1:]])   # empty docs first and last
    return [np.sort(rng.choice(N, 120, replace=False)), np.unique(ends), empty[:9], None], (0, 3)


@pytest.mark.parametrize("chunk", [0, 7])
@pytest.mark.parametrize("layout", ["edges", "mixed"])
def test_per_query_filters_ragged(dev, layout, chunk):
    """Row b of the ragged scan equals the single-filter search of query b alone and the dense path, bit for
    bit.  chunk = 7: lists span several work items (300 = 42 x 7 + 6) and surplus waves of the last workgroup exit."""
    N, B, lq, k = 300, 4, 32, 20
    docs, doclens, Q, _ = make_case(7, N, B, lq, 0.1)
    ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev), id_base=40)
    Qd = Q.bfloat16().to(dev)
    sets, (a, b) = ragged_sets(layout, N, doclens)
    sets[b] = sets[a]
    flts = [ix.filter(ids=E + 40) for E in sets]
    flts[b] = flts[a]                                  # two rows, one handle
    ix.set_option(_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk)
    fb = ix.filter_batch(flts)
    assert fb.max_count == max(len(E) for E in sets) and fb.pairs == sum(len(E) for E in sets)
    if chunk:
        items = sum(-(-len(E) // chunk) for E in sets)
        assert items % 8 != 0 and any(len(E) > chunk for E in sets)
    assert_subset_taken(ix, fb, B, lq, k, batch=True)  # (leaves FILTER_SUBSET set)
    s, i = _out(*ix.search(Qd, k, filters=fb))
    M = ix.score(Qd).cpu().numpy()
    for r, E in enumerate(sets):
        s1, i1 = _out(*ix.search(Qd[r:r + 1], k, filter=flts[r]))
        assert np.array_equal(i[r], i1[0]) and np.array_equal(s[r], s1[0]), (r, "differs from the single-filter search")
        rs, ri = orc.topk(M[r:r + 1, E], k)
        rid = np.where(ri >= 0, 40 + E[np.clip(ri, 0, None)] if len(E) else -1, -1)
        assert np.array_equal(i[r], rid[0]) and np.array_equal(s[r], _bits(rs[0])), (r, "differs from the unfiltered scores")
        kk = min(k, len(E))
        assert (i[r, kk:] == -1).all() and np.isneginf(s[r, kk:].view(np.float32)).all(), (r, "padding past min(k, m_b)")
    if layout == "edges":
        assert (i[0] == -1).all() and i[2, 0] == 40 + N - 1 and (i[2, 1:] == -1).all()
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    sd, idd = _out(*ix.search(Qd, k, filters=ix.filter_batch(flts)))
    assert np.array_equal(idd, i) and np.array_equal(sd, s)


# ------------------------------------------------------------------ e. capture and replay
@pytest.mark.parametrize("form", ["filter", "filters"])
def test_capture_and_replay(dev, form):
    """cbv2_search_filtered / cbv2_search_filtered_batch on the MXFP8 subset path
    (the queries' quantizer inside the capture), replayed over a poisoned
    workspace, poisoned outputs and changed query contents: the eager bits."""
    N, B, k = 600, 6, 25
    docs, doclens, Q, E = make_case(17, N, 2 * B, 32, 0.2)
    ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev))
    Qs = Q.bfloat16().to(dev)
    rng = np.random.default_rng(18)
    if form == "filter":
        flt = ix.filter(ids=E)
        assert_subset_taken(ix, flt, B, 32, k)
        kw = {"filter": flt}
    else:
        sets = [np.sort(rng.choice(N, int(m), replace=False)) for m in (200, 3, 0, 77, 240, 12)]
        fb = ix.filter_batch([ix.filter(ids=S) for S in sets])      # waits for the device: before the capture
        assert_subset_taken(ix, fb, B, 32, k, batch=True)
        kw = {"filters": fb}
    qs = torch.empty_like(Qs[:B])
    eager = {}
    for j in (1, 0):
        qs.copy_(Qs[j * B:(j + 1) * B])
        eager[j] = tuple(o.clone() for o in ix.search(qs, k, **kw))
    assert not torch.equal(eager[0][1], eager[1][1])
    ws = ix._ws
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    try:
        with torch.cuda.graph(g, stream=side):
            outs = ix.search(qs, k, **kw)
        assert ix._ws is ws, "the workspace was reallocated in the capture"
        for n, j in enumerate((0, 1, 0)):
            ws.view(torch.uint8).fill_(0xA5)
            outs[0].fill_(float("nan"))
            outs[1].fill_(-7)
            qs.copy_(Qs[j * B:(j + 1) * B])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[1], eager[j][1]), (n, j)
            assert torch.equal(outs[0].view(torch.int32), eager[j][0].view(torch.int32)), (n, j)
    finally:
        try:
            g.reset()
        except Exception:
            pass


# ------------------------------------------------------------------ f. guard bands
@pytest.fixture(scope="module")
def fp8_shard(dev):
    sh = Shard(dev, "fp8", N_SMALL, 128, False)
    yield sh
    del sh
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1, 3, 9, 33])
def test_guard_bands_subset(fp8_shard, B):
    """Tokens, scales, doclens, the id list, the queries, a workspace of exactly
    cbv2_search_filtered_workspace_size bytes and the outputs inside guard bands
    (winning values: e4m3 448, scale 2^11, full-length docs), the last allowed
    doc being doc n - 1: no guard byte changes and the results equal the
    wrappers' on clones of the inputs, bit for bit."""
    m, k, lq = 40, 10, 32
    with fp8_shard.case(seed=700 + B, opts=((_lib.OPT_FILTER_PATH, SUBSET),)) as c:
        L, h, n = c.L, c.h, fp8_shard.n
        mask = c.mask(m)
        assert bool(mask[n - 1])
        f, fref = c.make_filter("f", mask)
        q, qdt, Qr = c.queries(B, lq)
        assert qdt == _lib.DTYPE_MXFP8
        need = int(L.cbv2_search_filtered_workspace_size(h, f, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, DENSE))
        assert need + 4 * B * n <= int(L.cbv2_search_filtered_workspace_size(h, f, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, SUBSET))
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered(h, f, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k, filter=fref), valid=[m] * B)


@pytest.mark.parametrize("chunk", [0, 16])
def test_guard_bands_ragged(fp8_shard, chunk):
    """The same for cbv2_search_filtered_batch: 0, 1, 40, n and (a repeated handle) 40 docs per row."""
    counts, order = (0, 1, 40, N_SMALL), [0, 1, 2, 3, 2]
    opts = ((_lib.OPT_FILTER_PATH, SUBSET), (_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk))
    with fp8_shard.case(seed=800 + chunk, opts=opts) as c:
        L, h, B, lq, k = c.L, c.h, 5, 32, 64
        made = [c.make_filter(f"f{j}", c.mask(m)) for j, m in enumerate(counts)]
        handles = (ctypes.c_void_p * B)(*[made[j][0].value for j in order])
        c.out("table", int(L.cbv2_filter_batch_bytes(B)), align=16)
        fb = ctypes.c_void_p()
        c.run(lambda w, wb: L.cbv2_filter_batch_create(h, handles, B, w, wb, c.st, ctypes.byref(fb)), ws="table")
        c._batches.append(fb)
        c.A.freeze("table")
        fbref = c.ref.filter_batch([made[j][1] for j in order])
        q, qdt, Qr = c.queries(B, lq)
        need = int(L.cbv2_search_filtered_batch_workspace_size(h, fb, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, DENSE))
        assert need + 4 * B * N_SMALL <= int(L.cbv2_search_filtered_batch_workspace_size(h, fb, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, SUBSET))
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered_batch(h, fb, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k, filters=fbref), valid=[counts[j] for j in order])


# ------------------------------------------------------------------ g. API
WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon "
         "phi chi psi omega red green blue black white river stone cloud engine wing").split()


@pytest.mark.parametrize("path", [AUTO, SUBSET])
def test_retriever_and_hybrid_on_fp8_index(dev, tmp_path, path):
    """index_dtype="fp8": search(allowed_ids=), search_embeddings(filters=) and
    hybrid.retrieve(allowed_ids=) / retrieve_batch(filters=) return allowed ids
    only, with the unfiltered search's scores for those ids."""
    rng = np.random.default_rng(0)
    corpus = [" ".join(rng.choice(WORDS, int(rng.integers(4, 20)))) for _ in range(50)]
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"), bm25_index_path=str(tmp_path / "bm25"),
                    index_dtype="fp8")
    r = JinaColBERTRetriever(cfg, encoder=FakeEncoder(maxlen=32, dim=128))
    r.index(corpus)
    ix = r.corpus_embeddings
    assert ix.fp8 and ix.n == 50
    ix.set_option(_lib.OPT_FILTER_PATH, path)
    ids = [3, 4, 11, 17, 18, 19, 30, 42, 49]
    flt = r.make_filter([0, 7, 8, 25])
    queries = ["alpha river engine", "omega stone", "green cloud wing tau"]
    for q in queries:
        full = {g["document_id"]: g["score"] for g in r.search(q, k=50)}
        got = r.search(q, k=5, allowed_ids=ids)
        assert len(got) == 5 and all(g["document_id"] in ids for g in got)
        assert all(g["score"] == full[g["document_id"]] for g in got)
        best = sorted(ids, key=lambda d: (-full[d], d))[:5]
        assert [g["document_id"] for g in got] == best
    Q = torch.stack([r._encode_query(q) for q in queries])
    s, i = r.search_embeddings(Q, 6, filters=[flt, None, ids])
    fs, fi = r.search_embeddings(Q, 50)
    for b, S in enumerate(([0, 7, 8, 25], None, ids)):
        row = i[b][i[b] >= 0].tolist()
        assert len(row) == min(6, len(S) if S else 50) and (S is None or set(row) <= set(S))
        lookup = dict(zip(fi[b].tolist(), fs[b].view(torch.int32).tolist()))
        assert s[b].view(torch.int32).tolist()[: len(row)] == [lookup[d] for d in row]
        s1, i1 = r.search_embeddings(Q[b:b + 1], 6) if S is None else r.search_embeddings(Q[b:b + 1], 6, allowed_ids=S)
        assert torch.equal(i[b], i1[0]) and torch.equal(s[b].view(torch.int32), s1[0].view(torch.int32))
    # the hybrid pipeline over the same index
    ind = DualIndexer(cfg, encoder=r.model)
    ind.colbert_retriever = r
    ind.bm25_retriever = HostBM25()
    ind.bm25_retriever.index(ind.bm25_retriever.tokenize(corpus))
    store = ChunkStore([{"chunk_id": j, "text": t, "document_id": j % 5} for j, t in enumerate(corpus)])
    hyb = HybridRetriever(cfg, ind, store, verbose=False)
    S3 = store.ids_of_document(3)
    fin = hyb.retrieve(queries[0], allowed_ids=S3)
    assert fin and all(f["chunk_id"] in S3 for f in fin)
    bm = ind.bm25_retriever
    per_query = [S3, None, ids]
    masks = [None if S is None else np.isin(np.arange(50), S) for S in per_query]
    b_ids, _ = bm.retrieve_batch(bm.tokenize(queries), masks, k=cfg.bm25_top_k)
    bs, bi = hyb.retrieve_batch(Q, b_ids.astype(np.int32), filters=per_query)
    for b, S in enumerate(per_query):
        got = bi[b][bi[b] >= 0].tolist()
        assert got and (S is None or set(got) <= set(S))
        if S is not None:
            s1, i1 = hyb.retrieve_batch(Q[b:b + 1], b_ids[b:b + 1].astype(np.int32), filter=S)
            assert torch.equal(bi[b], i1[0]) and torch.equal(bs[b].view(torch.int32), s1[0].view(torch.int32)), b
