"""GPU: per-query filters -- cbv2_filter_batch_* / cbv2_search_filtered_batch on
the ragged subset scan, the faithful and the dense paths, and the Python
surface above them.

Reference for row b of a batch (allowed local ids E_b, ascending):
  1. the existing single-filter search of that query alone,
     ``ix.search(Q[b:b+1], k, filter=f_b)``: ids and score BITS equal;
  2. the oracle's top-k of the allowed columns of the library's own unfiltered
     matrix, ``orc.topk(ix.score(Q)[b, E_b], k)`` mapped to ``id_base + E_b[pos]``
     (the selection tests/test_gpu_filter.py makes): ids and score BITS equal;
  3. the scores are within tests/test_gpu_kernels.py's tolerances of the float64
     oracle (bf16 1e-3, fp32-faithful 1e-4, MXFP8 2e-3 on the dequantized values);
  4. ``assert_ranking_consistent`` on the allowed columns.
The unfiltered matrix and the float64 oracle are computed once per case.
"""
import ctypes

import numpy as np
import pytest
import torch

from _parity import assert_ranking_consistent
from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig, _lib
from hybrid_rag_colbertv2_amd.bm25 import HostBM25
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore, DualIndexer, HybridRetriever
from hybrid_rag_colbertv2_amd.index import ColbertIndex, FilterBatch, _stream_ptr, quantize_mxfp8
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ATOL, ATOL32, ATOL8 = 1e-3, 1e-4, 2e-3
SUBSET, DENSE, AUTO = _lib.FILTER_SUBSET, _lib.FILTER_DENSE, _lib.FILTER_AUTO
TIES = ((10, 150), (11, 12))      # (doc, its exact copy): equal scores for every query


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def rand_unit(g, *shape):
    x = torch.randn(*shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def make_corpus(seed, N, B, lq, ld=128, empties=True):
    """Random unit tokens (fp32), ragged doclens with ~4 % empty docs, a few
    exact copies of docs (TIES) and unit queries."""
    g = torch.Generator().manual_seed(seed)
    docs = rand_unit(g, N, ld, 128)
    doclens = torch.randint(1, ld + 1, (N,), generator=g, dtype=torch.int32)
    Q = rand_unit(g, B, lq, 128)
    if empties:
        rng = np.random.default_rng(seed)
        doclens[torch.from_numpy(rng.choice(np.arange(20, N), max(2, N // 25), replace=False))] = 0
    for a, b in TIES:
        docs[b] = docs[a]
        doclens[a] = doclens[b] = 40 + a
    return docs, doclens, Q


def random_sets(seed, N, B, doclens, lo=0.01, hi=0.6):
    """One allowed set per row, densities drawn in [lo, hi); rows of >= 8 docs also hold the tied pairs."""
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(B):
        m = max(1, int(rng.uniform(lo, hi) * N))
        E = rng.choice(N, m, replace=False)
        if m >= 8:
            E = np.union1d(E, np.array(TIES).ravel())
        sets.append(np.sort(E))
    return sets


def with_empty_ends(E, doclens):
    """E with empty docs as its first and its last entry."""
    empty = np.flatnonzero(doclens.numpy() == 0)
    inner = E[(E > empty[0]) & (E < empty[-1])]
    return np.concatenate([[empty[0]], inner, [empty[-1]]])


def chunk_items(sets, chunk):
    return sum(-(-len(E) // chunk) for E in sets)


def check_batch(ix, Qd, sets, k, ref, tol, scorer="maxsim", flts=None):
    """The four checks of the module docstring; ref: float64 oracle [B, n] over every doc."""
    B = Qd.shape[0]
    flts = flts or [ix.filter(ids=E + ix.id_base) for E in sets]
    assert [f.count for f in flts] == [len(E) for E in sets]
    # an explicit FilterBatch: always cbv2_search_filtered_batch, B = 1 and rows sharing a DocFilter included
    # (a plain list whose entries are one object takes the single-filter shortcut: test_search_filters_surface)
    fb = ix.filter_batch(flts)
    assert len(fb) == B and fb.pairs == sum(len(E) for E in sets) and fb.max_count == max(len(E) for E in sets)
    s, i = ix.search(Qd, k, scorer=scorer, filters=fb)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert s.shape == (B, k) and i.shape == (B, k)
    M = ix.score(Qd, scorer=scorer).cpu().numpy()
    for b, E in enumerate(sets):
        m = len(E)
        s1, i1 = ix.search(Qd[b:b + 1], k, scorer=scorer, filter=flts[b])
        assert np.array_equal(i[b], i1.cpu().numpy()[0]), (b, "ids differ from the single-filter search")
        assert np.array_equal(_bits(s[b]), _bits(s1.cpu().numpy()[0])), (b, "bits differ from the single-filter search")
        rs, ri = orc.topk(M[b:b + 1, E], k)
        rid = np.where(ri >= 0, ix.id_base + E[np.clip(ri, 0, None)] if m else -1, -1)
        assert np.array_equal(i[b], rid[0]), (b, "ids differ from the selection on the unfiltered scores")
        assert np.array_equal(_bits(s[b]), _bits(rs[0])), (b, "score bits differ from the unfiltered scorer's")
        kk = min(k, m)
        assert (i[b, kk:] == -1).all() and np.isneginf(s[b, kk:]).all(), (b, "padding past min(k, m_b)")
        pos = np.searchsorted(E, i[b, :kk] - ix.id_base)
        want = np.asarray(ref, np.float64)[b, E[pos]] if m else np.zeros(0)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(s[b, :kk]), fin), b
        np.testing.assert_allclose(s[b, :kk][fin], want[fin], atol=tol, rtol=0)
        full = np.full((1, k), -1, np.int64)
        full[0, :kk] = pos
        assert_ranking_consistent(full, np.asarray(ref)[b:b + 1, E], tol)
        row = (i[b, :kk] - ix.id_base).tolist()
        for a, c in TIES:        # exact ties: id ascending, so the copy follows its original at once
            if a in row and c in row:
                assert row.index(c) == row.index(a) + 1 and _bits(s[b, row.index(a)]) == _bits(s[b, row.index(c)])
    return s, i


# ------------------------------------------------------------------ subset path, bf16
def bf16_case(name):
    """-> (N, B, lq, k, id_base, docs, doclens, Q, sets, shared) of the named case."""
    N, B, lq, k = {"b1": (300, 1, 32, 20), "counts": (1000, 5, 32, 10), "mixed": (777, 17, 20, 50),
                   "b40": (2500, 40, 1, 100), "bigk": (2500, 3, 32, 2000)}[name]
    docs, doclens, Q = make_corpus(N + B, N, B, lq)
    rng = np.random.default_rng(N)
    shared = None
    if name == "counts":          # m_b = 0, 1, 7, 300, 1000
        empty = np.flatnonzero(doclens.numpy() == 0)                      # first and last entries: empty docs
        e7 = np.concatenate([empty[:1], np.sort(rng.choice(np.arange(empty[0] + 1, empty[-1]), 5, replace=False)),
                             empty[-1:]])
        e300 = np.union1d(np.array(TIES).ravel(), rng.choice(N, 320, replace=False))[:300]
        sets = [np.zeros(0, np.int64), np.array([N - 1]), e7, np.sort(e300), np.arange(N)]
    elif name == "mixed":
        sets = random_sets(N, N, B, doclens)
        sets[0] = with_empty_ends(sets[0], doclens)                       # first and last entries: empty docs
        sets[1] = np.flatnonzero(doclens.numpy() == 0)[:9]                # a list of empty docs only
        sets[2] = np.array([5])                                           # k above m_b
        sets[9] = sets[4]
        shared = (4, 9)                                                   # two rows, one DocFilter
    elif name == "bigk":
        sets = [np.arange(N), np.sort(rng.choice(N, 1500, replace=False)), np.sort(rng.choice(N, 1100, replace=False))]
    else:
        sets = random_sets(N, N, B, doclens, lo=0.05, hi=0.5)
    return N, B, lq, k, (1000 if name == "mixed" else 0), docs.bfloat16(), doclens, Q.bfloat16(), sets, shared


def run_bf16_case(dev, name, chunk):
    N, B, lq, k, id_base, docs, doclens, Q, sets, shared = bf16_case(name)
    ix = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=id_base)
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    ix.set_option(_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk)
    flts = [ix.filter(ids=E + id_base) for E in sets]
    if shared:
        flts[shared[1]] = flts[shared[0]]
    ref = orc.maxsim(Q.float().numpy(), docs.float().numpy(), doclens.numpy())
    s, i = check_batch(ix, Q.to(dev), sets, k, ref, ATOL, flts=flts)
    if chunk == 0:          # the automatic path choice (by the largest m_b) and the dense path: same bits
        for path in (AUTO, DENSE):
            ix.set_option(_lib.OPT_FILTER_PATH, path)
            s0, i0 = ix.search(Q.to(dev), k, filters=ix.filter_batch(flts))
            assert np.array_equal(i0.cpu().numpy(), i) and np.array_equal(_bits(s0.cpu().numpy()), _bits(s)), path
    return sets, s, i


@pytest.mark.parametrize("name", ["b1", "counts", "mixed", "b40", "bigk"])
def test_subset_bf16(dev, name):
    sets, s, i = run_bf16_case(dev, name, 0)
    if name == "counts":
        assert [len(E) for E in sets] == [0, 1, 7, 300, 1000]
        assert (i[0] == -1).all() and np.isneginf(s[0]).all()             # m_b = 0: all padding
    if name == "mixed":
        assert np.isneginf(s[1, :9]).all() and (i[1, :9] == 1000 + sets[1]).all()   # empty docs keep their ids, in id order


@pytest.mark.parametrize("chunk", [3, 64])
@pytest.mark.parametrize("name", ["counts", "mixed"])
def test_forced_work_split(dev, name, chunk):
    """Rows whose count is no multiple of the chunk, workgroups whose four waves
    sit in different rows, and a work-item total that is no multiple of 4."""
    sets = bf16_case(name)[8]
    items = chunk_items(sets, chunk)
    assert items % 4 != 0 and any(len(E) % chunk for E in sets) and any(0 < len(E) <= chunk for E in sets)
    run_bf16_case(dev, name, chunk)


# ------------------------------------------------------------------ faithful index
@pytest.mark.parametrize("N,B,lq,k", [(300, 3, 32, 20), (1000, 9, 32, 50)])
def test_faithful(dev, N, B, lq, k):
    docs, doclens, Q = make_corpus(N + B + 1, N, B, lq)
    ix = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev))
    assert ix.faithful
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    sets = random_sets(N + 1, N, B, doclens, lo=0.05, hi=0.4)
    sets[0] = np.zeros(0, np.int64)            # m_b = 0
    sets[B - 1] = np.arange(N)                 # a full row
    sets[1] = with_empty_ends(sets[1], doclens)
    ref = orc.maxsim(Q.numpy(), docs.numpy(), doclens.numpy())
    flts = [ix.filter(ids=E) for E in sets]
    s, i = check_batch(ix, Q.to(dev), sets, k, ref, ATOL32, flts=flts)      # (ix.score is cbv2_score_f32 here)
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    sd, idd = ix.search(Q.to(dev), k, filters=ix.filter_batch(flts))
    assert np.array_equal(idd.cpu().numpy(), i) and np.array_equal(_bits(sd.cpu().numpy()), _bits(s))


# ------------------------------------------------------------------ dense path
@pytest.mark.parametrize("kind", ["bf16", "mxfp8", "long256", "meanpool"])
def test_dense_path(dev, kind):
    N, B, lq, k = {"bf16": (300, 4, 32, 20), "mxfp8": (300, 3, 32, 20), "long256": (200, 2, 32, 20),
                   "meanpool": (300, 4, 8, 20)}[kind]
    ld = 256 if kind == "long256" else 128
    docs, doclens, Q = make_corpus(91, N, B, lq, ld=ld, empties=kind != "meanpool")
    sets = random_sets(92, N, B, doclens, lo=0.02, hi=0.7)
    sets[B - 1] = np.array([7])                # k above m_b
    scorer, tol = "maxsim", ATOL
    if kind == "mxfp8":
        ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev))
        Qd, tol = Q.bfloat16().to(dev), ATOL8
        qq, qs = quantize_mxfp8(Qd)
        ref = orc.maxsim(orc.mxfp8_dequant(qq.cpu().numpy(), qs.cpu().numpy()),
                         orc.mxfp8_dequant(ix.tokens.cpu().numpy(), ix.scales.cpu().numpy()), doclens.numpy())
    elif kind == "meanpool":
        ix = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))
        ix.build_means(docs.to(dev))
        scorer, tol, Qd = "ref_meanpool_cosine", 1e-5, Q.to(dev)
        ref = ix.score(Qd, scorer=scorer).cpu().numpy()      # (the scorer itself: tests/test_gpu_kernels.py)
    else:
        ix = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))
        Qd = Q.bfloat16().to(dev)
        ref = orc.maxsim(Qd.float().cpu().numpy(), docs.bfloat16().float().numpy(), doclens.numpy())
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    flts = [ix.filter(ids=E) for E in sets]
    s, i = check_batch(ix, Qd, sets, k, ref, tol, scorer=scorer, flts=flts)
    if kind != "bf16":       # no subset path exists: forcing it, and the automatic choice, take the dense path
        for path in (SUBSET, AUTO):
            ix.set_option(_lib.OPT_FILTER_PATH, path)
            s1, i1 = ix.search(Qd, k, scorer=scorer, filters=ix.filter_batch(flts))
            assert np.array_equal(i1.cpu().numpy(), i) and np.array_equal(_bits(s1.cpu().numpy()), _bits(s))


# ------------------------------------------------------------------ edges and errors
@pytest.fixture(scope="module")
def small(dev):
    docs, doclens, Q = make_corpus(5, 300, 3, 32)
    return docs.bfloat16(), doclens, Q.bfloat16().to(dev)


def test_all_rows_empty(dev, small):
    docs, doclens, Q = small
    for ix in (ColbertIndex(docs.to(dev), doclens.to(dev)), ColbertIndex.faithful_f32(docs.float().to(dev), doclens.to(dev))):
        none = [ix.filter(mask=np.zeros(300, bool)) for _ in range(3)]
        fb = ix.filter_batch(none)
        assert fb.pairs == 0 and fb.max_count == 0 and len(fb) == 3
        s, i = ix.search(Q.float() if ix.faithful else Q, 7, filters=fb)
        assert (i.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()


def _raw_search(ix, fb, Q, B, k, ws, ws_bytes, ws_ptr=None):
    L = _lib.lib()
    out_s = torch.empty((B, k), dtype=torch.float32, device=ix.device)
    out_i = torch.empty((B, k), dtype=torch.int32, device=ix.device)
    return L.cbv2_search_filtered_batch(ix._h, fb._h, _lib.SCORER_MAXSIM, Q.data_ptr(), _lib.DTYPE_BF16, B, 32, k,
                                        ws.data_ptr() if ws_ptr is None else ws_ptr, ws_bytes, out_s.data_ptr(),
                                        out_i.data_ptr(), _stream_ptr(ix.device))


def test_errors(dev, small):
    docs, doclens, Q = small
    L = _lib.lib()
    ix = ColbertIndex(docs.to(dev), doclens.to(dev))
    flts = [ix.filter(ids=np.arange(b, 300, 3)) for b in range(3)]
    fb = ix.filter_batch(flts)
    assert fb.pairs == 300 and fb.max_count == 100
    need = int(L.cbv2_search_filtered_batch_workspace_size(ix._h, fb._h, 3, 32, 10, _lib.SCORER_MAXSIM))
    assert need > 0
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    assert _raw_search(ix, fb, Q, 3, 10, ws, need) == 0
    # a batch built for another index (n, id_base)
    other_n = ColbertIndex(docs[:299].to(dev), doclens[:299].to(dev))
    other_base = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=5)
    for o in (other_n, other_base):
        assert _raw_search(o, fb, Q, 3, 10, ws, need) == _lib.ERR_EINVAL
        assert b"another index" in L.cbv2_last_error()
        with pytest.raises(ValueError, match="another index"):
            o.search(Q, 10, filters=fb)
        with pytest.raises(ValueError, match="another index"):      # refused at creation too
            o.filter_batch(flts)
    # B differing from the batch's B
    assert _raw_search(ix, fb, Q, 2, 10, ws, need) == _lib.ERR_EINVAL
    assert b"holds 3 queries" in L.cbv2_last_error()
    with pytest.raises(ValueError):
        ix.search(Q[:2], 10, filters=fb)
    # a short and a misaligned workspace
    assert _raw_search(ix, fb, Q, 3, 10, ws, need - 1) == _lib.ERR_EINVAL
    assert b"workspace" in L.cbv2_last_error()
    assert _raw_search(ix, fb, Q, 3, 10, ws, need, ws_ptr=ws.data_ptr() + 4) == _lib.ERR_EINVAL
    assert b"workspace" in L.cbv2_last_error()
    # a null entry, a short table buffer
    h = ctypes.c_void_p()
    arr = (ctypes.c_void_p * 3)(flts[0]._h.value, None, flts[2]._h.value)
    buf = torch.empty(int(L.cbv2_filter_batch_bytes(3)), dtype=torch.uint8, device=dev)
    assert L.cbv2_filter_batch_create(ix._h, arr, 3, buf.data_ptr(), buf.numel(), None, ctypes.byref(h)) == _lib.ERR_EINVAL
    assert b"null filter for query 1" in L.cbv2_last_error() and not h.value
    arr[1] = flts[1]._h.value
    assert L.cbv2_filter_batch_create(ix._h, arr, 3, buf.data_ptr(), buf.numel() - 1, None,
                                      ctypes.byref(h)) == _lib.ERR_EINVAL
    assert b"filter batch buffer" in L.cbv2_last_error() and not h.value
    with pytest.raises(ValueError):
        ix.set_option(_lib.OPT_FILTER_BATCH_CHUNK_DOCS, -1)


# ------------------------------------------------------------------ capture and replay
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_capture_and_replay(dev, kind):
    """One cbv2_search_filtered_batch captured on a single stream (the batch
    created before the capture), replayed twice over a poisoned workspace and
    poisoned outputs: the eager call's bits."""
    N, B, k = 600, 6, 25
    docs, doclens, Q = make_corpus(17, N, 2 * B, 32)
    if kind == "f32":
        ix, Qs = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev)), Q.to(dev)
    else:
        ix, Qs = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev)), Q.bfloat16().to(dev)
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    sets = random_sets(18, N, B, doclens, lo=0.02, hi=0.4)
    sets[2] = np.zeros(0, np.int64)
    fb = ix.filter_batch([ix.filter(ids=E) for E in sets])      # waits for the device: before the capture
    qs = torch.empty_like(Qs[:B])
    eager = {}
    for j in (1, 0):
        qs.copy_(Qs[j * B:(j + 1) * B])
        eager[j] = tuple(o.clone() for o in ix.search(qs, k, filters=fb))
    ws = ix._ws
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    try:
        with torch.cuda.graph(g, stream=side):
            outs = ix.search(qs, k, filters=fb)
        assert ix._ws is ws, "the workspace was reallocated in the capture"
        for n, j in enumerate((0, 1)):
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


# ------------------------------------------------------------------ Python surface
def test_search_filters_surface(dev, small):
    docs, doclens, Q = small
    ix = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=40)
    f0, f2 = ix.filter(ids=np.arange(40, 340, 7)), ix.filter(ids=[41, 44, 300])
    # None entries: every doc (the cached all-docs filter)
    s, i = ix.search(Q, 12, filters=[f0, None, f2])
    assert ix.all_docs_filter() is ix.all_docs_filter() and ix.all_docs_filter().count == 300
    for b, f in enumerate((f0, None, f2)):
        s1, i1 = ix.search(Q[b:b + 1], 12) if f is None else ix.search(Q[b:b + 1], 12, filter=f)
        assert torch.equal(i[b], i1[0]) and torch.equal(s[b].view(torch.int32), s1[0].view(torch.int32)), b
    # a FilterBatch is reusable; a tuple works as a list does
    fb = ix.filter_batch([f0, None, f2])
    assert isinstance(fb, FilterBatch) and fb.max_count == 300
    for form in (fb, (f0, None, f2)):
        s2, i2 = ix.search(Q, 12, filters=form)
        assert torch.equal(i2, i) and torch.equal(s2.view(torch.int32), s.view(torch.int32))
    # the same object for every row: the single-filter path, same results
    s3, i3 = ix.search(Q, 12, filters=[f0, f0, f0])
    s4, i4 = ix.search(Q, 12, filter=f0)
    assert torch.equal(i3, i4) and torch.equal(s3.view(torch.int32), s4.view(torch.int32))
    s5, i5 = ix.search(Q, 12, filters=ix.filter_batch([f0, f0, f0]))         # and through the batch call
    assert torch.equal(i5, i4) and torch.equal(s5.view(torch.int32), s4.view(torch.int32))
    # argument errors
    with pytest.raises(ValueError, match="not both"):
        ix.search(Q, 12, filter=f0, filters=[f0, f0, f0])
    with pytest.raises(ValueError, match="one entry per query"):
        ix.search(Q, 12, filters=[f0, f2])
    with pytest.raises(ValueError, match="one entry per query"):
        ix.search(Q, 12, filters=[f0, f2, None, None])
    with pytest.raises(TypeError):
        ix.search(Q, 12, filters=[f0, "x", f2])
    # long queries (lq > 32) take the single-filter route row by row
    g = torch.Generator().manual_seed(3)
    QL = rand_unit(g, 2, 70, 128).bfloat16().to(dev)
    sl, il = ix.search(QL, 9, filters=[f2, f0])
    for b, f in enumerate((f2, f0)):
        s1, i1 = ix.search(QL[b:b + 1], 9, filter=f)
        assert torch.equal(il[b], i1[0]) and torch.equal(sl[b].view(torch.int32), s1[0].view(torch.int32))


WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon "
         "phi chi psi omega red green blue black white river stone cloud engine wing").split()


def test_retriever_and_hybrid_filters(dev, tmp_path):
    """search_embeddings(filters=) and retrieve_batch(filters=) against the
    per-query single-filter calls, on a corpus of 200 chunks in 8 documents."""
    rng = np.random.default_rng(0)
    corpus = [" ".join(rng.choice(WORDS, int(rng.integers(4, 20)))) for _ in range(200)]
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"), bm25_index_path=str(tmp_path / "bm25"),
                    index_dtype="bf16")
    ind = DualIndexer(cfg, encoder=FakeEncoder(maxlen=32, dim=128))
    ind.colbert_retriever.index(corpus)
    ind.bm25_retriever = HostBM25()
    ind.bm25_retriever.index(ind.bm25_retriever.tokenize(corpus))
    store = ChunkStore([{"chunk_id": j, "text": t, "document_id": j % 8} for j, t in enumerate(corpus)])
    hyb = HybridRetriever(cfg, ind, store, verbose=False)
    r, bm = ind.colbert_retriever, ind.bm25_retriever
    queries = ["alpha river engine", "omega stone", "green cloud wing tau", "kappa", "psi chi phi blue"]
    Q = torch.stack([r._encode_query(q) for q in queries])
    per_query = [store.ids_of_document(3), None, store.ids_of_document(5), [17, 18, 19, 150], store.ids_of_document(3)]
    masks = []
    for S in per_query:
        if S is None:
            masks.append(None)
        else:
            m = np.zeros(200, bool)
            m[S] = True
            masks.append(m)
    # stage 2 alone
    s, i = r.search_embeddings(Q, 30, filters=per_query)
    for b, S in enumerate(per_query):
        s1, i1 = r.search_embeddings(Q[b:b + 1], 30, allowed_ids=S)
        assert torch.equal(i[b], i1[0]) and torch.equal(s[b].view(torch.int32), s1[0].view(torch.int32)), b
        if S is not None:
            got = i[b][i[b] >= 0].tolist()
            assert set(got) <= set(S) and len(got) == min(30, len(S))
    with pytest.raises(ValueError):
        r.search_embeddings(Q, 30, allowed_ids=per_query[0], filters=per_query)
    # stage 1 per query, then all three stages
    toks = bm.tokenize(queries)
    b_ids, _ = bm.retrieve_batch(toks, masks, k=cfg.bm25_top_k)
    for b, m in enumerate(masks):
        one, _ = bm.retrieve(bm.tokenize(queries[b]), k=cfg.bm25_top_k, allow=m)
        assert np.array_equal(b_ids[b], one[0]), b
    fs, fi = hyb.retrieve_batch(Q, b_ids.astype(np.int32), filters=per_query)
    assert fi.shape[0] == len(queries)
    for b, S in enumerate(per_query):
        if S is None:
            continue             # (an unfiltered single query takes the one-trip path: another composition)
        s1, i1 = hyb.retrieve_batch(Q[b:b + 1], b_ids[b:b + 1].astype(np.int32), filter=S)
        assert torch.equal(fi[b], i1[0]) and torch.equal(fs[b].view(torch.int32), s1[0].view(torch.int32)), b
        got = fi[b][fi[b] >= 0].tolist()
        assert got and set(got) <= set(S)
    with pytest.raises(ValueError):
        hyb.retrieve_batch(Q, b_ids.astype(np.int32), filter=per_query[0], filters=per_query)
