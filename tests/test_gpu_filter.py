"""GPU: filtered search -- the filter handle's compaction, cbv2_search_filtered
on its subset and dense paths, and the Python surface above it.

Reference for a filter with allowed local ids E (ascending): the oracle's
top-k of the allowed COLUMNS, ``orc.topk(M[:, E], k)``, positions mapped back
to ``id_base + E[pos]``.  Every search case makes three checks:
  1. ids and score BITS equal that selection on the library's own unfiltered
     matrix ``ix.score(Q)`` (the bit-identity contract and the tie rule: score
     descending, then id ascending; allowed empty docs score -inf, keep their
     id and rank last; slots past min(k, m) hold -inf / -1);
  2. the scores are within the tolerances of tests/test_gpu_kernels.py (bf16:
     1e-3 absolute against the float64 oracle; fp32-faithful: 1e-4 against the
     oracle on the fp32 tokens; MXFP8: 2e-3 on the dequantized values);
  3. ``assert_ranking_consistent`` on the allowed columns.
"""
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
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocFilter, pack_allow
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
ATOL, ATOL32, ATOL8 = 1e-3, 1e-4, 2e-3
SUBSET, DENSE = _lib.FILTER_SUBSET, _lib.FILTER_DENSE


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
    """The three checks of the module docstring; returns (scores, ids) as numpy."""
    s, i = ix.search(Qd, k, scorer=scorer, filter=flt)
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
    return s, i


# ------------------------------------------------------------------ compaction
@pytest.fixture(scope="module")
def tiny_tokens(dev):
    return torch.zeros((20011, 128, 128), dtype=torch.bfloat16, device=dev)


@pytest.mark.parametrize("id_base", [0, 1000])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 2049, 20011])
def test_compaction_matches_flatnonzero(dev, tiny_tokens, n, id_base):
    """n = 20011 (prime) spans three compaction workgroups of 8192 docs."""
    ix = ColbertIndex(tiny_tokens[:n], torch.ones(n, dtype=torch.int32, device=dev), id_base=id_base)
    rng = np.random.default_rng(n)
    one = np.zeros(n, bool)
    one[int(rng.integers(n))] = True
    last = np.zeros(n, bool)
    last[n - 1] = True
    masks = [np.zeros(n, bool), one, last, rng.random(n) < 0.01, rng.random(n) < 0.5, np.ones(n, bool)]
    for mask in masks:
        want = np.flatnonzero(mask)
        for src in (torch.from_numpy(mask), torch.from_numpy(mask).to(dev)):   # CPU and device masks
            f = ix.filter(mask=src)
            assert f.count == len(want) == len(f)
            assert np.array_equal(f.ids.cpu().numpy(), want + id_base)
            f.close()
        f = ix.filter(ids=(want + id_base).tolist())
        assert np.array_equal(f.local_ids.cpu().numpy(), want)
        # garbage in the bits past n of the last word is ignored
        words = pack_allow(torch.from_numpy(mask), n).numpy().copy()
        if n % 32:
            words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        g = DocFilter(ix, torch.from_numpy(words))
        assert g.count == len(want) and np.array_equal(g.local_ids.cpu().numpy(), want)
    with pytest.raises(ValueError):
        ix.filter(ids=[id_base + n])
    with pytest.raises(ValueError):
        ix.filter(ids=[0], mask=np.ones(n, bool))


# ------------------------------------------------------------------ subset path, bf16
BF16_CASES = [(300, 1, 32, 20, 0.5), (300, 2, 32, 20, 0.1), (1000, 3, 32, 10, 0.3), (1000, 16, 20, 100, 0.5),
              (777, 17, 32, 50, 0.2), (2500, 40, 1, 100, 0.05), (129, 33, 32, 200, 1.0), (5000, 4, 32, 1, 0.001),
              (300, 5, 32, 5, 1 / 300)]     # the last: m == 1


@pytest.mark.parametrize("N,B,lq,k,density", BF16_CASES)
def test_subset_bf16(dev, N, B, lq, k, density):
    docs, doclens, Q, E = make_case(N + B, N, B, lq, density)
    docs, Q = docs.bfloat16(), Q.bfloat16()
    ix = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=1000 if N == 777 else 0)
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    flt = ix.filter(ids=E + ix.id_base)
    assert flt.count == len(E)
    ref = orc.maxsim(Q.float().numpy(), docs[E].float().numpy(), doclens[E].numpy())
    s, i = check_search(ix, Q.to(dev), flt, E, k, ref, ATOL)
    if k > len(E):
        assert (i[:, len(E):] == -1).all() and np.isneginf(s[:, len(E):]).all()
    if len(E) >= 3 and k >= len(E):          # the allowed empty doc keeps its id, after every finite score
        empty = ix.id_base + int(E[len(E) // 2])
        assert all(empty in row for row in i)
    # the automatic choice (subset up to half the shard, dense beyond): same bits
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_AUTO)
    s0, i0 = ix.search(Q.to(dev), k, filter=flt)
    assert np.array_equal(i0.cpu().numpy(), i) and np.array_equal(_bits(s0.cpu().numpy()), _bits(s))


@pytest.mark.parametrize("B", [1, 2, 5, 20])
@pytest.mark.parametrize("path", [SUBSET, DENSE])
def test_poisoned_padding_and_disallowed_docs_never_score(dev, B, path):
    """Huge values in the padding rows and in EVERY disallowed doc change no bit."""
    N, k = 400, 30
    docs, doclens, Q, E = make_case(50 + B, N, B, 32, 0.3)
    docs, Q = docs.bfloat16(), Q.bfloat16()
    poisoned = docs.clone()
    poisoned[torch.arange(128)[None, :] >= doclens[:, None].long()] = 100.0
    off = np.ones(N, bool)
    off[E] = False
    poisoned[torch.from_numpy(off)] = 100.0
    out = []
    for d in (docs, poisoned):
        ix = ColbertIndex(d.to(dev), doclens.to(dev))
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        s, i = ix.search(Q.to(dev), k, filter=ix.filter(ids=E))
        out.append((_bits(s.cpu().numpy()), i.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------ subset path, faithful
@pytest.mark.parametrize("N,B,lq,k,density", [(300, 1, 32, 20, 0.5), (1000, 9, 32, 50, 0.3), (2500, 40, 7, 100, 0.05)])
def test_subset_faithful(dev, N, B, lq, k, density):
    docs, doclens, Q, E = make_case(N + B + 1, N, B, lq, density)
    ix = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev))
    assert ix.faithful
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    flt = ix.filter(ids=E)
    ref = orc.maxsim(Q.numpy(), docs[E].numpy(), doclens[E].numpy())
    s, i = check_search(ix, Q.to(dev), flt, E, k, ref, ATOL32)
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    sd, idd = ix.search(Q.to(dev), k, filter=flt)
    assert np.array_equal(idd.cpu().numpy(), i) and np.array_equal(_bits(sd.cpu().numpy()), _bits(s))


# ------------------------------------------------------------------ dense path
@pytest.mark.parametrize("kind", ["bf16", "faithful", "mxfp8", "long256", "meanpool"])
def test_dense_path(dev, kind):
    N, B, lq, k, density = (200 if kind == "long256" else 1000), 5, 32, 30, 0.5
    ld = 256 if kind == "long256" else 128
    docs, doclens, Q, E = make_case(77, N, B, lq, density, ld=ld, empties=kind != "meanpool")
    scorer, tol = "maxsim", ATOL
    if kind == "faithful":
        ix = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev))
        Qd, tol = Q.to(dev), ATOL32
        ref = orc.maxsim(Q.numpy(), docs[E].numpy(), doclens[E].numpy())
    elif kind == "mxfp8":
        ix = ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev))
        Qd, tol = Q.bfloat16().to(dev), ATOL8
        from hybrid_rag_colbertv2_amd.index import quantize_mxfp8
        qq, qs = quantize_mxfp8(Qd)
        q_deq = orc.mxfp8_dequant(qq.cpu().numpy(), qs.cpu().numpy())
        d_deq = orc.mxfp8_dequant(ix.tokens[torch.from_numpy(E).to(dev)].cpu().numpy(),
                                  ix.scales[torch.from_numpy(E).to(dev)].cpu().numpy())
        ref = orc.maxsim(q_deq, d_deq, doclens[E].numpy())
    elif kind == "meanpool":
        ix = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))
        ix.build_means(docs.to(dev))
        scorer, tol, Qd = "ref_meanpool_cosine", 1e-5, Q.to(dev)
        ref = ix.score(Qd, scorer=scorer).cpu().numpy()[:, E]      # (the scorer itself: tests/test_gpu_kernels.py)
    else:
        ix = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))
        Qd = Q.bfloat16().to(dev)
        ref = orc.maxsim(Qd.float().cpu().numpy(), docs[E].bfloat16().float().numpy(), doclens[E].numpy())
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    flt = ix.filter(ids=E)
    s, i = check_search(ix, Qd, flt, E, k, ref, tol, scorer=scorer)
    # where no subset path exists, forcing it (and the automatic choice) takes the dense path
    for path in (SUBSET, _lib.FILTER_AUTO):
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        s1, i1 = ix.search(Qd, k, scorer=scorer, filter=flt)
        assert np.array_equal(i1.cpu().numpy(), i) and np.array_equal(_bits(s1.cpu().numpy()), _bits(s))


# ------------------------------------------------------------------ exact grid
@pytest.mark.parametrize("kind", ["bf16", "faithful"])
@pytest.mark.parametrize("path", [SUBSET, DENSE])
def test_exact_grid_filtered(dev, kind, path):
    """k/16 grid: every score is exact, ties included -- ids, order and score bits
    against the golden scores restricted to the filter."""
    z = np.load(os.path.join(GOLDEN, "exact_grid.npz"))
    Qf = torch.from_numpy(z["q_num"].astype(np.float32) / 16)
    docs = torch.from_numpy(z["docs_num"].astype(np.float32) / 16)
    doclens = torch.from_numpy(z["doclens"])
    N = docs.shape[0]
    if kind == "faithful":
        ix, Q = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev)), Qf.to(dev)
    else:
        ix, Q = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev)), Qf.bfloat16().to(dev)
    ix.set_option(_lib.OPT_FILTER_PATH, path)
    planted = int(z["order"][0, 0])
    for E in (np.arange(0, N, 2), np.array([planted])):
        flt = ix.filter(ids=E)
        for k in (1, 10, N):
            s, i = ix.search(Q, k, filter=flt)
            rs, rid = filter_ref(z["scores"][:, E], E, k, 0)
            assert np.array_equal(i.cpu().numpy(), rid), (kind, path, k)
            assert np.array_equal(_bits(s.cpu().numpy()), _bits(rs)), (kind, path, k)


# ------------------------------------------------------------------ edges
def test_edges(dev):
    docs, doclens, Q, E = make_case(5, 300, 3, 32, 0.2)
    docs, Q = docs.bfloat16(), Q.bfloat16().to(dev)
    ix = ColbertIndex(docs.to(dev), doclens.to(dev))
    L = _lib.lib()
    # m == 0: padding only
    none = ix.filter(mask=np.zeros(300, bool))
    assert none.count == 0
    s, i = ix.search(Q, 7, filter=none)
    assert (i.cpu().numpy() == -1).all() and np.isneginf(s.cpu().numpy()).all()
    # a filter of another index (n, id_base) is refused before any launch
    other_n = ColbertIndex(docs[:299].to(dev), doclens[:299].to(dev))
    other_base = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=5)
    for o in (other_n, other_base):
        with pytest.raises(ValueError, match="another index"):
            ix.search(Q, 7, filter=o.filter(mask=np.ones(o.n, bool)))
    # a short filter buffer is refused
    import ctypes
    h = ctypes.c_void_p()
    words = pack_allow(np.ones(300, bool), 300).to(dev)
    buf = torch.empty(int(L.cbv2_filter_bytes(300)), dtype=torch.uint8, device=dev)
    assert L.cbv2_filter_create(ix._h, words.data_ptr(), buf.data_ptr(), buf.numel() - 1, None,
                                ctypes.byref(h)) == _lib.ERR_EINVAL
    assert b"filter buffer" in L.cbv2_last_error() and not h.value
    # filter with lb_reduce raises; filter=None is today's search, bit for bit
    fa = ColbertIndex.faithful_f32(docs.float().to(dev), doclens.to(dev))
    with pytest.raises(ValueError, match="lb_reduce"):
        fa.search(Q.float(), 5, lb_reduce=lambda fk: fk.min(dim=1).values, filter=fa.filter(ids=E))
    a_s, a_i = ix.search(Q, 20)
    b_s, b_i = ix.search(Q, 20, filter=None)
    assert torch.equal(a_i, b_i) and np.array_equal(_bits(a_s.cpu().numpy()), _bits(b_s.cpu().numpy()))
    # an all-allowed filter returns the unfiltered search
    c_s, c_i = ix.search(Q, 20, filter=ix.filter(mask=np.ones(300, bool)))
    assert torch.equal(a_i, c_i) and np.array_equal(_bits(a_s.cpu().numpy()), _bits(c_s.cpu().numpy()))
    with pytest.raises(ValueError):
        ix.set_option(_lib.OPT_FILTER_PATH, 3)


def test_long_queries_filtered(dev):
    """lq > 32: score(), column gather, topk_rows, id map (exact plumbing)."""
    docs, doclens, Q, E = make_case(9, 300, 2, 70, 0.3)
    docs, Q = docs.bfloat16(), Q.bfloat16().to(dev)
    ix = ColbertIndex(docs.to(dev), doclens.to(dev), id_base=40)
    s, i = ix.search(Q, 25, filter=ix.filter(ids=E + 40))
    rs, rid = filter_ref(ix.score(Q).cpu().numpy()[:, E], E, 25, 40)
    assert np.array_equal(i.cpu().numpy(), rid) and np.array_equal(_bits(s.cpu().numpy()), _bits(rs))


# ------------------------------------------------------------------ API
TOY = json.load(open(os.path.join(GOLDEN, "toy_c1.json")))


def _toy_system(tmp_path, scorer):
    cfg = RAGConfig(scorer=scorer, colbert_index_path=str(tmp_path / "colbert"),
                    bm25_index_path=str(tmp_path / "bm25"), index_dtype="bf16")
    ind = DualIndexer(cfg, encoder=FakeEncoder(**TOY["encoder"]))
    ind.colbert_retriever.index(TOY["corpus"])
    store = ChunkStore([{"chunk_id": c["id"], "text": t, "document_id": c["document_id"],
                         "heading_path": c["heading_path"], "has_images": c["has_images"],
                         "metadata": json.loads(c["metadata"]) if c["metadata"] else {}}
                        for c, t in zip(TOY["chunks"], TOY["corpus"])])
    return cfg, ind, store


def test_retriever_search_allowed_ids(dev, tmp_path):
    cfg, ind, store = _toy_system(tmp_path, "maxsim")
    r = ind.colbert_retriever
    doc_ids = sorted({c["document_id"] for c in TOY["chunks"]}, key=str)
    S = store.ids_of_document(doc_ids[0])
    assert S == sorted(c["id"] for c in TOY["chunks"] if c["document_id"] == doc_ids[0]) and S
    flt = r.make_filter(S)
    for q in TOY["queries"]:
        got = r.search(q, k=10, allowed_ids=S)
        assert got and all(g["document_id"] in S for g in got) and len(got) == min(10, len(S))
        qe = r._encode_query(q).unsqueeze(0)
        s, i = r.corpus_embeddings.search(qe, len(got), scorer=r.scorer, filter=flt)
        assert [g["document_id"] for g in got] == i[0].tolist()
        assert [g["score"] for g in got] == s[0].tolist()
        assert r.search(q, k=10, allowed_ids=flt) == got
        s2, i2 = r.search_embeddings(qe, len(got), allowed_ids=S)
        assert torch.equal(i2, i) and torch.equal(s2, s)


def test_hybrid_retrieve_allowed_ids(dev, tmp_path):
    cfg, ind, store = _toy_system(tmp_path, "maxsim")
    ind.bm25_retriever = HostBM25()
    ind.bm25_retriever.index(ind.bm25_retriever.tokenize(TOY["corpus"]))
    hyb = HybridRetriever(cfg, ind, store, verbose=False)
    r, bm = ind.colbert_retriever, ind.bm25_retriever
    doc_ids = sorted({c["document_id"] for c in TOY["chunks"]}, key=str)
    S = store.ids_of_document(doc_ids[-1])
    mask = np.zeros(len(TOY["corpus"]), bool)
    mask[S] = True
    for q in TOY["queries"]:
        fin = hyb.retrieve(q, allowed_ids=S)
        assert fin and all(f["chunk_id"] in S for f in fin)
        # the composition: filtered BM25 list, filtered ColBERT list, RRF, [:50], rerank
        b_ids, _ = bm.retrieve(bm.tokenize(q), k=cfg.bm25_top_k, allow=mask)
        b_list = [int(x) for x in b_ids[0] if x >= 0]
        assert all(x in S for x in b_list)
        c_list = [g["document_id"] for g in r.search(q, k=cfg.colbert_top_k, allowed_ids=S)]
        cand = [c for c, _ in orc.rrf(b_list, c_list, k=cfg.rrf_k)][: cfg.fused_candidates]
        qe = r._encode_query(q).unsqueeze(0)
        kk = min(cfg.final_top_k, len(cand))
        rs, _, rp = r.rerank_ids(qe, torch.tensor([cand], dtype=torch.int32, device=dev), kk)
        assert [f["chunk_id"] for f in fin] == [cand[p] for p in rp[0].tolist()]
        assert [f["score"] for f in fin] == rs[0].tolist()
        assert [f["rank"] for f in fin] == list(range(1, len(fin) + 1))
        # the batched entry point under the same filter: same ids
        bs, bi = hyb.retrieve_batch(qe, np.asarray([b_list], np.int32), filter=S)
        assert bi[0].tolist()[: len(fin)] == [f["chunk_id"] for f in fin]


def test_hybrid_retrieve_without_filter_is_unchanged(dev, tmp_path):
    """No ``allowed_ids``: the golden toy_c1.json dicts, as before."""
    cfg, ind, store = _toy_system(tmp_path, "ref_meanpool_cosine")

    class RecordedBM25:
        lists = {q: bm for q, bm in zip(TOY["queries"], TOY["bm25"])}

        def tokenize(self, q):
            return q

        def retrieve(self, q, k):
            bm = self.lists[q]
            return np.array([bm["ids"][:k]]), np.array([bm["scores"][:k]])

    ind.bm25_retriever = RecordedBM25()
    hyb = HybridRetriever(cfg, ind, store, verbose=False)
    for i, q in enumerate(TOY["queries"]):
        fin, ref = hyb.retrieve(q), TOY["retrieve"][i]
        assert [f["chunk_id"] for f in fin] == [x["chunk_id"] for x in ref]
        for f, x in zip(fin, ref):
            assert {k: v for k, v in f.items() if k not in ("score", "text")} == \
                {k: v for k, v in x.items() if k != "score"}
            assert abs(f["score"] - x["score"]) < 1e-5
