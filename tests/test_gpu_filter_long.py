"""GPU: filtered search on long-document indexes (ld = 256 / 512 / 1024 token
slots) -- the subset paths of bf16, MXFP8 and fp32-faithful indexes: the
streaming scans at run-time ld, the direct scan and the doc-interleaved scans
with the id-list indirection, the LONG pair kernel over the list, the faithful
band over the compact row and the ragged per-query scans.

Reference, as in tests/test_gpu_filter.py: for allowed local ids E (ascending)
  1. ids and score BITS equal the oracle's top-k of the allowed columns of the
     library's own unfiltered matrix, ``orc.topk(ix.score(Q)[:, E], k)`` mapped
     to ``id_base + E[pos]`` (score descending, then id ascending; an allowed
     empty doc scores -inf, keeps its id and ranks last; slots past min(k, m)
     hold -inf / -1) -- the unfiltered scorer is pinned to the float64 oracle by
     tests/test_gpu_long_docs.py;
  2. the scores are within the project's tolerances of the float64 oracle on
     the allowed docs (bf16 1e-3; MXFP8 2e-3 on the dequantized values;
     faithful 1e-4 against the fp32 values);
  3. ``assert_ranking_consistent`` on the allowed columns;
and the subset, the automatic and the dense path return the same bits.  Every
test that forces the subset path also checks that it was taken: the workspace
under FILTER_SUBSET holds no [B][n] block (the faithful band: ``last_band``).

One corpus per ld (N = 400 / 200 / 124 docs at 256 / 512 / 1024 slots), shared
by the tests: doc 0 has 129 tokens (one row in the second 128-token block), doc
1 is empty, doc 2 has 128 tokens, docs 3.. hold 1, 127, 255, 256, 257 (where ld
allows) tokens and doc N - 1 has ld.  An allowed set of m docs holds doc N - 1,
then doc 0, then docs 1 and 2 (so m >= 4 allows a doc of each kind), the rest
drawn at random.
"""
import ctypes
import gc
import re

import numpy as np
import pytest
import torch

from _parity import assert_ranking_consistent
from hybrid_rag_colbertv2_amd import RAGConfig, _build, _lib
from hybrid_rag_colbertv2_amd.bm25 import HostBM25
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore, DualIndexer, HybridRetriever
from hybrid_rag_colbertv2_amd.index import BAND_CAP, ColbertIndex, quantize_mxfp8
from hybrid_rag_colbertv2_amd.retriever import JinaColBERTRetriever
from oracle import oracle as orc
from test_gpu_bounds import N_SMALL, Shard          # the guard-band shard and its per-call buffers (tests/_arena.py)
from test_gpu_filter_fp8 import ragged_sets         # the "edges" and "mixed" per-query layouts
from test_gpu_long_docs import _LongChunkEncoder, make_f32_case

pytestmark = pytest.mark.gpu
TOL = {"bf16": 1e-3, "mxfp8": 2e-3, "faithful": 1e-4}     # test_gpu_long_docs.ATOL, ATOL8, ATOL32
KINDS = ("bf16", "mxfp8", "faithful")
SUBSET, DENSE, AUTO = _lib.FILTER_SUBSET, _lib.FILTER_DENSE, _lib.FILTER_AUTO
BAND_ON, BAND_OFF = _lib.FILTER_BAND_ON, _lib.FILTER_BAND_OFF
MAXSIM = _lib.SCORER_MAXSIM
NDOCS = {256: 400, 512: 200, 1024: 124}


def _const(name):
    """A dispatch threshold of csrc/colbert_mi355x.hip, read from the source."""
    with open(_build.SRC) as f:
        return int(re.search(rf"^constexpr int {name} = (\d+);", f.read(), re.M).group(1))


K_LONG_DIRECT, K_F8_DIRECT, K_F8_SMALL = _const("kLongDirectMaxB"), _const("kF8DirectMaxB"), _const("kF8SmallMaxB")
assert 3 < K_LONG_DIRECT < 32 and K_F8_DIRECT == 2 < K_F8_SMALL < 64


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _out(s, i):
    return _bits(s.cpu().numpy()), i.cpu().numpy()


def rand_unit(g, *shape):
    x = torch.randn(*shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def make_corpus(ld):
    """fp32 unit tokens [N, ld, 128] and the doclens of the module docstring, with nine more empty docs."""
    N = NDOCS[ld]
    g = torch.Generator().manual_seed(ld)
    docs = rand_unit(g, N, ld, 128)
    doclens = torch.randint(1, ld + 1, (N,), generator=g, dtype=torch.int32)
    rng = np.random.default_rng(ld)
    doclens[torch.from_numpy(rng.choice(np.arange(10, N - 1), 9, replace=False))] = 0
    special = [129, 0, 128, 1, 127, 255, 256] + ([257] if ld > 256 else [])
    doclens[: len(special)] = torch.tensor(special, dtype=torch.int32)
    doclens[N - 1] = ld
    return docs, doclens


def allowed(N, m, seed=0):
    """m allowed local ids, ascending: doc N - 1, doc 0, the empty doc 1, the 128-token doc 2, then random ones."""
    first = [N - 1, 0, 1, 2][:m]
    rest = np.setdiff1d(np.arange(N), first)
    more = np.random.default_rng(1000 * N + m + seed).choice(rest, m - len(first), replace=False)
    return np.sort(np.concatenate([np.asarray(first, np.int64), more]))


class World:
    """The corpora, their indexes per (kind, ld, id_base) and the queries, built once."""

    def __init__(self, dev):
        self.dev, self.corpora, self.indexes, self.queries = dev, {}, {}, {}

    def corpus(self, ld):
        if ld not in self.corpora:
            self.corpora[ld] = make_corpus(ld)
        return self.corpora[ld]

    def index(self, kind, ld, id_base=0):
        """The cached index, its options at their defaults."""
        key = (kind, ld, id_base)
        if key not in self.indexes:
            docs, doclens = self.corpus(ld)
            self.indexes[key] = build_index(self.dev, kind, docs, doclens, id_base)
        ix = self.indexes[key]
        for opt in (_lib.OPT_FILTER_PATH, _lib.OPT_FILTER_BAND, _lib.OPT_FILTER_BATCH_CHUNK_DOCS):
            ix.set_option(opt, 0)
        return ix

    def q(self, B, lq, seed=0):
        if (B, lq, seed) not in self.queries:
            self.queries[(B, lq, seed)] = rand_unit(torch.Generator().manual_seed(7000 + 100 * B + lq + seed), B, lq, 128)
        return self.queries[(B, lq, seed)]

    def ref_cols(self, kind, ix, ld, Q, E):
        """The float64 oracle's scores of the allowed docs [B, len(E)], on the values the index holds."""
        docs, doclens = self.corpus(ld)
        return oracle_cols(kind, ix, Q, docs, doclens, E)


def build_index(dev, kind, docs, doclens, id_base=0):
    if kind == "faithful":
        return ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev), id_base=id_base)
    if kind == "mxfp8":
        return ColbertIndex.mxfp8(docs.bfloat16().to(dev), doclens.to(dev), id_base=id_base)
    return ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev), id_base=id_base)


def dev_queries(kind, Q, dev):
    return Q.to(dev) if kind == "faithful" else Q.bfloat16().to(dev)


def oracle_cols(kind, ix, Q, docs, doclens, E):
    dl = doclens[E].numpy()
    if kind == "faithful":
        return orc.maxsim(Q.numpy(), docs[E].numpy(), dl)
    if kind == "bf16":
        return orc.maxsim(Q.bfloat16().float().numpy(), docs[E].bfloat16().float().numpy(), dl)
    qq, qs = quantize_mxfp8(Q.bfloat16().to(ix.device))
    sel = torch.from_numpy(E).to(ix.device)
    return orc.maxsim(orc.mxfp8_dequant(qq.cpu().numpy(), qs.cpu().numpy()),
                      orc.mxfp8_dequant(ix.tokens[sel].cpu().numpy(), ix.scales[sel].cpu().numpy()), dl)


@pytest.fixture(scope="module")
def world(dev):
    w = World(dev)
    yield w
    w.indexes.clear()
    w.corpora.clear()
    gc.collect()
    torch.cuda.empty_cache()


def ws_sizes(ix, flt, B, lq, k, batch=False):
    """(bytes under FILTER_SUBSET, bytes under FILTER_DENSE); leaves the option at SUBSET."""
    L = _lib.lib()
    fn = L.cbv2_search_filtered_batch_workspace_size if batch else L.cbv2_search_filtered_workspace_size
    out = []
    for path in (DENSE, SUBSET):
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        out.append(int(fn(ix._h, flt._h, B, lq, k, MAXSIM)))
    return out[1], out[0]


def cand_bytes(faithful, B, max_count):
    """Per-query filters on a faithful index: the subset path's workspace holds a candidate matrix int32 [B][M]
    (M the largest count, 256-byte rounded) in place of the dense path's [B][n] score block."""
    return (4 * B * max(int(max_count), 1) + 255) // 256 * 256 if faithful else 0


def assert_subset_taken(ix, flt, B, lq, k, batch=False):
    """The workspace under FILTER_SUBSET is smaller than the dense one by the whole [B][n] block (a faithful
    filter batch: once its candidate matrix is set aside)."""
    sub, dense = ws_sizes(ix, flt, B, lq, k, batch)
    cand = cand_bytes(ix.faithful, B, flt.max_count) if batch else 0
    assert sub - cand + 4 * B * ix.n <= dense, f"long-doc subset path not taken: workspace {sub} (subset) vs {dense} (dense)"


def check_search(ix, Qd, flt, E, k, ref_cols, tol):
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
        print(f"row {b}: max |score - oracle| = {err:.3e} (bound {tol:.0e})")
        np.testing.assert_allclose(s[b][live][fin], want[fin], atol=tol, rtol=0)
        assert np.isneginf(s[b][~live]).all()
    assert_ranking_consistent(pos, ref_cols, tol)
    return s, i


# ------------------------------------------------------------------ a. one filter, every dispatch shape
# B per slot: bf16 -- the streaming scan (1, 2), the direct scan (3, kLongDirectMaxB), 8 waves x 4 queries
# (kLongDirectMaxB + 1; 33: two query groups); MXFP8 -- the streaming scan, 4 waves x 2 queries (kF8SmallMaxB), 8 x 8
# (kF8SmallMaxB + 1; 65: two groups); faithful (the pair kernel, forced): 1, 5, 20.
BS = {"bf16": (1, 2, 3, K_LONG_DIRECT, K_LONG_DIRECT + 1, 33),
      "mxfp8": (1, 2, K_F8_SMALL, K_F8_SMALL, K_F8_SMALL + 1, 65),
      "faithful": (1, 1, 5, 5, 20, 20)}
# (slot, ld, lq, k, m, id_base); m = 0: every doc (m = n under forced SUBSET)
SHAPES = [
    (0, 256, 32, 20, 201, 0),       # m mod 4 = 1
    (0, 512, 32, 20, 1, 0),         # m = 1: doc n - 1 alone
    (1, 256, 32, 20, 2, 0),         # m = 2: docs 0 and n - 1
    (1, 1024, 32, 20, 62, 0),       # m mod 4 = 2
    (2, 256, 32, 10, 3, 0),         # m = 3: with the empty doc
    (2, 512, 32, 10, 51, 1000),     # m mod 4 = 3; id_base
    (3, 512, 20, 30, 100, 0),       # lq = 20
    (3, 1024, 32, 30, 37, 0),
    (4, 256, 32, 30, 153, 0),
    (4, 1024, 1, 10, 50, 0),        # lq = 1
    (4, 512, 32, 30, 0, 0),         # m = n
    (5, 256, 32, 20, 90, 0),
    (5, 512, 32, 20, 45, 0),
    (5, 1024, 32, 64, 30, 0),       # k > m
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("slot,ld,lq,k,m,id_base", SHAPES)
def test_subset_long(dev, world, kind, slot, ld, lq, k, m, id_base):
    B, N = BS[kind][slot], NDOCS[ld]
    m = m or N
    E = allowed(N, m)
    assert E[-1] == N - 1 and (m < 2 or E[0] == 0)
    ix = world.index(kind, ld, id_base)
    assert ix.ld == ld and ix.n == N and ix.faithful == (kind == "faithful") and ix.fp8 == (kind == "mxfp8")
    if m >= 4:       # an allowed doc of each kind: empty, 128 tokens, 129, ld
        assert {0, 128, 129, ld} <= set(ix.doclens.cpu().numpy()[E].tolist())
    Q = world.q(B, lq)
    Qd = dev_queries(kind, Q, dev)
    flt = ix.filter(ids=E + id_base)
    assert flt.count == m
    ix.set_option(_lib.OPT_FILTER_BAND, BAND_OFF)            # the faithful index: one score per (query, allowed doc)
    assert_subset_taken(ix, flt, B, lq, k)                   # (leaves FILTER_SUBSET set)
    s, i = check_search(ix, Qd, flt, E, k, world.ref_cols(kind, ix, ld, Q, E), TOL[kind])
    if kind == "faithful":
        assert (ix.last_band.cpu().numpy() == -1).all()
    if k > m:
        assert (i[:, m:] == -1).all() and np.isneginf(s[:, m:]).all()
    if m >= 3 and k >= m:                                    # the allowed empty doc keeps its id, after every finite score
        assert all(id_base + 1 in row for row in i) and np.isneginf(s[:, :m]).any(axis=1).all()
    for path in (AUTO, DENSE):                               # the automatic choice and the dense path: same bits
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        s0, i0 = ix.search(Qd, k, filter=flt)
        assert np.array_equal(i0.cpu().numpy(), i) and np.array_equal(_bits(s0.cpu().numpy()), _bits(s)), path


# ------------------------------------------------------------------ b. the feature is there
@pytest.mark.parametrize("kind", KINDS)
def test_long_docs_have_a_subset_path(dev, world, kind):
    """ld = 256: under FILTER_SUBSET the workspace of a filtered search (one
    filter, and per-query filters) is smaller than the dense path's by the whole
    [B][n] score block (per-query filters on the faithful index: [B][n] leaves and
    the candidate matrix [B][M] of the pair kernel comes in); on the faithful
    index the forced band runs (last_band >= k on every row)."""
    ld, B, lq, k = 256, 5, 32, 10
    N = NDOCS[ld]
    ix = world.index(kind, ld)
    flts = [ix.filter(ids=allowed(N, 100, seed=j)) for j in range(3)]
    ix.set_option(_lib.OPT_FILTER_BAND, BAND_OFF)
    sub, dense = ws_sizes(ix, flts[0], B, lq, k)
    assert sub + 4 * B * N <= dense, (sub, dense)
    fb = ix.filter_batch([flts[0], flts[1], flts[2], flts[0], flts[1]])
    sub, dense = ws_sizes(ix, fb, B, lq, k, batch=True)
    cand = cand_bytes(kind == "faithful", B, 100)      # the faithful rows' candidate matrix [B][100] replaces [B][n]
    assert sub - cand + 4 * B * N <= dense, (sub, dense, cand)
    if kind == "faithful":
        ix.set_option(_lib.OPT_FILTER_BAND, BAND_ON)
        ix.search(dev_queries(kind, world.q(B, lq), dev), k, filter=flts[0])
        band = ix.last_band.cpu().numpy()
        assert ((band >= k) & (band <= 100)).all(), band


# ------------------------------------------------------------------ c. the faithful band on long docs
def run_band(ix, Qd, k, flt, band, cap=BAND_CAP):
    """One filtered faithful search under CBV2_OPT_FILTER_BAND = band -> (score bits, ids, status)."""
    ix.set_option(_lib.OPT_FILTER_BAND, band)
    s, i = ix._search_filtered(Qd, k, "maxsim", flt, cap=cap)
    return _bits(s.cpu().numpy()), i.cpu().numpy(), ix.last_band.cpu().numpy()


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("ld,m", [(256, 150), (1024, 110)])      # (the 1024-slot corpus holds 124 docs)
def test_band_long(dev, world, ld, m, B):
    """FILTER_BAND = 1: the bits of the pair path and of cbv2_score_f32's columns; status in [k, m] (m <= the
    default cap of 16384, so no row can overflow)."""
    k, lq = 10, 32
    E = allowed(NDOCS[ld], m)
    ix = world.index("faithful", ld)
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    ix.set_option(_lib.OPT_FILTER_BAND, BAND_ON)
    Q = world.q(B, lq, seed=1)
    Qd, flt = Q.to(dev), ix.filter(ids=E)
    assert m <= BAND_CAP
    s, i = check_search(ix, Qd, flt, E, k, world.ref_cols("faithful", ix, ld, Q, E), TOL["faithful"])
    band = ix.last_band.cpu().numpy()
    print("band sizes", (ld, B, m), band.tolist())
    assert ((band >= k) & (band <= m)).all(), band
    pair = run_band(ix, Qd, k, flt, BAND_OFF)
    assert (pair[2] == -1).all()
    assert np.array_equal(pair[1], i) and np.array_equal(pair[0], _bits(s))


def test_band_overflow_long(dev):
    """cap = k on a corpus like test_gpu_long_docs.make_f32_case (ld = 256): 14 > k copies of query 0's best doc --
    its matching tokens past token 128 -- among the allowed docs share one T and one faithful score F, lb = F, and
    T >= F - beta for each of them (beta bounds |T - F|): row 0's band holds all 14 > cap.  It reports -1 and returns
    the exact bits; so does every other row."""
    N, ld, B, k = 300, 256, 3, 10
    docs, doclens, Q = make_f32_case(77, N, ld, B)
    planted = [5 + (97 * b + 31 * j) % (N - 5) for b in range(B) for j in range(3)]
    best = planted[0]                                      # query 0's tokens at [ld - 40, ld - 8): past token 128
    assert doclens[best] == ld
    E = np.setdiff1d(allowed(N, 120), planted[1:3])        # (query 0's two other planted docs score as high: out)
    copies = np.setdiff1d(E, [0, 1, 2, N - 1] + planted)[5:18]
    docs[torch.from_numpy(copies)] = docs[best].clone()
    doclens[torch.from_numpy(copies)] = ld
    E = np.union1d(E, [best])
    group = np.union1d(copies, [best])
    assert len(group) == 14 > k
    ix = ColbertIndex.faithful_f32(docs.to(dev), doclens.to(dev), id_base=7)
    ix.set_option(_lib.OPT_FILTER_PATH, SUBSET)
    flt, Qd = ix.filter(ids=E + 7), Q.to(dev)
    pair = run_band(ix, Qd, k, flt, BAND_OFF)
    rs, ri = orc.topk(ix.score(Qd).cpu().numpy()[:, E], k)
    assert np.array_equal(pair[1], 7 + E[ri]) and np.array_equal(pair[0], _bits(rs))
    assert np.array_equal(pair[1][0], 7 + group[:k])       # row 0: the tie, ids ascending
    small = run_band(ix, Qd, k, flt, BAND_ON, cap=k)
    print("status at cap = k", small[2].tolist())
    assert small[2][0] == -1 and ((small[2] == -1) | (small[2] == k)).all(), small[2]
    assert np.array_equal(small[1], pair[1]) and np.array_equal(small[0], pair[0])
    wide = run_band(ix, Qd, k, flt, BAND_ON)
    assert wide[2][0] >= 14 and ((wide[2] >= k) & (wide[2] <= len(E))).all(), wide[2]
    assert np.array_equal(wide[1], pair[1]) and np.array_equal(wide[0], pair[0])


# ------------------------------------------------------------------ d. poison
@pytest.fixture(scope="module")
def poison_case(dev, world):
    """Per kind, ld = 512: (clean index, poisoned index, E) -- the poisoned copy holds huge values in every padding
    row (t >= doclens: whole trailing 128-token blocks included) and in every row of every disallowed doc: bf16
    100.0; e4m3 0x7E under scale 0xFE; faithful 100 + 2^-10 (hi 100, residual 2^-10)."""
    cache = {}

    def get(kind):
        if kind not in cache:
            ld = 512
            docs, doclens = world.corpus(ld)
            N = NDOCS[ld]
            E = allowed(N, 60)
            bad = torch.arange(ld)[None, :] >= doclens[:, None].long()        # [N, ld] padding rows
            off = np.ones(N, bool)
            off[E] = False
            bad[torch.from_numpy(off)] = True                                  # every row of a disallowed doc
            clean = build_index(dev, kind, docs, doclens)
            if kind == "mxfp8":
                tok, sc = clean.tokens.clone(), clean.scales.clone()
                tok[bad.to(dev)] = 0x7E
                sc[bad.to(dev)] = 0xFE
                poisoned = ColbertIndex(tok, doclens.to(dev), scales=sc)
            else:
                p = docs.clone()
                p[bad] = 100.0 + 2.0 ** -10 if kind == "faithful" else 100.0
                poisoned = build_index(dev, kind, p, doclens)
                assert float(poisoned.tokens.float().max()) == 100.0
                if kind == "faithful":
                    assert float(poisoned.residual.float().abs().max()) > 0
            cache[kind] = (clean, poisoned, E)
        return cache[kind]

    yield get
    cache.clear()


@pytest.mark.parametrize("B", [1, 5, 20])
@pytest.mark.parametrize("path", [SUBSET, DENSE])
@pytest.mark.parametrize("kind", KINDS)
def test_poisoned_padding_and_disallowed_docs_never_score(dev, world, poison_case, kind, path, B):
    """Huge values in the padding rows and in EVERY disallowed doc change no bit (the faithful index: pair path and
    band alike -- the poisoned index has other bounds, so another beta and band size; the results may not move)."""
    k, lq = 30, 32
    clean, poisoned, E = poison_case(kind)
    Qd = dev_queries(kind, world.q(B, lq, seed=2), dev)
    for band in ((BAND_OFF, BAND_ON) if kind == "faithful" and path == SUBSET else (BAND_OFF,)):
        out = []
        for ix in (clean, poisoned):
            flt = ix.filter(ids=E)
            ix.set_option(_lib.OPT_FILTER_BAND, BAND_OFF)
            if path == SUBSET:
                assert_subset_taken(ix, flt, B, lq, k)
            ix.set_option(_lib.OPT_FILTER_PATH, path)
            ix.set_option(_lib.OPT_FILTER_BAND, band)
            out.append(_out(*ix.search(Qd, k, filter=flt)))
            if band == BAND_ON:
                st = ix.last_band.cpu().numpy()
                assert ((st >= k) & (st <= len(E))).all(), st
        assert np.isfinite(out[0][0].view(np.float32)[:, :10]).all()
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0]), band


# ------------------------------------------------------------------ e. per-query filters
@pytest.mark.parametrize("chunk", [0, 7])
@pytest.mark.parametrize("layout", ["edges", "mixed"])
@pytest.mark.parametrize("ld", [256, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_per_query_filters_ragged(dev, world, kind, ld, layout, chunk):
    """Row b of the ragged search equals the single-filter search of query b alone, the unfiltered columns and the
    dense path, bit for bit.  chunk = 7: lists span several work items and surplus waves of the last workgroup exit."""
    N, B, lq, k, base = NDOCS[ld], 4, 32, 20, 40
    _, doclens = world.corpus(ld)
    ix = world.index(kind, ld, base)
    Qd = dev_queries(kind, world.q(B, lq, seed=3), dev)
    sets, (a, b) = ragged_sets(layout, N, doclens)
    sets[b] = sets[a]
    flts = [ix.filter(ids=E + base) for E in sets]
    flts[b] = flts[a]                                  # two rows, one handle
    ix.set_option(_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk)
    ix.set_option(_lib.OPT_FILTER_BAND, BAND_OFF)
    fb = ix.filter_batch(flts)
    assert fb.max_count == max(len(E) for E in sets) and fb.pairs == sum(len(E) for E in sets)
    if chunk:
        assert any(len(E) > chunk for E in sets)
    assert_subset_taken(ix, fb, B, lq, k, batch=True)  # (leaves FILTER_SUBSET set)
    s, i = _out(*ix.search(Qd, k, filters=fb))
    M = ix.score(Qd).cpu().numpy()
    for r, E in enumerate(sets):
        s1, i1 = _out(*ix.search(Qd[r:r + 1], k, filter=flts[r]))
        assert np.array_equal(i[r], i1[0]) and np.array_equal(s[r], s1[0]), (r, "differs from the single-filter search")
        rs, ri = orc.topk(M[r:r + 1, E], k)
        rid = np.where(ri >= 0, base + E[np.clip(ri, 0, None)] if len(E) else -1, -1)
        assert np.array_equal(i[r], rid[0]) and np.array_equal(s[r], _bits(rs[0])), (r, "differs from the unfiltered scores")
        kk = min(k, len(E))
        assert (i[r, kk:] == -1).all() and np.isneginf(s[r, kk:].view(np.float32)).all(), (r, "padding past min(k, m_b)")
    if layout == "edges":
        assert (i[0] == -1).all() and i[2, 0] == base + N - 1 and (i[2, 1:] == -1).all()
    ix.set_option(_lib.OPT_FILTER_PATH, DENSE)
    sd, idd = _out(*ix.search(Qd, k, filters=ix.filter_batch(flts)))
    assert np.array_equal(idd, i) and np.array_equal(sd, s)


# ------------------------------------------------------------------ f. capture and replay
@pytest.mark.parametrize("form", ["bf16", "mxfp8", "faithful-band", "batch"])
def test_capture_and_replay(dev, world, form):
    """cbv2_search_filtered (bf16, MXFP8), cbv2_search_filtered_f32 with the band and cbv2_search_filtered_batch on
    ld = 256, captured once and replayed over a 0xA5 workspace, NaN / -7 outputs and changed query contents: the
    eager bits (the faithful search: its status too)."""
    ld, B, k, lq = 256, 6, 25, 32
    N = NDOCS[ld]
    kind = {"faithful-band": "faithful", "batch": "bf16"}.get(form, form)
    ix = world.index(kind, ld)
    Qs = dev_queries(kind, world.q(2 * B, lq, seed=4), dev)
    if form == "batch":
        rng = np.random.default_rng(18)
        sets = [np.sort(rng.choice(N, int(m), replace=False)) for m in (200, 3, 0, 77, 240, 12)]
        fb = ix.filter_batch([ix.filter(ids=S) for S in sets])      # waits for the device: before the capture
        assert_subset_taken(ix, fb, B, lq, k, batch=True)
        kw = {"filters": fb}
    else:
        flt = ix.filter(ids=allowed(N, 150))
        ix.set_option(_lib.OPT_FILTER_BAND, BAND_OFF)
        assert_subset_taken(ix, flt, B, lq, k)
        kw = {"filter": flt}
    band = form == "faithful-band"
    ix.set_option(_lib.OPT_FILTER_BAND, BAND_ON if band else BAND_OFF)

    def call():
        outs = ix.search(qs, k, **kw)
        return (*outs, ix.last_band) if band else outs

    qs = torch.empty_like(Qs[:B])
    eager = {}
    for j in (1, 0):
        qs.copy_(Qs[j * B:(j + 1) * B])
        eager[j] = tuple(o.clone() for o in call())
    assert not torch.equal(eager[0][1], eager[1][1])
    if band:
        assert all(((e[2] >= k) & (e[2] <= 150)).all() for e in eager.values())
    ws = ix._ws
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    try:
        with torch.cuda.graph(g, stream=side):
            outs = call()
        assert ix._ws is ws, "the workspace was reallocated in the capture"
        for n, j in enumerate((0, 1, 0)):
            ws.view(torch.uint8).fill_(0xA5)
            outs[0].fill_(float("nan"))
            for o in outs[1:]:
                o.fill_(-7)
            qs.copy_(Qs[j * B:(j + 1) * B])
            g.replay()
            torch.cuda.synchronize()
            for got, want in zip(outs, eager[j]):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, j)
    finally:
        try:
            g.reset()
        except Exception:
            pass


# ------------------------------------------------------------------ g. guard bands
GUARD_SHARDS = [("bf16", 256), ("fp8", 256), ("f32", 256), ("bf16", 1024)]


@pytest.fixture(scope="module")
def long_shards(dev):
    cache = {}

    def get(kind, ld):
        if (kind, ld) not in cache:
            cache[(kind, ld)] = Shard(dev, kind, N_SMALL, ld, False)
        return cache[(kind, ld)]

    yield get
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("B", [1, 3, 9, 33])
@pytest.mark.parametrize("kind,ld", GUARD_SHARDS)
def test_guard_bands_subset(long_shards, kind, ld, B):
    """Tokens, scales / residual, doclens, the id list, the queries, a workspace of exactly
    cbv2_search_filtered_workspace_size bytes (under SUBSET) and the outputs inside guard bands, the last allowed doc
    being doc n - 1: no guard byte changes and the results equal the wrappers' on clones of the inputs, bit for bit."""
    m, k, lq = 40, 10, 32
    sh = long_shards(kind, ld)
    with sh.case(seed=900 + B, opts=((_lib.OPT_FILTER_PATH, SUBSET), (_lib.OPT_FILTER_BAND, BAND_OFF))) as c:
        L, h, n = c.L, c.h, sh.n
        mask = c.mask(m)
        assert bool(mask[n - 1]) and bool(mask[0])
        f, fref = c.make_filter("f", mask)
        q, qdt, Qr = c.queries(B, lq)
        need = int(L.cbv2_search_filtered_workspace_size(h, f, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, DENSE))
        assert need + 4 * B * n <= int(L.cbv2_search_filtered_workspace_size(h, f, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, SUBSET))
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered(h, f, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k, filter=fref), valid=[m] * B)


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("band", [BAND_ON, BAND_OFF])
def test_guard_bands_f32(long_shards, band, B):
    """cbv2_search_filtered_f32 on the faithful ld = 256 shard, band and pair: a workspace of exactly its
    size-function's bytes, exact outputs and status."""
    m, k, lq, cap = 40, 10, 32, BAND_CAP
    sh = long_shards("f32", 256)
    with sh.case(seed=950 + B + band, opts=((_lib.OPT_FILTER_PATH, SUBSET), (_lib.OPT_FILTER_BAND, band))) as c:
        L, h, n = c.L, c.h, sh.n
        mask = c.mask(m)
        assert bool(mask[n - 1])
        f, fref = c.make_filter("f", mask)
        q, _, Qr = c.queries(B, lq)
        need = int(L.cbv2_search_filtered_f32_workspace_size(h, f, B, lq, k, cap))
        if band == BAND_OFF:
            _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, DENSE))
            assert need + 4 * B * n <= int(L.cbv2_search_filtered_f32_workspace_size(h, f, B, lq, k, cap))
            _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, SUBSET))
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        st_ = c.out("status", B * 4)
        c.run(lambda w, wb: L.cbv2_search_filtered_f32(h, f, q, B, lq, k, cap, w, wb, os_, oi, st_, c.st),
              outs=names + ["status"], ws="ws")
        c.check_topk(B, k, c.ref._search_filtered(Qr, k, "maxsim", fref, cap=cap), valid=[m] * B)
        status = c.view("status", torch.int32, B)
        assert torch.equal(status, c.ref.last_band)
        assert bool(((status >= k) & (status <= m)).all()) if band == BAND_ON else bool((status == -1).all()), status


@pytest.mark.parametrize("chunk", [0, 16])
@pytest.mark.parametrize("kind", ["bf16", "fp8", "f32"])
def test_guard_bands_ragged(long_shards, kind, chunk):
    """The same for cbv2_search_filtered_batch on ld = 256: 0, 1, 40, n and (a repeated handle) 40 docs per row."""
    counts, order = (0, 1, 40, N_SMALL), [0, 1, 2, 3, 2]
    opts = ((_lib.OPT_FILTER_PATH, SUBSET), (_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk))
    sh = long_shards(kind, 256)
    with sh.case(seed=980 + chunk, opts=opts) as c:
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
        cand = cand_bytes(kind == "f32", B, N_SMALL)
        assert need - cand + 4 * B * N_SMALL <= int(L.cbv2_search_filtered_batch_workspace_size(h, fb, B, lq, k, MAXSIM))
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_FILTER_PATH, SUBSET))
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered_batch(h, fb, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k, filters=fbref), valid=[counts[j] for j in order])


# ------------------------------------------------------------------ h. API
@pytest.mark.parametrize("path", [AUTO, SUBSET])
@pytest.mark.parametrize("index_dtype", ["fp32", "bf16", "fp8"])
def test_retriever_and_hybrid_on_long_chunks(dev, tmp_path, index_dtype, path):
    """A JinaColBERTRetriever over chunks of up to 600 tokens (a 1024-slot index): search(allowed_ids=),
    search_embeddings(filters=) and hybrid.retrieve(allowed_ids=) return allowed ids only, with the unfiltered
    search's score bits for those ids."""
    rng = np.random.default_rng(5)
    vocab = [f"w{i}" for i in range(400)]
    lens = rng.integers(20, 200, size=50)
    lens[[7, 33, 49]] = [600, 450, 300]
    corpus = [" ".join(rng.choice(vocab, size=int(n))) for n in lens]
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"), bm25_index_path=str(tmp_path / "bm25"),
                    index_dtype=index_dtype)
    r = JinaColBERTRetriever(cfg, encoder=_LongChunkEncoder())
    r.index(corpus, batch_size=16)
    ix = r.corpus_embeddings
    assert ix.ld == 1024 and ix.n == 50 and ix.faithful == (index_dtype == "fp32") and ix.fp8 == (index_dtype == "fp8")
    ix.set_option(_lib.OPT_FILTER_PATH, path)
    ids = [3, 4, 7, 17, 18, 19, 30, 33, 49]
    flt = r.make_filter([0, 7, 8, 25])
    queries = [" ".join(rng.choice(vocab, size=6)) for _ in range(2)] + [corpus[7][:60]]
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
    for q in queries:
        fin = hyb.retrieve(q, allowed_ids=S3)
        assert fin and all(f["chunk_id"] in S3 for f in fin)
        # its last stage reranks: the scores are rerank_ids' for those chunks, filter or not
        qe = r._encode_query(q).unsqueeze(0)
        cand = torch.tensor([[f["chunk_id"] for f in fin]], dtype=torch.int32, device=dev)
        rs, ri, _ = r.rerank_ids(qe, cand, len(fin))
        assert [f["chunk_id"] for f in fin] == ri[0].tolist() and [f["score"] for f in fin] == rs[0].tolist()
