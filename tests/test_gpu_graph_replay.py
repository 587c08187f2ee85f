"""GPU: hipGraph capture and replay of every compute entry point the header
lists as capturable (include/colbert_mi355x.h, Conventions).

A serving loop captures a call once and replays it per batch.  A captured
call freezes what the host decided at capture time -- pointers, work splits,
ring slots, whether a step was skipped -- so every replay must re-initialise
all the device state it depends on.  The eager tests cannot see that.

``_replay`` does, for every case of the table below:

 1. runs eager calls of other shapes and then the call itself on two input
    sets (the workspaces are allocated and at their final size before the
    capture; the eager results are the bit-for-bit reference);
 2. captures the call on one side stream (linear: no fork or join);
 3. before EACH of three replays (sets 0, 1, 0): runs the other-shape eager
    calls on the same handle and workspace, fills the workspace with 0xA5
    bytes and the outputs with NaN / -7, copies the set into the static
    input buffers, replays, synchronises, compares.

A row or slot a replay failed to write stays NaN / -7; a counter or flag
initialised only at capture time is 0xA5A5A5A5 at replay.  Each replay is
compared with the eager call (bit for bit: scores, ids, positions, status
words) and with the float64 oracle: on tests/_grid.py data every dtype is
exact, so ids, order and score BITS must equal the oracle's (bf16, MXFP8,
fp32-faithful); long documents and the literal scorer use random corpora,
bit-equality with eager and their files' tolerances.

The ring case pins what a capturing cbv2_score does with the handle's
128-slot counter ring (it takes no slot: a graph and eager calls never share
one), the timing case that captured launches are not timed.
"""
import re

import numpy as np
import pytest
import torch

from _grid import GridCorpus
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import (ColbertIndex, _stream_ptr, merge_topk, quantize_mxfp8, select_topk)
from oracle import oracle as orc

gpu = pytest.mark.gpu

# The case table's entry points: the header's list of capturable calls names
# exactly these (test_header_lists_the_case_table).
ENTRY_POINTS = (
    "cbv2_score", "cbv2_score_f32", "cbv2_quantize_mxfp8",
    "cbv2_search", "cbv2_search_f32", "cbv2_search_filtered",
    "cbv2_rerank", "cbv2_rerank_ws", "cbv2_rerank_f32",
    "cbv2_select_topk", "cbv2_topk_rows", "cbv2_merge_topk", "cbv2_split_f32",
)
HALF = 64          # query rows [0, B) are input set 0, [HALF, HALF + B) set 1
K2 = 100


def test_header_lists_the_case_table():
    text = open(_lib.HEADER).read()
    a = text.index("hipGraph capture.")
    b = text.index("Outside the list", a)
    listed = set(re.findall(r"\bcbv2_\w+", text[a:text.index("A replay re-initialises", a)]))
    assert listed == set(ENTRY_POINTS), sorted(listed ^ set(ENTRY_POINTS))
    assert not (set(re.findall(r"\bcbv2_\w+", text[b:text.index("*/", b)])) & set(ENTRY_POINTS))


# --------------------------------------------------------------------------- helpers
def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _poison(t: torch.Tensor) -> None:
    if t.is_floating_point():
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(0xF9)
    else:
        t.fill_(-7)


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _replay(dev, static, sets, call, workspaces=lambda: (), others=lambda: None, oracle=None, captured=None,
            order=(0, 1, 0)):
    """See the module docstring.  static: the input buffers the call reads;
    sets: two tuples of tensors copied into them; call() -> output tensor(s);
    workspaces() -> the workspace tensors the call uses (read after step 1);
    others(): eager calls of other shapes on the same handle and workspace;
    oracle(j, outs): the check of a replay of set j against the oracle;
    captured(): runs right after the capture (the captured call's scan plan)."""
    def load(j):
        for dst, src in zip(static, sets[j]):
            dst.copy_(src)

    others()
    eager = {}
    for j in (1, 0):
        load(j)
        eager[j] = tuple(o.clone() for o in _tuple(call()))
    ws = [w for w in workspaces() if w is not None]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    try:
        with torch.cuda.graph(g, stream=side):     # leaves the capture on an exception too
            outs = _tuple(call())
        if captured is not None:
            captured()
        now = [w for w in workspaces() if w is not None]
        assert len(now) == len(ws) and all(a is b for a, b in zip(now, ws)), "a workspace was reallocated in the capture"
        for n, j in enumerate(order):
            others()
            for w in ws:
                w.view(torch.uint8).fill_(0xA5)
            for o in outs:
                _poison(o)
            load(j)
            g.replay()
            torch.cuda.synchronize()
            for m, (o, e) in enumerate(zip(outs, eager[j])):
                assert _same(o, e), f"replay {n} (input set {j}): output {m} differs from the eager call"
            if oracle is not None:
                oracle(j, outs)
    finally:
        try:
            g.reset()
        except Exception:
            pass
    return outs


def _rows(j, B):
    return np.arange(B) + (HALF if j else 0)


def _full_scores(g: GridCorpus) -> np.ndarray:
    """Exact float64 maxsim of every query with every doc ([B, N]): the max over
    each doc's code set (an empty set scores -inf), summed over the query
    tokens, and the planted docs' own scores."""
    T = torch.from_numpy(np.asarray(g.T, np.float64))                       # [B, lq, K]
    K = T.shape[2]
    bits = ((g.masks[:, None].astype(np.int64) >> np.arange(K)) & 1).astype(bool)                    # [N, K]
    pop = bits.sum(axis=1)
    W = max(int(pop.max()), 1)
    codes = np.argsort(~bits, axis=1, kind="stable")[:, :W]                 # a doc's codes first, ascending
    codes = torch.from_numpy(np.where(np.arange(W)[None, :] < pop[:, None], codes, codes[:, :1]))    # padded by a repeat
    out = torch.empty((g.B, g.N), dtype=torch.float64)
    for a in range(0, g.N, 1024):
        out[:, a:a + 1024] = T[:, :, codes[a:a + 1024]].amax(dim=3).sum(dim=1)
    out = out.numpy()
    out[:, pop == 0] = -np.inf
    out[:, g.planted_flat] = g.planted_scores
    return out


class Grid:
    """A grid corpus with 2 * HALF (or ``B``) queries, its exact full score
    matrix and top-K2, and its indexes (built once per module, on demand)."""

    def __init__(self, dev, N, B=2 * HALF, k=K2, full=True):
        self.dev, self.g, self.k = dev, GridCorpus(N, B, seed=N % 1000 + 7), k
        self.full = _full_scores(self.g) if full else None
        self.es, self.ei = self.g.topk(k)
        self._ix = {}

    def index(self, kind) -> ColbertIndex:
        if kind not in self._ix:
            dl = self.g.doclens_on(self.dev)
            if kind == "f32":
                x = self.g.tokens_on(self.dev, torch.float32)
                ix = ColbertIndex.faithful_f32(x, dl)
                del x
            else:
                t = self.g.tokens_on(self.dev)
                ix = ColbertIndex.mxfp8(t, dl) if kind == "fp8" else ColbertIndex(t, dl)
            assert not ix.dense_docs          # ragged: B <= 2 takes the streaming scan by default
            self._ix[kind] = ix
        return self._ix[kind]

    def queries(self, rows, kind="bf16") -> torch.Tensor:
        return torch.from_numpy(self.g.Q[rows]).to(self.dev, torch.float32 if kind == "f32" else torch.bfloat16)

    def qsets(self, B, kind="bf16"):
        return [(self.queries(_rows(0, B), kind),), (self.queries(_rows(1, B), kind),)]

    def topk_oracle(self, k):
        """oracle(j, (scores, ids, ...)) of a search of rows _rows(j, B) for the top k <= self.k."""
        def check(j, outs):
            s, i = outs[0].cpu().numpy(), outs[1].cpu().numpy()
            r = _rows(j, s.shape[0])
            assert np.array_equal(i, self.ei[r, :k]), "ids / order differ from the float64 oracle"
            assert np.array_equal(_bits(s), _bits(self.es[r, :k])), "score bits differ from the float64 oracle"
        return check


@pytest.fixture(scope="module")
def g20k(dev):
    return Grid(dev, 20_000)


@pytest.fixture(scope="module")
def g70k(dev):
    return Grid(dev, 70_000, B=4, full=False)


def _others_search(G, ix, kind="bf16"):
    """Eager calls of other shapes on the same handle (and so the same workspace)."""
    qa, qb = G.queries(np.arange(5) + 17, kind), G.queries(np.arange(33) + 3, kind)

    def run():
        ix.search(qa, 37)
        ix.search(qb, K2)
        ix.score(qa)
    return run


# --------------------------------------------------------------------------- score
@gpu
@pytest.mark.parametrize("B,dense", [(1, 0), (1, 1), (2, 0), (2, 1), (4, 0), (12, 0), (64, 0)])
def test_score_bf16(dev, g20k, B, dense):
    ix = g20k.index("bf16")
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    big = g20k.queries(np.arange(HALF))
    try:
        ix.set_option(_lib.OPT_DENSE_DOCS, dense)
        ix.score(big)
        wide = ix.last_scan_plan()
        assert wide["dynamic_tail"]                  # B = 64, eager: a ring slot and the dynamic tail
        if B != 64:
            qs.copy_(g20k.queries(_rows(0, B)))
            ix.score(qs)
            # the streaming scan (B <= 2, ragged docs) plans no split; every other shape does
            assert (ix.last_scan_plan() == wide) == (B <= 2 and not dense), (B, dense, ix.last_scan_plan(), wide)

        def oracle(j, outs):
            assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(g20k.full[_rows(j, B)]))

        def captured():       # no ring slot inside a capture: the static split (same scores)
            assert B != 64 or not ix.last_scan_plan()["dynamic_tail"]

        _replay(dev, (qs,), g20k.qsets(B), lambda: ix.score(qs), others=lambda: (ix.score(big[:7]), ix.score(big[:33])),
                oracle=oracle, captured=captured)
    finally:
        ix.set_option(_lib.OPT_DENSE_DOCS, 0)


@gpu
@pytest.mark.parametrize("B", [1, 64])
def test_score_mxfp8_quantizer_inside(dev, g20k, B):
    """cbv2_quantize_mxfp8 of the queries and cbv2_score in one capture."""
    ix = g20k.index("fp8")
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    big = g20k.queries(np.arange(HALF))

    def oracle(j, outs):
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(g20k.full[_rows(j, B)]))

    _replay(dev, (qs,), g20k.qsets(B), lambda: ix.score(qs), others=lambda: ix.score(big[:9]), oracle=oracle)


@gpu
def test_quantize_mxfp8_alone(dev):
    g = torch.Generator().manual_seed(5)
    sets = [(torch.randn(300, 128, generator=g).to(dev),) for _ in range(2)]
    sets[1][0][::7] = 0
    x = torch.empty((300, 128), dtype=torch.float32, device=dev)

    def oracle(j, outs):
        q, sc = orc.mxfp8_quantize(sets[j][0].cpu().numpy())
        assert np.array_equal(outs[0].cpu().numpy(), q) and np.array_equal(outs[1].cpu().numpy(), sc)

    _replay(dev, (x,), sets, lambda: quantize_mxfp8(x), oracle=oracle)


@gpu
def test_score_f32(dev, g20k):
    B = 3
    ix = g20k.index("f32")
    qs = torch.empty((B, 32, 128), dtype=torch.float32, device=dev)

    def oracle(j, outs):
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(g20k.full[_rows(j, B)]))

    _replay(dev, (qs,), g20k.qsets(B, "f32"), lambda: ix.score(qs), workspaces=lambda: (ix._ws,),
            others=_others_search(g20k, ix, "f32"), oracle=oracle)


@gpu
def test_score_long_docs(dev):
    from test_gpu_long_docs import ATOL, make_case
    N, ld, B = 3000, 256, 40
    docs, doclens, Q0 = make_case(11, N, ld, B)
    Q1 = Q0.flip(0).contiguous()          # the second input set: the rows in reverse (one oracle pass serves both)
    ix = ColbertIndex(docs.to(dev), doclens.to(dev))
    assert ix.ld == ld
    ref = orc.maxsim(Q0.float().numpy(), docs.float().numpy(), doclens.numpy())
    ref = np.concatenate([ref, ref[::-1]])
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    ix.score(Q0.to(dev))
    assert ix.last_scan_plan()["workgroups"] > 0

    def oracle(j, outs):
        got, want = outs[0].cpu().numpy(), ref[j * B:(j + 1) * B]
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], atol=ATOL, rtol=0)

    _replay(dev, (qs,), [(Q0.to(dev),), (Q1.to(dev),)], lambda: ix.score(qs),
            others=lambda: ix.score(Q1[:5].to(dev)), oracle=oracle)


@gpu
def test_score_ref_meanpool_cosine(dev):
    N, B = 300, 3
    g = torch.Generator().manual_seed(21)
    docs = torch.randn(N, 128, 128, generator=g)
    doclens = torch.randint(1, 129, (N,), generator=g, dtype=torch.int32)
    Q = torch.randn(2 * B, 20, 128, generator=g)
    ix = ColbertIndex(docs.bfloat16().to(dev), doclens.to(dev))
    ix.build_means(docs.to(dev))                        # not capturable: before the capture
    ref = orc.meanpool_cosine(Q.numpy(), docs.numpy(), doclens.numpy())
    qs = torch.empty((B, 20, 128), dtype=torch.float32, device=dev)

    def oracle(j, outs):
        np.testing.assert_allclose(outs[0].cpu().numpy(), ref[j * B:(j + 1) * B], atol=1e-5, rtol=0)

    _replay(dev, (qs,), [(Q[:B].to(dev),), (Q[B:].to(dev),)], lambda: ix.score(qs, scorer="ref_meanpool_cosine"),
            others=lambda: ix.score(Q[:1].to(dev), scorer="ref_meanpool_cosine"), oracle=oracle)


# --------------------------------------------------------------------------- search
@gpu
@pytest.mark.parametrize("B,k,fused", [(1, 10, 0), (5, 100, 0), (64, 100, 0), (64, 100, 1)])
def test_search_bf16(dev, g20k, B, k, fused):
    ix = g20k.index("bf16")
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    try:
        ix.set_option(_lib.OPT_FUSED_TOPK, fused)
        assert (ix.fused_topk_slots(B, k) > 0) == bool(fused)
        if B == 64:
            ix.search(g20k.queries(_rows(0, B)), k)
            assert ix.last_scan_plan()["dynamic_tail"]

        def captured():       # the counters are in the workspace: a captured search keeps its tail
            assert B != 64 or ix.last_scan_plan()["dynamic_tail"]

        _replay(dev, (qs,), g20k.qsets(B), lambda: ix.search(qs, k), workspaces=lambda: (ix._ws,),
                others=_others_search(g20k, ix), oracle=g20k.topk_oracle(k), captured=captured)
    finally:
        ix.set_option(_lib.OPT_FUSED_TOPK, 0)


@gpu
@pytest.mark.parametrize("bmax", [1, 0])
def test_search_bf16_70k_select_counters(dev, g70k, bmax):
    """Rows long enough for the block-max select (its arrival counters) and,
    with CBV2_OPT_TOPK_BMAX 0, for the sampled filter (its cnt)."""
    ix = g70k.index("bf16")
    B = 2
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    sets = [(g70k.queries(np.arange(2)),), (g70k.queries(np.arange(2) + 2),)]
    q3 = g70k.queries(np.array([1, 2, 3]))

    def oracle(j, outs):
        r = np.arange(2) + 2 * j
        assert np.array_equal(outs[1].cpu().numpy(), g70k.ei[r])
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(g70k.es[r]))

    try:
        ix.set_option(_lib.OPT_TOPK_BMAX, bmax)
        _replay(dev, (qs,), sets, lambda: ix.search(qs, K2), workspaces=lambda: (ix._ws,),
                others=lambda: (ix.search(q3, 10), ix.search(q3[:1], K2)), oracle=oracle)
    finally:
        ix.set_option(_lib.OPT_TOPK_BMAX, 1)


@gpu
def test_search_bf16_multipass_select(dev):
    N, B, k = 6000, 3, 2000
    G = Grid(dev, N, B=2 * B, k=k, full=False)
    ix = G.index("bf16")
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    sets = [(G.queries(np.arange(B)),), (G.queries(np.arange(B) + B),)]

    def oracle(j, outs):
        r = np.arange(B) + B * j
        assert np.array_equal(outs[1].cpu().numpy(), G.ei[r])
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(G.es[r]))

    _replay(dev, (qs,), sets, lambda: ix.search(qs, k), workspaces=lambda: (ix._ws,),
            others=lambda: ix.search(sets[1][0][:2], 1500), oracle=oracle)


@gpu
def test_search_mxfp8(dev, g20k):
    B = 64
    ix = g20k.index("fp8")
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    _replay(dev, (qs,), g20k.qsets(B), lambda: ix.search(qs, K2), workspaces=lambda: (ix._ws,),
            others=_others_search(g20k, ix), oracle=g20k.topk_oracle(K2))


@gpu
@pytest.mark.parametrize("B,cap,p1", [(1, None, 1), (1, None, 0), (12, None, 1), (1, K2, 1), (12, K2, 1)])
def test_search_f32(dev, g20k, B, cap, p1):
    """cbv2_search_f32: split_query_kernel zeroes count / lb / done / arrive;
    cap = k makes rows overflow into the on-device full-scan fallback (-1)."""
    ix = g20k.index("f32")
    qs = torch.empty((B, 32, 128), dtype=torch.float32, device=dev)

    def call():
        s, i = ix.search(qs, K2) if cap is None else ix._search_f32(qs, B, 32, K2, cap=cap)
        return s, i, ix.last_band

    check = g20k.topk_oracle(K2)
    seen = []

    def oracle(j, outs):
        check(j, outs)
        st = outs[2].cpu().numpy()
        seen.append(st)
        assert ((st >= K2) | (st == -1)).all() if cap else (st >= K2).all(), st

    try:
        ix.set_option(_lib.OPT_P1_COLLECT_FUSED, p1)
        _replay(dev, (qs,), g20k.qsets(B, "f32"), call, workspaces=lambda: (ix._ws,),
                others=_others_search(g20k, ix, "f32"), oracle=oracle)
    finally:
        ix.set_option(_lib.OPT_P1_COLLECT_FUSED, 1)
    if cap:
        assert any((st == -1).any() for st in seen), "no row overflowed cap = k: the fallback did not run"


# --------------------------------------------------------------------------- filtered search
@pytest.fixture(scope="module")
def gflt(dev):
    G = Grid(dev, 2500, B=18, k=1)
    rng = np.random.default_rng(3)
    G.mask = rng.random(2500) < 0.3
    return G


@gpu
@pytest.mark.parametrize("kind", ["bf16", "f32"])
@pytest.mark.parametrize("path", [_lib.FILTER_SUBSET, _lib.FILTER_DENSE])
@pytest.mark.parametrize("B", [1, 9])
def test_search_filtered(dev, gflt, kind, path, B):
    k = 40
    ix = gflt.index(kind)
    allowed = np.nonzero(gflt.mask)[0]
    flt = ix.filter(mask=torch.from_numpy(gflt.mask))     # waits for the device: created before the capture
    assert flt.count == len(allowed)
    qs = torch.empty((B, 32, 128), dtype=torch.float32 if kind == "f32" else torch.bfloat16, device=dev)
    sets = [(gflt.queries(np.arange(B), kind),), (gflt.queries(np.arange(B) + 9, kind),)]
    q4 = gflt.queries(np.arange(4) + 3, kind)

    def oracle(j, outs):
        r = np.arange(B) + 9 * j
        es, ep = orc.topk(gflt.full[r][:, allowed], k)
        assert np.array_equal(outs[1].cpu().numpy(), allowed[ep])
        assert np.array_equal(_bits(outs[0].cpu().numpy()), _bits(es))

    try:
        ix.set_option(_lib.OPT_FILTER_PATH, path)
        _replay(dev, (qs,), sets, lambda: ix.search(qs, k, filter=flt), workspaces=lambda: (ix._ws,),
                others=lambda: (ix.search(q4, 7, filter=flt), ix.search(q4, 25)), oracle=oracle)
    finally:
        ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_AUTO)
        flt.close()


@gpu
def test_search_filtered_empty_filter(dev, gflt):
    """m = 0: the call writes only the padding -- at every replay."""
    ix, B, k = gflt.index("bf16"), 5, 12
    flt = ix.filter(mask=torch.zeros(2500, dtype=torch.bool))
    assert flt.count == 0
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    sets = [(gflt.queries(np.arange(B)),), (gflt.queries(np.arange(B) + 9),)]

    def oracle(j, outs):
        assert torch.isneginf(outs[0]).all() and (outs[1] == -1).all()

    _replay(dev, (qs,), sets, lambda: ix.search(qs, k, filter=flt), workspaces=lambda: (ix._ws,),
            others=lambda: ix.search(sets[0][0], 20), oracle=oracle)
    flt.close()


# --------------------------------------------------------------------------- rerank, selection, conversion
def _rerank_oracle(G, B, cands):
    def check(j, outs):
        r, cand = _rows(j, B), cands[j]
        s, i, p = (o.cpu().numpy() for o in outs)
        k = s.shape[1]
        for b in range(B):
            exp = orc.rerank_select(G.full[r[b], cand[b]], k)
            assert p[b].tolist() == [e[0] for e in exp], b
            assert i[b].tolist() == [int(cand[b, e[0]]) for e in exp], b
            assert np.array_equal(_bits(s[b]), _bits(np.array([e[1] for e in exp]))), b
    return check


def _cand_sets(G, B, C, kind="bf16"):
    rng = np.random.default_rng(B * C)
    cands = [rng.integers(0, G.g.N, size=(B, C)).astype(np.int32) for _ in range(2)]
    for j in range(2):        # the planted docs of each row (score ties included) among its candidates
        cands[j][:, :10] = G.g.planted[_rows(j, B)]
    sets = [(G.queries(_rows(j, B), kind), torch.from_numpy(cands[j]).to(G.dev)) for j in range(2)]
    return cands, sets


@gpu
@pytest.mark.parametrize("kind,B", [("bf16", 1), ("f32", 5)])
def test_rerank_ws_and_f32(dev, g20k, kind, B):
    """cbv2_rerank_ws (bf16 index, its candidate-parallel workspace) and cbv2_rerank_f32."""
    C, k = 50, 10
    ix = g20k.index(kind)
    cands, sets = _cand_sets(g20k, B, C, kind)
    qs, cs = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])
    other = _cand_sets(g20k, 3, 20, kind)[1][0]
    _replay(dev, (qs, cs), sets, lambda: ix.rerank(qs, cs, k),
            workspaces=lambda: (ix._rr_ws,) if kind == "bf16" else (ix._ws,),
            others=lambda: ix.rerank(other[0], other[1], 5), oracle=_rerank_oracle(g20k, B, cands))


@gpu
@pytest.mark.parametrize("B,C", [(40, 50), (2, 3000)])
def test_rerank_no_workspace(dev, g20k, B, C):
    """cbv2_rerank (C = 3000: the dynamic-LDS kernel)."""
    k = 10
    ix = g20k.index("bf16")
    cands, sets = _cand_sets(g20k, B, C)
    qs, cs = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])
    out = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev),
           torch.empty((B, k), dtype=torch.int32, device=dev))

    def call():
        _lib.check(_lib.lib().cbv2_rerank(ix._h, qs.data_ptr(), B, 32, cs.data_ptr(), C, k, out[0].data_ptr(),
                                          out[1].data_ptr(), out[2].data_ptr(), _stream_ptr(dev)))
        return out

    _replay(dev, (qs, cs), sets, call, others=lambda: ix.rerank(qs[:1], cs[:1, :33], 0),
            oracle=_rerank_oracle(g20k, B, cands))


def _tied_rows(seed, B, n):
    """Scores on a coarse grid: thousands of exact ties per row."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, n, generator=g) * 64).round() / 64


@gpu
@pytest.mark.parametrize("C,k", [(1024, 10), (5000, 100)])
def test_select_topk(dev, C, k):
    B = 4
    sets = [(_tied_rows(C + j, B, C).to(dev), torch.randperm(B * C, generator=torch.Generator().manual_seed(j))
             .view(B, C).to(dev, torch.int32)) for j in range(2)]
    sc, ids = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])

    def oracle(j, outs):
        s, i, p = (o.cpu().numpy() for o in outs)
        raw, rid = sets[j][0].cpu().numpy(), sets[j][1].cpu().numpy()
        for b in range(B):
            exp = orc.rerank_select(raw[b], k)
            assert p[b].tolist() == [e[0] for e in exp] and i[b].tolist() == [int(rid[b, e[0]]) for e in exp]
            assert np.array_equal(_bits(s[b]), _bits(np.array([e[1] for e in exp])))

    _replay(dev, (sc, ids), sets, lambda: select_topk(sc, k, ids=ids),
            others=lambda: select_topk(sets[0][0][:2, :700], 3), oracle=oracle)


@gpu
@pytest.mark.parametrize("n,k,with_ws", [(100_000, 100, True), (5000, 1025, False)])
def test_topk_rows(dev, n, k, with_ws):
    B = 2
    L = _lib.lib()
    sets = [(_tied_rows(n + j, B, n).to(dev),) for j in range(2)]
    sets[1][0][0, ::3] = float("-inf")
    x = torch.empty_like(sets[0][0])
    need = int(L.cbv2_topk_workspace_bytes(B, n)) if with_ws else 0
    assert need > 0 or not with_ws
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    out = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev))

    def call():
        _lib.check(L.cbv2_topk_rows(x.data_ptr(), B, n, n, k, 5, ws.data_ptr() if need else None, need,
                                    out[0].data_ptr(), out[1].data_ptr(), _stream_ptr(dev)))
        return out

    def other():
        o = (torch.empty((1, 7), dtype=torch.float32, device=dev), torch.empty((1, 7), dtype=torch.int32, device=dev))
        _lib.check(L.cbv2_topk_rows(x.data_ptr(), 1, n - 3, n, 7, 0, ws.data_ptr() if need else None, need,
                                    o[0].data_ptr(), o[1].data_ptr(), _stream_ptr(dev)))

    def oracle(j, outs):
        es, ei = orc.topk(sets[j][0].cpu().numpy(), k, id_base=5)
        assert np.array_equal(outs[1].cpu().numpy(), ei) and np.array_equal(_bits(outs[0].cpu().numpy()), _bits(es))

    _replay(dev, (x,), sets, call, workspaces=lambda: (ws,) if need else (), others=other, oracle=oracle)


@gpu
@pytest.mark.parametrize("G,k", [(4, 100), (9, 1000)])
def test_merge_topk(dev, G, k):
    """k = 1000: lists longer than the kernel's LDS staging."""
    B, n = 3, 12_000
    cuts = np.linspace(0, n, G + 1).astype(int)
    raws = [_tied_rows(G + j, B, n).numpy() for j in range(2)]
    parts = [[orc.topk(r[:, a:b], k, id_base=a) for a, b in zip(cuts[:-1], cuts[1:])] for r in raws]
    sets = [(torch.from_numpy(np.stack([p[0] for p in ps]).astype(np.float32)).to(dev),
             torch.from_numpy(np.stack([p[1] for p in ps]).astype(np.int32)).to(dev)) for ps in parts]
    sc, ids = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])

    def oracle(j, outs):
        es, ei = orc.merge_topk(np.stack([p[0] for p in parts[j]]), np.stack([p[1] for p in parts[j]]), k)
        assert np.array_equal(outs[1].cpu().numpy(), ei) and np.array_equal(_bits(outs[0].cpu().numpy()), _bits(es))

    _replay(dev, (sc, ids), sets, lambda: merge_topk(sc, ids, k),
            others=lambda: merge_topk(sets[0][0][:2, :, :10].contiguous(), sets[0][1][:2, :, :10].contiguous(), 10),
            oracle=oracle)


@gpu
def test_split_f32_with_bounds_zeroed_in_front(dev):
    """cbv2_split_f32 accumulates its bounds by atomic max: the serving loop
    captures ``bounds.zero_()`` in front of it."""
    n, ld = 70, 128
    g = torch.Generator().manual_seed(8)
    doclens = torch.randint(0, ld + 1, (n,), generator=g, dtype=torch.int32)
    doclens[:3] = torch.tensor([0, 1, ld], dtype=torch.int32)
    xs = [torch.randn(n, ld, 128, generator=g) * sc for sc in (1.0, 0.25)]
    xs[0][5, int(doclens[5]):] = 1e6          # garbage padding: split, outside the bounds
    x = torch.empty((n, ld, 128), dtype=torch.float32, device=dev)
    dl = doclens.to(dev)
    hi, lo = (torch.empty((n, ld, 128), dtype=torch.bfloat16, device=dev) for _ in range(2))
    bounds = torch.empty(2, dtype=torch.float32, device=dev)

    def call():
        bounds.zero_()
        _lib.check(_lib.lib().cbv2_split_f32(x.data_ptr(), n * ld, ld, dl.data_ptr(), hi.data_ptr(), lo.data_ptr(),
                                             bounds.data_ptr(), _stream_ptr(dev)))
        return hi, lo, bounds

    def oracle(j, outs):
        eh, el, (E, M) = orc.split_f32(xs[j].numpy(), doclens.numpy())
        assert np.array_equal(outs[0].float().cpu().numpy(), eh) and np.array_equal(outs[1].float().cpu().numpy(), el)
        b = outs[2].tolist()
        assert E <= b[0] <= E * (1 + 2 ** -9) and M <= b[1] <= M * (1 + 2 ** -9), (b, E, M)

    _replay(dev, (x,), [(xs[0].to(dev),), (xs[1].to(dev),)], call, oracle=oracle)


# --------------------------------------------------------------------------- ring and replay counts
@gpu
def test_score_ring_not_shared_between_graph_and_eager(dev, g20k):
    """A captured cbv2_score and 300 eager ones (more than the ring's 128
    slots) on one handle, the graph replayed on a third stream in between:
    no call fails, every eager result and every replayed row is right.  Then
    two graphs of the handle replayed concurrently, 20 times."""
    B = 64
    ix = ColbertIndex(g20k.g.tokens_on(dev), g20k.g.doclens_on(dev))       # a ring no other test has advanced
    Q, Q2 = g20k.queries(_rows(0, B)), g20k.queries(_rows(1, B))
    ref, ref2 = ix.score(Q).clone(), ix.score(Q2).clone()
    assert ix.last_scan_plan()["dynamic_tail"]
    assert np.array_equal(_bits(ref.cpu().numpy()), _bits(g20k.full[_rows(0, B)]))
    assert np.array_equal(_bits(ref2.cpu().numpy()), _bits(g20k.full[_rows(1, B)]))
    streams = [torch.cuda.Stream(dev) for _ in range(3)]
    torch.cuda.synchronize()
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g1, stream=streams[2]):
            row1 = ix.score(Q)
        assert not ix.last_scan_plan()["dynamic_tail"]     # capturing: the static split, no ring slot
        outs, reps = [], []
        for j in range(300):
            with torch.cuda.stream(streams[j & 1]):
                outs.append(ix.score(Q)[:, ::997].clone())
            if j % 7 == 3:
                with torch.cuda.stream(streams[2]):
                    row1.fill_(float("nan"))
                    g1.replay()
                    reps.append(row1.clone())
        assert ix.last_scan_plan()["dynamic_tail"]         # the eager calls kept their tail
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, ref[:, ::997])
        assert len(reps) > 40
        for r in reps:
            assert _same(r, ref)
        with torch.cuda.graph(g2, stream=streams[2]):
            row2 = ix.score(Q2)
        for _ in range(20):
            row1.fill_(float("nan"))
            row2.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(streams[0]):
                g1.replay()
            with torch.cuda.stream(streams[1]):
                g2.replay()
            torch.cuda.synchronize()
            assert _same(row1, ref) and _same(row2, ref2)
    finally:
        for g in (g1, g2):
            try:
                g.reset()
            except Exception:
                pass


@gpu
def test_search_graph_replayed_300_times(dev, g20k):
    """Nothing in a replay may depend on a counter the host advanced at capture."""
    B, k = 12, K2
    ix = g20k.index("bf16")
    sets = g20k.qsets(B)
    qs = torch.empty((B, 32, 128), dtype=torch.bfloat16, device=dev)
    want = []
    for j in range(2):
        qs.copy_(sets[j][0])
        want.append(tuple(o.clone() for o in ix.search(qs, k)))
        g20k.topk_oracle(k)(j, want[j])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
            s, i = ix.search(qs, k)
        bad = torch.zeros((), dtype=torch.int64, device=dev)
        for n in range(300):
            j = n & 1
            s.fill_(float("nan"))
            i.fill_(-7)
            qs.copy_(sets[j][0])
            g.replay()
            bad += (i != want[j][1]).sum() + (s.view(torch.int32) != want[j][0].view(torch.int32)).sum()
        torch.cuda.synchronize()
        assert int(bad) == 0, f"{int(bad)} ids / score words differ over 300 replays"
    finally:
        try:
            g.reset()
        except Exception:
            pass


# --------------------------------------------------------------------------- timing
@gpu
@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_captured_launches_are_not_timed(dev, g20k, kind):
    """With time_scans on, a capture records none of the handle's timing
    events: scan_times / band_times succeed and report the eager launches."""
    B = 5
    ix = g20k.index(kind)
    qs = g20k.queries(_rows(0, B), kind)
    ix.time_scans(True)
    want = tuple(o.clone() for o in ix.search(qs, K2))
    n_scans = len(ix.scan_times())                    # scan launches of one eager search
    assert n_scans >= 1
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        ix.time_scans(True)
        with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
            s, i = ix.search(qs, K2)
        for _ in range(3):
            s.fill_(float("nan"))
            g.replay()
        torch.cuda.synchronize()
        assert _same(s, want[0]) and _same(i, want[1])
        es, ei = ix.search(qs, K2)                    # the one eager, timed search
        torch.cuda.synchronize()
        assert _same(es, want[0]) and _same(ei, want[1])
        if kind == "f32":
            bands = ix.band_times()
            assert len(bands) == 1 and bands[0] > 0, bands
        scans = ix.scan_times()
        assert len(scans) == n_scans and all(0 < t < 1000 for t in scans), scans
    finally:
        ix.time_scans(False)
        try:
            g.reset()
        except Exception:
            pass
