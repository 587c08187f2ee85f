"""GPU: grouped search -- the top-k groups (documents), each with its best chunks
(cbv2_groups_*, cbv2_group_topk_rows, cbv2_search_grouped; the contract is in
include/colbert_mi355x.h).

The oracle (tests/_groups.py) is a numpy group-reduce and sort of the GPU's OWN
score matrix -- ``ix.score(...)`` (cbv2_score / cbv2_score_f32) or the crafted
matrix of the selection tests -- on the scores' order-preserving bits, so
scores, group indices, chunk ids, chunk scores and padding are compared bit
for bit: there is no tolerance anywhere in this file.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from _grid import GridCorpus
from _groups import groupings, oracle, same_bits
from conftest import GOLDEN
from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig, _lib
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocGroups, _stream_ptr, group_topk_rows
from hybrid_rag_colbertv2_amd.retriever import JinaColBERTRetriever
from test_gpu_bounds import N_SMALL, _first_difference, _same     # the guard-band shard (tests/_arena.py)
from test_gpu_graph_replay import _replay

pytestmark = pytest.mark.gpu
MAXSIM, MEANPOOL = _lib.SCORER_MAXSIM, _lib.SCORER_REF_MEANPOOL_COSINE
NAMES = ("out_scores", "out_groups", "out_ids", "out_chunk_scores")


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        if not same_bits(g, w):
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            at = tuple(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {g.size} slots, first at {at}: "
                                 f"got {g[at]!r}, the oracle {w[at]!r}")
    s, c = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (got[0], got[3]))
    assert same_bits(s, np.ascontiguousarray(c[:, :, 0])), f"{what}: out_chunk_scores[..., 0] is not out_scores"


class ShapeIndex:
    """An index handle of n chunks that is never scanned (one dummy token row):
    what cbv2_groups_create needs of an index is its n, id_base and device, and
    the selection tests hand cbv2_group_topk_rows their own score matrices."""

    def __init__(self, dev, n, id_base=0):
        self.device, self.n, self.id_base = dev, n, id_base
        self._tok = torch.zeros(256, dtype=torch.uint8, device=dev)
        self._dl = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().cbv2_index_create(dev.index or 0, self._tok.data_ptr(), _lib.DTYPE_BF16, n, 128, 128,
                                                self._dl.data_ptr(), id_base, ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h.value:
            _lib.lib().cbv2_index_destroy(self._h)
            self._h = ctypes.c_void_p()


def _crafted(rng, B, n, ld, group_of, G):
    """[B, ld] scores on a 16-level grid (heavy ties: both tie rules decide),
    -inf columns, one group -inf throughout, +inf in the slack columns."""
    S = ((rng.integers(0, 16, size=(B, ld)) - 8) / 4.0).astype(np.float32)
    S[:, rng.random(ld) < 0.1] = -np.inf
    used = np.unique(group_of[group_of >= 0])
    if used.size > 1:
        S[:, :n][:, group_of == used[rng.integers(used.size)]] = -np.inf
    S[:, n:] = np.inf
    return S


def _raw_select(L, dev, groups, S, ld, k, r):
    """cbv2_group_topk_rows with a poisoned workspace of exactly its size and poisoned outputs."""
    B = S.shape[0]
    need = int(L.cbv2_group_topk_workspace_size(groups._h, B, k, r))
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    out_s = torch.full((B, k), float("nan"), dtype=torch.float32, device=dev)
    out_g = torch.full((B, k), -7, dtype=torch.int32, device=dev)
    out_i = torch.full((B, k, r), -7, dtype=torch.int32, device=dev)
    out_c = torch.full((B, k, r), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(L.cbv2_group_topk_rows(groups._h, S.data_ptr(), ld, B, k, r, ws.data_ptr(), need, out_s.data_ptr(),
                                      out_g.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), _stream_ptr(dev)))
    return out_s, out_g, out_i, out_c


# --------------------------------------------------------------------------- selection on crafted matrices
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049, 20011, 200003])
def test_selection_on_crafted_matrices(dev, n):
    """Every grouping of the host test (one group spanning every tile, groups
    smaller than r, memberless groups, 30 % of the chunks in no group) x B in
    {1, 3, 40} x r in {1, 3, 8} x k in {1, 10, G' + 7, 1500}: B and r rotate
    over the groupings so that each n sees all of them; k = G' + 7 (padding)
    where G' is small, k = 1500 (the k > 1024 route) where G' >= 2000."""
    L = _lib.lib()
    rng = np.random.default_rng(n)
    ix = ShapeIndex(dev, n, id_base=5000)
    ld = n + 5
    try:
        for gi, (name, (group_of, G)) in enumerate(groupings(n).items()):
            B = (1, 3, 40)[(gi + n) % 3]
            if n > 100_000 and B == 40 and name != "runs":
                B = 3                                         # (the oracle's time, not the kernels')
            r = (1, 3, 8)[(gi // 3 + gi + n) % 3]
            grp = DocGroups(ix, group_of, G)
            Gp = grp.count
            assert Gp == np.unique(group_of[group_of >= 0]).size
            S = _crafted(rng, B, n, ld, group_of, G)
            Sd = torch.from_numpy(S).to(dev)
            ks = [1, 10] + ([Gp + 7] if Gp <= 100 else []) + ([1500] if Gp >= 2000 else [])
            for k in ks:
                got = _raw_select(L, dev, grp, Sd, ld, k, r)
                _check(got, oracle(S, group_of, G, k, r, id_base=5000), f"n={n} {name} B={B} k={k} r={r}")
            assert torch.equal(Sd.cpu(), torch.from_numpy(S))          # the scores are an input
            grp.close()
    finally:
        ix.close()


def test_selection_is_independent_of_the_row_stride(dev):
    """ld = n and ld = n + 133 give the same rows; a second batch size on the same handle too."""
    L, n = _lib.lib(), 2049
    ix = ShapeIndex(dev, n)
    try:
        group_of, G = groupings(n)["ragged"]
        grp = DocGroups(ix, group_of, G)
        rng = np.random.default_rng(5)
        S = _crafted(rng, 9, n, n + 133, group_of, G)
        wide = _raw_select(L, dev, grp, torch.from_numpy(S).to(dev), n + 133, 10, 3)
        tight = _raw_select(L, dev, grp, torch.from_numpy(np.ascontiguousarray(S[:, :n])).to(dev), n, 10, 3)
        for a, b in zip(wide, tight):
            assert _same(a, b)
        _check(group_topk_rows(torch.from_numpy(S).to(dev)[:, :n], 10, grp, 3), oracle(S, group_of, G, 10, 3),
               "the Python wrapper on a strided view")
    finally:
        ix.close()


# --------------------------------------------------------------------------- cbv2_search_grouped
def _unit(gen, dev, *shape):
    x = torch.randn(*shape, device=dev, generator=gen)
    return x / x.norm(dim=-1, keepdim=True)


def _make_index(dev, kind, n, id_base, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    ld = 256 if kind == "ld256" else 128
    x = _unit(gen, dev, n, ld, 128)
    dl = torch.randint(1, ld + 1, (n,), device=dev, generator=gen, dtype=torch.int32)
    dl[::17] = 0                                              # empty docs: -inf, keep their ids
    if kind == "f32":
        return ColbertIndex.faithful_f32(x, dl, id_base=id_base)
    if kind == "fp8":
        return ColbertIndex.mxfp8(x.bfloat16(), dl, id_base=id_base)
    ix = ColbertIndex(x.bfloat16(), dl, id_base=id_base)
    if kind == "meanpool":
        ix.build_means(x)
    return ix


@pytest.fixture(scope="module")
def indexes(dev):
    cache = {}

    def get(kind, n, id_base):
        key = (kind, n, id_base)
        if key not in cache:
            cache[key] = _make_index(dev, kind, n, id_base, seed=n + id_base)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["bf16", "fp8", "f32", "ld256", "meanpool"])
def test_search_grouped_equals_the_oracle_on_its_own_scores(dev, indexes, kind):
    scorer = "ref_meanpool_cosine" if kind == "meanpool" else "maxsim"
    gen = torch.Generator(device=dev).manual_seed(11)
    for n, id_base in ((2203 if kind != "ld256" else 1203, 1000), (131, 0)):
        ix = indexes(kind, n, id_base)
        gs = groupings(n)
        for ci, (B, lq) in enumerate(((1, 7), (9, 32), (40, 7), (40, 32))):
            name = ("ragged", "holes", "interleaved", "runs")[ci]
            group_of, G = gs[name]
            grp = ix.groups(group_of=group_of, G=G)
            Q = _unit(gen, dev, B, lq, 128)
            S = ix.score(Q, scorer).cpu().numpy()
            assert np.isneginf(S).any() or kind == "meanpool"                  # the empty docs
            for k, r in ((10, 3), (grp.count + 7, 8), (1, 1)):
                got = ix.search_grouped(Q, k, grp, per_group=r, scorer=scorer)
                _check(got, oracle(S, group_of, G, k, r, id_base=id_base), f"{kind} n={n} {name} B={B} lq={lq} k={k} r={r}")
            grp.close()


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_all_singletons_is_the_plain_search(dev, indexes, kind):
    ix = indexes(kind, 2203, 1000)
    grp = ix.groups(group_of=np.arange(ix.n))
    Q = _unit(torch.Generator(device=dev).manual_seed(3), dev, 9, 32, 128)
    for k in (1, 100, 1500):
        s, i = ix.search(Q, k)
        gs, gg, gi, gc = ix.search_grouped(Q, k, grp, per_group=1)
        assert _same(gs, s), _first_difference("scores", gs, s)
        assert _same(gi[:, :, 0], i), _first_difference("ids", gi[:, :, 0], i)
        assert _same(gc[:, :, 0], s) and torch.equal(gg, i - 1000)


def test_exact_grid_ties_in_real_scores(dev):
    """tests/_grid.py: scores on an exact grid, so groups and chunks tie for real."""
    g = GridCorpus(3000, 12, seed=41)
    for kind in ("bf16", "fp8", "f32"):
        dl = g.doclens_on(dev)
        if kind == "f32":
            ix = ColbertIndex.faithful_f32(g.tokens_on(dev, torch.float32), dl)
        else:
            ix = ColbertIndex.mxfp8(g.tokens_on(dev), dl) if kind == "fp8" else ColbertIndex(g.tokens_on(dev), dl)
        Q = torch.from_numpy(g.Q).to(dev)
        S = ix.score(Q).cpu().numpy()
        group_of = (np.arange(g.N) % 211).astype(np.int32)
        group_of[g.planted[:, -1]] = 211                       # the planted exact copies tie with their originals' groups
        grp = ix.groups(group_of=group_of, G=212)
        want = oracle(S, group_of, 212, 100, 3)
        ws = want[0][:, :100]
        assert (np.diff(ws, axis=1) == 0).any(), "no tied group scores: the case does not exercise the tie rule"
        _check(ix.search_grouped(Q, 100, grp, per_group=3), want, f"grid {kind}")
        ix.close()


def test_long_queries_take_the_summed_blocks(dev, indexes):
    ix = indexes("bf16", 2203, 1000)
    group_of, G = groupings(ix.n)["ragged"]
    grp = ix.groups(group_of=group_of, G=G)
    Q = _unit(torch.Generator(device=dev).manual_seed(4), dev, 5, 40, 128)
    S = ix.score(Q).cpu().numpy()
    _check(ix.search_grouped(Q, 10, grp, per_group=3), oracle(S, group_of, G, 10, 3, id_base=1000), "lq = 40")
    keys = ["doc%d" % g if g >= 0 else None for g in group_of]
    by_key = ix.groups(keys=keys)                               # labels in order of first appearance
    assert by_key.count == grp.count and by_key.labels[0] == keys[next(i for i, x in enumerate(keys) if x is not None)]
    s, gidx, ids, cs = ix.search_grouped(Q, 10, by_key, per_group=3)
    w = oracle(S, by_key.group_of.numpy(), by_key.G, 10, 3, id_base=1000)
    _check((s, gidx, ids, cs), w, "keys")


def test_edges_and_errors(dev, indexes):
    L = _lib.lib()
    ix, other = indexes("bf16", 131, 0), indexes("bf16", 2203, 1000)
    Q = _unit(torch.Generator(device=dev).manual_seed(6), dev, 3, 32, 128)
    grp = ix.groups(group_of=np.arange(131) % 5)
    with pytest.raises(ValueError, match="another index"):      # CBV2_EINVAL before any launch
        other.search_grouped(Q, 5, grp)
    with pytest.raises(ValueError, match="per_group"):
        ix.search_grouped(Q, 5, grp, per_group=9)
    need = int(L.cbv2_search_grouped_workspace_size(ix._h, grp._h, 3, 32, 5, 2, MAXSIM))
    ws = torch.empty(need + 32, dtype=torch.uint8, device=dev)
    qb = Q.bfloat16().contiguous()
    o = [torch.empty(3 * 5 * 2, dtype=torch.int32, device=dev) for _ in range(4)]
    base = ws.data_ptr() + (-ws.data_ptr()) % 16
    for k, r in ((0, 1), (5, 0), (5, 9)):                      # k < 1, r outside [1, 8]
        assert L.cbv2_search_grouped(ix._h, grp._h, MAXSIM, qb.data_ptr(), _lib.DTYPE_BF16, 3, 32, k, r, base, need,
                                     *(t.data_ptr() for t in o), _stream_ptr(dev)) == _lib.ERR_EINVAL
        assert L.cbv2_group_topk_rows(grp._h, o[0].data_ptr(), 131, 3, k, r, base, need,
                                      *(t.data_ptr() for t in o), _stream_ptr(dev)) == _lib.ERR_EINVAL
    # a short and a misaligned workspace
    for addr, nbytes in ((base, need - 1), (base + 4, need), (None, need)):
        assert L.cbv2_search_grouped(ix._h, grp._h, MAXSIM, qb.data_ptr(), _lib.DTYPE_BF16, 3, 32, 5, 2, addr, nbytes,
                                     *(t.data_ptr() for t in o), _stream_ptr(dev)) == _lib.ERR_EINVAL
    assert L.cbv2_search_grouped(ix._h, grp._h, MAXSIM, qb.data_ptr(), _lib.DTYPE_BF16, 3, 32, 5, 2, base, need,
                                 o[0].data_ptr(), None, o[2].data_ptr(), o[3].data_ptr(), None) == _lib.ERR_EINVAL
    with pytest.raises(ValueError, match="outside"):             # a bad grouping never reaches the device
        ix.groups(group_of=np.full(131, 5), G=5)
    h = ctypes.c_void_p()
    bad = torch.full((131,), -2, dtype=torch.int32)
    buf = torch.empty(int(L.cbv2_groups_bytes(131, 5)), dtype=torch.uint8, device=dev)
    assert L.cbv2_groups_create(ix._h, bad.data_ptr(), 5, buf.data_ptr(), buf.numel(), None,
                                ctypes.byref(h)) == _lib.ERR_EINVAL and h.value is None
    assert L.cbv2_groups_create(ix._h, bad.data_ptr(), 5, buf.data_ptr(), buf.numel() - 1, None,
                                ctypes.byref(h)) == _lib.ERR_EINVAL
    # G' == 0: padding only
    none = ix.groups(group_of=np.full(131, -1), G=4)
    assert none.count == 0
    S = ix.score(Q).cpu().numpy()
    for got in (ix.search_grouped(Q, 6, none, per_group=2), group_topk_rows(ix.score(Q), 6, none, 2)):
        _check(got, oracle(S, np.full(131, -1), 4, 6, 2), "no members")
        assert torch.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all()
    # k past G': padding after the 5 groups
    s, gidx, ids, cs = ix.search_grouped(Q, 9, grp, per_group=2)
    assert torch.isneginf(s[:, 5:]).all() and (gidx[:, 5:] == -1).all() and (ids[:, 5:] == -1).all()
    assert sorted(gidx[0, :5].tolist()) == [0, 1, 2, 3, 4]


# --------------------------------------------------------------------------- hipGraph
@pytest.mark.parametrize("kind,B", [("bf16", 1), ("bf16", 12), ("fp8", 12), ("f32", 4)])
def test_graph_replay_of_search_grouped(dev, indexes, kind, B):
    ix = indexes(kind, 2203, 1000)
    group_of, G = groupings(ix.n)["ragged"]
    grp = ix.groups(group_of=group_of, G=G)                      # created before the capture
    gen = torch.Generator(device=dev).manual_seed(B)
    qdt = torch.float32 if kind == "f32" else torch.bfloat16
    sets = [(_unit(gen, dev, B, 32, 128).to(qdt),), (_unit(gen, dev, B, 32, 128).to(qdt),)]
    qs = torch.empty((B, 32, 128), dtype=qdt, device=dev)

    def check(j, outs):
        S = ix.score(sets[j][0]).cpu().numpy()
        _check(outs, oracle(S, group_of, G, 20, 3, id_base=1000), f"replay of set {j}")

    _replay(dev, (qs,), sets, lambda: ix.search_grouped(qs, 20, grp, per_group=3), workspaces=lambda: (ix._ws,),
            others=lambda: ix.search(sets[0][0][:1], 7), oracle=check)


def test_graph_replay_of_group_topk_rows(dev):
    L, n, B, k, r = _lib.lib(), 20011, 7, 1500, 3
    ix = ShapeIndex(dev, n)
    try:
        group_of, G = groupings(n)["singletons"]
        grp = DocGroups(ix, group_of, G)
        rng = np.random.default_rng(8)
        hosts = [_crafted(rng, B, n, n + 5, group_of, G) for _ in range(2)]
        sets = [(torch.from_numpy(h).to(dev),) for h in hosts]
        S = torch.empty((B, n + 5), dtype=torch.float32, device=dev)
        need = int(L.cbv2_group_topk_workspace_size(grp._h, B, k, r))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        outs = (torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int32, device=dev),
                torch.empty((B, k, r), dtype=torch.int32, device=dev),
                torch.empty((B, k, r), dtype=torch.float32, device=dev))

        def call():
            _lib.check(L.cbv2_group_topk_rows(grp._h, S.data_ptr(), n + 5, B, k, r, ws.data_ptr(), need,
                                              *(o.data_ptr() for o in outs), _stream_ptr(dev)))
            return outs

        _replay(dev, (S,), sets, call, workspaces=lambda: (ws,),
                oracle=lambda j, o: _check(o, oracle(hosts[j], group_of, G, k, r), f"replay of set {j}"))
    finally:
        ix.close()


# --------------------------------------------------------------------------- guard bands (tests/_arena.py)
@pytest.fixture(scope="module")
def shards(dev):
    from test_gpu_bounds import Shard
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Shard(dev, kind, N_SMALL, 128, False)
        return cache[kind]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _arena_groups(c, group_of, G):
    """cbv2_groups_create into a buf of exactly cbv2_groups_bytes inside the arena -> (handle, the wrappers' DocGroups)."""
    L, n = c.L, c.sh.n
    host = torch.from_numpy(np.ascontiguousarray(group_of, dtype=np.int32))
    c.out("groups_buf", int(L.cbv2_groups_bytes(n, G)), align=16)
    h = ctypes.c_void_p()
    c.run(lambda w, wb: L.cbv2_groups_create(c.h, host.data_ptr(), G, w, wb, c.st, ctypes.byref(h)), ws="groups_buf")
    c.A.freeze("groups_buf")                                      # the handle borrows it: read-only from here on
    ref = c.ref.groups(group_of=group_of, G=G)
    assert int(L.cbv2_groups_count(h)) == ref.count
    return h, ref


@pytest.mark.parametrize("kind,B", [("bf16", 1), ("bf16", 9), ("fp8", 9), ("f32", 5)])
def test_guard_bands_search_grouped(shards, kind, B):
    """Workspace, outputs and the groups buffer at exactly their sizes, 16-B
    aligned and no better; guards that win when read (doc n: full length, 100.0
    tokens); results equal the wrappers' on clones, inputs unwritten."""
    sh = shards(kind)
    group_of, G = groupings(sh.n)["holes"]
    k, r, lq = 10, 3, 32
    with sh.case(seed=B) as c:
        L = c.L
        h, ref = _arena_groups(c, group_of, G)
        try:
            q, qdt, Qr = c.queries(B, lq)
            c.out("ws", int(L.cbv2_search_grouped_workspace_size(c.h, h, B, lq, k, r, MAXSIM)), align=16)
            o = [c.out(nm, B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES]
            c.run(lambda w, wb: L.cbv2_search_grouped(c.h, h, MAXSIM, q, qdt, B, lq, k, r, w, wb, *o, c.st),
                  outs=list(NAMES), ws="ws")
            want = c.ref.search_grouped(Qr, k, ref, per_group=r)
            shapes = ((B, k), (B, k), (B, k, r), (B, k, r))
            for nm, w, shp in zip(NAMES, want, shapes):
                g = c.view(nm, w.dtype, *shp)
                assert _same(g, w), _first_difference(nm, g, w)
            S = c.ref.score(Qr).cpu().numpy()
            _check(want, oracle(S, group_of, G, k, r, id_base=c.ref.id_base), f"guard bands {kind} B={B}")
        finally:
            torch.cuda.synchronize()
            L.cbv2_groups_destroy(h)


def test_guard_bands_group_topk_rows(shards):
    """The selection alone: a score matrix of exactly (B - 1) ld + n floats with
    +inf in the slack columns [n, ld) and in the guards."""
    sh = shards("bf16")
    n, B, ld, k, r = sh.n, 9, sh.n + 5, 12, 8
    group_of, G = groupings(n)["ragged"]
    with sh.case(seed=77) as c:
        L = c.L
        h, ref = _arena_groups(c, group_of, G)
        try:
            S = _crafted(np.random.default_rng(1), B, n, ld, group_of, G)
            flat = torch.from_numpy(S.reshape(-1)[: (B - 1) * ld + n].copy())
            sc = c.put("scores", flat, "scores", align=4)
            c.out("ws", int(L.cbv2_group_topk_workspace_size(h, B, k, r)), align=16)
            o = [c.out(nm, B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES]
            c.run(lambda w, wb: L.cbv2_group_topk_rows(h, sc, ld, B, k, r, w, wb, *o, c.st), outs=list(NAMES), ws="ws")
            got = [c.view(nm, torch.float32 if nm in (NAMES[0], NAMES[3]) else torch.int32, *shp)
                   for nm, shp in zip(NAMES, ((B, k), (B, k), (B, k, r), (B, k, r)))]
            _check(got, oracle(S, group_of, G, k, r, id_base=c.ref.id_base), "guard bands, selection")
        finally:
            torch.cuda.synchronize()
            L.cbv2_groups_destroy(h)


# --------------------------------------------------------------------------- retriever level
def test_retriever_search_grouped(dev, tmp_path):
    toy = json.load(open(os.path.join(GOLDEN, "toy_c1.json")))
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"), index_dtype="bf16")
    retr = JinaColBERTRetriever(cfg, encoder=FakeEncoder(**toy["encoder"]))
    retr.index(toy["corpus"])
    n = len(toy["corpus"])
    # documents of unequal chunk counts: 25, 3, 1, then the toy's own documents; chunk 40 belongs to none
    doc = {i: "big" for i in range(25)} | {25: "three", 26: "three", 27: "three", 28: "one"}
    store = ChunkStore([{"chunk_id": i, "text": t, "document_id": doc.get(i, "toy-%d" % toy["chunks"][i]["document_id"])}
                        for i, t in enumerate(toy["corpus"]) if i != 40])
    keys = store.document_keys(n)
    assert keys[40] is None and len({k for k in keys if k is not None}) == 6
    groups = retr.make_groups(keys)
    assert groups.count == 6 and groups.labels[:3] == ["big", "three", "one"]
    for q in toy["queries"][:4]:
        res = retr.search_grouped(q, k=4, groups=groups, per_group=3)
        assert len(res) == 4 and all(set(x) == {"group", "score", "chunks"} for x in res)
        labels = [x["group"] for x in res]
        assert len(set(labels)) == 4 and set(labels) <= set(groups.labels)          # distinct documents
        assert [x["score"] for x in res] == sorted((x["score"] for x in res), reverse=True)
        flat = retr.search(q, k=n)                                                    # the chunk ranking
        rank = {d["document_id"]: j for j, d in enumerate(flat)}
        for x in res:
            ch = x["chunks"]
            assert 1 <= len(ch) <= 3 and all(set(d) == {"document_id", "score", "text"} for d in ch)
            assert ch[0]["score"] == x["score"] and all(keys[d["document_id"]] == x["group"] for d in ch)
            assert all(d["text"] == toy["corpus"][d["document_id"]] for d in ch)
            assert len(ch) == min(3, keys.count(x["group"]))
            # a group's chunks are its best in the chunk ranking, in that order
            mine = [d["document_id"] for d in flat if keys[d["document_id"]] == x["group"]][:3]
            assert [d["document_id"] for d in ch] == mine and rank[ch[0]["document_id"]] is not None
        assert all(d["document_id"] != 40 for x in res for d in x["chunks"])
        assert retr.search_grouped(q, k=50, groups=keys, per_group=1)[:4] == \
            [{**x, "chunks": x["chunks"][:1]} for x in res]
