"""GPU: the sharded grouped search (include/colbert_mi355x.h) on
ONE GPU through the loopback communicator, one host thread and one stream per
rank as in tests/test_gpu_loopback.py.

  merges alone   cbv2_merge_group_topk / cbv2_merge_group_chunks on synthetic
                 gathered lists against the numpy model (tests/_groups_sharded.py),
                 bit for bit, up to G k = 16384 and the refusal past it;
  rows form      cbv2_group_topk_sharded on hand-made score matrices: every rank
                 equals the unsharded oracle of tests/_groups.py bit for bit;
  search form    cbv2_search_grouped_sharded on the exact corpora of
                 tests/_exact.py: every rank equals the unsharded
                 cbv2_search_grouped of the whole index bit for bit (and the
                 oracle on the exact reference scores);
  contract       two collectives per call, guard bands (tests/_arena.py) around
                 every output and workspace of the five device calls, argument
                 errors that launch and write nothing, the Python searcher.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

import _exact as ex
import _exact_shapes as shapes
from _groups import groupings, oracle, same_bits
from _groups_sharded import (merge_group_chunks, merge_group_topk, planted_fact2, shards as shard_ranges, tie_scores)
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.distributed import NativeExchange, ShardedSearcher, loopback_comms
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocGroups, _stream_ptr
from test_gpu_bounds import N_SMALL, Shard, _first_difference, _same
from test_gpu_group import ShapeIndex

pytestmark = pytest.mark.gpu
MAXSIM = _lib.SCORER_MAXSIM
NAMES = ("out_scores", "out_groups", "out_ids", "out_chunk_scores")
GROUPINGS = ("runs", "interleaved", "one_group", "singletons", "holes", "memberless", "ragged")


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _check(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = _np(g), _np(w)
        if not same_bits(g, w):
            assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
            bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
            at = tuple(bad[0])
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {g.size} slots, first at {at}: "
                                 f"got {g[at]!r}, want {w[at]!r}")
    s, c = _np(got[0]), _np(got[3])
    assert same_bits(s, np.ascontiguousarray(c[:, :, 0])), f"{what}: out_scores is not out_chunk_scores[..., 0]"


def _run_ranks(G, fn):
    """fn(r) on its own thread and stream per rank; -> the ranks' results."""
    out, errs = [None] * G, []
    torch.cuda.synchronize()                                      # what the main thread prepared is in place

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
        t.join(timeout=240)
    assert not any(t.is_alive() for t in ts), "a rank thread hung"
    if errs:
        raise errs[0][1]
    return out


class Comms:
    """G loopback handles, destroyed on exit."""

    def __init__(self, G):
        self.G = G

    def __enter__(self):
        self.h = loopback_comms(self.G)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        for h in self.h:
            _lib.lib().cbv2_comm_destroy(h)

    def gathers(self, r):
        out = (ctypes.c_int64 * 2)()
        _lib.check(_lib.lib().cbv2_comm_stats(self.h[r], out))
        return int(out[0]), int(out[1])


def _poisoned(dev, B, k, r):
    return (torch.full((B, k), float("nan"), dtype=torch.float32, device=dev),
            torch.full((B, k), -7, dtype=torch.int32, device=dev),
            torch.full((B, k, r), -7, dtype=torch.int32, device=dev),
            torch.full((B, k, r), float("nan"), dtype=torch.float32, device=dev))


# --------------------------------------------------------------------------- the merges alone
def _gathered(rng, G, B, k, r):
    """Synthetic gathered lists: few groups (the same group in many lists, one in
    every list), tie-heavy scores with +-0.0 and -inf (equal scores across
    lists), random padding, row 0 all padding; chunk ids distinct per slot."""
    in_s = tie_scores(rng, G * B, k).reshape(G, B, k)
    in_g = rng.integers(-1, max(3, k // 2), size=(G, B, k)).astype(np.int32)
    in_g[:, :, k - 1] = 2                                         # one group in every list
    in_s[:, :, k - 1] = np.where(rng.random((G, B)) < 0.5, 0.0, -0.0)
    if B > 1:
        in_g[:, 0] = -1
    in_c = tie_scores(rng, G * B * k, r).reshape(G, B, k, r)
    in_i = np.argsort(rng.random((B, k, G * r)), axis=2).astype(np.int32) + 1000   # distinct per (b, j)
    in_i = np.ascontiguousarray(in_i.reshape(B, k, G, r).transpose(2, 0, 1, 3))
    in_i[rng.random(in_i.shape) < 0.3] = -1
    if B > 1:
        in_i[:, 0] = -1
    return in_s, in_g, in_i, in_c


def _strided(dev, a, slack):
    """[G, ...] -> a device buffer with `slack` poisoned elements between the ranks' blocks, its stride."""
    G, per = a.shape[0], int(np.prod(a.shape[1:]))
    flat = np.full((G, per + slack), -7 if a.dtype == np.int32 else np.inf, dtype=a.dtype)
    flat[:, :per] = a.reshape(G, per)
    return torch.from_numpy(flat).to(dev), per + slack


def _merge_calls(dev, in_s, in_g, in_i, in_c, slack):
    L, st = _lib.lib(), _stream_ptr(dev)
    G, B, k, r = in_i.shape
    ds, stride1 = _strided(dev, in_s, slack)
    dg, _ = _strided(dev, in_g, slack)
    di, stride2 = _strided(dev, in_i, slack)
    dc, _ = _strided(dev, in_c, slack)
    o = _poisoned(dev, B, k, r)
    rc1 = L.cbv2_merge_group_topk(ds.data_ptr(), dg.data_ptr(), G, B, k, stride1, o[0].data_ptr(), o[1].data_ptr(), st)
    rc2 = L.cbv2_merge_group_chunks(di.data_ptr(), dc.data_ptr(), G, B, k, r, stride2, o[2].data_ptr(),
                                    o[3].data_ptr(), st)
    torch.cuda.synchronize()
    return rc1, rc2, o


@pytest.mark.parametrize("G", [1, 2, 8])
def test_merges_equal_the_model(dev, G):
    shapes_ = [(1, 1, 1), (5, 7, 3), (300, 100, 8), (1, 100, 3), (5, 1, 8), (300, 7, 1), (5, 100, 1), (1, 7, 8)]
    for ci, (B, k, r) in enumerate(shapes_):
        rng = np.random.default_rng(100 * G + ci)
        in_s, in_g, in_i, in_c = _gathered(rng, G, B, k, r)
        rc1, rc2, o = _merge_calls(dev, in_s, in_g, in_i, in_c, slack=0 if ci % 2 else 5)
        assert (rc1, rc2) == (0, 0), _lib.lib().cbv2_last_error()
        ws, wg = merge_group_topk(in_s, in_g, k)
        wi, wc = merge_group_chunks(in_i, in_c)
        what = f"G={G} B={B} k={k} r={r}"
        for name, g, w in zip(NAMES, o, (ws, wg, wi, wc)):
            assert same_bits(_np(g), w), f"{what}: {name} differs from the model"


@pytest.mark.parametrize("G,k", [(64, 256), (8, 2048)])
def test_merge_group_topk_at_its_limit(dev, G, k):
    """G k = 16384 is taken (128 KiB of keys in LDS); one more k is refused and nothing is written."""
    L, st, B = _lib.lib(), _stream_ptr(dev), 2
    rng = np.random.default_rng(G)
    in_s = rng.standard_normal((G, B, k)).astype(np.float32)
    in_g = rng.integers(-1, 3 * k, size=(G, B, k)).astype(np.int32)
    ds, dg = torch.from_numpy(in_s).to(dev), torch.from_numpy(in_g).to(dev)
    o = _poisoned(dev, B, k, 1)
    assert L.cbv2_merge_group_topk(ds.data_ptr(), dg.data_ptr(), G, B, k, B * k, o[0].data_ptr(), o[1].data_ptr(),
                                   st) == 0, L.cbv2_last_error()
    torch.cuda.synchronize()
    ws, wg = merge_group_topk(in_s, in_g, k)
    assert same_bits(_np(o[0]), ws) and same_bits(_np(o[1]), wg)
    k1 = k + 1
    big_s = torch.zeros((G, B, k1), dtype=torch.float32, device=dev)
    big_g = torch.zeros((G, B, k1), dtype=torch.int32, device=dev)
    o = _poisoned(dev, B, k1, 1)
    rc = L.cbv2_merge_group_topk(big_s.data_ptr(), big_g.data_ptr(), G, B, k1, B * k1, o[0].data_ptr(),
                                 o[1].data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == _lib.ERR_EUNSUPPORTED, (rc, L.cbv2_last_error())
    assert torch.isnan(o[0]).all() and (o[1] == -7).all(), "a refused merge wrote its outputs"


def test_graph_replay_of_the_merges_and_the_chunk_stage(dev):
    """The three collective-free pieces are capturable: a replay over poisoned
    outputs recomputes them from the buffers' contents at replay time (G k =
    4800: 64 KiB of keys, the dynamic-LDS attribute set inside the capture)."""
    from hybrid_rag_colbertv2_amd.index import group_chunks_rows
    from hybrid_rag_colbertv2_amd.index import merge_group_chunks as chunks_dev
    from hybrid_rag_colbertv2_amd.index import merge_group_topk as merge_dev
    from test_gpu_graph_replay import _replay
    G, B, k, r, n = 8, 3, 600, 3, 257
    group_of, Gg = groupings(n)["ragged"]
    ix = ShapeIndex(dev, n, id_base=40)
    grp = DocGroups(ix, group_of, Gg)
    sets, models = [], []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        in_s, in_g, in_i, in_c = _gathered(rng, G, B, k, r)
        S = tie_scores(rng, B, n)
        sel = rng.integers(-1, Gg + 2, size=(B, k)).astype(np.int32)
        sets.append(tuple(torch.from_numpy(x).to(dev) for x in (in_s, in_g, in_i, in_c, S, sel)))
        models.append((in_s, in_g, in_i, in_c, S, sel))
    static = [torch.empty_like(t) for t in sets[0]]

    def call():
        return (*merge_dev(static[0], static[1], k), *chunks_dev(static[2], static[3]),
                *group_chunks_rows(static[4], static[5], grp, r))

    def check(j, outs):
        from _groups_sharded import local_chunks
        in_s, in_g, in_i, in_c, S, sel = models[j]
        want = (*merge_group_topk(in_s, in_g, k), *merge_group_chunks(in_i, in_c),
                *local_chunks(S, group_of, Gg, sel, r, id_base=40))
        for m, (o, w) in enumerate(zip(outs, want)):
            assert same_bits(_np(o), w), f"replayed output {m} of input set {j} differs from the model"

    try:
        _replay(dev, static, sets, call, oracle=check)
    finally:
        torch.cuda.synchronize()
        grp.close()
        ix.close()


# --------------------------------------------------------------------------- the rows form
class RowRanks:
    """One ShapeIndex + DocGroups + score slice per contiguous shard of the columns."""

    def __init__(self, dev, S, group_of, G_groups, cuts):
        self.dev, self.parts = dev, shard_ranges(S.shape[1], cuts)
        self.G = len(self.parts)
        self.ix = [ShapeIndex(dev, b - a, id_base=a) for a, b in self.parts]
        self.grp = [DocGroups(ix, group_of[a:b], G_groups) for ix, (a, b) in zip(self.ix, self.parts)]
        # (row stride n_local + 3: the slack columns hold +inf and must never be read)
        self.S = []
        for a, b in self.parts:
            s = np.full((S.shape[0], b - a + 3), np.inf, np.float32)
            s[:, : b - a] = S[:, a:b]
            self.S.append(torch.from_numpy(s).to(dev))

    def close(self):
        torch.cuda.synchronize()
        for g in self.grp:
            g.close()
        for ix in self.ix:
            ix.close()

    def call(self, comms, r, B, k, rr):
        """cbv2_group_topk_sharded on rank r: a poisoned workspace of exactly its size, poisoned outputs."""
        L = _lib.lib()
        need = int(L.cbv2_group_sharded_workspace_bytes(self.grp[r]._h, comms.h[r], B, k, rr))
        assert need > 0
        ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=self.dev)
        o = _poisoned(self.dev, B, k, rr)
        c0 = comms.gathers(r)
        _lib.check(L.cbv2_group_topk_sharded(self.grp[r]._h, comms.h[r], self.S[r].data_ptr(), self.S[r].shape[1], B,
                                             k, rr, ws.data_ptr(), need, *(x.data_ptr() for x in o),
                                             _stream_ptr(self.dev)))
        c1 = comms.gathers(r)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 0), "two all-gathers per call, no all-reduce"
        torch.cuda.current_stream().synchronize()
        return [x.cpu().numpy() for x in o]


def _cut_configs(n):
    """(G, cuts): even cuts, an empty shard, a shard smaller than k, a duplicate cut."""
    return [(2, [n // 2]),
            (3, [0, n // 2]),                                            # rank 0 is empty
            (4, [2, n // 3, 2 * n // 3]),                                # rank 0 holds 2 chunks (< k)
            (8, sorted([n * (g + 1) // 8 for g in range(7)][:5] + [n // 8, n // 8]))]   # duplicate cuts: empty ranks


@pytest.mark.parametrize("name", GROUPINGS)
def test_rows_form_equals_the_unsharded_oracle(dev, name):
    n, B = 300, 3
    group_of, G_groups = groupings(n)[name]
    Gp = np.unique(group_of[group_of >= 0]).size
    rng = np.random.default_rng(GROUPINGS.index(name))
    S = tie_scores(rng, B, n)
    used = np.unique(group_of[group_of >= 0])
    if used.size > 1:
        S[:, group_of == used[rng.integers(used.size)]] = -np.inf     # one group -inf everywhere
    ks = (1, 5, Gp + 3)
    for ci, (G, cuts) in enumerate(_cut_configs(n)):
        ranks = RowRanks(dev, S, group_of, G_groups, cuts)
        try:
            with Comms(G) as comms:
                for ki, k in enumerate(ks):
                    r = (1, 3, 8)[(ci + ki + GROUPINGS.index(name)) % 3]
                    want = oracle(S, group_of, G_groups, k, r)
                    outs = _run_ranks(G, lambda rank: ranks.call(comms, rank, B, k, r))
                    for rank, got in enumerate(outs):
                        _check(got, want, f"{name} G={G} cuts={cuts} k={k} r={r} rank {rank}")
        finally:
            ranks.close()


def test_rows_form_planted_runner_up(dev):
    """Fact 2: group 0's runner-up sits on rank 1, where group 0 is outside the local top-1."""
    S, group_of, G_groups, k, r, cuts = planted_fact2()
    ranks = RowRanks(dev, S, group_of, G_groups, cuts)
    try:
        with Comms(2) as comms:
            outs = _run_ranks(2, lambda rank: ranks.call(comms, rank, 1, k, r))
        want = oracle(S, group_of, G_groups, k, r)
        assert want[2].tolist() == [[[0, 4]]]
        for rank, got in enumerate(outs):
            _check(got, want, f"planted, rank {rank}")
    finally:
        ranks.close()


# --------------------------------------------------------------------------- the search form
def _build(kind, x, dl, id_base, dev):
    x, dl = torch.from_numpy(x).to(dev), torch.from_numpy(dl).to(dev)
    if kind == "fp32":
        return ColbertIndex.faithful_f32(x, dl, id_base=id_base)
    if kind == "mxfp8":
        return ColbertIndex.mxfp8(x, dl, id_base=id_base)
    return ColbertIndex(x.to(torch.bfloat16), dl, id_base=id_base)


def _empty_index(kind, ld, dev, id_base):
    tok = torch.empty((0, ld, 128), dtype=torch.uint8 if kind == "mxfp8" else torch.bfloat16, device=dev)
    dl = torch.empty((0,), dtype=torch.int32, device=dev)
    if kind == "mxfp8":
        return ColbertIndex(tok, dl, id_base=id_base, scales=torch.empty((0, ld, 2), dtype=torch.uint8, device=dev))
    if kind == "fp32":
        return ColbertIndex(tok, dl, id_base=id_base, residual=torch.empty_like(tok), bounds=(0.0, 0.0))
    return ColbertIndex(tok, dl, id_base=id_base)


SEARCH_CASES = [(kind, ld) for kind in ex.KINDS for ld in (128, 256)]


@pytest.mark.parametrize("kind,ld", SEARCH_CASES, ids=[f"{k}-{ld}" for k, ld in SEARCH_CASES])
def test_search_form_equals_the_unsharded_search(dev, kind, ld):
    """Four shards, one of them empty.  Groups: chunk i in group i % 37, but three
    chunks are emptied (doclens 0, score -inf) and put into two groups of their
    own -- group 37: an empty chunk on rank 0 and a scoring chunk on the last
    rank (-inf on one rank, finite on another); group 38: empty chunks on two
    ranks (-inf everywhere) -- and group 39 has no member at all."""
    n, nq = shapes.SIZE[ld]
    c = ex.cached_corpus(kind, ld, n, nq, seed=1)
    X = c.docs_f32()
    dl = c.doclens.copy()
    parts = shard_ranges(n, [n // 4, n // 4, 3 * n // 4])              # rank 1 is empty
    z0, z1, z2, live = 3, 7, n - 5, n - 9
    dl[[z0, z1, z2]] = 0
    assert dl[live] > 0
    group_of = (np.arange(n) % 37).astype(np.int32)
    group_of[[z0, live]] = 37
    group_of[[z1, z2]] = 38
    G_groups, Gp = 40, 39
    ref = c.ref.astype(np.float32)                                   # [nq, 32, n], exact
    ref[:, :, [z0, z1, z2]] = -np.inf
    full = _build(kind, X, dl, 0, dev)
    full_g = full.groups(group_of=group_of, G=G_groups)
    shards_ = [_build(kind, X[a:b], dl[a:b], a, dev) if b > a else _empty_index(kind, ld, dev, a) for a, b in parts]
    grps = [ix.groups(group_of=group_of[a:b], G=G_groups) for ix, (a, b) in zip(shards_, parts)]
    G = len(parts)
    comms = loopback_comms(G)
    nxs = [NativeExchange(shards_[r], comm=comms[r]) for r in range(G)]
    Qall = torch.from_numpy(c.queries_f32()).to(dev)
    try:
        for bi, B in enumerate((1, 5, 17)):
            Q = Qall[:B].contiguous() if kind == "fp32" else Qall[:B].to(torch.bfloat16).contiguous()
            k, r = ((5, 3), (Gp + 3, 8), (1, 1))[bi]

            def rank(rk):
                c0 = nxs[rk].comm_stats()
                out = [x.cpu() for x in nxs[rk].search_grouped(Q, k, grps[rk], per_group=r)]
                c1 = nxs[rk].comm_stats()
                assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 0)
                return out

            outs = _run_ranks(G, rank)
            want = [x.cpu() for x in full.search_grouped(Q, k, full_g, per_group=r)]
            exact = oracle(ref[:B, ex.LQ - 1], group_of, G_groups, k, r)
            _check(want, exact, f"{kind} ld={ld} B={B}: the unsharded search vs the exact reference")
            for rk, got in enumerate(outs):
                _check(got, want, f"{kind} ld={ld} B={B} k={k} r={r} rank {rk}")
            if k > Gp:
                g = outs[0][1].numpy()
                assert (g[:, Gp:] == -1).all() and 37 in g[0] and 38 in g[0] and 39 not in g[0]
                j = int(np.flatnonzero(g[0] == 38)[0])
                assert outs[0][2][0, j, :2].tolist() == [z1, z2] and np.isneginf(outs[0][3][0, j, :2].numpy()).all()
    finally:
        torch.cuda.synchronize()
        del nxs
        for g in grps + [full_g]:
            g.close()


def test_python_searcher_agrees_with_the_c_abi(dev):
    """ShardedSearcher.search_grouped: native (the C ABI over a loopback handle)
    on every rank, the torch path's device ops at world 1, long queries through
    score() and the rows form, and the refusal of keyed groups."""
    gen = torch.Generator().manual_seed(5)
    n, B, k, r = 500, 4, 9, 3
    docs = torch.randn(n, 128, 128, generator=gen).bfloat16().to(dev)
    lens = torch.randint(0, 129, (n,), generator=gen, dtype=torch.int32).to(dev)
    Q = torch.randn(B, 32, 128, generator=gen).bfloat16().to(dev)
    Qlong = torch.randn(2, 70, 128, generator=gen).bfloat16().to(dev)
    group_of = (np.arange(n) * 7 % 41).astype(np.int32)
    full = ColbertIndex(docs, lens)
    full_g = full.groups(group_of=group_of, G=41)
    want = [x.cpu() for x in full.search_grouped(Q, k, full_g, per_group=r)]
    want_long = [x.cpu() for x in full.search_grouped(Qlong, k, full_g, per_group=r)]
    one = ShardedSearcher(full, world=1)                             # the torch path: _DeviceOps, no collective
    _check([x.cpu() for x in one.search_grouped(Q, k, full_g, per_group=r)], want, "world 1, device ops")
    with pytest.raises(ValueError, match="group_of"):
        one.search_grouped(Q, k, full.groups(keys=[i % 5 for i in range(n)]), per_group=r)
    parts = shard_ranges(n, [100, 350])
    G = len(parts)
    shards_ = [ColbertIndex(docs[a:b].contiguous(), lens[a:b].contiguous(), id_base=a) for a, b in parts]
    grps = [ix.groups(group_of=group_of[a:b], G=41) for ix, (a, b) in zip(shards_, parts)]
    comms = loopback_comms(G)
    sss = [ShardedSearcher(shards_[rk], world=G, comm=comms[rk]) for rk in range(G)]

    def rank(rk):
        a = [x.cpu() for x in sss[rk].search_grouped(Q, k, grps[rk], per_group=r)]
        b = [x.cpu() for x in sss[rk].search_grouped(Qlong, k, grps[rk], per_group=r)]
        return a, b

    try:
        for rk, (a, b) in enumerate(_run_ranks(G, rank)):
            _check(a, want, f"native searcher, rank {rk}")
            _check(b, want_long, f"native searcher, long queries, rank {rk}")
    finally:
        torch.cuda.synchronize()
        del sss


def test_retriever_uses_its_searcher(dev, tmp_path):
    """JinaColBERTRetriever.search_grouped goes through ``searcher`` when it has one
    (world 1 here: the same answer as without), and then takes no per-chunk keys."""
    import json
    import os

    from conftest import GOLDEN
    from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig
    from hybrid_rag_colbertv2_amd.retriever import JinaColBERTRetriever
    toy = json.load(open(os.path.join(GOLDEN, "toy_c1.json")))
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"), index_dtype="bf16")
    retr = JinaColBERTRetriever(cfg, encoder=FakeEncoder(**toy["encoder"]))
    retr.index(toy["corpus"])
    n = len(toy["corpus"])
    group_of = (np.arange(n) % 6).astype(np.int32)
    grp = retr.corpus_embeddings.groups(group_of=group_of, G=9)           # groups 6-8: on no shard
    want = [retr.search_grouped(q, k=4, groups=grp, per_group=3) for q in toy["queries"][:3]]

    class Counting(ShardedSearcher):
        calls = 0

        def search_grouped(self, *a, **kw):
            Counting.calls += 1
            return super().search_grouped(*a, **kw)

    retr.searcher = Counting(retr.corpus_embeddings, world=1)
    got = [retr.search_grouped(q, k=4, groups=grp, per_group=3) for q in toy["queries"][:3]]
    assert got == want and Counting.calls == 3
    assert len(retr.search_grouped(toy["queries"][0], k=8, groups=grp)) == 6   # k past the non-empty groups
    with pytest.raises(ValueError, match="group_of"):
        retr.search_grouped(toy["queries"][0], k=4, groups=[i % 6 for i in range(n)])
    grp.close()


# --------------------------------------------------------------------------- guard bands (tests/_arena.py)
def _arena_groups(c, group_of, G):
    L, n = c.L, c.sh.n
    host = torch.from_numpy(np.ascontiguousarray(group_of, dtype=np.int32))
    c.out("groups_buf", int(L.cbv2_groups_bytes(n, G)), align=16)
    h = ctypes.c_void_p()
    c.run(lambda w, wb: L.cbv2_groups_create(c.h, host.data_ptr(), G, w, wb, c.st, ctypes.byref(h)), ws="groups_buf")
    c.A.freeze("groups_buf")
    return h


def _views(c, B, k, r):
    shp = ((B, k), (B, k), (B, k, r), (B, k, r))
    return [c.view(nm, torch.float32 if nm in (NAMES[0], NAMES[3]) else torch.int32, *s) for nm, s in zip(NAMES, shp)]


def test_guard_bands_merges_and_chunk_stage(dev):
    """cbv2_merge_group_topk, cbv2_merge_group_chunks and cbv2_group_chunks_rows
    with every buffer at exactly its size between guards that win when read
    (+inf scores, group / id 7 that no list holds)."""
    sh = Shard(dev, "bf16", N_SMALL, 128, False)
    G, B, k, r = 4, 9, 12, 8
    rng = np.random.default_rng(3)
    in_s, in_g, in_i, in_c = _gathered(rng, G, B, k, r)
    with sh.case(seed=1) as c:
        L = c.L
        ps = c.put("in_s", torch.from_numpy(in_s), "scores", align=4)
        pg = c.put("in_g", torch.from_numpy(in_g), "ids", align=4, fill=7)
        pi = c.put("in_i", torch.from_numpy(in_i), "ids", align=4, fill=7)
        pc = c.put("in_c", torch.from_numpy(in_c), "scores", align=4)
        o = [c.out(nm, B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES]
        c.run(lambda w, wb: L.cbv2_merge_group_topk(ps, pg, G, B, k, B * k, o[0], o[1], c.st), outs=NAMES[:2])
        c.run(lambda w, wb: L.cbv2_merge_group_chunks(pi, pc, G, B, k, r, B * k * r, o[2], o[3], c.st),
              outs=NAMES[2:])
        got = _views(c, B, k, r)
        ws, wg = merge_group_topk(in_s, in_g, k)
        wi, wc = merge_group_chunks(in_i, in_c)
        for name, g, w in zip(NAMES, got, (ws, wg, wi, wc)):
            assert same_bits(_np(g), w), f"guard bands: {name} differs from the model"
    # the chunk stage: the selection of the merged groups, +inf in the slack columns and the guards
    n, ld = sh.n, sh.n + 5
    group_of, Gg = groupings(n)["ragged"]
    with sh.case(seed=2) as c:
        L = c.L
        h = _arena_groups(c, group_of, Gg)
        try:
            S = tie_scores(rng, B, ld)
            S[:, n:] = np.inf
            sc = c.put("scores", torch.from_numpy(S.reshape(-1)[: (B - 1) * ld + n].copy()), "scores", align=4)
            sel = rng.integers(-1, Gg + 2, size=(B, k)).astype(np.int32)     # padding and indices >= G among them
            psel = c.put("sel", torch.from_numpy(sel), "ids", align=4, fill=0)
            c.out("ws", int(L.cbv2_group_chunks_workspace_size(B, k)), align=16)
            oi, oc = c.out("out_ids", B * k * r * 4), c.out("out_chunk_scores", B * k * r * 4)
            c.run(lambda w, wb: L.cbv2_group_chunks_rows(h, sc, ld, B, k, r, psel, w, wb, oi, oc, c.st),
                  outs=["out_ids", "out_chunk_scores"], ws="ws")
            from _groups_sharded import local_chunks
            wi, wc = local_chunks(S[:, :n], group_of, Gg, sel, r, id_base=c.ref.id_base)
            assert same_bits(_np(c.view("out_ids", torch.int32, B, k, r)), wi)
            assert same_bits(_np(c.view("out_chunk_scores", torch.float32, B, k, r)), wc)
        finally:
            torch.cuda.synchronize()
            L.cbv2_groups_destroy(h)


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_guard_bands_sharded_calls(dev, kind):
    """Two ranks, each with its own arena over the same shard: rank 0 groups the
    even chunks, rank 1 the odd ones, so together they hold the grouping once
    and the result is the wrappers' grouped search of the one shard.  Both
    sharded calls, workspaces and outputs at exactly their sizes."""
    G, B, k, r, lq = 2, 5, 10, 3, 32
    shs = [Shard(dev, kind, N_SMALL, 128, False) for _ in range(G)]
    n = shs[0].n
    group_of, Gg = groupings(n)["holes"]
    mine = [np.where(np.arange(n) % 2 == rk, group_of, -1).astype(np.int32) for rk in range(G)]
    with Comms(G) as comms:
        def rank(rk):
            with shs[rk].case(seed=11) as c:                       # the same seed: the same queries on both ranks
                L = c.L
                h = _arena_groups(c, mine[rk], Gg)
                try:
                    q, qdt, Qr = c.queries(B, lq)
                    c.out("ws", int(L.cbv2_search_grouped_sharded_workspace_size(c.h, h, comms.h[rk], B, lq, k, r,
                                                                                 MAXSIM)), align=16)
                    o = [c.out(nm, B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES]
                    c.run(lambda w, wb: L.cbv2_search_grouped_sharded(c.h, h, comms.h[rk], MAXSIM, q, qdt, B, lq, k,
                                                                      r, w, wb, *o, c.st), outs=list(NAMES), ws="ws")
                    ref_g = c.ref.groups(group_of=group_of, G=Gg)
                    want = c.ref.search_grouped(Qr, k, ref_g, per_group=r)
                    got = _views(c, B, k, r)
                    for nm, g, w in zip(NAMES, got, want):
                        assert _same(g, w), _first_difference(nm, g, w)
                    # the rows form over the wrappers' scores of this shard
                    S = c.ref.score(Qr).contiguous()
                    sc = c.put("scores", S, "scores", align=4)
                    c.out("ws2", int(L.cbv2_group_sharded_workspace_bytes(h, comms.h[rk], B, k, r)), align=16)
                    o2 = [c.out(nm + "2", B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES]
                    c.run(lambda w, wb: L.cbv2_group_topk_sharded(h, comms.h[rk], sc, n, B, k, r, w, wb, *o2, c.st),
                          outs=[nm + "2" for nm in NAMES], ws="ws2")
                    for nm, w in zip(NAMES, want):
                        g = c.view(nm + "2", w.dtype, *w.shape)
                        assert _same(g, w), _first_difference(nm + " (rows form)", g, w)
                    ref_g.close()
                finally:
                    torch.cuda.synchronize()
                    L.cbv2_groups_destroy(h)
            return True

        assert _run_ranks(G, rank) == [True] * G


# --------------------------------------------------------------------------- argument errors
def test_argument_errors_launch_and_write_nothing(dev):
    L, st = _lib.lib(), _stream_ptr(dev)
    n, B, k, r = 50, 2, 4, 2
    ix = ShapeIndex(dev, n)
    grp = DocGroups(ix, np.arange(n) % 5, 5)
    S = torch.zeros((B, n), dtype=torch.float32, device=dev)
    sel = torch.zeros((B, k), dtype=torch.int32, device=dev)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=dev)
    o = _poisoned(dev, B, k, r)
    p = [x.data_ptr() for x in o]

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(o[0]).all() and (o[1] == -7).all() and (o[2] == -7).all() and torch.isnan(o[3]).all()
                    and (ws == 0xA5).all())

    try:
        need = int(L.cbv2_group_chunks_workspace_size(B, k))
        assert need == 2 * 256 and L.cbv2_group_chunks_workspace_size(0, k) == 0
        chunk = lambda **kw: L.cbv2_group_chunks_rows(                                              # noqa: E731
            kw.get("g", grp._h), kw.get("S", S.data_ptr()), kw.get("ld", n), kw.get("B", B), kw.get("k", k),
            kw.get("r", r), kw.get("sel", sel.data_ptr()), kw.get("ws", ws.data_ptr()), kw.get("wb", need), p[2], p[3],
            st)
        for bad in (dict(g=None), dict(S=None), dict(ld=n - 1), dict(B=0), dict(k=0), dict(r=0), dict(r=9),
                    dict(sel=None), dict(ws=None), dict(wb=need - 1), dict(ws=ws.data_ptr() + 4)):
            assert chunk(**bad) == _lib.ERR_EINVAL, bad
            assert untouched(), bad
        ins, ing = S.data_ptr(), sel.data_ptr()
        for args in ((None, ing, 1, B, k, B * k), (ins, None, 1, B, k, B * k), (ins, ing, 0, B, k, B * k),
                     (ins, ing, 65, B, k, B * k), (ins, ing, 1, 0, k, B * k), (ins, ing, 1, B, 0, B * k),
                     (ins, ing, 2, B, k, B * k - 1)):
            assert L.cbv2_merge_group_topk(*args, p[0], p[1], st) == _lib.ERR_EINVAL, args
            assert untouched(), args
        for args in ((None, ins, 1, B, k, r, B * k * r), (ing, ins, 0, B, k, r, B * k * r),
                     (ing, ins, 65, B, k, r, B * k * r), (ing, ins, 1, B, k, 0, B * k * r),
                     (ing, ins, 1, B, k, 9, B * k * r), (ing, ins, 2, B, k, r, B * k * r - 1)):
            assert L.cbv2_merge_group_chunks(*args, p[2], p[3], st) == _lib.ERR_EINVAL, args
            assert untouched(), args
        # the sharded calls: a refusal comes before any collective, so one rank alone may ask
        with Comms(2) as comms:
            cm = comms.h[0]
            assert L.cbv2_group_sharded_workspace_bytes(None, cm, B, k, r) == 0
            assert L.cbv2_group_sharded_workspace_bytes(grp._h, None, B, k, r) == 0
            for bad in ((0, k, r), (B, 0, r), (B, k, 0), (B, k, 9)):
                assert L.cbv2_group_sharded_workspace_bytes(grp._h, cm, *bad) == 0, bad
            wb = int(L.cbv2_group_sharded_workspace_bytes(grp._h, cm, B, k, r))
            assert 0 < wb <= ws.numel()
            call = lambda **kw: L.cbv2_group_topk_sharded(                                           # noqa: E731
                kw.get("g", grp._h), kw.get("c", cm), kw.get("S", S.data_ptr()), kw.get("ld", n), kw.get("B", B),
                kw.get("k", k), kw.get("r", r), kw.get("ws", ws.data_ptr()), kw.get("wb", wb),
                kw.get("o0", p[0]), p[1], p[2], p[3], st)
            for bad in (dict(g=None), dict(c=None), dict(S=None), dict(ld=n - 1), dict(B=0), dict(k=0), dict(r=0),
                        dict(r=9), dict(ws=None), dict(wb=wb - 1), dict(ws=ws.data_ptr() + 4), dict(o0=None)):
                assert call(**bad) == _lib.ERR_EINVAL, (bad, L.cbv2_last_error())
                assert untouched(), bad
            assert comms.gathers(0) == (0, 0)
        with Comms(64) as comms:                                    # G k = 64 * 257 > 16384
            kk = 257
            big = _poisoned(dev, B, kk, 1)
            wb = int(L.cbv2_group_sharded_workspace_bytes(grp._h, comms.h[0], B, kk, 1))
            wsb = torch.full((wb,), 0xA5, dtype=torch.uint8, device=dev)
            rc = L.cbv2_group_topk_sharded(grp._h, comms.h[0], S.data_ptr(), n, B, kk, 1, wsb.data_ptr(), wb,
                                           *(x.data_ptr() for x in big), st)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_EUNSUPPORTED, (rc, L.cbv2_last_error())
            assert comms.gathers(0) == (0, 0) and (wsb == 0xA5).all() and torch.isnan(big[0]).all()
    finally:
        torch.cuda.synchronize()
        grp.close()
        ix.close()
