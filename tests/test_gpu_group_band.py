"""GPU: the grouped faithful search's certified band (cbv2_search_grouped_f32,
CBV2_OPT_GROUP_BAND; the contract is in include/colbert_mi355x.h, the
certificates in DESIGN.md 3.9).

The expectation is always tests/_groups.oracle on ``ix.score(Q)`` -- the full
faithful scan's bits (cbv2_score_f32) -- compared with ``same_bits``: there is
no tolerance anywhere in this file.  The band may only change the work done,
never one bit of a result.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import _adversarial as adv
from _groups import groupings, oracle, same_bits
from conftest import GOLDEN
from hybrid_rag_colbertv2_amd import FakeEncoder, RAGConfig, _lib
from hybrid_rag_colbertv2_amd.index import BAND_CAP, ColbertIndex, _stream_ptr
from hybrid_rag_colbertv2_amd.retriever import JinaColBERTRetriever
from test_gpu_bounds import N_SMALL, Shard, _first_difference, _same
from test_gpu_graph_replay import _replay
from test_gpu_group import NAMES, _arena_groups, _check, _unit

pytestmark = pytest.mark.gpu
AUTO, ON, OFF = _lib.GROUP_BAND_AUTO, _lib.GROUP_BAND_ON, _lib.GROUP_BAND_OFF
MAXSIM = _lib.SCORER_MAXSIM
FOUR = ("ragged", "holes", "interleaved", "runs")


def _faithful(dev, n, ld, id_base, seed):
    """test_gpu_group._make_index's doc lengths (an empty chunk at every 17th id) on a faithful index of either ld."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = _unit(gen, dev, n, ld, 128)
    dl = torch.randint(1, ld + 1, (n,), device=dev, generator=gen, dtype=torch.int32)
    dl[::17] = 0
    return ColbertIndex.faithful_f32(x, dl, id_base=id_base)


def _poisoned(dev, B, k, r):
    return (torch.full((B, k), float("nan"), dtype=torch.float32, device=dev),
            torch.full((B, k), -7, dtype=torch.int32, device=dev),
            torch.full((B, k, r), -7, dtype=torch.int32, device=dev),
            torch.full((B, k, r), float("nan"), dtype=torch.float32, device=dev),
            torch.full((B,), -7, dtype=torch.int32, device=dev))


def _raw(ix, grp, Q, k, r, cap=BAND_CAP):
    """cbv2_search_grouped_f32 over a poisoned workspace of exactly its size and poisoned outputs -> the five outputs."""
    L, dev = _lib.lib(), ix.device
    Q = Q.to(torch.float32).contiguous()
    B, lq = int(Q.shape[0]), int(Q.shape[1])
    need = int(L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, B, lq, k, r, cap))
    assert need > 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    o = _poisoned(dev, B, k, r)
    _lib.check(L.cbv2_search_grouped_f32(ix._h, grp._h, Q.data_ptr(), B, lq, k, r, cap, ws.data_ptr(), need,
                                         *(t.data_ptr() for t in o), _stream_ptr(dev)))
    return o


def _raw_routed(ix, grp, Q, k, r):
    """cbv2_search_grouped with f32 queries, its own workspace size."""
    L, dev = _lib.lib(), ix.device
    Q = Q.to(torch.float32).contiguous()
    B, lq = int(Q.shape[0]), int(Q.shape[1])
    need = int(L.cbv2_search_grouped_workspace_size(ix._h, grp._h, B, lq, k, r, MAXSIM))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    o = _poisoned(dev, B, k, r)[:4]
    _lib.check(L.cbv2_search_grouped(ix._h, grp._h, MAXSIM, Q.data_ptr(), _lib.DTYPE_F32, B, lq, k, r, ws.data_ptr(),
                                     need, *(t.data_ptr() for t in o), _stream_ptr(dev)))
    return o


def _same_outputs(a, b, what):
    for nm, x, y in zip(NAMES, a, b):
        assert _same(x, y), f"{what}: " + _first_difference(nm, x, y)


# --------------------------------------------------------------------------- 1. parity
@pytest.fixture(scope="module")
def indexes(dev):
    cache = {}

    def get(ld, n, id_base):
        if (ld, n) not in cache:
            cache[(ld, n)] = _faithful(dev, n, ld, id_base, seed=n + ld)
        return cache[(ld, n)]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", FOUR)
@pytest.mark.parametrize("ld", [128, 256])
def test_band_equals_the_oracle_under_every_option(dev, indexes, ld, name):
    gen = torch.Generator(device=dev).manual_seed(11 + ld)
    for n, id_base in ((2203 if ld == 128 else 1203, 1000), (131, 0)):
        ix = indexes(ld, n, id_base)
        group_of, G = groupings(n)[name]
        grp = ix.groups(group_of=group_of, G=G)
        Gp = grp.count
        for B, lq in ((1, 7), (9, 32), (40, 7)):
            Q = _unit(gen, dev, B, lq, 128)
            S = ix.score(Q).cpu().numpy()
            assert np.isneginf(S).any()                                        # the empty chunks
            for k, r in ((10, 3), (1, 1), (10, 8), (Gp - 1, 2), (Gp + 7, 8)):
                what = f"ld={ld} n={n} {name} B={B} lq={lq} k={k} r={r}"
                want = oracle(S, group_of, G, k, r, id_base=id_base)
                ix.set_option(_lib.OPT_GROUP_BAND, ON)
                on = _raw(ix, grp, Q, k, r)
                _check(on[:4], want, what + " band")
                st = on[4].cpu().numpy()
                if Gp > k:                                                     # supported: no row can overflow 16384
                    assert ((st >= 1) & (st <= grp.members)).all(), (what, st)
                else:
                    assert (st == -1).all(), (what, st)
                _same_outputs(_raw_routed(ix, grp, Q, k, r), on, what + " cbv2_search_grouped")
                for opt in (AUTO, OFF):
                    ix.set_option(_lib.OPT_GROUP_BAND, opt)
                    got = _raw(ix, grp, Q, k, r)
                    _same_outputs(got, on, what + f" option {opt}")
                    assert opt == AUTO or (got[4] == -1).all()
                ix.set_option(_lib.OPT_GROUP_BAND, AUTO)
        grp.close()


# --------------------------------------------------------------------------- 2. the certificate
N_ADV, K_ADV, B_ADV = 600, 10, 4
SEEDS = (0, 1, 2, 3, 4)


def _planted_together(case):
    """Group b = every decoy and hidden doc of query b; the fillers in groups of 5 by ascending id."""
    gof = np.full(N_ADV, -1, np.int32)
    for b in range(B_ADV):
        gof[case.decoys[b]] = b
        gof[case.hidden[b]] = b
    fill = np.flatnonzero(gof < 0)
    gof[fill] = B_ADV + np.arange(len(fill)) // 5
    return gof, int(gof.max()) + 1


@functools.lru_cache(maxsize=None)
def _cert_case(lq, seed):
    """-> (case, usable): usable when, in float64, group b of the planted-together
    grouping has its best three by T among the decoys and its best three by S
    among the hidden docs, each more than beta / 2 below those decoys in T."""
    case = adv.adversarial_case(seed, N=N_ADV, B=B_ADV, lq=lq, K=K_ADV)
    pre = adv.check_preconditions(case, K_ADV)
    T, F, beta = pre["T"], pre["F"], pre["beta"]
    ok = True
    for b in range(B_ADV):
        m = np.concatenate([case.decoys[b], case.hidden[b]])
        by_t = m[np.argsort(-T[b, m], kind="stable")[:3]]
        by_s = m[np.argsort(-F[b, m], kind="stable")[:3]]
        ok = ok and set(by_t) <= set(case.decoys[b]) and set(by_s) <= set(case.hidden[b])
        ok = ok and bool(T[b, by_s].max() < T[b, by_t].min() - beta[b] / 2)
    return case, ok


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("lq", [32, 7])
def test_certificate_on_adversarial_residuals(dev, lq, seed):
    """tests/_adversarial.py: |T - S| / beta reaches 0.82 .. 0.88, the bf16 scan
    ranks ten anti-aligned decoys first and the faithful top-10 are ten aligned
    hidden docs 0.53 .. 0.64 beta below lb.  (a) singletons: the plain faithful
    search; (b) i % 300: the hidden docs lead two-chunk groups; (c) planted
    together, r = 3: the group's best three by T are decoys, its best three by
    S hidden docs more than beta / 2 below them -- the per-group band of step 7.
    A seed whose corpus does not deliver (c) on the CPU is dropped
    (test_enough_seeds_remain counts the others)."""
    case, usable = _cert_case(lq, seed)
    if not usable:
        return
    ix = ColbertIndex.faithful_f32(torch.from_numpy(case.docs).to(dev), torch.from_numpy(case.doclens).to(dev), id_base=7)
    adv.check_preconditions(case, K_ADV, bounds=ix.bounds)
    ix.set_option(_lib.OPT_GROUP_BAND, ON)
    Q = torch.from_numpy(case.Q).to(dev)
    S = ix.score(Q).cpu().numpy()
    hidden = [set((case.hidden[b] + 7).tolist()) for b in range(B_ADV)]
    together, Gt = _planted_together(case)
    cases = (("singletons", np.arange(N_ADV, dtype=np.int32), N_ADV, 1),
             ("mod 300", (np.arange(N_ADV) % 300).astype(np.int32), 300, 1), ("together", together, Gt, 3))
    for name, gof, G, r in cases:
        grp = ix.groups(group_of=gof, G=G)
        got = _raw(ix, grp, Q, K_ADV, r)
        _check(got[:4], oracle(S, gof, G, K_ADV, r, id_base=7), f"lq={lq} seed={seed} {name}")
        st = got[4].cpu().numpy()
        assert ((st >= 0) & (st < grp.members)).all(), (name, st)          # the band pruned; no row fell back
        ids = got[2].cpu().numpy()
        for b in range(B_ADV):
            if name == "singletons":
                assert set(ids[b, :, 0].tolist()) == hidden[b], (name, b)
            elif name == "mod 300":
                if len({int(h) % 300 for h in case.hidden[b]}) == K_ADV:   # no two hidden docs share a group
                    assert set(ids[b, :, 0].tolist()) == hidden[b], (name, b)
            else:
                assert got[1][b, 0].item() == b and set(ids[b, 0].tolist()) <= hidden[b], (name, b, ids[b, 0])
        if name == "singletons":
            s, i = ix.search(Q, K_ADV)
            assert _same(got[0], s) and _same(got[2][:, :, 0], i)
        grp.close()
    ix.close()


def test_enough_seeds_remain():
    for lq in (32, 7):
        assert sum(_cert_case(lq, s)[1] for s in SEEDS) >= 4, lq


# --------------------------------------------------------------------------- 3. overflow and mixed rows
# the GPU's beta is at most oracle.band_beta * kBoundUp^2 (1 + 2^-18) (tests/test_gpu_band_certificate.py);
# 1e-3 more covers the difference between the float64 T / S here and the GPU's fp32 ones many times over
BETA_UP = (1.0 + 1.0 / 1024.0) ** 2 * (1 + 2.0 ** -18)
SLACK = 1e-3


def test_overflow_and_mixed_rows(dev):
    """The four adversarial rows plus an all-zero query: every non-empty chunk
    scores 0 for it (beta = 0), its band is every non-empty member and it
    overflows any cap below that, while the planted rows' bands are their 2 K
    planted chunks.  The zero row also pins the all-ties order: group index
    ascending, chunk id ascending."""
    lq, seed = 7, 0
    case, usable = _cert_case(lq, seed)
    assert usable
    pre = adv.check_preconditions(case, K_ADV)
    T, F, beta = pre["T"], pre["F"], pre["beta"] * BETA_UP
    ix = ColbertIndex.faithful_f32(torch.from_numpy(case.docs).to(dev), torch.from_numpy(case.doclens).to(dev), id_base=7)
    ix.set_option(_lib.OPT_GROUP_BAND, ON)
    Q = torch.cat([torch.from_numpy(case.Q), torch.zeros(1, lq, 128)]).to(dev)
    S = ix.score(Q).cpu().numpy()
    nonempty = int((case.doclens > 0).sum())
    assert (S[B_ADV][case.doclens > 0] == 0).all() and np.isneginf(S[B_ADV][case.doclens == 0]).all()

    # (1) singletons, r = 1: a cap that holds the planted rows' bands but not the zero row's
    cap = 64
    for b in range(B_ADV):
        band = int((T[b] >= pre["lb"][b] - beta[b] - SLACK).sum())            # an upper bound of the row's band
        assert 2 * K_ADV <= band <= cap, (b, band)
    assert nonempty > cap
    gof = np.arange(N_ADV, dtype=np.int32)
    grp = ix.groups(group_of=gof, G=N_ADV)
    got = _raw(ix, grp, Q, K_ADV, 1, cap=cap)
    _check(got[:4], oracle(S, gof, N_ADV, K_ADV, 1, id_base=7), "mixed rows, singletons")
    st = got[4].cpu().numpy()
    assert (st[:B_ADV] >= 2 * K_ADV).all() and (st[:B_ADV] <= cap).all() and st[B_ADV] == -1, st
    if np.unique(S[B_ADV][case.doclens > 0].view(np.uint32)).size == 1:       # (+0 everywhere: the oracle's order, spelt out)
        first = np.flatnonzero(case.doclens > 0)[:K_ADV] + 7
        assert got[2][B_ADV, :, 0].tolist() == first.tolist()                  # all ties: ascending
    grp.close()

    # (2) planted together, r = 3: a cap the global band fits and the per-group bands do not
    gof, G = _planted_together(case)
    c4 = []
    for b in range(B_ADV):
        gT = np.array([T[b, gof == g].max() for g in range(G)])
        order = np.argsort(-gT, kind="stable")
        assert gT[order[K_ADV - 1]] - gT[order[K_ADV]] > 1e-4, b                # the GPU selects the same ten groups by T
        lead = [np.flatnonzero(gof == g)[np.argmax(T[b, gof == g])] for g in order[:K_ADV]]
        c4.append(int((T[b] >= F[b, lead].min() - beta[b] - SLACK).sum()))
        m = np.concatenate([case.decoys[b], case.hidden[b]])
        sg = F[b, m[np.argsort(-T[b, m], kind="stable")[:3]]].min()
        assert (T[b, m] >= sg - pre["beta"][b] + SLACK).all(), b                # step 7 collects all 2 K chunks of group b
    cap = max(max(c4), 3 * K_ADV)
    # step 7 collects at least min(r, size) chunks of each selected group: 2 K + 9 * 3 with group b
    assert cap < 2 * K_ADV + 3 * (K_ADV - 1), (c4, cap)
    grp = ix.groups(group_of=gof, G=G)
    got = _raw(ix, grp, Q, K_ADV, 3, cap=cap)
    _check(got[:4], oracle(S, gof, G, K_ADV, 3, id_base=7), "step 7 overflows")
    assert (got[4] == -1).all(), got[4]
    roomy = _raw(ix, grp, Q[:B_ADV], K_ADV, 3)
    assert (roomy[4] >= 0).all()
    _same_outputs([t[:B_ADV] for t in got[:4]], roomy, "overflow vs roomy cap")
    grp.close()
    ix.close()


# --------------------------------------------------------------------------- 4. errors
def test_errors_launch_nothing(dev, indexes):
    L = _lib.lib()
    ix, other = indexes(128, 131, 0), indexes(128, 2203, 1000)
    ix.set_option(_lib.OPT_GROUP_BAND, ON)
    gof, G = groupings(131)["interleaved"]                                      # G' = 7
    grp = ix.groups(group_of=gof, G=G)
    B, lq, k, r = 3, 32, 5, 2
    Q = _unit(torch.Generator(device=dev).manual_seed(6), dev, B, lq, 128)
    need = int(L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, B, lq, k, r, BAND_CAP))
    assert need > 0
    ws = torch.full((need + 32,), 0xA5, dtype=torch.uint8, device=dev)
    base = ws.data_ptr() + (-ws.data_ptr()) % 16
    o = _poisoned(dev, B, k, r)
    st = _stream_ptr(dev)

    def call(index=ix, groups=grp, cap=BAND_CAP, addr=base, nbytes=need, outs=None, kk=k):
        ptrs = [t.data_ptr() for t in o] if outs is None else outs
        return L.cbv2_search_grouped_f32(index._h, groups._h, Q.data_ptr(), B, lq, kk, r, cap, addr, nbytes, *ptrs, st)

    assert call(cap=k - 1) == _lib.ERR_EINVAL and b"cap must be" in L.cbv2_last_error()
    assert call(cap=BAND_CAP + 1) == _lib.ERR_EINVAL and b"cap must be" in L.cbv2_last_error()
    assert L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, B, lq, k, r, k - 1) == 0
    assert L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, B, lq, k, r, BAND_CAP + 1) == 0
    for bad in ((0, lq, k, r), (B, 0, k, r), (B, 33, k, r), (B, lq, 0, r), (B, lq, k, 0), (B, lq, k, 9)):
        assert L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, *bad, BAND_CAP) == 0, bad
    assert call(index=other) == _lib.ERR_EINVAL and b"another index" in L.cbv2_last_error()
    assert call(outs=[t.data_ptr() for t in o[:4]] + [None]) == _lib.ERR_EINVAL
    assert call(nbytes=need - 1) == _lib.ERR_EINVAL and call(addr=base + 4) == _lib.ERR_EINVAL
    assert call(addr=None) == _lib.ERR_EINVAL
    plain = ColbertIndex(torch.zeros(131, 128, 128, dtype=torch.bfloat16, device=dev),
                         torch.ones(131, dtype=torch.int32, device=dev))           # no residual
    pgrp = plain.groups(group_of=gof, G=G)
    assert call(index=plain, groups=pgrp) == _lib.ERR_ESTATE
    assert L.cbv2_search_grouped_f32_workspace_size(plain._h, pgrp._h, B, lq, k, r, BAND_CAP) == 0
    with pytest.raises(ValueError):
        ix.set_option(_lib.OPT_GROUP_BAND, 3)
    torch.cuda.synchronize()
    assert (ws == 0xA5).all()
    want = _poisoned(dev, B, k, r)
    assert all(_same(a, b) for a, b in zip(o, want)), "an output was written by a call that returned an error"
    # where the band is not taken, cap is not read
    ix.set_option(_lib.OPT_GROUP_BAND, OFF)
    small = int(L.cbv2_search_grouped_f32_workspace_size(ix._h, grp._h, B, lq, k, r, -5))
    assert 0 < small <= need
    _lib.check(call(cap=-5, nbytes=small))
    torch.cuda.synchronize()
    assert (o[4] == -1).all()
    # no member anywhere: padding and status 0
    ix.set_option(_lib.OPT_GROUP_BAND, ON)
    none = ix.groups(group_of=np.full(131, -1), G=4)
    got = _raw(ix, none, Q, k, r)
    assert torch.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all() and (got[4] == 0).all()
    ix.set_option(_lib.OPT_GROUP_BAND, AUTO)


# --------------------------------------------------------------------------- 5. hipGraph
def test_graph_replay_with_the_band_forced(dev, indexes):
    ix = indexes(128, 2203, 1000)
    ix.set_option(_lib.OPT_GROUP_BAND, ON)
    try:
        B, k, r = 4, 20, 3
        group_of, G = groupings(ix.n)["ragged"]
        grp = ix.groups(group_of=group_of, G=G)                      # created before the capture
        gen = torch.Generator(device=dev).manual_seed(B)
        sets = [(_unit(gen, dev, B, 32, 128),), (_unit(gen, dev, B, 32, 128),)]
        qs = torch.empty((B, 32, 128), dtype=torch.float32, device=dev)

        def call():
            out = ix.search_grouped(qs, k, grp, per_group=r)
            return (*out, ix.last_band)

        def check(j, outs):
            S = ix.score(sets[j][0]).cpu().numpy()
            _check(outs[:4], oracle(S, group_of, G, k, r, id_base=1000), f"replay of set {j}")
            assert (outs[4] >= 1).all()                                # the band ran in the replay

        _replay(dev, (qs,), sets, call, workspaces=lambda: (ix._ws,), others=lambda: ix.search(sets[0][0][:1], 7),
                oracle=check)
    finally:
        ix.set_option(_lib.OPT_GROUP_BAND, AUTO)


# --------------------------------------------------------------------------- 6. guard bands
def test_guard_bands(dev):
    """Workspace of exactly cbv2_search_grouped_f32_workspace_size bytes, exact
    outputs, 16-B aligned and no better, a nonzero id_base; guards that win
    when read; inputs unwritten; the wrappers' results on clones."""
    sh = Shard(dev, "f32", N_SMALL, 128, False)
    group_of, G = groupings(sh.n)["holes"]
    B, k, r, lq = 5, 10, 3, 32
    with sh.case(seed=B, opts=((_lib.OPT_GROUP_BAND, ON),)) as c:
        L = c.L
        assert c.ref.id_base != 0
        h, ref = _arena_groups(c, group_of, G)
        try:
            q, qdt, Qr = c.queries(B, lq)
            assert qdt == _lib.DTYPE_F32
            c.out("ws", int(L.cbv2_search_grouped_f32_workspace_size(c.h, h, B, lq, k, r, BAND_CAP)), align=16)
            names = list(NAMES) + ["out_status"]
            o = [c.out(nm, B * k * (r if nm in NAMES[2:] else 1) * 4) for nm in NAMES] + [c.out("out_status", B * 4)]
            c.run(lambda w, wb: L.cbv2_search_grouped_f32(c.h, h, q, B, lq, k, r, BAND_CAP, w, wb, *o, c.st),
                  outs=names, ws="ws")
            S = c.ref.score(Qr).cpu().numpy()
            got = [c.view(nm, torch.float32 if nm in (NAMES[0], NAMES[3]) else torch.int32, *shp)
                   for nm, shp in zip(NAMES, ((B, k), (B, k), (B, k, r), (B, k, r)))]
            _check(got, oracle(S, group_of, G, k, r, id_base=c.ref.id_base), "guard bands")
            st = c.view("out_status", torch.int32, B)
            assert ((st >= 1) & (st <= ref.members)).all(), st
            _same_outputs(got, c.ref.search_grouped(Qr, k, ref, per_group=r), "the wrapper on clones")
        finally:
            torch.cuda.synchronize()
            L.cbv2_groups_destroy(h)


# --------------------------------------------------------------------------- 7. Python
def test_retriever_returns_the_same_dicts(dev, tmp_path):
    toy = json.load(open(os.path.join(GOLDEN, "toy_c1.json")))
    cfg = RAGConfig(scorer="maxsim", colbert_index_path=str(tmp_path / "colbert"))
    retr = JinaColBERTRetriever(cfg, encoder=FakeEncoder(**toy["encoder"]))
    retr.index(toy["corpus"])
    ix = retr.corpus_embeddings
    assert ix.faithful
    n = len(toy["corpus"])
    keys = ["doc%d" % (i % 9) for i in range(n)]
    groups = retr.make_groups(keys)
    for q in toy["queries"][:3]:
        res = {}
        for opt in (OFF, ON, AUTO):
            ix.set_option(_lib.OPT_GROUP_BAND, opt)
            res[opt] = retr.search_grouped(q, k=4, groups=groups, per_group=3)
            band = ix.last_band
            assert isinstance(band, torch.Tensor) and band.dtype == torch.int32 and tuple(band.shape) == (1,)
            assert opt == AUTO or (band.item() >= 1) == (opt == ON)
        assert res[ON] == res[OFF] == res[AUTO] and len(res[ON]) == 4
