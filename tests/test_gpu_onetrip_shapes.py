"""GPU: the one-round-trip retrieve (csrc/retrieve.cpp) at every result path x
buffer layout, against an exact CPU pipeline (tests/_onetrip_oracle.py) --
not against the library's own composed stages.

The corpora are on the k/16 grid, so ids, positions and float32 score BITS
must equal the oracle's for the bf16, fp32-faithful and MXFP8 shard alike;
with ``host=True`` the host arrays must also equal the device outputs.
Corpus A is ranked whole (k = N): negative scores (sign bit set, like a
call's tag), -inf and -1 padding pass through the tagged words and through
the host rerank's keys.  The stage-1 lists are built by hand (planted, empty,
lowest-scoring, out-of-range, stage-1-only, -1-tailed, all -1, repeated ids).

SHAPES are (k, kb_cap, kb_returned, C, final_k); PATHS are forced with the lab
knobs (restored in ``finally``) and checked through the deltas of
cbv2_retrieve_pool_stats [2] (host results from the final select's words) and
[3] (host rerank).  The layout sweep over ONE pooled buffer and the forged
tags run in a fresh child process (tests/onetrip_sweep_child.py), so the
pool starts empty; this file reads the child's JSON.  Loopback shards (G = 2)
take the same oracle, C > 1024 through cbv2_rerank_sharded's all-reduce.
"""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import _onetrip_oracle as oto
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.distributed import NativeExchange, loopback_comms
from hybrid_rag_colbertv2_amd.hybrid import OneTripRetriever
from hybrid_rag_colbertv2_amd.index import ColbertIndex

pytestmark = pytest.mark.gpu

SHAPES = (
    (100, 100, 100, 50, 10),      # 0 the shape every other one-trip test runs
    (10, 0, 0, 1, 1),             # 1 no stage 1
    (1, 1, 1, 1, 1),              # 2
    (200, 100, 60, 100, 50),      # 3 stage 1 returns fewer columns than begin's bound
    (100, 100, 100, 100, 100),    # 4 final_k = C
    (40, 100, 100, 20, 7),        # 5
    (20, 16, 16, 64, 64),         # 6 C > k + kb: candidates and results -1 padded
    (100, 100, 100, 50, 60),      # 7 final_k > C
)
SHAPE_258 = (100, 100, 100, 50, 258)   # B = 8, host: 8 (2 100 + 50) + 3 8 258 = 8192 words = a 64 KiB buffer
SHAPE_A = (256, 16, 16, 300, 300)      # corpus A, ranked whole

# path -> (index kinds, (host_rerank, prearm) knobs, batch sizes per shape index)
PATHS = {
    "host_rerank":        (("fp32",), (1, 1), (1, 2, 8, 5, 3, 8, 4, 1)),
    "host_rerank_stream": (("fp32",), (2, 1), (2, 8, 1, 3, 8, 1, 5, 4)),
    "gpu_prearmed":       (("fp32", "bf16"), (0, 1), (8, 1, 2, 4, 1, 3, 8, 5)),
    "gpu_launched":       (("bf16", "fp32"), (0, 0), (3, 4, 8, 1, 2, 8, 1, 8)),
    "final_words_mid":    (("bf16", "fp32"), (1, 1), (9, 32, 17, 9, 32, 12, 9, 32)),
    "copied":             (("bf16",), (1, 1), (40,) * 8),
    "mxfp8":              (("mxfp8",), (1, 1), (5, 8, 1, 2, 3, 4, 8, 1)),
}
SMALL = ("host_rerank", "host_rerank_stream", "gpu_prearmed", "gpu_launched", "mxfp8")


def _cases():
    out = []
    for path, (kinds, _, batches) in PATHS.items():
        for si, shape in enumerate(SHAPES):
            bs = [batches[si]]
            if si in (0, 6):       # B in {1, 2, 8, 9, 32, 40} on the first and the seventh shape
                bs = {"final_words_mid": [9, 32], "copied": [40]}.get(path, [1, 2, 8])
            for j, B in enumerate(bs):
                out.append(pytest.param(path, kinds[(si + j) % len(kinds)], "B", shape, B, id=f"{path}-s{si}-B{B}"))
        if path in SMALL:
            out.append(pytest.param(path, kinds[0], "B", SHAPE_258, 8, id=f"{path}-s258-B8"))
        out.append(pytest.param(path, kinds[-1], "A", SHAPE_A, min(batches[0], 40), id=f"{path}-A-B{batches[0]}"))
    return out


_runners = {}


def _runner(corpus, kind, dev):
    if (corpus, kind) not in _runners:
        _runners[corpus, kind] = oto.Runner(oto.corpus_a() if corpus == "A" else oto.corpus_b(), kind, dev)
    return _runners[corpus, kind]


def _expected_stats(path, kind, B, shape, host):
    """(delta of [2], delta of [3]) of one call; None where the pooled buffer's
    size decides (the 258 shape fits the host rerank's words only in a buffer
    above 64 KiB)."""
    if shape == SHAPE_258:
        return None
    if path.startswith("host_rerank"):
        return (0, 1)
    # the GPU rerank's select mirrors the final top-k into host words for a
    # faithful shard at any B and for bf16 / MXFP8 up to B = 32 (C <= 1024)
    return (1 if host and (kind == "fp32" or B <= 32) else 0, 0)


@pytest.mark.parametrize("path,kind,corpus,shape,B", _cases())
def test_path_x_shape_equals_exact_pipeline(dev, path, kind, corpus, shape, B):
    L = _lib.lib()
    r = _runner(corpus, kind, dev)
    host_rerank, prearm = PATHS[path][1]
    b0 = (7 * B + shape[0]) % r.c.B
    L.cbv2_set_host_rerank(host_rerank)
    L.cbv2_set_prearm(prearm)
    try:
        for host, mode in ((True, "array"),) if shape == SHAPE_258 else ((False, "callable"), (True, "array")):
            s0 = oto.pool_stats()
            bad = r.call(shape, b0, B, mode=mode, host=host, rot=B + shape[3])
            torch.cuda.synchronize()
            s1 = oto.pool_stats()
            assert not bad, f"{path} {kind} corpus {corpus} {shape} B={B} host={host}: " + "; ".join(bad)
            d = (s1[2] - s0[2], s1[3] - s0[3])
            want = _expected_stats(path, kind, B, shape, host)
            assert want is None or d == want, \
                f"{path} {kind} {shape} B={B} host={host}: pool stats [2], [3] moved by {d}, path expects {want}"
            assert s1[1] == s1[0], "a mapped buffer was not returned to its pool"
    finally:
        L.cbv2_set_host_rerank(1)
        L.cbv2_set_prearm(1)


# ---------------------------------------------------------------------- one pooled buffer, forged tags
@pytest.fixture(scope="module")
def sweep():
    """The child's report: {"created", "calls", "failures": [...], "forged": [...]}."""
    here = os.path.dirname(os.path.abspath(__file__))
    p = subprocess.run([sys.executable, os.path.join(here, "onetrip_sweep_child.py")], timeout=300,
                       capture_output=True, text=True)
    assert p.returncode == 0, f"the sweep child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_layout_sweep_on_one_pooled_buffer(dev, sweep):
    """>= 60 calls cycling shapes, B, kinds, stage-1 modes and host / device
    results over ONE buffer (the largest layout's call came first), stage-1
    and candidate ids covering 1..400 in both word halves: every call equals
    the oracle."""
    assert sweep["sweep_calls"] >= 60
    assert sweep["created"] == 1, f"{sweep['created']} mapped buffers: the calls did not share one"
    assert sorted(set(sweep["low_ids_seen"])) == list(range(1, 401)), "stage-1 / candidate ids should cover 1..400"
    # (counted on the CPU from the layouts: stale ids, in words a call polls first, equal to its plain counter)
    assert sweep["plain_counter_hits"] >= 1,"the sweep would not notice a small plain counter as the tag"
    assert not sweep["sweep_failures"], "\n".join(sweep["sweep_failures"][:8])


def test_forged_tags_never_pass_stale_words(dev, sweep):
    """A call whose tag equals plain data an earlier call left in the polled
    words (-1, -inf, a negative score's bits), per polled region, and the
    counter's wrap: results equal the oracle."""
    regions = {f["region"] for f in sweep["forged"]}
    assert regions == {"stage2", "prescore", "candidates", "final_host", "final_copy", "wrap"}, regions
    counters = {f["counter"] for f in sweep["forged"] if f["region"] != "wrap"}
    assert {0x7FFFFFFF, 0x7F800000} <= counters and len(counters) >= 3, [hex(c) for c in counters]
    for f in sweep["forged"]:
        if f["region"] != "wrap":
            assert f["stale_hits"] >= 1, f"{f}: no polled word's stale high half equalled the forged tag"
    bad = [f"{f['region']} counter {f['counter']:#x}: {f['bad']}" for f in sweep["forged"] if f["bad"]]
    assert not bad, "\n".join(bad[:8])


# ---------------------------------------------------------------------- loopback shards
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
        t.join(timeout=240)
    assert not any(t.is_alive() for t in ts), "a rank thread hung"
    if errs:
        raise errs[0][1]
    return out


@pytest.mark.parametrize("kind,shape", [("bf16", SHAPES[1]), ("fp32", SHAPES[1]), ("bf16", SHAPES[5]),
                                        ("fp32", SHAPES[5]), ("bf16", (100, 100, 100, 1100, 10))])
def test_loopback_shapes_equal_exact_pipeline(dev, kind, shape):
    """G = 2 loopback shards: every rank's device and host results equal the
    oracle of the whole corpus.  Each rank's stage 1 returns its own shard's
    part of the hand-built list (the exchange merges by score).  C = 1100 >
    1024 takes cbv2_rerank_sharded's all-reduce."""
    G, B = 2, 3
    c = oto.corpus_b()
    k, kb_cap, kb_ret, C, final_k = shape
    cut = 1777
    ranges = [(0, cut), (cut, c.N)]
    dt = torch.float32 if kind == "fp32" else torch.bfloat16
    tok = c.g.tokens_on(dev, dt)
    dl = c.g.doclens_on(dev)
    mk = ColbertIndex.faithful_f32 if kind == "fp32" else ColbertIndex
    shards = [mk(tok[a:b].contiguous(), dl[a:b].contiguous(), id_base=a) for a, b in ranges]
    del tok
    rows = list(range(4, 4 + B))
    Q = torch.from_numpy(c.g.Q[rows]).to(dev, dt).contiguous()
    # stage 1: in-range ids only (a shard's BM25 returns its own docs), scores descending with the rank
    lex = None
    parts = [None] * G
    if kb_ret > 0:
        lex = oto.stage1_lists(c, rows, kb_ret, k, rot=0)
        lex[(lex >= c.N)] = -1
        lex = np.stack([np.array([x for x in row if x >= 0] + [-1] * int((row < 0).sum()), np.int32) for row in lex])
        sc = np.where(lex >= 0, 1000.0 - np.arange(kb_ret, dtype=np.float32)[None, :], -np.inf).astype(np.float32)
        for g, (a, b) in enumerate(ranges):
            mine = (lex >= a) & (lex < b)
            pi = np.full(lex.shape, -1, np.int32)
            ps = np.full(lex.shape, -np.inf, np.float32)
            for r in range(B):
                n = int(mine[r].sum())
                pi[r, :n], ps[r, :n] = lex[r][mine[r]], sc[r][mine[r]]
            parts[g] = (pi, ps)
    want = oto.pipeline(c, rows, lex, k, C, final_k)
    comms = loopback_comms(G)
    ones = [OneTripRetriever(NativeExchange(shards[g], comm=comms[g]), colbert_k=k, fused=C, final_k=final_k,
                             lexical_k=kb_cap) for g in range(G)]
    lexical = [(lambda g=g: parts[g]) if kb_ret > 0 else None for g in range(G)]
    outs = _run_ranks(G, lambda g: [x.cpu().numpy() for x in ones[g](Q, lexical[g])])
    hosts = _run_ranks(G, lambda g: ones[g](Q, lexical[g], host=True))
    torch.cuda.synchronize()
    for g in range(G):
        for got, what in ((outs[g], "device"), (hosts[g], "host")):
            assert np.array_equal(oto.bits(got[0]), oto.bits(want[0])), f"rank {g} {what}: score bits differ"
            assert np.array_equal(got[1], want[1]), f"rank {g} {what}: ids differ\n{got[1]}\n{want[1]}"
            assert np.array_equal(got[2], want[2]), f"rank {g} {what}: positions differ"
    del ones
