#!/usr/bin/env python3
"""Grouped-search sweep: what "top-k documents, each with its best chunks" costs
on top of the chunk search, and what the over-fetch people use today costs and
misses, on one synthetic index per kind (bf16, mxfp8, fp32-faithful), one GPU.

    python tools/group_sweep.py [--docs 1000000] [--kinds bf16,mxfp8,faithful] [--batches 1,16,256]
                                [--reps 5] [--out profiles/group_sweep.jsonl]

Three groupings of the shard's chunks: "ten" (10 consecutive chunks per
document), "zipf" (Zipf-sized documents of consecutive chunks, the largest
capped at 5 % of the shard) and "half" (one document holding the first half of
the shard, 10 chunks per document after it).  k = 100 documents.

Legs of one (grouping, B) point, timed in the same process, interleaved round
by round, after one warm-up round; medians of --reps:
  search     the chunk search with k = 100 on the same handle (cbv2_search;
             cbv2_search_f32 on the faithful index): the yardstick -- device
             events around the call;
  grouped_r1 cbv2_search_grouped with 1 chunk per document; grouped_r3: with 3 --
             device events; grouped - search is what grouping adds;
  overfetch  what users do today: the chunk search with k' = 1000, a D2H copy
             of the ids and a host de-duplication by document -- wall clock from
             the call to the end of the de-duplication (it has a host part), and
             `short_rows`: the rows that end with fewer than 100 documents.
A faithful point of more than --pair-cap (query, chunk) pairs is recorded as
not measured: the grouped faithful call pays the full faithful scan, one
faithful score per pair (B = 256 over 1M chunks is 2.6e8 of them).
`agree`: on every row the over-fetch filled, its 100 documents are the grouped
call's, in order (the grouped call is exact; the over-fetch is, when it fills).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, K_OVER = 100, 1000


def make_groupings(n, rng):
    import numpy as np
    i = np.arange(n, dtype=np.int64)
    out = {"ten": (i // 10).astype(np.int32)}
    sizes = np.minimum(rng.zipf(1.3, size=n), max(1, n // 20))
    ends = np.cumsum(sizes)
    ends = ends[: int(np.searchsorted(ends, n)) + 1]
    out["zipf"] = np.searchsorted(ends, i, side="right").astype(np.int32)
    half = n // 2
    out["half"] = np.where(i < half, 0, 1 + (i - half) // 10).astype(np.int32)
    return out


def child(a):
    import numpy as np
    import torch
    from hybrid_rag_colbertv2_amd import synth
    from hybrid_rag_colbertv2_amd.index import ColbertIndex

    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    Bmax = max(batches)
    Qf = synth.make_queries(Bmax, 32, seed=1)
    planted = synth.planted_ids(max(Bmax, 8), a.docs, 10, seed=2)[:Bmax]
    if a.kind == "faithful":
        x, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0, dtype=torch.float32)
        ix = ColbertIndex.faithful_f32(x, dl)
        del x
        Qall = Qf.to(dev)
    else:
        tok, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0)
        ix = ColbertIndex.mxfp8(tok, dl) if a.kind == "mxfp8" else ColbertIndex(tok, dl)
        del tok
        Qall = Qf.to(dev, torch.bfloat16)
    torch.cuda.empty_cache()
    out = open(a.out, "a")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for gname, group_of in make_groupings(a.docs, np.random.default_rng(7)).items():
        grp = ix.groups(group_of=group_of)
        sizes = np.bincount(group_of)
        for B in batches:
            Q = Qall[:B]
            if a.kind == "faithful" and B * a.docs > a.pair_cap:
                rec = {"kind": a.kind, "docs": a.docs, "grouping": gname, "B": B, "k": K,
                       "not_measured": f"{B * a.docs} faithful pairs > cap {a.pair_cap}"}
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                continue

            def overfetch():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids = ix.search(Q, K_OVER)[1].cpu().numpy()
                docs = np.full((B, K), -1, dtype=np.int64)
                for b in range(B):
                    g = group_of[ids[b][ids[b] >= 0]]
                    first = np.sort(np.unique(g, return_index=True)[1])[:K]
                    docs[b, : first.size] = g[first]
                return (time.perf_counter() - t0) * 1e3, docs

            legs = {"search": lambda: timed(lambda: ix.search(Q, K)),
                    "grouped_r1": lambda: timed(lambda: ix.search_grouped(Q, K, grp, per_group=1)),
                    "grouped_r3": lambda: timed(lambda: ix.search_grouped(Q, K, grp, per_group=3)),
                    "overfetch": overfetch}
            ts, res = {n: [] for n in legs}, {}
            for r in range(a.reps + 1):              # round 0 warms every leg up
                for n, fn in legs.items():
                    t, res[n] = fn()
                    if r:
                        ts[n].append(t)
            torch.cuda.synchronize()
            med = {n: statistics.median(v) for n, v in ts.items()}
            docs, gg = res["overfetch"], res["grouped_r1"][1].cpu().numpy()
            filled = (docs >= 0).all(axis=1)
            rec = {"kind": a.kind, "docs": a.docs, "grouping": gname, "groups": int(grp.count),
                   "largest_group": int(sizes.max()), "B": B, "k": K, "k_overfetch": K_OVER, "reps": a.reps,
                   "ms": {n: round(v, 4) for n, v in med.items()},
                   "min_ms": {n: round(min(v), 4) for n, v in ts.items()},
                   "max_ms": {n: round(max(v), 4) for n, v in ts.items()},
                   "grouped_minus_search_ms": {r: round(med[f"grouped_{r}"] - med["search"], 4) for r in ("r1", "r3")},
                   "grouped_over_search": {r: round(med[f"grouped_{r}"] / med["search"], 4) for r in ("r1", "r3")},
                   "search_spread_ms": round(max(ts["search"]) - min(ts["search"]), 4),
                   "reduce_bytes_gb": round(4.0 * B * a.docs / 1e9, 4),
                   "short_rows": int((~filled).sum()), "rows": B,
                   "agree": bool((docs[filled] == gg[filled]).all())}
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        grp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--kinds", default="bf16,mxfp8,faithful")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-cap", type=int, default=20_000_000)
    ap.add_argument("--limit", type=int, default=420, help="seconds per index kind (one child process each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_sweep.jsonl"))
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)     # set for the child
    a = ap.parse_args()
    if a.kind is not None:
        return child(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()
    for kind in a.kinds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--docs", str(a.docs), "--batches", a.batches,
               "--reps", str(a.reps), "--pair-cap", str(a.pair_cap), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"[group_sweep] {kind}: time limit of {a.limit} s reached; stopping the chain", flush=True)
            return 124
        if rc != 0:
            print(f"[group_sweep] {kind}: exit {rc}; stopping the chain", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
