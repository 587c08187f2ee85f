#!/usr/bin/env python3
"""What the sharded grouped search adds to one shard's grouped search: the two
merges and the local chunk stage, timed on one GPU next to the local grouped
search of one shard at the same batch size.

    python tools/group_sharded_time.py [--docs 125000] [--ranks 8] [--batch 256] [--k 100] [--per-group 3]
                                       [--reps 7] [--inner 20] [--out profiles/group_sharded_time.jsonl]

One bf16 shard of --docs chunks (one of --ranks shards of a corpus of docs *
ranks chunks), 10 consecutive chunks per document, the corpus-wide group count.
Legs, each warmed up once, then --reps windows of --inner back-to-back calls
between two device events (a merge is microseconds: one call is too short a
window); the figure is the median window over --inner:
  local_grouped      cbv2_search_grouped of the shard (scan + selection), r chunks;
  round1_local       cbv2_group_topk_rows with r = 1 over the shard's score matrix
                     (what round 1 runs after the scan);
  merge_group_topk   cbv2_merge_group_topk of --ranks gathered [B, k] lists;
  chunk_stage        cbv2_group_chunks_rows over the score matrix for the merged groups;
  merge_group_chunks cbv2_merge_group_chunks of --ranks gathered [B, k, r] lists.
The gathered lists are this shard's own, once per rank with the group indices
and chunk ids shifted per rank (both merges do the same work whatever the
values: a sort network and a fixed number of wave reductions).  The
all-gathers themselves are not timed here: the loopback communicator's device
copies say nothing about RCCL; their payloads are recorded in bytes.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--per-group", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_sharded_time.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from hybrid_rag_colbertv2_amd import synth
    from hybrid_rag_colbertv2_amd.index import (ColbertIndex, group_chunks_rows, group_topk_rows, merge_group_chunks,
                                                merge_group_topk)

    if not torch.cuda.is_available():
        sys.exit("group_sharded_time: needs a ROCm GPU")
    dev = torch.device("cuda:0")
    n, G, B, k, r = a.docs, a.ranks, a.batch, a.k, a.per_group
    Qf = synth.make_queries(B, 32, seed=1)
    planted = synth.planted_ids(max(B, 8), n, 10, seed=2)[:B]
    tok, dl = synth.make_shard(0, n, Qf, planted, dev, seed=0)
    ix = ColbertIndex(tok, dl)
    del tok
    Q = Qf.to(dev, torch.bfloat16)
    groups_total = (n * G + 9) // 10
    grp = ix.groups(group_of=(np.arange(n, dtype=np.int64) // 10).astype(np.int32), G=groups_total)
    S = ix.score(Q).contiguous()
    s1, g1, _, _ = group_topk_rows(S, k, grp, 1)
    per_shard = (n + 9) // 10
    all_s = s1.unsqueeze(0).repeat(G, 1, 1).contiguous()
    all_g = torch.stack([torch.where(g1 >= 0, g1 + rk * per_shard, g1) for rk in range(G)]).contiguous()
    _, sel = merge_group_topk(all_s, all_g, k)
    ci, cs = group_chunks_rows(S, sel, grp, r)
    all_i = torch.stack([torch.where(ci >= 0, ci + rk * n, ci) for rk in range(G)]).contiguous()
    all_c = cs.unsqueeze(0).repeat(G, 1, 1, 1).contiguous()

    legs = {
        "local_grouped": lambda: ix.search_grouped(Q, k, grp, per_group=r),
        "round1_local": lambda: group_topk_rows(S, k, grp, 1),
        "merge_group_topk": lambda: merge_group_topk(all_s, all_g, k),
        "chunk_stage": lambda: group_chunks_rows(S, sel, grp, r),
        "merge_group_chunks": lambda: merge_group_chunks(all_i, all_c),
    }
    inner = {name: (max(1, a.inner // 10) if name == "local_grouped" else a.inner) for name in legs}
    ts = {name: [] for name in legs}
    for rep in range(a.reps + 1):                # round 0 warms every leg up
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner[name]):
                fn()
            e1.record()
            e1.synchronize()
            if rep:
                ts[name].append(e0.elapsed_time(e1) / inner[name])
    med = {name: statistics.median(v) for name, v in ts.items()}
    added = med["merge_group_topk"] + med["chunk_stage"] + med["merge_group_chunks"]
    rec = {"kind": "bf16", "docs_per_shard": n, "ranks": G, "B": B, "k": k, "r": r, "groups": groups_total,
           "reps": a.reps, "calls_per_window": inner,
           "ms": {name: round(v, 4) for name, v in med.items()},
           "min_ms": {name: round(min(v), 4) for name, v in ts.items()},
           "max_ms": {name: round(max(v), 4) for name, v in ts.items()},
           "exchange_compute_ms": round(added, 4),
           "exchange_compute_over_local_grouped": round(added / med["local_grouped"], 5),
           "gather1_bytes_per_rank": 8 * B * k, "gather2_bytes_per_rank": 8 * B * k * r,
           "note": "windows include the Python wrappers' output allocations; the all-gathers are not timed"}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    grp.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
