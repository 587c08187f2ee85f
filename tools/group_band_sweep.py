#!/usr/bin/env python3
"""Grouped faithful search: the certified band (CBV2_OPT_GROUP_BAND = 1) against
the full faithful scan (= 2, the path before the band existed) on one synthetic
fp32-faithful index, one GPU.  The points the automatic rule's constants come
from (csrc/colbert_mi355x.hip, group_band_wanted).

    python tools/group_band_sweep.py [--docs 1000000] [--batches 1,16,256] [--reps 5]
                                     [--members 2000,5000,10000,30000,100000]
                                     [--out profiles/group_band_sweep.jsonl]

The method is tools/group_sweep.py's: the legs of one point run in the same
process on the same handle, interleaved round by round after one warm-up round,
device events around each call, medians of --reps.  Legs:
  search_f32  the faithful chunk search with the same k (cbv2_search_f32): what
              grouping adds is band - search_f32;
  band        cbv2_search_grouped_f32 under option 1, with the rows' status (the
              global band's size; -1 = the row fell back to the full scan);
  full        the same call under option 2.  A point of more than --pair-cap
              (query, chunk) pairs skips this leg and says so.
Points: the groupings "ten", "zipf" and "half" of tools/group_sweep.py over
every chunk, B in --batches, r in {1, 3}, k = 100; then, at B = 1, "ten" over
the first m chunks only (the others in no group) for m in --members: where the
full path's B m faithful pairs stop paying for the band's extra launches.
The sweep runs in one child process (one index build) under --limit seconds.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
K = 100


def child(a):
    import numpy as np
    import torch
    from group_sweep import make_groupings
    from hybrid_rag_colbertv2_amd import _lib, synth
    from hybrid_rag_colbertv2_amd.index import ColbertIndex

    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    Bmax = max(batches)
    Qf = synth.make_queries(Bmax, 32, seed=1)
    planted = synth.planted_ids(max(Bmax, 8), a.docs, 10, seed=2)[:Bmax]
    x, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0, dtype=torch.float32)
    ix = ColbertIndex.faithful_f32(x, dl)
    del x
    Qall = Qf.to(dev)
    torch.cuda.empty_cache()
    out = open(a.out, "a")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def point(gname, group_of, B, r):
        grp = ix.groups(group_of=group_of)
        Q = Qall[:B]
        members = int(grp.members)

        def grouped(opt):
            ix.set_option(_lib.OPT_GROUP_BAND, opt)
            res = ix.search_grouped(Q, K, grp, per_group=r)
            return res, ix.last_band

        legs = {"search_f32": lambda: timed(lambda: ix.search(Q, K)),
                "band": lambda: timed(lambda: grouped(_lib.GROUP_BAND_ON))}
        full = B * members <= a.pair_cap
        if full:
            legs["full"] = lambda: timed(lambda: grouped(_lib.GROUP_BAND_OFF))
        ts, res = {n: [] for n in legs}, {}
        for rnd in range(a.reps + 1):            # round 0 warms every leg up
            for n, fn in legs.items():
                t, res[n] = fn()
                if rnd:
                    ts[n].append(t)
        torch.cuda.synchronize()
        ix.set_option(_lib.OPT_GROUP_BAND, _lib.GROUP_BAND_AUTO)
        med = {n: statistics.median(v) for n, v in ts.items()}
        st = res["band"][1].cpu().numpy()
        rec = {"docs": a.docs, "grouping": gname, "members": members, "groups": int(grp.count), "B": B, "k": K, "r": r,
               "reps": a.reps, "ms": {n: round(v, 4) for n, v in med.items()},
               "min_ms": {n: round(min(v), 4) for n, v in ts.items()},
               "max_ms": {n: round(max(v), 4) for n, v in ts.items()},
               "band_rows_fallen_back": int((st < 0).sum()),
               "band_size_median": int(np.median(st[st >= 0])) if (st >= 0).any() else -1,
               "band_size_max": int(st.max()), "band_minus_search_ms": round(med["band"] - med["search_f32"], 4)}
        if full:
            rec["full_over_band"] = round(med["full"] / med["band"], 3)
            rec["same_bits"] = all(torch.equal(p.view(torch.int32), q.view(torch.int32))
                                   for p, q in zip(res["band"][0], res["full"][0]))
        else:
            rec["full"] = f"not measured: {B * members} faithful pairs > --pair-cap {a.pair_cap}"
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        grp.close()

    whole = make_groupings(a.docs, np.random.default_rng(7))
    for gname in a.grouping.split(","):
        if gname == "members":
            i = np.arange(a.docs, dtype=np.int64)
            for m in (int(v) for v in a.members.split(",")):
                gof = np.where(i < m, i // 10, -1).astype(np.int32)
                for r in (1, 3):
                    point(f"ten, first {m}", gof, 1, r)
            continue
        for B in batches:
            for r in (1, 3):
                point(gname, whole[gname], B, r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--members", default="2000,5000,10000,30000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-cap", type=int, default=300_000_000)
    ap.add_argument("--limit", type=int, default=900, help="seconds for the child process that runs the points")
    ap.add_argument("--groupings", default="ten,zipf,half,members")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_band_sweep.jsonl"))
    ap.add_argument("--grouping", default=None, help=argparse.SUPPRESS)     # set for the child
    a = ap.parse_args()
    if a.grouping is not None:
        return child(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()
    cmd = [sys.executable, os.path.abspath(__file__), "--grouping", a.groupings, "--docs", str(a.docs), "--batches",
           a.batches, "--members", a.members, "--reps", str(a.reps), "--pair-cap", str(a.pair_cap), "--out", a.out]
    try:
        rc = subprocess.run(cmd, timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"[group_band_sweep] time limit of {a.limit} s reached", flush=True)
        return 124
    if rc != 0:
        print(f"[group_band_sweep] exit {rc}", flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
