#!/usr/bin/env python3
"""Per-query filter sweep: one cbv2_search_filtered_batch call against the loop
of single-query cbv2_search_filtered calls it replaces, on one synthetic index
per kind (bf16, fp32-faithful), one GPU.

    python tools/filter_batch_sweep.py [--docs 1000000] [--kinds bf16,faithful] [--batch 256]
                                       [--counts 100,1000,10000] [--reps 5]
                                       [--out profiles/filter_batch_sweep.jsonl]

Every query of the batch has its own random filter of m docs.  Three legs per
(kind, m), timed in the same process with device events around each leg,
interleaved round by round (a, b, c, a, ...), after one warm-up round; the
medians are reported:
  a  the batch call (the filter batch built beforehand);
  b  the baseline: B single-query cbv2_search_filtered calls on one stream, each
     writing its row of one preallocated output (the C entry point directly,
     one workspace: no allocation and no Python search wrapper inside the leg);
  c  for information: ONE cbv2_search_filtered call with all B queries under one
     filter of the same m -- what re-streaming the docs per query costs.
Legs a and b must return identical bits (asserted).  Hard condition: at
m = 1000, a is faster than b for every kind; the exit status is 1 otherwise.

One child process per index kind, each under its own time limit (--limit
seconds); a child that fails or runs out of time stops the chain.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import torch
    from hybrid_rag_colbertv2_amd import _lib, synth
    from hybrid_rag_colbertv2_amd.index import ColbertIndex, _stream_ptr

    dev = torch.device("cuda:0")
    B, k, lq = a.batch, 100, 32
    Qf = synth.make_queries(B, lq, seed=1)
    planted = synth.planted_ids(max(B, 8), a.docs, 10, seed=2)[:B]
    if a.kind == "faithful":
        x, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0, dtype=torch.float32)
        ix = ColbertIndex.faithful_f32(x, dl)
        del x
        torch.cuda.empty_cache()
        Q = Qf.to(dev)
    else:
        tok, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0)
        ix = ColbertIndex(tok, dl)
        Q = Qf.to(dev, torch.bfloat16)
    L = _lib.lib()
    sid = _lib.SCORER_MAXSIM
    _keep, qptr, qdt, _, _ = ix._prep_query(Q, "maxsim")
    qrow = _keep.shape[1] * _keep.shape[2] * _keep.element_size()      # bytes of one query
    g = torch.Generator(device=dev).manual_seed(5)
    out = open(a.out, "a")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for m in [int(x) for x in a.counts.split(",")]:
        flts = [ix.filter(ids=torch.randperm(a.docs, device=dev, generator=g)[:m]) for _ in range(B)]
        fb = ix.filter_batch(flts)
        need1 = int(L.cbv2_search_filtered_workspace_size(ix._h, flts[0]._h, 1, lq, k, sid))    # (every m_b = m)
        ws1 = torch.empty(need1, dtype=torch.uint8, device=dev)
        loop_s = torch.empty((B, k), dtype=torch.float32, device=dev)
        loop_i = torch.empty((B, k), dtype=torch.int32, device=dev)
        st = _stream_ptr(dev)

        def leg_a():
            return ix.search(Q, k, filters=fb)

        def leg_b():
            for b in range(B):
                _lib.check(L.cbv2_search_filtered(ix._h, flts[b]._h, sid, qptr + b * qrow, qdt, 1, lq, k, ws1.data_ptr(),
                                                  need1, loop_s.data_ptr() + 4 * b * k, loop_i.data_ptr() + 4 * b * k, st))
            return loop_s, loop_i

        def leg_c():
            return ix.search(Q, k, filter=flts[0])

        legs = {"batch": leg_a, "loop": leg_b, "shared": leg_c}
        ts = {n: [] for n in legs}
        res = {}
        for r in range(a.reps + 1):          # round 0 warms every leg up
            for n, fn in legs.items():
                t, got = timed(fn)
                res[n] = tuple(x.clone() for x in got)
                if r:
                    ts[n].append(t)
        same = bool(torch.equal(res["batch"][1], res["loop"][1])
                    and torch.equal(res["batch"][0].view(torch.int32), res["loop"][0].view(torch.int32)))
        ms = {n: round(statistics.median(v), 4) for n, v in ts.items()}
        per_doc = 128 * 128 * 2 * (2 if a.kind == "faithful" else 1)        # hi (+ lo) bytes of a doc
        rec = {"kind": a.kind, "docs": a.docs, "B": B, "m": m, "k": k, "reps": a.reps, "pairs": fb.pairs, "ms": ms,
               "min_ms": {n: round(min(v), 4) for n, v in ts.items()}, "identical": same,
               "loop_over_batch": round(ms["loop"] / ms["batch"], 2),
               "batch_over_shared": round(ms["batch"] / ms["shared"], 2),
               "batch_gbs_over_pair_bytes": round(fb.pairs * per_doc / 1e9 / (ms["batch"] * 1e-3), 1)}
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        assert same, "the batch call and the loop of single-query calls returned different bits"
        fb.close()
        for f in flts:
            f.close()
        del flts, fb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--kinds", default="bf16,faithful")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--counts", default="100,1000,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420, help="seconds per index kind (one child process each)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_batch_sweep.jsonl"))
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)     # set for the child
    a = ap.parse_args()
    if a.kind is not None:
        return child(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for kind in a.kinds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--docs", str(a.docs), "--batch", str(a.batch),
               "--counts", a.counts, "--reps", str(a.reps), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"[filter_batch_sweep] {kind}: time limit of {a.limit} s reached; stopping the chain", flush=True)
            return 124
        if rc != 0:
            print(f"[filter_batch_sweep] {kind}: exit {rc}; stopping the chain", flush=True)
            return rc
    rows = [json.loads(x) for x in open(a.out)]
    gate = [r for r in rows if r["m"] == 1000]
    ok = bool(gate) and all(r["ms"]["batch"] < r["ms"]["loop"] for r in gate)
    print(json.dumps({"hard_condition_m1000_batch_faster_than_loop": ok,
                      "ratios": {r["kind"]: r["loop_over_batch"] for r in gate}}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
