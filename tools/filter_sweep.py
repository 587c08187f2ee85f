#!/usr/bin/env python3
"""Filtered-search sweep: the unfiltered search (the yardstick) against the
subset and the dense path of cbv2_search_filtered over filter densities, on one
synthetic index per kind (bf16, fp32-faithful, mxfp8), one GPU.

    python tools/filter_sweep.py [--docs 1000000] [--kinds bf16,faithful] [--batches 1,16,256]
                                 [--densities 0.001,0.01,0.1,0.25,0.5,1.0] [--reps 5]
                                 [--out profiles/filter_sweep.jsonl]
    python tools/filter_sweep.py --kinds mxfp8      (-> profiles/filter_sweep_mxfp8.jsonl)
    python tools/filter_sweep.py --ld 512 --kinds bf16,faithful,mxfp8      (-> profiles/filter_sweep_long.jsonl)

--ld 256 / 512 / 1024: a long-document index of the same bytes -- --docs * 128 /
ld full-length docs (250,000 at ld = 512), the synthetic corpus's 128-token docs
taken ld / 128 at a time.

One child process per index kind, each under its own time limit (--limit
seconds); a child that fails or runs out of time stops the chain.  Inside a
child everything of one (B, density) point is timed in the same process,
interleaved round by round (unfiltered, subset, dense, unfiltered, ...), with
device events around each call, after one warm-up round; the medians are
reported.  A faithful point whose path would score more than --pair-cap
(query, doc) pairs is recorded as not measured (one faithful score per pair:
B = 256 over 1M docs is 2.6e8 of them).

Per point: ms of the three, the subset path's allowed bytes / FLOP and the
rate it reached over them (B = 1: share of the 8 TB/s HBM peak; B = 256: share
of the 2.5 PFLOP/s bf16 MFMA peak; mxfp8: of the 5 PFLOP/s fp8 dense peak,
bytes per doc 128 * 128 + 256), the same two rates of the unfiltered scan over
the whole shard, and whether subset and dense returned the same bits (an mxfp8
child stops at a point where they differ).  The mxfp8 index is
ColbertIndex.mxfp8 and every leg quantizes its bf16 queries inside the call.  f of a kind = the largest measured density at which the subset
path is still faster than the dense path at every measured B.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM_GBS, PEAK_BF16_TFLOPS, PEAK_FP8_TFLOPS = 8000.0, 2500.0, 5000.0


def child(a):
    import numpy as np
    import torch
    from hybrid_rag_colbertv2_amd import _lib, synth
    from hybrid_rag_colbertv2_amd.index import ColbertIndex

    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    dens = [float(x) for x in a.densities.split(",")]
    Bmax, k = max(batches), 100
    Qf = synth.make_queries(Bmax, 32, seed=1)
    planted = synth.planted_ids(max(Bmax, 8), a.docs, 10, seed=2)[:Bmax]
    per = a.ld // 128                    # 128-token docs of the synthetic corpus per doc of the index
    ndocs = a.docs // per

    def long_docs(t, dl):
        if per == 1:
            return t, dl
        return t[: ndocs * per].view(ndocs, a.ld, 128), torch.full((ndocs,), a.ld, dtype=torch.int32, device=dev)

    if a.kind == "faithful":
        x, dl = long_docs(*synth.make_shard(0, a.docs, Qf, planted, dev, seed=0, dtype=torch.float32))
        ix = ColbertIndex.faithful_f32(x, dl)
        del x
        torch.cuda.empty_cache()
        Qall = Qf.to(dev)
    else:
        tok, dl = long_docs(*synth.make_shard(0, a.docs, Qf, planted, dev, seed=0))
        if a.kind == "mxfp8":
            ix = ColbertIndex.mxfp8(tok, dl)
            del tok
            torch.cuda.empty_cache()
        else:
            ix = ColbertIndex(tok, dl)
        Qall = Qf.to(dev, torch.bfloat16)
    a.docs = ndocs                       # from here on: the docs of the index
    rng = np.random.default_rng(5)
    out = open(a.out, "a")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for s in dens:
        m = max(1, int(round(s * a.docs)))
        E = np.sort(rng.choice(a.docs, m, replace=False)) if m < a.docs else np.arange(a.docs)
        flt = ix.filter(ids=E)
        for B in batches:
            Q = Qall[:B]
            legs = {"unfiltered": lambda: ix.search(Q, k)}
            skipped = {}
            for name, path, pairs in (("subset", _lib.FILTER_SUBSET, B * m), ("dense", _lib.FILTER_DENSE, B * a.docs)):
                if a.kind == "faithful" and pairs > a.pair_cap:
                    skipped[name] = f"not measured: {pairs} faithful pairs > cap {a.pair_cap}"
                    continue

                def leg(path=path):
                    ix.set_option(_lib.OPT_FILTER_PATH, path)
                    return ix.search(Q, k, filter=flt)
                legs[name] = leg
            ts = {n: [] for n in legs}
            res = {}
            for r in range(a.reps + 1):          # round 0 warms every leg up
                for n, fn in legs.items():
                    t, res[n] = timed(fn)
                    if r:
                        ts[n].append(t)
            rec = {"kind": a.kind, "docs": a.docs, "ld": a.ld, "B": B, "density": s, "m": m, "k": k, "reps": a.reps,
                   "ms": {n: round(statistics.median(v), 4) for n, v in ts.items()},
                   "min_ms": {n: round(min(v), 4) for n, v in ts.items()},
                   "max_ms": {n: round(max(v), 4) for n, v in ts.items()}, **skipped}
            if "subset" in res and "dense" in res:
                rec["identical"] = bool(torch.equal(res["subset"][0], res["dense"][0])
                                        and torch.equal(res["subset"][1], res["dense"][1]))
            if "subset" in ts:
                # bytes of a doc: hi (+ lo) bf16 tokens; mxfp8: e4m3 tokens + 2 scale bytes per token
                per_doc = per * (128 * 128 + 256 if a.kind == "mxfp8" else 128 * 128 * 2 * (2 if a.kind == "faithful" else 1))
                flop = 2.0 * B * 32 * m * a.ld * 128 * (3 if a.kind == "faithful" else 1)
                peak = PEAK_FP8_TFLOPS if a.kind == "mxfp8" else PEAK_BF16_TFLOPS
                sec = rec["ms"]["subset"] * 1e-3
                rec["subset_allowed_gb"] = round(m * per_doc / 1e9, 4)
                rec["subset_gbs_over_allowed_bytes"] = round(m * per_doc / 1e9 / sec, 1)
                rec["subset_hbm_share"] = round(m * per_doc / 1e9 / sec / PEAK_HBM_GBS, 4)
                rec["subset_tflops_over_allowed_flop"] = round(flop / 1e12 / sec, 2)
                rec["subset_mfma_share"] = round(flop / 1e12 / sec / peak, 4)
                if a.kind == "mxfp8":       # the unfiltered search of the same run, over the whole shard
                    usec = rec["ms"]["unfiltered"] * 1e-3
                    rec["unfiltered_gbs"] = round(a.docs * per_doc / 1e9 / usec, 1)
                    rec["unfiltered_tflops"] = round(flop * a.docs / m / 1e12 / usec, 2)
                    rec["unfiltered_mfma_share"] = round(flop * a.docs / m / 1e12 / usec / peak, 4)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            if a.kind == "mxfp8" and not rec.get("identical", True):
                sys.exit(f"[filter_sweep] mxfp8 B={B} density={s}: subset and dense differ")
        flt.close()
    ix.set_option(_lib.OPT_FILTER_PATH, _lib.FILTER_AUTO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000, help="128-token docs of the corpus (the index: docs * 128 / ld)")
    ap.add_argument("--ld", type=int, default=128, choices=(128, 256, 512, 1024), help="token slots per doc of the index")
    ap.add_argument("--kinds", default="bf16,faithful")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--densities", default="0.001,0.01,0.1,0.25,0.5,1.0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-cap", type=int, default=20_000_000)
    ap.add_argument("--limit", type=int, default=540, help="seconds per index kind (one child process each)")
    ap.add_argument("--out", default=None, help="profiles/filter_sweep.jsonl (--kinds mxfp8: filter_sweep_mxfp8.jsonl)")
    ap.add_argument("--kind", default=None, help=argparse.SUPPRESS)     # set for the child
    a = ap.parse_args()
    if a.out is None:
        name = "filter_sweep_long.jsonl" if a.ld != 128 else \
            "filter_sweep_mxfp8.jsonl" if a.kinds == "mxfp8" else "filter_sweep.jsonl"
        a.out = os.path.join(ROOT, "profiles", name)
    if a.kind is not None:
        return child(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").close()
    for kind in a.kinds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--docs", str(a.docs), "--ld", str(a.ld), "--batches", a.batches,
               "--densities", a.densities, "--reps", str(a.reps), "--pair-cap", str(a.pair_cap), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"[filter_sweep] {kind}: time limit of {a.limit} s reached; stopping the chain", flush=True)
            return 124
        if rc != 0:
            print(f"[filter_sweep] {kind}: exit {rc}; stopping the chain", flush=True)
            return rc
    # f per kind: the largest measured density at which subset beats dense at every measured B
    rows = [json.loads(x) for x in open(a.out)]
    for kind in a.kinds.split(","):
        f = None
        for s in sorted({r["density"] for r in rows if r["kind"] == kind}):
            pts = [r for r in rows if r["kind"] == kind and r["density"] == s and "subset" in r["ms"] and "dense" in r["ms"]]
            if pts and all(r["ms"]["subset"] < r["ms"]["dense"] for r in pts):
                f = s
        print(json.dumps({"kind": kind, "f": f}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
