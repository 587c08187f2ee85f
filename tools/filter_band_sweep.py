#!/usr/bin/env python3
"""Filtered faithful search: the band over the compact row against the pair
path and the unfiltered faithful search, over batch sizes and filter densities,
on one synthetic fp32-faithful index of full 128-token docs, one GPU, k = 100
(--k: another k).

    python tools/filter_band_sweep.py [--docs 1000000] [--batches 1,16,256]
                                      [--densities 0.001,0.003,0.01,0.03,0.1,0.25,0.5] [--reps 5] [--k 100]
                                      [--baseline-lib PATH/libcolbert_mi355x.so]
                                      [--out profiles/filter_band_sweep.jsonl]

Legs of a (B, density) point, timed in one process with device events around
each call, interleaved round by round after one warm-up round, median / min /
max of --reps rounds:
  band    CBV2_OPT_FILTER_BAND = 1 (the band forced on)
  pair    CBV2_OPT_FILTER_BAND = 2 (one faithful score per (query, allowed doc));
          not measured beyond --pair-cap pairs (2e7)
  auto    CBV2_OPT_FILTER_BAND = 0 (the default)
  full    the unfiltered cbv2_search_f32 over every doc
  overflow  the band forced on with cap = k, so that every row overflows and is
          recomputed on the device (measured where pair is)
band and pair must return identical bits (asserted); the band's status per row
(band size; -1 = overflow) is recorded as median and max.

--baseline-lib: a libcolbert_mi355x.so built from the parent commit.  At the
points B = 16 / 0.1, B = 256 / 0.01 and B = 1 / 0.001 its cbv2_search_filtered
(a handle of that library over the same device arrays, the same bitmap) is
timed against this build's cbv2_search_filtered under the default and under
CBV2_OPT_FILTER_BAND = 2, all three through the C ABI with preallocated
outputs, interleaved round by round; the results must be identical bits.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASELINE_POINTS = ((16, 0.1), (256, 0.01), (1, 0.001))


def stats(v):
    return {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--densities", default="0.001,0.003,0.01,0.03,0.1,0.25,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--pair-cap", type=int, default=20_000_000)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_band_sweep.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from hybrid_rag_colbertv2_amd import _lib, synth
    from hybrid_rag_colbertv2_amd.index import ColbertIndex, _stream_ptr, pack_allow

    dev = torch.device("cuda:0")
    batches = [int(x) for x in a.batches.split(",")]
    dens = [float(x) for x in a.densities.split(",")]
    Bmax, k, lq = max(batches), a.k, 32
    Qf = synth.make_queries(Bmax, lq, seed=1)
    planted = synth.planted_ids(max(Bmax, 8), a.docs, 10, seed=2)[:Bmax]
    x, dl = synth.make_shard(0, a.docs, Qf, planted, dev, seed=0, dtype=torch.float32)
    assert int(dl.min()) == 128                      # full 128-token docs
    ix = ColbertIndex.faithful_f32(x, dl)
    del x
    torch.cuda.empty_cache()
    Qall = Qf.to(dev)
    rng = np.random.default_rng(5)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")
    L, st = _lib.lib(), _stream_ptr(dev)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def timed(leg):
        prep, fn = leg if isinstance(leg, tuple) else (None, leg)
        if prep is not None:
            prep()                                   # the leg's option: set outside the timed region
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def rounds(legs):
        ts, res = {n: [] for n in legs}, {}
        for r in range(a.reps + 1):                  # round 0 warms every leg up
            for n, fn in legs.items():
                t, res[n] = timed(fn)
                if r:
                    ts[n].append(t)
        return ts, res

    # the parent's library: its own index handle over the same device arrays
    P, ph = None, ctypes.c_void_p()
    if a.baseline_lib:
        P = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        for name in ("cbv2_index_create", "cbv2_index_attach_residual", "cbv2_index_destroy", "cbv2_filter_bytes",
                     "cbv2_filter_create", "cbv2_filter_destroy", "cbv2_search_filtered_workspace_size",
                     "cbv2_search_filtered", "cbv2_build_stamp"):
            fn = getattr(P, name)
            fn.restype, fn.argtypes = _lib._SIGS[name]
        assert P.cbv2_build_stamp() != L.cbv2_build_stamp(), "the baseline library is this build"
        assert P.cbv2_index_create(0, ix.tokens.data_ptr(), _lib.DTYPE_BF16, ix.n, 128, 128, ix.doclens.data_ptr(), 0,
                                   ctypes.byref(ph)) == 0
        assert P.cbv2_index_attach_residual(ph, ix.residual.data_ptr(), ix.bounds[0], ix.bounds[1]) == 0

    for s in dens:
        m = max(1, int(round(s * a.docs)))
        E = np.sort(rng.choice(a.docs, m, replace=False))
        flt = ix.filter(ids=E)
        for B in batches:
            Q = Qall[:B].contiguous()
            band_status = {}

            def leg(mode):
                def fn():
                    r = ix.search(Q, k, filter=flt)
                    band_status[mode] = ix.last_band
                    return r
                return (lambda: ix.set_option(_lib.OPT_FILTER_BAND, mode)), fn
            legs = {"band": leg(_lib.FILTER_BAND_ON), "auto": leg(_lib.FILTER_BAND_AUTO), "full": lambda: ix.search(Q, k)}
            rec = {"docs": a.docs, "B": B, "density": s, "m": m, "k": k, "reps": a.reps}
            if B * m > a.pair_cap:
                rec["pair"] = f"not measured: {B * m} faithful pairs > cap {a.pair_cap}"
            else:
                legs["pair"] = leg(_lib.FILTER_BAND_OFF)
                # every row overflowing (cap = k): the band's launches, then the device-side recomputation
                legs["overflow"] = ((lambda: ix.set_option(_lib.OPT_FILTER_BAND, _lib.FILTER_BAND_ON)),
                                    (lambda: ix._search_filtered(Q, k, "maxsim", flt, cap=k)))
            ts, res = rounds(legs)
            rec.update({n: stats(v) for n, v in ts.items()})
            stt = band_status[_lib.FILTER_BAND_ON].cpu().numpy()
            rec["band_status"] = {"median": float(np.median(stt)), "max": int(stt.max()), "overflowed": int((stt < 0).sum())}
            rec["auto_takes_band"] = bool((band_status[_lib.FILTER_BAND_AUTO].cpu().numpy() >= 0).all())
            if "pair" in res:
                same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(res["band"], res["pair"]))
                rec["identical"] = bool(same)
                assert same, f"band and pair path differ at B={B}, density={s}"
            emit(rec)

            if P is not None and (B, s) in BASELINE_POINTS:
                words = pack_allow(E, ix.n).to(dev)
                pbuf = torch.empty(int(P.cbv2_filter_bytes(ix.n)), dtype=torch.uint8, device=dev)
                pf = ctypes.c_void_p()
                assert P.cbv2_filter_create(ph, words.data_ptr(), pbuf.data_ptr(), pbuf.numel(), st, ctypes.byref(pf)) == 0
                outs = {n: (torch.empty((B, k), dtype=torch.float32, device=dev),
                            torch.empty((B, k), dtype=torch.int32, device=dev)) for n in ("parent", "default", "pair")}
                ix.set_option(_lib.OPT_FILTER_BAND, _lib.FILTER_BAND_AUTO)
                need = max(int(P.cbv2_search_filtered_workspace_size(ph, pf, B, lq, k, 0)),
                           int(L.cbv2_search_filtered_workspace_size(ix._h, flt._h, B, lq, k, 0)))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)

                def raw(lib, h, f, name, mode=_lib.FILTER_BAND_AUTO):
                    def fn():
                        rc = lib.cbv2_search_filtered(h, f, 0, Q.data_ptr(), _lib.DTYPE_F32, B, lq, k, ws.data_ptr(),
                                                      ws.numel(), outs[name][0].data_ptr(), outs[name][1].data_ptr(), st)
                        assert rc == 0, (name, rc)
                    # (the parent leg sets the same option on this build's handle: equal host work before each leg)
                    return (lambda: ix.set_option(_lib.OPT_FILTER_BAND, mode)), fn
                ts, _ = rounds({"parent": raw(P, ph, pf, "parent"),
                                "default": raw(L, ix._h, flt._h, "default", _lib.FILTER_BAND_AUTO),
                                "pair": raw(L, ix._h, flt._h, "pair", _lib.FILTER_BAND_OFF)})
                torch.cuda.synchronize()
                for n in ("default", "pair"):
                    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                               for x, y in zip(outs[n], outs["parent"])), f"{n} differs from the parent at B={B}, density={s}"
                emit({"baseline": True, "docs": a.docs, "B": B, "density": s, "m": m, "k": k, "reps": a.reps,
                      "identical_to_parent": True, **{n: stats(v) for n, v in ts.items()}})
                P.cbv2_filter_destroy(pf)
        ix.set_option(_lib.OPT_FILTER_BAND, _lib.FILTER_BAND_AUTO)
        flt.close()
    if P is not None:
        P.cbv2_index_destroy(ph)
    return 0


if __name__ == "__main__":
    sys.exit(main())
