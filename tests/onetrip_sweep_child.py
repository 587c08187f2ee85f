"""Child process of tests/test_gpu_onetrip_shapes.py: the one-trip retrieve's
layout sweep and forged tags on ONE pooled mapped buffer (a fresh process:
the pool starts empty).  Prints one JSON line; the parent test asserts on it.

1. The largest layout's call first (it creates the buffer), then SWEEP_CALLS
   single-thread calls cycling shapes, batch sizes, index kinds, result paths,
   stage-1 modes and host / device results, each against the exact pipeline
   (tests/_onetrip_oracle.py); stage-1 ids are drawn from 1..400, so words of
   every layout hold small ids in both halves.  Between them PAIRS planter /
   victim pairs: a host-rerank call leaves its plain stage-1 ids where the
   next call's pre-armed rerank (candidate words) or copy kernel (final
   words) polls before the call has published anything; the stale ids that
   equal the victim's plain COUNTER are counted on the CPU
   (``plain_counter_hits``): a tag without its top bit would take them.
   ``created`` must end at 1: every call reused that buffer over other
   layouts' words.
2. Forged tags (lab knob cbv2_set_tag_lab): call 1 (host rerank, corpus A)
   leaves plain data in the buffer -- its stage-1 ids (-1 tails) and their raw
   prescores (-inf, negative scores) -- and call 2, of another layout whose
   polled region lies over that data, runs with its counter forged so that
   its tag EQUALS the data: 0x7FFFFFFF (-1), 0x7F800000 (-inf), the low 31
   bits of a negative prescore.  Once per polled region: the stage-2 id and
   score words and the prescore words (host), the candidate words (pre-armed
   rerank), the final words (host; the host rerank's copy kernel).  Before
   call 2 the stale words whose high half equals the tag are counted on the
   CPU from the buffer's layout (csrc/retrieve.cpp mapped_words).  Last, four
   calls from counter 0x7FFFFFFE on, through the wrap.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import _onetrip_oracle as oto  # noqa: E402
from hybrid_rag_colbertv2_amd import _lib  # noqa: E402

SHAPES = ((100, 100, 100, 50, 10), (10, 0, 0, 1, 1), (1, 1, 1, 1, 1), (200, 100, 60, 100, 50),
          (100, 100, 100, 100, 100), (40, 100, 100, 20, 7), (20, 16, 16, 64, 64), (100, 100, 100, 50, 60),
          (256, 16, 16, 300, 300))          # the last one on corpus A
KINDS = ("fp32", "bf16", "mxfp8")
KNOBS = ((1, 1), (2, 1), (0, 1), (0, 0))    # (host_rerank, prearm)
BATCHES = (1, 2, 8, 9, 32, 40, 5, 3)
SWEEP_CALLS = 48
PAIRS = 12


def layout(B, k, C, fk, kb):
    """Word offsets of a call's regions in its mapped buffer (mapped_words)."""
    o = {"ids": 0, "scores": B * k, "cand": 2 * B * k}
    o["final"] = o["cand"] + B * C
    o["prescore"] = o["final"] + 3 * B * fk
    o["lex_plain"] = o["prescore"] + B * kb        # [B][kb] int32 ids + [B][kb] float prescores, two per word
    o["words"] = B * (2 * k + C + 3 * fk + 2 * kb + 1) + 2
    return o


def main():
    dev = torch.device("cuda:0")
    L = _lib.lib()
    runners = {}

    def runner(corpus, kind):
        if (corpus, kind) not in runners:
            runners[corpus, kind] = oto.Runner(oto.corpus_a() if corpus == "A" else oto.corpus_b(), kind, dev)
        return runners[corpus, kind]

    def call(corpus, kind, shape, b0, B, knobs, mode, host, rot, low_ids=True):
        L.cbv2_set_host_rerank(knobs[0])
        L.cbv2_set_prearm(knobs[1])
        try:
            bad = runner(corpus, kind).call(shape, b0, B, mode=mode, host=host, rot=rot, low_ids=low_ids)
            torch.cuda.synchronize()       # the buffer's last reader has run: the next begin takes it again
        finally:
            L.cbv2_set_host_rerank(1)
            L.cbv2_set_prearm(1)
        return bad

    # ---- 1. the sweep
    sched = []
    for i in range(SWEEP_CALLS):
        si = i % len(SHAPES)
        sched.append(dict(corpus="A" if si == len(SHAPES) - 1 else "B", kind=KINDS[(i + i // 9) % 3], shape=SHAPES[si],
                          B=BATCHES[(3 * i + i // 8) % 8], knobs=KNOBS[(i + i // 4) % 4],
                          mode=("callable", "array")[(i // 3) % 2], host=bool((i // 2) % 2), rot=i, b0=(5 * i) % 8))
    # ... with planter / victim pairs in between: a host-rerank call leaves its plain stage-1 ids (1..400) in
    # words that the next call, of another layout, polls before anything of its own is there -- the
    # pre-armed rerank its candidate words, the host rerank's copy kernel the final words
    victim = layout(8, *[SHAPES[4][j] for j in (0, 3, 4, 2)])
    for i in range(PAIRS):
        planter, (lo, hi), knobs = ((SHAPES[5], ("cand", "final"), (0, 1)),
                                    (SHAPES[0], ("final", "prescore"), (1, 1)))[i % 2]
        sched.insert(5 * i + 2, dict(corpus="B", kind="fp32", shape=planter, B=8, knobs=(1, 1), mode="array",
                                     host=True, rot=100 + i, b0=i % 8))
        sched.insert(5 * i + 3, dict(corpus="B", kind="fp32", shape=SHAPES[4], B=8, knobs=knobs, mode="callable",
                                     host=False, rot=200 + i, b0=(i + 3) % 8, polls=(victim[lo], victim[hi])))
    words = [layout(c["B"], c["shape"][0], c["shape"][3], c["shape"][3], c["shape"][1])["words"] for c in sched]
    first = dict(sched[int(np.argmax(words))])
    first.pop("polls", None)
    seen = set()                              # (id, word half) of the stage-1 and candidate ids in 1..400
    failures = []
    plain_counter_hits = 0                    # stale stage-1 ids, in a victim's polled words, equal to its COUNTER
    prev = None
    for n, c in enumerate([first] + sched):
        c = dict(c)
        polls = c.pop("polls", None)
        bad = call(**c)
        if n == 0 and oto.pool_stats()[0] != 1:
            failures.append(f"the first call created {oto.pool_stats()[0]} buffers")
        if bad:
            failures.append(f"call {n} {c}: " + "; ".join(bad))
        r = runner(c["corpus"], c["kind"])
        key = (c["shape"], c["b0"], c["B"], c["rot"], True)
        lex = r.want(*key)[0]
        for arr in ([] if lex is None else [lex]) + [r.cands[key]]:
            flat = arr.reshape(-1)
            for half in (0, 1):
                seen.update((int(x), half) for x in flat[half::2] if 1 <= x <= 400)
        if polls is not None:                 # one buffer: this call's counter is its number, n + 1
            k, _, kb, C, fk = prev[0]
            at = layout(8, k, C, fk, kb)["lex_plain"]
            flat = prev[1].reshape(-1)
            plain_counter_hits += sum(1 for j in range(1, len(flat), 2)
                                      if polls[0] <= at + j // 2 < polls[1] and int(flat[j]) == n + 1)
        prev = (c["shape"], lex)
    low_ids_seen = sorted(x for x in range(1, 401) if (x, 0) in seen and (x, 1) in seen)

    # ---- 2. forged tags
    forged = []
    if "--sweep-only" in sys.argv[1:]:
        st = oto.pool_stats()
        print(json.dumps({"created": st[0], "idle": st[1], "sweep_calls": len(sched), "sweep_failures": failures,
                          "low_ids_seen": low_ids_seen, "plain_counter_hits": plain_counter_hits, "forged": forged}),
              flush=True)
        return
    shape2, B2 = SHAPES[4], 8
    lay2 = layout(B2, shape2[0], shape2[3], shape2[4], shape2[2])
    # region -> (call 1's (k, C, final_k) putting its plain words inside call 2's region, call 2's polled
    #            words, call 2's knobs, host results)
    regions = {
        "stage2":     ((24, 4, 1), (0, lay2["cand"]), (1, 1), True),
        "prescore":   ((256, 16, 4), (lay2["prescore"], lay2["lex_plain"]), (1, 1), True),
        "candidates": ((64, 4, 1), (lay2["cand"], lay2["final"]), (0, 1), False),
        "final_host": ((180, 4, 1), (lay2["final"], lay2["prescore"]), (0, 1), True),
        "final_copy": ((180, 4, 1), (lay2["final"], lay2["prescore"]), (1, 1), False),
    }
    rA = runner("A", "fp32")
    for region, ((k1, C1, fk1), (lo, hi), knobs2, host2) in regions.items():
        shape1, B1 = (k1, 64, 64, C1, fk1), 8
        lex1 = rA.want(shape1, 0, B1, 0, False)[0]
        pres = np.stack([rA.c.g.exact_scores([b], lex1[b:b + 1])[0] for b in range(B1)])
        image = np.concatenate([lex1.reshape(-1).view(np.uint32), oto.bits(pres).reshape(-1)])   # int32 units
        at = layout(B1, k1, C1, fk1, 64)["lex_plain"]
        high = {at + j // 2: int(image[j]) for j in range(1, len(image), 2)}       # word -> its stale high half
        neg = [v for j, v in enumerate(oto.bits(pres).reshape(-1).tolist())
               if j % 2 == 1 and v & 0x80000000 and v != 0xFF800000]
        for counter in (0x7FFFFFFF, 0x7F800000, (neg[0] & 0x7FFFFFFF) if neg else 0):
            rec = {"region": region, "counter": counter, "bad": []}
            s0 = oto.pool_stats()
            rec["bad"] += call("A", "fp32", shape1, 0, B1, (1, 1), "array", True, 0, low_ids=False)   # call 1
            if oto.pool_stats()[3] != s0[3] + 1:
                rec["bad"].append("call 1 did not take the host rerank (no plain stage-1 words left)")
            tag = 0x80000000 | counter
            rec["stale_hits"] = sum(1 for w, v in high.items() if lo <= w < hi and v == tag)
            L.cbv2_set_tag_lab(ctypes.c_uint32(counter))
            s0 = oto.pool_stats()
            rec["bad"] += call("B", "fp32", shape2, 0, B2, knobs2, "array", host2, 3, low_ids=True)   # call 2
            d3 = oto.pool_stats()[3] - s0[3]
            if d3 != (1 if knobs2[0] else 0):
                rec["bad"].append(f"call 2 took another path (host rerank calls moved by {d3})")
            forged.append(rec)
    rec = {"region": "wrap", "counter": 0x7FFFFFFE, "stale_hits": 0, "bad": []}
    L.cbv2_set_tag_lab(ctypes.c_uint32(0x7FFFFFFE))
    for i, (knobs, host) in enumerate((((1, 1), True), ((0, 1), True), ((1, 1), False), ((0, 1), False))):
        rec["bad"] += call("B", "fp32", SHAPES[0], i, 2, knobs, "callable", host, i, low_ids=True)
    forged.append(rec)

    st = oto.pool_stats()
    print(json.dumps({"created": st[0], "idle": st[1], "sweep_calls": len(sched), "sweep_failures": failures,
                      "low_ids_seen": low_ids_seen, "plain_counter_hits": plain_counter_hits, "forged": forged}),
              flush=True)


if __name__ == "__main__":
    main()
