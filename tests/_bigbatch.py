"""Scripted walks at large batch sizes (test infrastructure): every compute
entry point at the B where the dispatch in csrc/colbert_mi355x.hip changes
behaviour between 255 and 65535, and just past 65535, on the exact pools of
tests/_exact.py.  numpy only; tests/test_bigbatch_model.py plays the walks
through the brute-force backend and its mutants, tests/test_gpu_bigbatch.py
through the C ABI.

The batch-size table.  Above B = 16 every MaxSim scan is a doc-interleaved
launch of ceil(B / qpb) query groups; plan_split gives each group
max(1, per_cu * CUs / groups) static chunks and, while groups * slices <= 512
counters (kRingInts; slices = 8, or 1 under CBV2_OPT_DYNAMIC_TAIL = 2) and
0.9 n / chunks >= 64 docs, a dynamic tail.  The shapes (pick_shape's cost
tables, restated in scan_shape and checked on the device through
cbv2_index_last_scan_plan):

  index            shape picked for B >= 255         qpb  per CU
  bf16, fp32 (hi)  8 waves x 4, every ld              32    1     (the 4-wave shapes win only below B = 145)
  MXFP8 ld = 128   8 x 8; 4 x 8 for B = 64 m + 1..32  64    1     (4 x 8: 32 / 2, while m <= 10: 257 is one)
  MXFP8 long       8 x 8                              64    1

  class   B                          what changes there
  256     255, 256, 257              the largest B any earlier test reaches, and the first beyond
  gate    2048, 2049  (qpb 32)       64 / 65 query groups: the ring of 64 x 8 tail counters is full; the tail
          4096, 4097  (qpb 64)       goes on under DYNAMIC_TAIL = 2 (1 slice), off under 1, is off under 0
  cu      32 CUs, 32 CUs + 1         groups outnumber the resident workgroups: target / groups = 0, clamped to 1
          (64 CUs, + 1 for MXFP8)    (one chunk spans the shard, grid = groups); computed from the device's CU
          16384, 16385 (qpb 32)      count (over_target); and 512 / 513 groups, where the one-slice ring of
          32768, 32769 (qpb 64)      DYNAMIC_TAIL = 2 is full too (ld = 128 only)
  max     65535                      the last B of the bounded calls; grid.y = 65535 (ld = 128, n = 63 / 64 / 65)
  over    65536                      EINVAL from every call bounded at 65535 (nothing launched, outputs
                                     untouched): the calls that take f32 queries on a faithful index (BOUNDED)
                                     and cbv2_search_filtered_batch, whose batch cbv2_filter_batch_create bounds;
          65536, 70001               accepted by the four selection calls (cbv2_select_topk, _topk_rows,
                                     _merge_topk, _group_topk_rows) and, with bf16 / MXFP8 queries, by cbv2_score,
                                     cbv2_search_filtered and cbv2_search_grouped (check_query: B >= 1 only; their
                                     launches clamp grid.y to 65535 and loop)
  large-n 2049 at n = 70003          cbv2_search / cbv2_search_f32 under block-max, sampled and fused top-k.  The
                                     case was asked for so that the [B][n] matrix passes 2^29 elements; at the
                                     stated sizes it holds 143,436,147 scores = 2^27.1 elements (2^29.1 bytes),
                                     and a matrix past 2^29 elements is 2 GiB, over WS_BUDGET: the two demands
                                     exclude each other, the stated sizes are kept, and NO 2^31- or 2^32-byte
                                     offset of a score matrix is crossed by these walks (tests/
                                     test_gpu_high_offsets.py crosses them at small B)

A 16-query workgroup (64 groups at B = 1024) is picked by no scan at that B:
8 x 4 costs 32 x 17.4 there against 64 x 9.6.  gate_edges keeps only the
edges of shapes that scan_shape picks on one side of them.

Shapes: n = 300 at the gates (0.9 * 300 / 4 chunks = 67 >= 64: the tail is on
at 64 groups and the ring alone turns it off at 65; the 200-doc pools of ld =
512 / 1024 are drawn with replacement), 600 for the 256 class at ld = 128;
lq rotates over 32 / 17 / 1 up to the cu class and over 4 / 1 / 3 from 65535
on (a query buffer under 256 MiB); k <= 100, cap = 64, C = 50, r <= 3.

A step carries ``tile`` = 1: its rows repeat with the pool's query count
(_walk.one_period), so the model answers one period and repeats it.  Filter
batches cycle through CYCLE, whose length 5 divides 65 and 40.
"""
import functools
from collections import Counter

import numpy as np

import _exact as ex
import _walk as wk

CUS = 256                                        # an MI355X; the GPU test passes the device's own count
WS_BUDGET = 2 << 30                              # every workspace a walk asks for stays under this
RING_INTS, MIN_CHUNK = 512, 64                   # kRingInts = 64 groups x 8 slices, kMinChunkDocs
# pick_shape's tables: (queries per workgroup, ms per group, workgroups per CU, dynamic share)
BF16_SHAPES = ((4, 4.6, 2, None), (8, 6.1, 2, None), (16, 9.6, 2, None), (32, 17.4, 1, 0.10))
F8_SHAPES = ((4, 2.45, 2, 0.3), (8, 3.0, 2, 0.3), (16, 5.2, 3, 0.6), (32, 9.5, 2, 0.6), (64, 18.2, 1, 0.10))
CYCLE = (None, 0, 3, 2, 3)                       # a filter batch's rows: all docs, the empty filter, a repeated handle
PLAN_EPS = ("score", "search", "search_f32")     # their last scan launch is the index kind's plain scan of B queries
SELECTIONS = ("topk_rows", "select_topk", "merge_topk", "group_topk_rows")
CLASSES = ("256", "gate", "cu", "max", "over", "large-n")
# the calls whose B is bounded at 65535: CBV2_REQUIRE in check_f32 and in the faithful branch (f32 queries on an index
# with a residual) of cbv2_search_filtered / _filtered_batch / _grouped, in their _f32 forms, and in
# cbv2_filter_batch_create -- a filtered batch search takes the B of its batch, so it is bounded on every index
BOUNDED = {"fp32": ("score", "search_f32", "search_f32_split", "rerank_f32", "search_filtered", "search_filtered_f32",
                    "search_filtered_batch", "search_grouped", "search_grouped_f32"),
           "bf16": ("search_filtered_batch",),
           "mxfp8": ("search_filtered_batch",)}
UNBOUNDED_SCANS = ("score", "search_filtered", "search_grouped")       # ... with bf16 / MXFP8 queries: B >= 1 only


# ---------------------------------------------------------------------------- the dispatch, restated
def pick_shape(table, B):
    best, best_ms = table[0], np.float32(1e30)
    for row in table:
        ms = np.float32((B + row[0] - 1) // row[0]) * np.float32(row[1])
        if ms <= best_ms:
            best, best_ms = row, ms
    return best


@functools.lru_cache(maxsize=None)
def scan_shape(kind, ld, B):
    """(qpb, workgroups per CU, dynamic share) of the doc-interleaved scan of B > 16 queries."""
    assert B > 16
    if kind == "mxfp8":
        row = pick_shape(F8_SHAPES, B) if ld == 128 else F8_SHAPES[-1]
    else:
        row = pick_shape(BF16_SHAPES, B) if ld == 128 else BF16_SHAPES[-1]
    assert row[3] is not None, f"{kind} ld={ld} B={B}: a shape whose dynamic share this module does not restate"
    return row[0], row[2], float(np.float32(row[3]))


def plan(kind, ld, n, B, dynamic_tail, cus=CUS):
    """plan_split: what cbv2_index_last_scan_plan reports after the plain scan of B queries over n docs."""
    qpb, per_cu, frac = scan_shape(kind, ld, B)
    groups, target = -(-B // qpb), per_cu * cus
    chunks = min(max(target // groups, 1), n)
    tail_chunk = (int(n * (1.0 - frac)) // chunks) & ~63
    slices = 1 if dynamic_tail == 2 else 8
    tail = bool(dynamic_tail) and groups * slices <= RING_INTS and tail_chunk >= MIN_CHUNK
    if tail:
        chunk, static = tail_chunk, tail_chunk * chunks
    else:
        chunk = -(-n // chunks)
        chunks, static = -(-n // chunk), n
    return {"workgroups": groups * chunks, "chunk_docs": chunk, "static_docs": static, "dynamic_tail": tail,
            "groups": groups, "qpb": qpb, "target": target}


def _tables(kind, ld):
    t = F8_SHAPES if kind == "mxfp8" else BF16_SHAPES
    return t if ld == 128 else t[-1:]


def gate_edges(kind, ld, slices=8):
    """Both neighbours of every B at which a shape's group count passes the
    counter ring (512 / slices groups), for the shapes picked on one side."""
    out = []
    for qpb, _, _, _ in _tables(kind, ld):
        B = RING_INTS // slices * qpb
        if B + 1 <= 65535 and qpb in (scan_shape(kind, ld, B)[0], scan_shape(kind, ld, B + 1)[0]):
            out += [B, B + 1]
    return sorted(out)


@functools.lru_cache(maxsize=None)
def over_target(kind, ld, cus=CUS):
    """The first B whose query groups outnumber the launch's resident workgroups."""
    for B in range(257, 65536):
        qpb, per_cu, _ = scan_shape(kind, ld, B)
        if -(-B // qpb) > per_cu * cus:
            return B
    raise ValueError("no B below 65536 outnumbers the workgroups")


def class_bs(kind, ld, cls, cus=CUS):
    if cls == "256":
        return [255, 256, 257]
    if cls == "gate":
        return gate_edges(kind, ld)
    if cls == "cu":
        t = over_target(kind, ld, cus)
        return sorted({t - 1, t} | set(gate_edges(kind, ld, slices=1)))
    return {"max": [65535], "over": [65536, 70001], "large-n": [2049]}[cls]


def b_class(kind, ld, B, cus=CUS, n=0):
    if n > 65535:
        return "large-n"
    for cls in ("256", "gate", "cu", "max", "over"):
        if B in class_bs(kind, ld, cls, cus):
            return cls
    return None


def required_gates(kind, ld, cls, cus=CUS):
    """(gate, B, DYNAMIC_TAIL) of every plan assertion a class's walks must make."""
    if cls == "gate":
        return {("ring of 8 slices", B, dt) for B in gate_edges(kind, ld) for dt in (0, 1, 2)}
    if cls == "cu":
        t = over_target(kind, ld, cus)
        return {("groups over target", B, 1) for B in (t - 1, t)} | \
            {("ring of 1 slice", B, 2) for B in gate_edges(kind, ld, slices=1)}
    return set()


def gates_of(kind, ld, B, dt, cus=CUS):
    out = set()
    if B in gate_edges(kind, ld):
        out.add(("ring of 8 slices", B, dt))
    if B in gate_edges(kind, ld, slices=1) and dt == 2:
        out.add(("ring of 1 slice", B, dt))
    t = over_target(kind, ld, cus)
    if B in (t - 1, t) and dt == 1:
        out.add(("groups over target", B, dt))
    return out


def check_gates_flip(kind, ld, n, cus=CUS):
    """The model itself changes at every gate (a changed constant must not turn the assertions into no-ops)."""
    for lo, hi in zip(*[iter(gate_edges(kind, ld))] * 2):
        assert plan(kind, ld, n, lo, 1, cus)["dynamic_tail"] and not plan(kind, ld, n, hi, 1, cus)["dynamic_tail"], (lo, hi)
        assert plan(kind, ld, n, lo, 2, cus)["dynamic_tail"] and plan(kind, ld, n, hi, 2, cus)["dynamic_tail"], (lo, hi)
        assert not plan(kind, ld, n, lo, 0, cus)["dynamic_tail"]
        assert plan(kind, ld, n, lo, 1, cus)["groups"] == 64 and plan(kind, ld, n, hi, 1, cus)["groups"] == 65
    t = over_target(kind, ld, cus)
    a, b = plan(kind, ld, n, t - 1, 1, cus), plan(kind, ld, n, t, 1, cus)
    assert a["groups"] == a["target"] and b["groups"] == b["target"] + 1 and b["workgroups"] == b["groups"]
    if ld == 128:
        for lo, hi in zip(*[iter(gate_edges(kind, ld, slices=1))] * 2):
            assert plan(kind, ld, n, lo, 2, cus)["groups"] == 512 and not plan(kind, ld, n, hi, 2, cus)["dynamic_tail"]


# ---------------------------------------------------------------------------- the steps
DEFAULTS = {name: vals[0] for name, _, vals in wk.OPTIONS}
VEC_A = dict(FUSED_TOPK=1, TOPK_BMAX=1, BAND_DOC_MAJOR=0, RESCORE_SPLIT=1, DYNAMIC_TAIL=1)
VEC_B = dict(FUSED_TOPK=0, TOPK_BMAX=0, BAND_DOC_MAJOR=3, RESCORE_SPLIT=0, DYNAMIC_TAIL=2)


def options(**switched):
    v = dict(DEFAULTS, **switched)
    return {"ep": "set_options", "values": tuple(int(v[nm]) for nm in wk.OPT_NAMES)}


class _Script:
    """Writes the steps of one walk: ds, q0, lq, k rotate deterministically."""

    def __init__(self, kind, ld, lqs, n_batches=()):
        self.kind, self.ld, self.lqs, self.i = kind, ld, lqs, 0
        self.Bp = wk.SIZE[ld][1]
        self.steps, self.batch_bs = [], list(n_batches)

    def opts(self, **switched):
        self.steps.append(options(**switched))

    def base(self, ep, B):
        self.i += 1
        i = self.i
        return {"ep": ep, "ds": 1000 + 7919 * i, "B": int(B), "lq": self.lqs[i % len(self.lqs)], "q0": (11 * i) % self.Bp,
                "tile": 1}

    def args(self, ep, B, between=True):
        a, i = self.base(ep, B), self.i
        k = (10, 1, 100)[i % 3]
        if ep in SELECTIONS:
            a["zeros"] = i % 2
            if ep == "topk_rows":
                a.update(k=k, pad=(0, 3)[i % 2], sampled=(i // 2) % 2)
            elif ep == "select_topk":
                a.update(C=50, k=(10, 50, 51)[i % 3], ids=i % 2)
            elif ep == "merge_topk":
                a.update(G=(3, 1, 2)[i % 3], k=k)
            else:
                a.update(g=i % 2, k=k, r=1 + i % 3)
            return a
        if ep == "score":
            return a
        if ep == "search_filtered_batch":
            if B not in self.batch_bs and between:             # (an invalid step takes batch 0: no batch of its B exists)
                self.batch_bs.append(B)
            a.update(fb=self.batch_bs.index(B) if B in self.batch_bs else 0, k=k)
            return {key: a[key] for key in ("ep", "ds", "fb", "B", "lq", "q0", "tile", "k")}
        if ep in ("rerank", "rerank_ws", "rerank_f32"):
            a.update(C=50, k=(10, 0, 50)[i % 3])
            return a
        if ep == "retrieve":
            a.update(k=10, kb=(10, 0)[i % 2], C=20, final_k=7, how=("finish", "finish_host", "cancel")[i % 3])
            return a
        a["k"] = k
        if ep in ("search_filtered", "search_filtered_f32"):
            a["f"] = (3, 2, 5, 1, 4, 0)[i % 6]
        if ep in ("search_grouped", "search_grouped_f32"):
            a.update(g=i % 2, r=1 + i % 3)
        if ep in wk.FAITHFUL_EPS:
            a["cap"] = max(64, k)
        if self.kind == "fp32" and ep in ("search_filtered", "search_grouped") and B >= 16384:
            # with f32 queries these two size their band with the library's own cap (16384: B * cap * 8 bytes pass
            # WS_BUDGET from B = 16384 on) wherever they take the band; k = 100 with the 5 % filter (m <= k) or with
            # n < 4 k r keeps them on the pair / full path, whose workspace is the [B][m] / [B][n] matrix
            a["k"] = 100
            if ep == "search_filtered":
                a["f"] = 2
        if ep == "search_f32_split" and between:
            a["between"] = self.args(("score", "search_f32", "rerank_f32")[i % 3], B, between=False)
        return a

    def add(self, ep, B):
        self.steps.append(self.args(ep, B))

    def invalid(self, ep, B):
        a = self.args(ep, B, between=False)
        a = {"ep": "invalid", "what": f"B{B}", "on": ep, **{key: val for key, val in a.items() if key not in ("ep", "tile")}}
        a.update(ws_delta=0, ws_offset=0, null_status=0)
        self.steps.append(a)


def _finish(kind, ld, n, sc, tag, cls, large=False):
    w = wk.scripted(kind, ld, 0, sc.steps, tag, large=large, n=n)
    w.batches = [[CYCLE[b % len(CYCLE)] for b in range(B)] for B in sc.batch_bs] or [list(CYCLE)]
    w.cls = cls
    return w


def _plan_sweep(sc, kind, Bs):
    """The calls whose scan plan is asserted, at every B under DYNAMIC_TAIL = 1, 0, 2."""
    for dt in (1, 0, 2):
        sc.opts(DYNAMIC_TAIL=dt, FUSED_TOPK=int(dt == 2))
        for B in Bs:
            if kind == "fp32":
                sc.add("search_f32", B)
            else:
                sc.add("score", B)
                sc.add("search", B)


def _every_entry_point(sc, kind, Bs, skip=()):
    """Every entry point of the kind at every B, under VEC_A and under VEC_B."""
    eps = [e for e in wk.entry_points(kind) if e not in skip]
    for vec in (VEC_A, VEC_B):
        sc.opts(**vec)
        for ep in eps:
            for B in Bs:
                sc.add(ep, B)


def gate_n(kind, ld):
    return 600 if ld == 128 else 300


def class_walk(kind, ld, cls, cus=CUS):
    """The walk of one (kind, ld, class) for the classes 256 / gate / cu."""
    Bs = class_bs(kind, ld, cls, cus)
    n = gate_n(kind, ld) if cls == "256" else 300
    sc = _Script(kind, ld, (32, 17, 1))
    _plan_sweep(sc, kind, Bs)
    skip = () if max(Bs) <= 2049 else ("retrieve",)
    _every_entry_point(sc, kind, Bs, skip)
    return _finish(kind, ld, n, sc, f"big batch {cls}", cls)


def max_walks(kind, cus=CUS):
    """B = 65535 over 63 / 64 / 65 docs (ld = 128), and just past it."""
    out = []
    for n, vec in ((63, VEC_A), (64, VEC_B), (65, {})):
        sc = _Script(kind, 128, (4, 1, 3))
        if n == 64:
            _plan_sweep(sc, kind, [65535])
        sc.opts(**vec)
        for ep in wk.entry_points(kind):
            if ep != "retrieve":
                sc.add(ep, 65535)
        if n == 63:                                            # every bounded call rejects 65536
            for ep in BOUNDED[kind]:
                sc.invalid(ep, 65536)
        else:                                                  # ... and the unbounded ones go on
            B = 65536 if n == 64 else 70001
            for ep in SELECTIONS + (UNBOUNDED_SCANS if kind != "fp32" else ()):
                sc.add(ep, B)
        out.append(_finish(kind, 128, n, sc, f"big batch max n={n}", "max"))
    return out


def large_n_walk(kind):
    """70003 docs at B = 2049: the [B][n] matrix of a search's workspace under the three row selections."""
    sc = _Script(kind, 128, (32, 17, 1))
    ep = "search_f32" if kind == "fp32" else "search"
    for vec in ({}, dict(TOPK_BMAX=0), dict(FUSED_TOPK=1)):
        sc.opts(**vec)
        sc.add(ep, 2049)
    return _finish(kind, 128, 70003, sc, "big batch large n", "large-n", large=True)


def cases():
    """(kind, ld, class) of every GPU test case."""
    out = []
    for kind in ex.KINDS:
        for ld in wk.LDS:
            out += [(kind, ld, "256"), (kind, ld, "gate")]
        out += [(kind, 128, "cu"), (kind, 128, "max"), (kind, 128, "large-n")]
    return out


def case_walks(kind, ld, cls, cus=CUS):
    if cls == "max":
        return max_walks(kind, cus)
    if cls == "large-n":
        return [large_n_walk(kind)]
    return [class_walk(kind, ld, cls, cus)]


def all_walks(cus=CUS):
    return [w for case in cases() for w in case_walks(*case, cus)]


def truncation_walk():
    """CPU only: the one shape at which ``b * n`` passes 2^32 with B <= 65535
    (rows 65533 and 65534 of a 65540-doc shard); its [B][n] matrix would take
    17 GB, far over WS_BUDGET, so no GPU test plays it."""
    sc = _Script("bf16", 512, (1,))
    sc.opts()
    sc.add("search", 65535)
    sc.steps[-1]["k"] = 1
    return _finish("bf16", 512, 65540, sc, "b * n past 2^32", "max")


# ---------------------------------------------------------------------------- coverage
def steps_of(walks):
    for w in walks:
        for i, st in enumerate(w.steps):
            yield w, i, st
            if "between" in st:
                yield w, i, dict(st["between"], opts=st["opts"])


def required_cells():
    """(kind, entry point, B class) of every cell the walks must visit."""
    cells = set()
    for kind in ex.KINDS:
        for ep in wk.entry_points(kind):
            for cls in ("256", "gate", "cu", "max"):
                if ep == "retrieve" and (cls in ("cu", "max") or max(class_bs(kind, 128, cls)) > 2049):
                    continue                                   # retrieve: B up to the 2049 class only
                cells.add((kind, ep, cls))
        for ep in BOUNDED[kind]:
            cells.add((kind, "invalid:" + ep, "over"))
        for ep in SELECTIONS + (UNBOUNDED_SCANS if kind != "fp32" else ()):
            cells.add((kind, ep, "over"))
        cells.add((kind, "search_f32" if kind == "fp32" else "search", "large-n"))
    return cells


def coverage(walks, cus=CUS):
    c = Counter()
    for w, _, st in steps_of(walks):
        if "B" not in st:
            continue
        cls = b_class(w.kind, w.ld, st["B"], cus, w.n)
        c[w.kind, ("invalid:" + st["on"]) if st["ep"] == "invalid" else st["ep"], cls] += 1
    return c


def gate_steps(walks, cus=CUS):
    """(gate, B, DYNAMIC_TAIL) -> steps of PLAN_EPS that sit on it."""
    c = Counter()
    for w, _, st in steps_of(walks):
        if st["ep"] in PLAN_EPS and not (st["ep"] == "score" and w.kind == "fp32"):
            dt = dict(zip(wk.OPT_NAMES, st["opts"]))["DYNAMIC_TAIL"]
            for g in gates_of(w.kind, w.ld, st["B"], dt, cus):
                c[(w.kind, w.ld) + g] += 1
    return c
