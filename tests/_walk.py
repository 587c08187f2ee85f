"""Seeded walks over the C ABI on exact corpora (test infrastructure): the
generator of call sequences, the exact model of every call, the transcript and
the player that compares a backend's answers with the model bit for bit.

numpy only: no torch, no GPU library.  tests/test_walk_model.py plays the walks
through a brute-force CPU backend and its mutants, tests/test_gpu_walk.py
through the C ABI.

A WALK is one index handle, one workspace, one query buffer and 8-12 steps:
  pool      ExactCorpus(kind, ld, N, B, seed=1) with the sizes of
            tests/test_gpu_exact_scores.py (SIZE); every kernel must return its
            reference's bits in any accumulation order (tests/_exact.py).
  corpus    n docs drawn WITH replacement from the pool (sel); the index holds
            docs[sel], the reference row of pool query q at lq tokens is
            ref[q, lq - 1, sel].  Neighbouring docs are unrelated and about a
            third of the docs of a full-size walk are exact duplicates: mass
            ties for the (score desc, id asc) rule of every selection.
  handles   six filters (one per size class, garbage bits past n), two filter
            batches (None entries, repeats, the empty filter) and two groupings
            of tests/_groups.py, created once per walk and reused by its steps
            across option changes.
  steps     step 0 sets a legal vector over all 17 handle options (the filter
            batches are created under it; _draw_options: uniform vectors and
            vectors near the defaults, half and half); the others are drawn
            from a shuffled deck of the entry points legal for the pool's kind,
            with option changes and invalid calls mixed in.  A step takes the
            previous call's B and lq with probability 1/4 (the stale-split
            case), else the next B of a deck over the edge list.  Its queries are
            the pool's queries q0, q0 + 1, ... (mod the pool's B), written in
            place into the walk's one query buffer: the contents at that
            address change from step to step.
  seeds     the draws are stratified so that few seeds visit every cell of the
            coverage table (tests/test_walk_model.py): an even seed takes the
            next n of the edge list (1, 2, 15 ... 257, the whole pool), an odd
            one a uniform n in [1, N]; consecutive seeds start the entry-point
            deck five places and the B deck seven places further on.
            Everything else is drawn from the
            edge lists by numpy's default_rng seeded with (seed, ld, kind).
  large     the large walks (ld = 128): n in LARGE_N gathered from the same
            pool, the steps of LARGE_EPS, B of LARGE_BS, k up to 1100, and a
            theme per seed (THEMES): the default option vector throughout, or
            the defaults with one A/B switched and the batch sizes its path
            needs.  large_paths restates the dispatch's conjunctions, so the
            coverage counts the steps that launch a path.
Every step renders as one line (entry point, every argument, the option vector
in force); data (candidates, matrices, stage-1 lists) derive from the walk's
seed and the step's ``ds``, so a transcript replays the walk.

The model reuses what other tests pin: oracle.topk (on the keys),
oracle.rerank_select, tests/_groups.oracle and oracle.rrf (the Python RRF that
cbv2_rrf_fuse / hybrid.rrf_fuse are pinned against: this module loads no
library).  A faithful call's status word is checked as -1 or a band size in
[min(k, scoring docs), cap]; what begin writes besides fk is not compared.

The model works on score BITS: every ranking is by the order-preserving uint32
key of the float (tests/_groups.f2u), the key the kernels rank by, so -0.0
ranks below +0.0.  The selection steps' matrices hold both zeros beside each
other at the k-th place.
"""
from __future__ import annotations

import hashlib

import numpy as np

import _exact as ex
import _exact_shapes as shapes
import _groups as grp
from oracle import oracle as orc

EINVAL = -1
LQ_MAX = 32
BAND_CAP = 16384
RRF_K = 60
SIZE, LDS = shapes.SIZE, shapes.LDS            # ld -> (pool docs, pool queries)
LARGE_N = (65536, 65537, 70003)
N_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LQS = (1, 2, 7, 15, 16, 17, 31, 32)
CS = (1, 50, 1024, 1025, 1100)
FILTER_CLASSES = ("none", "one", "5pct", "half", "over_half", "all")

# name, CBV2_OPT_* id, legal values drawn (the first is the handle's default)
OPTIONS = (
    ("FUSED_TOPK", 1, (0, 1, 2)),
    ("DYNAMIC_TAIL", 2, (1, 0, 2)),
    ("BAND_DOC_MAJOR", 3, (0, 1, 2, 3, 4)),
    ("BAND_LOWER_BOUND", 4, (1, 0)),
    ("TOPK_BMAX", 5, (1, 0)),
    ("BAND_FUSED", 6, (0, 1)),
    ("RESCORE_SPLIT", 7, (1, 0)),
    ("BAND_REUSE", 8, (1, 0)),
    ("BAND_BLOCK_SKIP", 9, (1, 0)),
    ("RESCORE_GRID", 10, (0, 1, 7, 64)),
    ("DENSE_DOCS", 11, (0, 1)),
    ("P1_COLLECT_FUSED", 12, (1, 0)),
    ("FOLD_KEYS", 13, (1, 0)),
    ("FILTER_PATH", 14, (0, 1, 2)),
    ("FILTER_BATCH_CHUNK_DOCS", 15, (0, 1, 7, 64)),
    ("FILTER_BAND", 16, (0, 1, 2)),
    ("GROUP_BAND", 17, (0, 1, 2)),
)
OPT_NAMES = tuple(o[0] for o in OPTIONS)
OPT_INDEX = {name: i for i, name in enumerate(OPT_NAMES)}
BAND_OPTIONS = ("BAND_DOC_MAJOR", "BAND_LOWER_BOUND", "BAND_FUSED", "RESCORE_SPLIT", "BAND_REUSE", "BAND_BLOCK_SKIP",
                "P1_COLLECT_FUSED", "FOLD_KEYS")

FAITHFUL_EPS = ("search_f32", "search_f32_split", "rerank_f32", "search_filtered_f32", "search_grouped_f32")
PLAIN_EPS = ("search", "rerank", "rerank_ws")                      # bf16 / MXFP8 queries only
COMMON_EPS = ("score", "search_filtered", "search_filtered_batch", "search_grouped", "topk_rows", "select_topk",
              "merge_topk", "group_topk_rows", "retrieve")
LARGE_EPS = {"topk_rows", "score", "search", "search_f32", "search_f32_split", "search_filtered", "search_filtered_f32",
             "search_filtered_batch", "search_grouped", "search_grouped_f32", "rerank", "rerank_ws", "rerank_f32"}
# the entry points that read each option: the header's "Handle options" and the dispatch in csrc/colbert_mi355x.hip
_SCANS = ("score", "search", "search_f32", "search_f32_split", "retrieve")
_FAITHFUL_RESCORE = ("search_f32", "search_f32_split", "rerank_f32", "search_filtered_f32", "search_grouped_f32")
READS = {
    "FUSED_TOPK": ("search", "search_f32", "search_f32_split", "retrieve"),      # fused_slots, and through it bmax_eligible
    "DYNAMIC_TAIL": _SCANS + ("search_grouped",),
    "TOPK_BMAX": ("search", "search_f32", "search_f32_split", "retrieve"),       # bmax_eligible
    "DENSE_DOCS": _SCANS,
    "RESCORE_SPLIT": _FAITHFUL_RESCORE + ("rerank", "rerank_ws", "retrieve"),     # rerank_impl reads it on bf16 too
    "RESCORE_GRID": _FAITHFUL_RESCORE,
    "FILTER_PATH": ("search_filtered", "search_filtered_f32", "search_filtered_batch"),
    "FILTER_BATCH_CHUNK_DOCS": ("search_filtered_batch",),
    "FILTER_BAND": ("search_filtered_f32",),
    "GROUP_BAND": ("search_grouped_f32",),
}
for _o in BAND_OPTIONS:
    READS.setdefault(_o, ("search_f32", "search_f32_split"))
INVALID_KINDS = ("k0", "r0", "r9", "lq0", "lq33", "ws_short", "ws_misaligned", "batch_B")
INVALID_FAITHFUL = ("cap_lo", "cap_hi", "null_status")


LARGE_BS = (1, 2, 3, 4, 5, 8, 9, 32, 33, 65)     # the large walks: folded keys <= 4, pair band <= 8, dynamic tail >= 33


def score_batches(kind, ld, large=False):
    """The batch sizes of tests/test_gpu_exact_scores.py (tests/_exact_shapes.py):
    both neighbours of every dispatch threshold; the large walks keep those of
    LARGE_BS."""
    bs = shapes.score_batches(kind, ld)
    return [b for b in bs if b in LARGE_BS] if large else bs


def scan_family(kind, ld):
    return "fp32" if kind == "fp32" else (f"{kind}-128" if ld == 128 else f"{kind}-long")


def entry_points(kind, large=False):
    eps = COMMON_EPS + (FAITHFUL_EPS if kind == "fp32" else PLAIN_EPS)
    return tuple(e for e in eps if not large or e in LARGE_EPS)


def k_class(k, n):
    return ">1024" if k > 1024 else ("<n" if k < n else ("=n" if k == n else ">n"))


# ---------------------------------------------------------------------------- the dispatch, restated
# The conjunctions csrc/colbert_mi355x.hip decides its large-size paths by,
# restated on (kind, ld, n, B, k, options) so that the coverage of the large
# walks counts the steps that LAUNCH a path, not the steps that set its option.
SCAN_EPS = ("score", "search", "search_f32", "search_f32_split", "search_filtered", "search_filtered_f32",
            "search_filtered_batch", "search_grouped", "search_grouped_f32", "retrieve")   # run the kind's MaxSim scan
SAMPLED_MIN_N, BM_MAX_N, TOPK_MAX, FUSED_MAX_K, BAND_PAIR_MAX_B = 65536, 64 * 24576, 1024, 104, 8


def fused_topk(w, B, k, o):
    """fused_slots() > 0: the bf16 doc-interleaved scan (B > 16) keeps the top-k itself."""
    return bool(o["FUSED_TOPK"]) and w.kind != "mxfp8" and w.ld == 128 and k <= FUSED_MAX_K and B > 16


def bmax_eligible(w, B, k, o):
    return bool(o["TOPK_BMAX"]) and w.ld == 128 and SAMPLED_MIN_N <= w.n <= BM_MAX_N and k <= TOPK_MAX \
        and not fused_topk(w, B, k, o)


def band_reuses_topk(w, B, k, o):
    return bool(o["BAND_REUSE"] and o["RESCORE_SPLIT"]) and w.n >= k \
        and not (B <= BAND_PAIR_MAX_B and w.ld == 128 and o["BAND_FUSED"])


def phase1_collect_fused(w, B, k, o):
    return bool(o["P1_COLLECT_FUSED"]) and B <= BAND_PAIR_MAX_B and k <= TOPK_MAX and band_reuses_topk(w, B, k, o) \
        and bmax_eligible(w, B, k, o) and bool(o["BAND_BLOCK_SKIP"]) and not o["BAND_DOC_MAJOR"]


def large_paths(w, step):
    """The large-size dispatch paths a step of a large walk launches, as
    (path, position of the option that switches it): "on" where the path runs,
    "off" where everything else it needs holds and only its own option keeps it
    out -- the two sides of an A/B."""
    ep, o = step["ep"], dict(zip(OPT_NAMES, step["opts"]))
    B, k = step.get("B", 0), step.get("k", 0)
    out = set()
    if ep in ("search", "search_f32", "search_f32_split") and k <= TOPK_MAX and not fused_topk(w, B, k, o) \
            and w.n >= SAMPLED_MIN_N:
        out.add(("block-max top-k", "on") if o["TOPK_BMAX"] else ("block-max top-k", "off: sampled filter"))
    if ep in ("search_f32", "search_f32_split"):
        on = dict(o, FOLD_KEYS=1, P1_COLLECT_FUSED=1, BAND_BLOCK_SKIP=1)
        if bmax_eligible(w, B, k, o) and B <= 4 and o["DENSE_DOCS"] and w.kind != "mxfp8":
            out.add(("folded keys", "on" if o["FOLD_KEYS"] else "off"))
        # phase1_collect_kernel: cbv2_search_f32 alone (begin passes fk, finish no lbu), the two-pass band
        p1 = ep == "search_f32" and bool(o["BAND_LOWER_BOUND"])
        if p1 and phase1_collect_fused(w, B, k, on) and o["BAND_BLOCK_SKIP"]:
            out.add(("fused phase-1 collect", "on" if o["P1_COLLECT_FUSED"] else "off"))
        launched = p1 and phase1_collect_fused(w, B, k, o)
        if bmax_eligible(w, B, k, o) and not launched and not (B <= BAND_PAIR_MAX_B and o["BAND_FUSED"]):
            out.add(("band block skip", "on" if o["BAND_BLOCK_SKIP"] else "off"))
        if ep == "search_f32" and B <= BAND_PAIR_MAX_B and all(o[nm] == v[0] for nm, _, v in OPTIONS):
            out.add(("default option vector, B <= 8", "on"))
    if ep in ("score", "search", "search_f32", "search_f32_split") and B >= 33:
        out.add(("dynamic tail (B >= 33)", str(o["DYNAMIC_TAIL"])))
    if ep == "topk_rows" and step["sampled"] and w.n >= SAMPLED_MIN_N and k <= TOPK_MAX:
        out.add(("sampled filter on signed zeros", "on" if step["zeros"] else "plain"))
    return out


# ---------------------------------------------------------------------------- keys
f2u, u2f = grp.f2u, grp.u2f
NAN_BITS = np.float32(np.nan).view(np.uint32)
POISON_I = -7


def topk_keys(S, k, id_base=0):
    """Row top-k by (key desc, index asc) -> (scores f32 [B, k], positions int64
    [B, k] (-1 padded), ids int32 [B, k]).  oracle.topk ranks the keys (as
    float64: a uint32 is exact there), so its tie rule is the one applied; long
    rows take a partition on the same composite key first."""
    S = np.ascontiguousarray(np.atleast_2d(S), np.float32)
    B, N = S.shape
    keys = f2u(S)
    if N > 8192 and k < N // 4:                          # the large walks: cut each row to the keys that can win
        comp = (keys.astype(np.uint64) << np.uint64(32)) | (~np.arange(N, dtype=np.uint32)).astype(np.uint64)
        pos = np.full((B, k), -1, np.int64)
        part = np.argpartition(comp, N - k, axis=1)[:, N - k:]
        for b in range(B):
            cols = np.sort(part[b])
            _, p = orc.topk(keys[b, cols].astype(np.float64)[None], k)
            pos[b] = cols[p[0]]
    else:
        _, pos = orc.topk(keys.astype(np.float64), k)
    out_s = np.full((B, k), -np.inf, np.float32)
    ok = pos >= 0
    out_s[ok] = np.take_along_axis(S, np.maximum(pos, 0), axis=1)[ok]
    ids = np.where(ok, pos + id_base, -1).astype(np.int32)
    return out_s, pos, ids


def select_rows(raw, ids, k):
    """cbv2_select_topk / the rerank's select: (key desc, position asc) ->
    (scores [B, k], ids [B, k], positions [B, k]), -inf / -1 / -1 past C."""
    s, pos, _ = topk_keys(raw, k)
    ok = pos >= 0
    src = np.broadcast_to(np.arange(raw.shape[1], dtype=np.int32), raw.shape) if ids is None else ids
    out_i = np.where(ok, np.take_along_axis(src, np.maximum(pos, 0), axis=1), -1).astype(np.int32)
    return s, out_i, pos.astype(np.int32)


# ---------------------------------------------------------------------------- pools
class Pool:
    """What the model needs of a pool: ref float32 [B, 32, N] (-inf for an
    empty doc) and the sizes."""

    def __init__(self, kind, ld, ref):
        self.kind, self.ld = kind, ld
        self.ref = np.ascontiguousarray(ref, np.float32)
        self.B, _, self.N = self.ref.shape


_pools = {}


def exact_pool(kind, ld):
    """The real pool (4-5 s each), once per session (tests/_exact.cached_corpus)."""
    if (kind, ld) not in _pools:
        n, b = SIZE[ld]
        c = ex.cached_corpus(kind, ld, n, b, seed=1)
        p = Pool(kind, ld, c.ref)
        p.corpus = c
        _pools[kind, ld] = p
    return _pools[kind, ld]


def synthetic_pool(kind, ld):
    """A stand-in reference with the pools' shape for the CPU tests (built in
    milliseconds): dyadic prefix sums below 64, one empty doc, one tied pair per
    query row.  The model and the CPU backends read nothing else of a pool."""
    n, b = SIZE[ld]
    rng = np.random.default_rng([99, ld, ex.KINDS.index(kind)])
    m = rng.integers(-(1 << 12), 1 << 16, size=(b, LQ_MAX, n)).astype(np.float64) / float(1 << 16)
    ref = np.cumsum(m, axis=1)
    for q in range(b):
        i, j = rng.choice(n, 2, replace=False)
        ref[q, :, j] = ref[q, :, i]
    ref[:, :, int(rng.integers(n))] = -np.inf
    return Pool(kind, ld, ref)


# ---------------------------------------------------------------------------- the walk
class Filter:
    def __init__(self, cls, mask, words):
        self.cls, self.mask, self.words = cls, mask, words


class Walk:
    def __init__(self, kind, ld, seed, large=False):
        self.kind, self.ld, self.seed, self.large = kind, ld, int(seed), bool(large)
        self.N, self.Bp = SIZE[ld]
        self.steps = []

    @property
    def name(self):
        return f"{self.kind}:{self.ld}:{self.seed}" + (":large" if self.large else "") + \
            (f" ({self.tag})" if getattr(self, "tag", None) else "")

    def rng(self, ds):
        return np.random.default_rng([self.seed, self.ld, ex.KINDS.index(self.kind), int(self.large), int(ds)])


def _filter(rng, n, cls):
    m = {"none": 0, "one": 1, "5pct": max(1, int(round(0.05 * n))), "half": n // 2, "over_half": n // 2 + 1,
         "all": n}[cls]
    m = min(m, n)
    mask = np.zeros(n, bool)
    mask[rng.choice(n, m, replace=False)] = True
    nw = (n + 31) // 32
    bits = np.zeros(nw * 32, np.uint64)
    bits[:n] = mask
    bits[n:] = rng.integers(0, 2, nw * 32 - n)                  # garbage past n, which the library ignores
    if nw * 32 > n:
        bits[n] = 1
    words = (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return Filter(cls, mask, words)


def _draw_k(rng, n):
    if n > BAND_CAP:                     # the large walks: the k around n would make every output a score matrix
        return int(rng.choice([1, 2, 10, 100, 1024, 1025, 1100]))
    return max(1, int(rng.choice([1, 2, 10, 100, n - 1, n, n + 1, 1024, 1025, 1100])))


def _draw_cap(rng, k):
    return int(rng.choice([c for c in (k, k + 1, 64, BAND_CAP) if k <= c <= BAND_CAP]))


def _draw_args(w, rng, ep, in_split=False):
    """The arguments of one call of ``ep``, every one from its edge list."""
    n = w.n
    a = {"ep": ep, "ds": int(rng.integers(1, 1 << 30))}
    if ep in ("topk_rows", "select_topk", "merge_topk", "group_topk_rows"):
        a.update(B=int(rng.choice(w.bs)), lq=int(rng.choice(LQS)), q0=int(rng.integers(w.Bp)),
                 zeros=int(rng.random() < 0.75))
        if ep == "topk_rows":
            a.update(k=_draw_k(rng, n), pad=int(rng.choice([0, 3])), sampled=int(rng.integers(2)))
        elif ep == "select_topk":
            C = int(rng.choice(CS))
            a.update(C=C, k=max(1, int(rng.choice([1, 10, C - 1, C, C + 1, 1100]))), ids=int(rng.integers(2)))
        elif ep == "merge_topk":
            a.update(G=int(rng.choice([1, 2, 3, 8])), k=_draw_k(rng, n))
        else:
            a.update(g=int(rng.integers(len(w.groupings))), k=_draw_k(rng, n), r=int(rng.integers(1, 9)))
        return a
    if ep == "search_filtered_batch":
        j = int(rng.integers(len(w.batches)))
        a.update(fb=j, B=len(w.batches[j]), lq=int(rng.choice(LQS)))
    elif w.prev is not None and rng.random() < 0.25:
        a.update(B=w.prev[0], lq=w.prev[1])                    # the previous call's B and lq, other contents at the address
    else:
        if not w.bdeck:                  # the next 8 batch sizes of the seed's rotation, in random order
            w.bdeck, w.bs = [w.bs[i] for i in rng.permutation(min(8, len(w.bs)))], w.bs[8:] + w.bs[:8]
        a.update(B=int(w.bdeck.pop()), lq=int(rng.choice(LQS)))
    w.prev = (a["B"], a["lq"])
    a.update(q0=int(rng.integers(w.Bp)))
    if ep == "score":
        return a
    if ep in ("rerank", "rerank_ws", "rerank_f32"):
        C = int(rng.choice(CS))
        a.update(C=C, k=max(0, int(rng.choice([0, 1, 10, 100, C - 1, C, C + 1]))))
        return a
    if ep == "retrieve":
        C = int(rng.choice([1, 20, 50]))
        a.update(k=int(rng.choice([1, 10, 100])), kb=int(rng.choice([0, 10])), C=C,
                 final_k=int(rng.choice([1, 7, 10, C, C + 10])), how=str(rng.choice(["finish", "finish_host", "cancel"],
                                                                                    p=[0.4, 0.4, 0.2])))
        return a
    a.update(k=_draw_k(rng, n))
    if ep in ("search_filtered", "search_filtered_f32"):
        a.update(f=int(rng.integers(len(w.filters))))
    if ep in ("search_grouped", "search_grouped_f32"):
        a.update(g=int(rng.integers(len(w.groupings))), r=int(rng.integers(1, 9)))
    if ep in FAITHFUL_EPS:
        a.update(cap=_draw_cap(rng, a["k"]))
    if ep == "search_f32_split" and not in_split:
        # one unrelated call on ANOTHER workspace between begin and finish; it
        # overwrites the walk's query buffer, which finish does not read
        a["between"] = _draw_args(w, rng, str(rng.choice(["score", "search_f32", "rerank_f32"])), in_split=True)
    return a


def _draw_invalid(w, rng):
    """A call whose rejection the header documents and that would stay inside
    its buffers even if it were launched: the valid arguments of its entry
    point with one of them out of range."""
    faithful = w.kind == "fp32"
    what = str(rng.choice(INVALID_KINDS + (INVALID_FAITHFUL if faithful else ())))
    search = "search_f32" if faithful else "search"
    on = {"r0": "search_grouped", "r9": "search_grouped", "lq0": "score", "lq33": "score",
          "batch_B": "search_filtered_batch"}.get(what, search)
    prev = w.prev
    a = _draw_args(w, rng, on)
    w.prev = prev                                              # a rejected call leaves no queries behind
    a = {"ep": "invalid", "what": what, "on": on, **{k: v for k, v in a.items() if k != "ep"}}
    a.update(ws_delta=0, ws_offset=0, null_status=0)
    if what == "k0":
        a["k"] = 0
    elif what in ("r0", "r9"):
        a["r"] = 0 if what == "r0" else 9
    elif what in ("lq0", "lq33"):
        a["lq"] = 0 if what == "lq0" else 33                   # the query buffer holds 33 tokens per query
    elif what == "cap_lo":
        a["k"] = max(a["k"], 2)
        a["cap"] = a["k"] - 1
    elif what == "cap_hi":
        a["cap"] = BAND_CAP + 1
    elif what == "ws_short":
        a["ws_delta"] = -1                                     # workspace_bytes one short, the buffer itself full size
    elif what == "ws_misaligned":
        a["ws_offset"] = 8                                     # 8 bytes into a buffer with slack
    elif what == "null_status":
        a["null_status"] = 1
    elif what == "batch_B":
        a["B"] = a["B"] + 1                                    # a filter batch of another B
    return a


# The large walks' themes, seed by seed: (options switched away from the
# defaults, the range the walk's batch sizes are taken from, the probability
# with which every other option moves).  Each large-size path is launched and
# left out with everything else it needs in place -- the two sides of an A/B --
# and two themes stay under the default vector (production) throughout.
THEMES = (({}, (1, 8), 0.0), ({}, (33, 65), 0.0), ({"TOPK_BMAX": 0}, (1, 65), 0.1),
          ({"DYNAMIC_TAIL": 0}, (33, 65), 0.1), ({"DYNAMIC_TAIL": 2}, (33, 65), 0.1),
          ({"P1_COLLECT_FUSED": 0}, (1, 8), 0.0), ({"DENSE_DOCS": 1}, (1, 4), 0.0),
          ({"DENSE_DOCS": 1, "FOLD_KEYS": 0}, (1, 4), 0.0), ({"BAND_BLOCK_SKIP": 0}, (1, 65), 0.1),
          ({"FUSED_TOPK": 1}, (1, 65), 0.1), ({"BAND_FUSED": 1}, (1, 65), 0.1), ({"RESCORE_SPLIT": 0}, (1, 65), 0.1),
          ({"BAND_LOWER_BOUND": 0}, (1, 65), 0.1), ({"BAND_DOC_MAJOR": 3}, (1, 65), 0.1))


def _draw_options(rng, theme=None):
    """A legal vector over all 17 options.  The dispatch reads the options in
    conjunction (phase1_collect_fused needs nine of them in one position), and
    a uniform vector almost never satisfies such a conjunction; so half of a
    small walk's vectors are uniform over every option's values and the other
    half start from the defaults and move each option with probability 0.15.
    A large walk's vectors are the defaults with its theme's switches set and
    every other option moved with the theme's probability."""
    if theme is not None:
        sw, _, p = theme
        return [int(sw[nm]) if nm in sw else (int(rng.choice(v)) if rng.random() < p else int(v[0]))
                for nm, _, v in OPTIONS]
    if rng.random() < 0.5:
        return [int(rng.choice(v)) for _, _, v in OPTIONS]
    return [int(rng.choice(v)) if rng.random() < 0.15 else int(v[0]) for _, _, v in OPTIONS]


def generate(kind, ld, seed, large=False, n=None):
    """The walk (kind, ld, seed): needs no pool, only its sizes.  ``n`` (the
    scripted big-batch walks of tests/_bigbatch.py) replaces the drawn corpus
    size and leaves every draw before it as it is."""
    w = Walk(kind, ld, seed, large)
    rng = w.rng(0)
    N = w.N
    if large:
        w.n = int(rng.choice(LARGE_N))
    elif seed % 2 == 0:                 # every other seed an edge, stratified so that few seeds visit them all
        edges = [x for x in N_EDGES if x <= N] + [N]
        w.n = edges[(seed // 2 + 7 * (3 * LDS.index(ld) + ex.KINDS.index(kind))) % len(edges)]
    else:
        w.n = int(rng.integers(1, N + 1))
    if n is not None:
        w.n = int(n)
    n = w.n
    w.id_base = int(rng.choice([0, 3, 123456, 2 ** 31 - 2 - n]))
    w.sel = rng.integers(0, N, n)
    w.filters = [_filter(rng, n, cls) for cls in FILTER_CLASSES]
    bs = score_batches(kind, ld, large)
    theme = THEMES[seed % len(THEMES)] if large else None
    if large:
        bs = [b for b in bs if theme[1][0] <= b <= theme[1][1]]
    w.bs = bs[(7 * seed) % len(bs):] + bs[: (7 * seed) % len(bs)]     # consecutive seeds start the B deck 7 further on
    w.bdeck, w.prev = [], None
    w.batches = []
    for _ in range(2):
        B = int(rng.choice(bs))
        row = [None if x == len(w.filters) else int(x) for x in rng.integers(0, len(w.filters) + 1, B)]
        for pos, val in zip(rng.permutation(B)[:4], (None, 0, 3, 3)):   # a None, the empty filter, a repeated handle
            row[int(pos)] = val
        w.batches.append(row)
    gs = grp.groupings(n, seed)
    names = sorted(gs)
    w.groupings = [(nm,) + tuple(gs[nm]) for nm in (names[i] for i in rng.choice(len(names), 2, replace=False))]
    nsteps = int(rng.integers(8, 13))
    opts = _draw_options(rng, theme)
    w.steps.append({"ep": "set_options", "values": tuple(opts), "opts": tuple(opts)})
    deck = []
    eps = entry_points(kind, large)
    eps = eps[(5 * seed) % len(eps):] + eps[: (5 * seed) % len(eps)]   # consecutive seeds start the deck 5 further on
    if large:                            # the calls a theme is about come in every large walk's first eight
        first = tuple(e for e in ("search_f32", "search", "score", "topk_rows") if e in eps)
        eps = first + tuple(e for e in eps if e not in first)
    while len(w.steps) < nsteps:
        u = rng.random()
        if u < 0.085 and not large:
            st = _draw_invalid(w, rng)
        elif u < 0.23:
            opts = _draw_options(rng, theme)
            st = {"ep": "set_options", "values": tuple(opts)}
        else:
            if not deck:                 # the next 8 entry points of the rotation, in random order
                deck, eps = [eps[i] for i in rng.permutation(min(8, len(eps)))], eps[8:] + eps[:8]
            st = _draw_args(w, rng, deck.pop())
        st["opts"] = tuple(opts)
        w.steps.append(st)
    return w


def scripted(kind, ld, seed, steps, tag, large=False, n=None):
    """The corpus and handles of walk (kind, ld, seed) under a written-out list
    of steps (a named regression): the first must be a set_options."""
    w = generate(kind, ld, seed, large, n)
    w.tag, w.steps, opts = tag, [], None
    for st in steps:
        opts = st["values"] if st["ep"] == "set_options" else opts
        w.steps.append(dict(st, opts=tuple(opts)))
    return w


# ---------------------------------------------------------------------------- transcript
def _opts_text(o):
    return ",".join(str(v) for v in o)


def render(i, step):
    parts = [f"{i:02d} {step['ep']}"]
    for key, val in step.items():
        if key in ("ep", "opts"):
            continue
        if key == "between":
            parts.append("between=[" + render(i, val)[3:] + "]")
        elif key == "values":
            parts.append("values=" + _opts_text(val))
        else:
            parts.append(f"{key}={val}")
    if "opts" in step:
        parts.append("| opts=" + _opts_text(step["opts"]))
    return " ".join(parts)


def header(w):
    fb = ";".join(",".join("N" if x is None else str(x) for x in row[:70]) + (f",... x{len(row)}" if len(row) > 70 else "")
                  for row in w.batches)
    return (f"walk {w.name}: n={w.n} id_base={w.id_base} sel#{hashlib.sha256(w.sel.tobytes()).hexdigest()[:8]} "
            f"filters={[int(f.mask.sum()) for f in w.filters]} batches=[{fb}] "
            f"groupings={[(g[0], g[2]) for g in w.groupings]} options=({','.join(OPT_NAMES)})")


def transcript(w, upto=None):
    steps = w.steps if upto is None else w.steps[: upto + 1]
    return "\n".join([header(w)] + [render(i, s) for i, s in enumerate(steps)])


def transcripts_hash(walks):
    return hashlib.sha256("\n".join(transcript(w) for w in walks).encode()).hexdigest()


# ---------------------------------------------------------------------------- inputs of a step
def one_period(w, step):
    """A big-batch step (tests/_bigbatch.py marks it ``tile``) with more queries
    than the pool has: its queries repeat with the pool's query count P, its
    drawn inputs are those of the first P rows repeated, its filter batch
    cycles with a period that divides P -- so row b of every input and of every
    expected output is row b mod P.  -> the step of the first P rows, or None."""
    if step.get("tile") and step.get("B", 0) > w.Bp and step["ep"] not in ("set_options", "invalid"):
        return {key: val for key, val in dict(step, B=w.Bp).items() if key != "tile"}
    return None


def tile_rows(a, B, axis=0):
    """Rows 0 .. P-1 along ``axis`` repeated to B rows: row b is row b mod P."""
    return np.take(a, np.arange(B) % a.shape[axis], axis=axis)


def query_rows(w, step):
    """The pool queries a step's query buffer holds: q0, q0 + 1, ... (mod the pool's B)."""
    return (step["q0"] + np.arange(step["B"])) % w.Bp


def ref_rows(w, pool, step):
    """float32 [B, n]: the exact scores of the step's queries against the walk's docs."""
    lq = step["lq"]
    return np.ascontiguousarray(pool.ref[query_rows(w, step), lq - 1][:, w.sel])


def candidates(w, step):
    """int32 [B, C] global ids: docs of the shard with repeats, -1, negative ids
    and ids just outside the shard on either side."""
    sub = one_period(w, step)
    if sub is not None:
        return tile_rows(candidates(w, sub), step["B"])
    rng = w.rng(step["ds"])
    B, C, n, base = step["B"], step["C"], w.n, w.id_base
    cand = (rng.integers(0, n, (B, C)) + base).astype(np.int64)
    outside = [-1, -(n + 3)]
    if base > 0:
        outside.append(base - 1)
    if base + n + 7 < 2 ** 31:
        outside += [base + n, base + n + 7]
    hit = rng.random((B, C)) < 0.15
    cand[hit] = rng.choice(outside, int(hit.sum()))
    if C > 4:
        cand[:, 1] = cand[:, 2]                                 # a repeat: tie -> lower position
    return cand.astype(np.int32)


def selection_matrix(w, pool, step, cols, k):
    """The score matrix of a selection step: columns ``cols`` of the step's
    reference rows and, with ``zeros``, shifted by each row's k-th largest
    value so that the k-th place holds zeros, half of them turned to -0.0 and
    the value ranked next set to a zero too: +0.0 and -0.0 lie beside each
    other where the selection cuts."""
    M = ref_rows(w, pool, step)[:, cols].copy()
    if not step["zeros"]:
        return M
    rng = w.rng(step["ds"] + 1)
    for b in range(M.shape[0]):
        fin = np.isfinite(M[b])
        if not fin.any():
            continue
        order = np.sort(M[b][fin])[::-1]
        kk = min(k, len(order))
        M[b][fin] = M[b][fin] - order[kk - 1]                   # x - x = +0.0 for the k-th value and its ties
        if kk < len(order):
            M[b][M[b] == order[kk] - order[kk - 1]] = 0.0       # the next value down joins them
        z = np.flatnonzero(M[b] == 0)
        M[b][z[rng.random(len(z)) < 0.5]] = -0.0
    return M


def select_inputs(w, pool, step):
    """cbv2_select_topk: (scores [B, C], ids [B, C] or None)."""
    sub = one_period(w, step)
    if sub is not None:
        M, ids = select_inputs(w, pool, sub)
        return tile_rows(M, step["B"]), None if ids is None else tile_rows(ids, step["B"])
    cols = w.rng(step["ds"]).integers(0, w.n, step["C"])
    M = selection_matrix(w, pool, step, cols, step["k"])
    ids = np.broadcast_to((cols + w.id_base).astype(np.int32), M.shape).copy() if step["ids"] else None
    return M, ids


def topk_inputs(w, pool, step):
    """cbv2_topk_rows / cbv2_group_topk_rows: scores [B, n + pad], the padding
    columns larger than any score (a read past n would win)."""
    sub = one_period(w, step)
    if sub is not None:
        return tile_rows(topk_inputs(w, pool, sub), step["B"])
    M = selection_matrix(w, pool, step, np.arange(w.n), step["k"])
    pad = step.get("pad", 0)
    return np.concatenate([M, np.full((M.shape[0], pad), 1e30, np.float32)], axis=1) if pad else M


def merge_inputs(w, pool, step):
    """cbv2_merge_topk: G shards of contiguous doc ranges, each one's sorted
    top-k list (-inf / -1 padded): scores [G, B, k], global ids [G, B, k]."""
    sub = one_period(w, step)
    if sub is not None:
        M, in_s, in_i = merge_inputs(w, pool, sub)
        return tile_rows(M, step["B"]), tile_rows(in_s, step["B"], 1), tile_rows(in_i, step["B"], 1)
    M = selection_matrix(w, pool, step, np.arange(w.n), step["k"])
    G, k = step["G"], step["k"]
    cuts = np.linspace(0, w.n, G + 1).astype(np.int64)
    in_s = np.full((G, M.shape[0], k), -np.inf, np.float32)
    in_i = np.full((G, M.shape[0], k), -1, np.int32)
    for g in range(G):
        if cuts[g + 1] > cuts[g]:
            in_s[g], _, in_i[g] = topk_keys(M[:, cuts[g]:cuts[g + 1]], k, w.id_base + int(cuts[g]))
    return M, in_s, in_i


def lexical_ids(w, step):
    """The stage-1 lists of a retrieve: int32 [B, kb] global ids, rows with a -1
    tail, ids outside the shard and repeats."""
    sub = one_period(w, step)
    if sub is not None:
        return tile_rows(lexical_ids(w, sub), step["B"])
    rng = w.rng(step["ds"] + 2)
    B, kb = step["B"], step["kb"]
    lex = (rng.integers(0, w.n, (B, kb)) + w.id_base).astype(np.int64)
    if w.id_base + w.n + 7 < 2 ** 31:
        lex[rng.random((B, kb)) < 0.1] = w.id_base + w.n + 7
    for b in range(B):
        cut = int(rng.integers(0, kb + 1))
        if b % 3 == 1:
            lex[b, cut:] = -1
    return lex.astype(np.int32)


# ---------------------------------------------------------------------------- the model
def status_range(S, k, cap):
    """A faithful call's status: -1, or the band size in [min(k, scoring docs), cap]."""
    return ("status", np.minimum(k, np.isfinite(S).sum(axis=1)).astype(np.int64), int(cap))


def rerank_expect(S, cand, k, w):
    local = cand.astype(np.int64) - w.id_base
    inside = (cand >= 0) & (local >= 0) & (local < w.n)
    raw = np.where(inside, np.take_along_axis(S, np.clip(local, 0, w.n - 1), axis=1), -np.inf).astype(np.float32)
    if k == 0:
        return {"scores": raw}
    B, C = cand.shape
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int32)
    out_p = np.full((B, k), -1, np.int32)
    for b in range(B):
        for j, (p, _, _) in enumerate(orc.rerank_select(raw[b], k)):
            out_s[b, j], out_i[b, j], out_p[b, j] = raw[b, p], cand[b, p], p
    return {"scores": out_s, "ids": out_i, "pos": out_p}


def filtered_expect(S, allowed_rows, k, w):
    """allowed_rows: per row the ascending local ids of its filter."""
    B = S.shape[0]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_i = np.full((B, k), -1, np.int32)
    for b, allowed in enumerate(allowed_rows):
        if len(allowed):
            s, pos, _ = topk_keys(S[b, allowed][None], k)
            out_s[b] = s[0]
            out_i[b] = np.where(pos[0] >= 0, allowed[np.maximum(pos[0], 0)] + w.id_base, -1)
    return out_s, out_i


def grouped_expect(S, w, step):
    _, gof, G = w.groupings[step["g"]]
    s, g, i, c = grp.oracle(S, gof, G, step["k"], step["r"], w.id_base)
    return {"scores": s, "groups": g, "ids": i, "chunk_scores": c}


def expected(w, pool, step, tiled=True):
    """name -> the array the call must write, bit for bit; "rc" the return code;
    ("status", lo [B], cap) for a faithful call's status word.  A big-batch
    step (one_period) is answered for one period of its rows and repeated;
    ``tiled`` = False answers it row by row from the same inputs
    (tests/test_bigbatch_model.py pins the two against each other)."""
    ep = step["ep"]
    sub = one_period(w, step) if tiled else None
    if sub is not None:
        B, out = step["B"], {}
        for name, x in expected(w, pool, sub).items():
            if name in ("rc", "between"):                      # the call between has its own B (and its own period)
                out[name] = x
            elif isinstance(x, tuple):
                out[name] = (x[0], tile_rows(x[1], B), x[2])
            else:
                out[name] = tile_rows(x, B)
        return out
    if ep == "set_options":
        return {"rc": 0}
    if ep == "invalid":
        return {"rc": EINVAL, "untouched": True}
    out = {"rc": 0}
    k = step.get("k")
    if ep in ("select_topk", "topk_rows", "merge_topk", "group_topk_rows"):
        if ep == "select_topk":
            M, ids = select_inputs(w, pool, step)
            out["scores"], out["ids"], out["pos"] = select_rows(M, ids, k)
        elif ep == "topk_rows":
            M = topk_inputs(w, pool, step)[:, : w.n]
            out["scores"], _, out["ids"] = topk_keys(M, k, w.id_base)
        elif ep == "merge_topk":
            M, _, _ = merge_inputs(w, pool, step)              # ids are unique across shards: the row's own top-k
            out["scores"], _, out["ids"] = topk_keys(M, k, w.id_base)
        else:
            out.update(grouped_expect(topk_inputs(w, pool, step)[:, : w.n], w, step))
        return out
    S = ref_rows(w, pool, step)
    if ep == "score":
        out["scores"] = S
    elif ep in ("search", "search_f32", "search_f32_split"):
        out["scores"], _, out["ids"] = topk_keys(S, k, w.id_base)
        if ep != "search":
            out["status"] = status_range(S, k, step["cap"])
        if "between" in step:
            out["between"] = expected(w, pool, step["between"], tiled)
    elif ep in ("rerank", "rerank_ws", "rerank_f32"):
        out.update(rerank_expect(S, candidates(w, step), k, w))
    elif ep in ("search_filtered", "search_filtered_f32"):
        allowed = np.flatnonzero(w.filters[step["f"]].mask)
        out["scores"], out["ids"] = filtered_expect(S, [allowed] * S.shape[0], k, w)
        if ep == "search_filtered_f32":
            if len(allowed):
                out["status"] = status_range(S[:, allowed], k, step["cap"])
            else:
                out["status"] = np.zeros(S.shape[0], np.int32)
    elif ep == "search_filtered_batch":
        rows = [np.arange(w.n) if f is None else np.flatnonzero(w.filters[f].mask)
                for f in w.batches[step["fb"]][: S.shape[0]]]
        out["scores"], out["ids"] = filtered_expect(S, rows, k, w)
    elif ep in ("search_grouped", "search_grouped_f32"):
        out.update(grouped_expect(S, w, step))
        if ep == "search_grouped_f32":
            gof = w.groupings[step["g"]][1]
            if (gof >= 0).any():                               # the k leaders (of k distinct groups) are in the band
                lo = [min(k, len(np.unique(gof[(gof >= 0) & np.isfinite(S[b])]))) for b in range(S.shape[0])]
                out["status"] = ("status", np.asarray(lo, np.int64), int(step["cap"]))
            else:
                out["status"] = np.zeros(S.shape[0], np.int32)
    elif ep == "retrieve":
        if step["how"] == "cancel":                            # begin + cancel, then a plain search of the same queries
            out["scores"], _, out["ids"] = topk_keys(S, k, w.id_base)
            return out
        _, _, ids = topk_keys(S, k, w.id_base)
        lex = lexical_ids(w, step) if step["kb"] else np.zeros((S.shape[0], 0), np.int32)
        C = step["C"]
        cand = np.full((S.shape[0], C), -1, np.int32)
        for b in range(S.shape[0]):
            fused = [cid for cid, _ in orc.rrf([int(x) for x in lex[b] if x >= 0], [int(x) for x in ids[b] if x >= 0],
                                               k=RRF_K)[:C]]
            cand[b, : len(fused)] = fused
        out.update(rerank_expect(S, cand, step["final_k"], w))
        if step["how"] == "finish_host":                       # the same three arrays on the host at return
            out.update({"host_" + name: out[name] for name in ("scores", "ids", "pos")})
    else:
        raise ValueError(ep)
    return out


# ---------------------------------------------------------------------------- the player
class WalkFailure(AssertionError):
    def __init__(self, walk, index, message):
        self.walk, self.index = walk, index
        super().__init__(f"walk {walk.name} fails at step {index}: {message}\n{transcript(walk, index)}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.int64)


def first_difference(name, got, want):
    """None, or words on the first differing (row, slot) with both bit patterns."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, want {want.shape}"
    g, x = _bits(got), _bits(want)
    bad = np.argwhere(g != x)
    if not len(bad):
        return None
    at = tuple(int(v) for v in bad[0])
    row, slot = at[0], at[1:] if len(at) > 2 else (at[1] if len(at) > 1 else 0)
    if got.dtype == np.float32:
        return (f"{name}: {len(bad)} of {g.size} differ; first at (row {row}, slot {slot}): got 0x{int(g[at]):08x} "
                f"({float(got[at])!r}), want 0x{int(x[at]):08x} ({float(want[at])!r})")
    return f"{name}: {len(bad)} of {g.size} differ; first at (row {row}, slot {slot}): got {int(g[at])}, want {int(x[at])}"


def compare(backend, got, want):
    """None, or the first difference between a backend's answer and the model's."""
    if got.get("rc") != want["rc"]:
        return f"return code {got.get('rc')}, want {want['rc']}"
    if want.get("untouched"):
        for name, arr in got.items():
            if name != "rc" and not backend.untouched(arr):
                return f"{name}: a rejected call wrote into its poisoned output"
        return None
    for name, x in want.items():
        if name == "rc":
            continue
        if name == "between":
            msg = compare(backend, got["between"], x)
            if msg:
                return "the call between begin and finish: " + msg
            continue
        if name not in got:
            return f"{name}: not returned"
        if isinstance(x, tuple):                                # ("status", lo, cap)
            st = np.asarray(backend.host(got[name])).astype(np.int64)
            bad = np.flatnonzero(~((st == -1) | ((st >= x[1]) & (st <= x[2]))))
            if len(bad):
                b = int(bad[0])
                return f"{name}: row {b} holds {int(st[b])}, want -1 or a band size in [{int(x[1][b])}, {x[2]}]"
            continue
        if backend.same(got[name], x):
            continue
        msg = first_difference(name, backend.host(got[name]), x)
        if msg:
            return msg
    return None


def play(w, pool, backend):
    """Every step of the walk through ``backend``, compared with the model after
    each; raises WalkFailure naming the step, with the transcript up to it."""
    backend.start(w, pool)
    failure = None
    for i, step in enumerate(w.steps):
        want = expected(w, pool, step)
        got = backend.call(i, step)                             # an exception here (a fault) leaves at once: the
        msg = compare(backend, got, want)                       # backend is not touched again, nothing masks it
        if msg:
            more = backend.diagnose(i, step, want) if hasattr(backend, "diagnose") else ""
            failure = WalkFailure(w, i, msg + (f" [{more}]" if more else ""))
            break
    backend.finish()
    if failure is not None:
        raise failure
