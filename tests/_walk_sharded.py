"""Seeded SHARDED walks over the C ABI on exact corpora (test infrastructure,
beside tests/_walk.py and reusing it): one corpus as _walk.py draws it (pool,
sel, n, id_base) cut into G contiguous shards, one rank per shard, and 6-8
steps of the sharded calls (cbv2_search_sharded / _local / _exchange,
cbv2_rerank_sharded, cbv2_rerank_sharded_prescored, cbv2_retrieve_* with a
comm) after the step that sets every rank's option vector.

numpy only.  tests/test_walk_sharded_model.py plays the walks through a
brute-force backend that really shards (and its mutants),
tests/test_gpu_walk_sharded.py through the C ABI on loopback communicators.

The MODEL knows nothing about shards: what every rank must return is the
answer of the whole corpus (_walk.topk_keys, oracle.rerank_select, oracle.rrf),
and the merged stage-1 list is the top-kb of the row's global list.  The cuts
enter only the INPUTS: which stage-1 entries a rank is handed, and which
in-corpus ids no rank lists (the prescored step's strays).

  G         GS[t % 4], t = 13 * seed + the (kind, ld) case: every case meets
            every G, every seed all four three times.
  cuts      the classes of CUT_CLASSES legal for (G, n), taken in rotation by
            t // 4.  For n < G some shards are necessarily empty.  ``empty_docs``
            gives shard 1 one to three docs that are all the pool's empty doc
            (bind): a shard that is not empty and scores -inf throughout.
  n         as _walk.generate: an even seed the next edge of _walk.N_EDGES (and
            the whole pool), an odd one uniform in [1, N].
  options   every rank draws its OWN legal vector (_walk._draw_options) at step
            0 and at each set_options step: the ranks differ on purpose, every
            option promises identical results.
  stage 1   per row a global list of distinct in-range ids with scores >= +0.0
            from a few values (mass ties across shards, a zero-score tail); a
            rank is handed the ids it owns, sorted (score desc, id asc), cut to
            kb, padded -1 / -inf: the header's "this rank's top-kb over its doc
            shard".
  comm      the model also states each step's cbv2_comm_stats delta:
            {all-gathers, all-reduces}.
An invalid step issues the SAME bad call on every rank (rejected before any
collective, so no rank waits); a call invalid on one rank only is never issued.
Every step renders as one line; data derive from the walk's seed and the
step's ``ds``, so a transcript replays the walk.
"""
from __future__ import annotations

import hashlib

import numpy as np

import _exact as ex
import _walk as wk
from oracle import oracle as orc

GS = (1, 2, 3, 8)
ID_BASES = (0, 1000, None)                       # None: 2^31 - 1 - n, the last ids an int32 holds
CUT_CLASSES = ("even", "first_empty", "last_empty", "middle_empty", "one_doc", "one_owner", "small_first", "random",
               "empty_docs")
KBS = (0, 1, 10, 100, 1025)
STEP_EPS = ("search_sharded", "search_split", "rerank_sharded", "prescored", "retrieve_sharded")
INVALID_KINDS = ("k0", "B0", "lq33", "kb_neg", "ws_short", "pre_C1025", "pre_fk0")
LEX_VALUES = (0.0, 0.0, 0.5, 1.0, 1.0, 2.5)       # few values: ties across shards; zeros: the tail
MERGE_MAX = 8192                                 # kMergeMax: G * k above it takes the in-place merge
CASES = [(kind, ld) for kind in ex.KINDS for ld in wk.LDS]
# The committed sharded walks: seeds 0 .. SEEDS - 1 of every (kind, ld), the
# smallest count at which every cell of the coverage table of
# tests/test_walk_sharded_model.py is visited at least 3 times.
SEEDS = 20
TRANSCRIPTS_SHA256 = "2be9448cfe6f0e61ec297f41d6c47003448e60b8ab63155abe37bc4bdbfe2099"


def committed(seeds=None):
    return [(kind, ld, seed) for kind, ld in CASES for seed in range(SEEDS if seeds is None else seeds)]


def legal_cuts(G, n):
    if G == 1:
        return ("even",)
    out = ["even", "first_empty", "last_empty", "one_doc", "one_owner", "small_first", "random", "empty_docs"]
    if G >= 3:
        out.insert(3, "middle_empty")
    return tuple(out)


def make_cuts(cls, G, n, rng):
    """int64 [G + 1]: shard r holds docs [cuts[r], cuts[r + 1])."""
    even = lambda a, b, parts: [a + (b - a) * j // parts for j in range(parts + 1)]      # noqa: E731
    if G == 1 or cls == "even":
        c = even(0, n, G)
    elif cls == "first_empty":
        c = [0] + even(0, n, G - 1)
    elif cls == "last_empty":
        c = even(0, n, G - 1) + [n]
    elif cls == "middle_empty":
        m = G // 2
        left = even(0, n // 2, m)
        c = left + even(n // 2, n, G - 1 - m)
    elif cls == "one_doc":                          # shard 1 holds exactly one doc
        at = int(rng.integers(0, n))
        c = [0, at, at + 1] + even(at + 1, n, G - 2)[1:] if G > 2 else [0, n - 1, n]
    elif cls == "empty_docs":                       # shard 1: 1-3 docs, every one the pool's empty doc (bind)
        m = min(n, int(rng.integers(1, 4)))
        at = int(rng.integers(0, n - m + 1))
        c = [0, at, at + m] + even(at + m, n, G - 2)[1:] if G > 2 else [0, n - m, n]
    elif cls == "one_owner":
        own = int(rng.integers(0, G))
        c = [0] * (own + 1) + [n] * (G - own)
    elif cls == "small_first":                      # fewer docs than most k of the edge list
        first = max(1, min(5, n // 2)) if n > 1 else 1
        c = [0] + even(first, n, G - 1)
    else:
        c = [0] + sorted(int(x) for x in rng.integers(0, n + 1, G - 1)) + [n]
    c = np.asarray(c, np.int64)
    assert len(c) == G + 1 and c[0] == 0 and c[-1] == n and (np.diff(c) >= 0).all(), (cls, G, n, c)
    return c


class SWalk(wk.Walk):
    def __init__(self, kind, ld, seed):
        super().__init__(kind, ld, seed)

    @property
    def name(self):
        return f"sharded {self.kind}:{self.ld}:{self.seed}" + (f" ({self.tag})" if getattr(self, "tag", None) else "")

    def rng(self, ds):                               # a stream of its own: _walk's fourth word is 0 / 1
        return np.random.default_rng([self.seed, self.ld, ex.KINDS.index(self.kind), 7, int(ds)])

    def shard(self, r):
        return int(self.cuts[r]), int(self.cuts[r + 1])


def empty_doc(pool):
    """The pool's doc without tokens: it scores -inf for every query."""
    return int(np.flatnonzero(np.isneginf(pool.ref[0, -1]))[0])


def bind(w, pool):
    """An ``empty_docs`` walk's shard 1 holds only copies of the pool's empty doc: a
    NON-empty shard whose local lists are (-inf, valid id) entries, not padding.
    Which pool doc that is, is known only with the pool, so the generator leaves
    those sel entries at 0 and every consumer of a (walk, pool) pair binds them
    first (idempotent)."""
    if w.cut_class == "empty_docs":
        a, e = w.shard(1)
        w.sel[a:e] = empty_doc(pool)
    return w


def _draw_B(w, rng):
    if w.prev is not None and rng.random() < 0.25:
        return w.prev
    if not w.bdeck:
        w.bdeck, w.bs = [w.bs[i] for i in rng.permutation(min(8, len(w.bs)))], w.bs[8:] + w.bs[:8]
    w.prev = (int(w.bdeck.pop()), int(rng.choice(wk.LQS)))
    return w.prev


def _search_args(w, rng, ep):
    B, lq = _draw_B(w, rng)
    a = {"ep": ep, "ds": int(rng.integers(1, 1 << 30)), "B": B, "lq": lq, "q0": int(rng.integers(w.Bp)),
         "k": wk._draw_k(rng, w.n), "kb": int(rng.choice(KBS))}
    if ep != "search_sharded":                      # _local then _exchange
        a.update(kb_local=a["kb"] + int(rng.choice([0, 7])), with_q=int(rng.integers(2)))
    return a


def _rerank_args(w, rng, same_q=None):
    B, lq = same_q if same_q else _draw_B(w, rng)
    C = int(rng.choice(wk.CS))
    return {"ep": "rerank_sharded", "ds": int(rng.integers(1, 1 << 30)), "B": B, "lq": lq, "q0": int(rng.integers(w.Bp)),
            "C": C, "k": max(1, int(rng.choice([1, 10, 100, C - 1, C, C + 1])))}


def _draw_args(w, rng, ep):
    if ep in ("search_sharded", "search_split"):
        return _search_args(w, rng, ep)
    if ep == "rerank_sharded":
        return _rerank_args(w, rng)
    if ep == "prescored":
        a = _search_args(w, rng, str(rng.choice(["search_sharded", "search_split"])))
        a["how"], a["ep"] = a["ep"], "prescored"
        if "with_q" in a:
            a["with_q"] = 1                         # the precondition: an exchange with Q (or kb = 0)
        C = int(rng.choice([1, 50, 1024]))
        a.update(C=C, final_k=int(rng.choice([1, 10, C, C + 3])), strays=int(rng.integers(2)))
        if rng.random() < 0.4:                       # a rerank_sharded on every rank's SECOND workspace first
            a["between"] = _rerank_args(w, rng)
        return a
    B, lq = _draw_B(w, rng)                          # retrieve_sharded
    kb = int(rng.choice(KBS))
    C = int(rng.choice(wk.CS))
    return {"ep": ep, "ds": int(rng.integers(1, 1 << 30)), "B": B, "lq": lq, "q0": int(rng.integers(w.Bp)),
            "k": wk._draw_k(rng, w.n), "kb": kb, "kb_begin": kb + int(rng.choice([0, 7])), "C": C,
            "final_k": int(rng.choice([1, 10, C, C + 3])), "how": str(rng.choice(["finish", "finish_host"]))}


def _draw_invalid(w, rng):
    what = str(rng.choice(INVALID_KINDS))
    prev = w.prev
    a = _search_args(w, rng, "search_sharded")
    w.prev = prev
    a = dict(a, ep="invalid", what=what, on="prescored" if what.startswith("pre_") else "search_sharded",
             ws_delta=0, C=50, final_k=10)
    if what == "k0":
        a["k"] = 0
    elif what == "B0":
        a["B"] = 0
    elif what == "lq33":
        a["lq"] = 33
    elif what == "kb_neg":
        a["kb"] = -1
    elif what == "ws_short":
        a["ws_delta"] = -1
    elif what == "pre_C1025":
        a["C"] = 1025
    else:
        a["final_k"] = 0
    return a


def _draw_all_options(w, rng):
    """One legal vector per rank; with two or more ranks, redrawn until not all are the same."""
    while True:
        vs = tuple(tuple(wk._draw_options(rng)) for _ in range(w.G))
        if w.G == 1 or len(set(vs)) > 1:
            return vs


def generate(kind, ld, seed):
    w = SWalk(kind, ld, seed)
    rng = w.rng(0)
    N = w.N
    t = 13 * seed + CASES.index((kind, ld))
    if seed % 2 == 0:
        edges = [x for x in wk.N_EDGES if x <= N] + [N]
        w.n = edges[(seed // 2 + 7 * CASES.index((kind, ld))) % len(edges)]
    else:
        w.n = int(rng.integers(1, N + 1))
    n = w.n
    base = ID_BASES[(t // 4) % 3]
    w.id_base = 2 ** 31 - 1 - n if base is None else base
    w.sel = rng.integers(0, N, n)
    w.G = GS[t % 4]
    legal = legal_cuts(w.G, n)
    w.cut_class = legal[(t // 4) % len(legal)]
    w.cuts = make_cuts(w.cut_class, w.G, n, rng)
    if w.cut_class == "empty_docs":
        w.sel[w.cuts[1]: w.cuts[2]] = 0             # bind() puts the pool's empty doc there
    bs = wk.score_batches(kind, ld)
    w.bs = bs[(7 * seed) % len(bs):] + bs[: (7 * seed) % len(bs)]
    w.bdeck, w.prev = [], None
    nsteps = 1 + int(rng.integers(6, 9))
    opts = _draw_all_options(w, rng)
    w.steps.append({"ep": "set_options", "values": opts, "opts": opts})
    eps = STEP_EPS[(2 * t) % len(STEP_EPS):] + STEP_EPS[: (2 * t) % len(STEP_EPS)]
    deck = []
    while len(w.steps) < nsteps:
        u = rng.random()
        if u < 0.085:
            st = _draw_invalid(w, rng)
        elif u < 0.2:
            opts = _draw_all_options(w, rng)
            st = {"ep": "set_options", "values": opts}
        else:
            if not deck:
                deck = [eps[i] for i in rng.permutation(len(eps))]
            st = _draw_args(w, rng, deck.pop())
        st["opts"] = opts
        w.steps.append(st)
    return w


def scripted(kind, ld, seed, steps, tag):
    """The corpus, ranks and cuts of walk (kind, ld, seed) under written-out steps (a named regression)."""
    w = generate(kind, ld, seed)
    w.tag, w.steps, opts = tag, [], None
    for st in steps:
        opts = st["values"] if st["ep"] == "set_options" else opts
        w.steps.append(dict(st, opts=opts))
    return w


# ---------------------------------------------------------------------------- transcript
def _vectors(vs):
    return "/".join(wk._opts_text(v) for v in vs)


def render(i, step):
    parts = [f"{i:02d} {step['ep']}"]
    for key, val in step.items():
        if key in ("ep", "opts"):
            continue
        if key == "between":
            parts.append("between=[" + render(i, val)[3:] + "]")
        elif key == "values":
            parts.append("values=" + _vectors(val))
        else:
            parts.append(f"{key}={val}")
    if "opts" in step:
        parts.append("| opts=" + _vectors(step["opts"]))
    return " ".join(parts)


def header(w):
    sel = w.sel.copy()
    if w.cut_class == "empty_docs":
        sel[w.cuts[1]: w.cuts[2]] = 0               # as generated: bind() names the pool's empty doc there
    return (f"walk {w.name}: n={w.n} id_base={w.id_base} sel#{hashlib.sha256(sel.tobytes()).hexdigest()[:8]} "
            f"G={w.G} cuts={w.cut_class}:{','.join(str(int(c)) for c in w.cuts)} "
            f"options=({','.join(wk.OPT_NAMES)}) one vector per rank")


def transcript(w, upto=None):
    steps = w.steps if upto is None else w.steps[: upto + 1]
    return "\n".join([header(w)] + [render(i, s) for i, s in enumerate(steps)])


def transcripts_hash(walks):
    return hashlib.sha256("\n".join(transcript(w) for w in walks).encode()).hexdigest()


# ---------------------------------------------------------------------------- inputs of a step
def _sort_lex(ids, s):
    order = np.lexsort((ids, -s.astype(np.float64)))             # score desc, id asc (scores >= +0.0: no signed zeros)
    return ids[order], s[order]


def lex_global(w, step):
    """Per row the global stage-1 list: (ids int64 [m_b], scores f32 [m_b]) sorted
    (score desc, id asc), distinct in-range ids."""
    rng = w.rng(step["ds"] + 2)
    kb = step["kb"]
    rows = []
    for _ in range(step["B"]):
        m = int(rng.integers(0, min(w.n, 2 * kb + 8) + 1))
        ids = rng.choice(w.n, m, replace=False).astype(np.int64) + w.id_base
        rows.append(_sort_lex(ids, rng.choice(LEX_VALUES, m).astype(np.float32)))
    return rows


def _pad_lists(rows, B, kb):
    ids, s = np.full((B, kb), -1, np.int32), np.full((B, kb), -np.inf, np.float32)
    for b, (i, v) in enumerate(rows):
        ids[b, : min(kb, len(i))], s[b, : min(kb, len(i))] = i[:kb], v[:kb]
    return ids, s


def lex_rank(w, step, r, glob=None):
    """What rank r is handed: the entries it owns, its top-kb, -1 / -inf padded:
    (ids int32 [B, kb], scores f32 [B, kb])."""
    a, b = w.shard(r)
    rows = []
    for ids, s in glob if glob is not None else lex_global(w, step):
        own = (ids >= w.id_base + a) & (ids < w.id_base + b)
        rows.append((ids[own], s[own]))
    return _pad_lists(rows, step["B"], step["kb"])


def lex_merged(w, step, glob=None):
    """The merged stage-1 ids every rank must return: the global list's top-kb."""
    return _pad_lists(glob if glob is not None else lex_global(w, step), step["B"], step["kb"])[0]


def fused(lex, ids, C):
    """cbv2_retrieve_finish's candidates: RRF of (stage-1, stage-2) lists, the first C, -1 padded."""
    B = ids.shape[0]
    cand = np.full((B, C), -1, np.int32)
    for b in range(B):
        f = [cid for cid, _ in orc.rrf([int(x) for x in lex[b] if x >= 0], [int(x) for x in ids[b] if x >= 0],
                                       k=wk.RRF_K)[:C]]
        cand[b, : len(f)] = f
    return cand


def prescored_candidates(w, pool, step):
    """(cand int32 [B, C], miss bool [B, C]): the RRF of the merged lists cut to C
    and, with ``strays``, positions overwritten with candidates from elsewhere:
    -1, ids on either side of the corpus, a repeat of the position before (a
    stray repeated counts twice) and -- bf16 / MXFP8, whose ranks list exactly
    their shard's top-k -- an in-corpus id that no rank's stage-2 list and no
    stage-1 list holds (a faithful rank lists only what can reach the global
    top-k: which unlisted docs it lists is not fixed by the header).  miss marks
    the positions with id >= 0 that are in no gathered list."""
    S = wk.ref_rows(w, pool, step)
    B, C, k, n, base = step["B"], step["C"], step["k"], w.n, w.id_base
    _, _, ids = wk.topk_keys(S, k, base)
    glob = lex_global(w, step) if step["kb"] > 0 else [(np.zeros(0, np.int64), np.zeros(0, np.float32))] * B
    cand = fused(lex_merged(w, step, glob) if step["kb"] > 0 else np.zeros((B, 0), np.int32), ids, C)
    miss = np.zeros((B, C), bool)
    if not step["strays"]:
        return cand, miss
    rng = w.rng(step["ds"] + 3)
    outside = [-1]
    if base > 0:
        outside.append(base - 1)
    if base + n < 2 ** 31:
        outside.append(base + n)
    listed = None
    if w.kind != "fp32":                             # the docs some rank's top-k holds, per row
        listed = np.zeros((B, n), bool)
        for r in range(w.G):
            a, e = w.shard(r)
            if e > a:
                _, pos, _ = wk.topk_keys(S[:, a:e], k)
                for b in range(B):
                    listed[b, a + pos[b][pos[b] >= 0]] = True
    for b in range(B):
        free = None
        if listed is not None:
            free = np.flatnonzero(~listed[b])
            free = np.setdiff1d(free, glob[b][0] - base)
        for j in range(C):
            u = rng.random()
            if u < 0.12:
                cand[b, j] = int(rng.choice(outside))
                miss[b, j] = cand[b, j] >= 0
            elif u < 0.2 and free is not None and len(free):
                cand[b, j], miss[b, j] = int(rng.choice(free)) + base, True
            elif u < 0.3 and j > 0:
                cand[b, j], miss[b, j] = cand[b, j - 1], miss[b, j - 1]
    return cand, miss


# ---------------------------------------------------------------------------- the model
def _select(raw, cand, k):
    B = raw.shape[0]
    s, i, p = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int32), np.full((B, k), -1, np.int32)
    for b in range(B):
        for j, (pos, _, _) in enumerate(orc.rerank_select(raw[b], k)):
            s[b, j], i[b, j], p[b, j] = raw[b, pos], cand[b, pos], pos
    return s, i, p


def gathers(w):
    return 2 if w.kind == "fp32" else 1               # a faithful local call gathers fk first


def expected(w, pool, step):
    """name -> the array EVERY rank must hold, bit for bit; "rc"; "comm" the
    (all-gathers, all-reduces) the step adds to every rank's cbv2_comm_stats."""
    ep = step["ep"]
    if ep == "set_options":
        return {"rc": 0, "comm": (0, 0)}
    if ep == "invalid":
        return {"rc": wk.EINVAL, "untouched": True, "comm": (0, 0)}
    bind(w, pool)
    S = wk.ref_rows(w, pool, step)
    out = {"rc": 0}
    if ep == "rerank_sharded":
        out.update(wk.rerank_expect(S, wk.candidates(w, step), step["k"], w), comm=(0, 1))
        return out
    k, kb = step["k"], step["kb"]
    out["scores"], _, out["ids"] = wk.topk_keys(S, k, w.id_base)
    lex = lex_merged(w, step) if kb > 0 else np.zeros((S.shape[0], 0), np.int32)
    if ep in ("search_sharded", "search_split"):
        if kb > 0:
            out["lex"] = lex
        out["comm"] = (gathers(w), 0)
    elif ep == "prescored":
        if kb > 0:
            out["lex"] = lex
        g, r = gathers(w), 0
        if "between" in step:
            btw = expected(w, pool, step["between"])
            out.update({"btw_" + nm: btw[nm] for nm in ("scores", "ids", "pos")})
            r = 1
        cand, miss = prescored_candidates(w, pool, step)
        local = np.clip(cand.astype(np.int64) - w.id_base, 0, w.n - 1)
        raw = np.where((cand >= 0) & ~miss, np.take_along_axis(S, local, axis=1), -np.inf).astype(np.float32)
        out["pre_scores"], out["pre_ids"], out["pre_pos"] = _select(raw, cand, step["final_k"])
        out["misses"] = np.asarray([int(miss.sum())], np.int32)
        out["comm"] = (g, r)
    elif ep == "retrieve_sharded":
        del out["scores"], out["ids"]
        cand = fused(lex, wk.topk_keys(S, k, w.id_base)[2], step["C"])
        res = wk.rerank_expect(S, cand, step["final_k"], w)
        out.update(res)
        if step["how"] == "finish_host":
            out.update({"host_" + nm: res[nm] for nm in ("scores", "ids", "pos")})
        out["comm"] = (gathers(w), 0 if step["C"] <= 1024 else 1)   # C <= 1024: the prescored stage 3
    else:
        raise ValueError(ep)
    return out


# ---------------------------------------------------------------------------- the player
class ShardedFailure(AssertionError):
    def __init__(self, walk, index, rank, message):
        self.walk, self.index, self.rank = walk, index, rank
        super().__init__(f"walk {walk.name} fails at step {index} on rank {rank}: {message}\n{transcript(walk, index)}")


def play(w, pool, backend):
    """Every step on every rank through ``backend`` (call -> one dict per rank),
    compared with the model after each step; the first difference raises
    ShardedFailure naming step and rank, with the transcript up to the step."""
    bind(w, pool)
    backend.start(w, pool)
    failure = None
    for i, step in enumerate(w.steps):
        want = expected(w, pool, step)
        comm = want.pop("comm")
        got = backend.call(i, step)                             # an exception here (a fault, a rank that hung) leaves
        assert len(got) == w.G                                  # at once: the backend is not touched again
        for r, g in enumerate(got):
            g = dict(g)
            have = tuple(g.pop("comm"))
            msg = wk.compare(backend, g, want)
            if msg is None and have != comm:
                msg = f"cbv2_comm_stats moved by {have} (all-gathers, all-reduces), want {comm}"
            if msg:
                failure = ShardedFailure(w, i, r, msg)
                break
        if failure:
            break
    backend.finish()
    if failure is not None:
        raise failure
