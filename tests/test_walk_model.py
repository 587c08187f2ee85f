"""CPU: the walk infrastructure of tests/_walk.py pinned -- the committed seed
list yields the same transcripts on every run, visits every cell of the
coverage table at least 3 times, and can SEE bugs: a brute-force backend
(Python sorts on (-(key), id) tuples over the reference row, written
independently of the model) passes every committed walk, and each of eleven
mutants of it fails at least one, at a step that exercises the mutated code.

The backends read a pool's reference only; the CPU tests take
_walk.synthetic_pool (milliseconds) for all twelve (kind, ld) and the real
fp32 / 128 pool once.
"""
import itertools
from collections import Counter

import numpy as np
import pytest

import _exact as ex
import _walk as wk
import _walk_seeds as ws

LEAST = 3


# ---------------------------------------------------------------------------- the brute-force backend
def _key(bits):
    return (~bits & 0xFFFFFFFF) if bits >> 31 else (bits | 0x80000000)


class Brute:
    """Answers every step from the reference row by sorting Python tuples."""
    mutant = None

    def start(self, w, pool):
        self.w, self.pool = w, pool
        self.opts = {name: vals[0] for name, _, vals in wk.OPTIONS}
        self.prev_q = None                                      # (B, lq, rows) of the previous call with queries

    def finish(self):
        pass

    def same(self, got, want):
        got = np.ascontiguousarray(got)
        return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()

    def host(self, got):
        return got

    def untouched(self, arr):
        return arr is None

    # ----- hooks the mutants override
    def keys(self, row):
        """The order-preserving integer key of every float32 of a row."""
        return [_key(u) for u in np.asarray(row, np.float32).view(np.uint32).tolist()]

    def tie(self, i):
        return i

    def chunk_tie(self, i):
        return i

    def allowed(self, flt):
        n = self.w.n
        return [i for i in range(n) if (int(flt.words[i >> 5]) >> (i & 31)) & 1]

    def pad(self, arr, start):
        arr[start:] = -np.inf if arr.dtype == np.float32 else -1

    def outside(self, row):
        return -np.inf

    def keep_empty(self):
        return True

    # ----- pieces
    def rows(self, step):
        w = self.w
        q = [(step["q0"] + b) % w.Bp for b in range(step["B"])]
        if self.mutant == "stale_split" and self.prev_q is not None and self.prev_q[:2] == (step["B"], step["lq"]):
            q = self.prev_q[2]                                  # the previous contents of the same buffer
        self.prev_q = (step["B"], step["lq"], q)
        return [self.pool.ref[b, step["lq"] - 1][w.sel] for b in q]

    def rank(self, scores, ids, k, tie=None):
        """positions of the best k by (key desc, tie(id) asc)."""
        tie = tie or self.tie
        ks = self.keys(scores)
        return sorted(range(len(ks)), key=lambda j: (-ks[j], tie(ids[j])))[:k]

    def topk(self, rows, ids, k, base):
        B = len(rows)
        per_row = len(ids) == B and all(isinstance(x, list) for x in ids)
        s = np.empty((B, k), np.float32)
        i = np.empty((B, k), np.int32)
        for b, row in enumerate(rows):
            idb = ids[b] if per_row else ids
            order = self.rank(row, idb, k)
            s[b, : len(order)] = [row[j] for j in order]
            i[b, : len(order)] = np.asarray([idb[j] + base for j in order], np.int64).astype(np.int32)
            self.pad(s[b], len(order))
            self.pad(i[b], len(order))
        return s, i

    def select(self, raw, ids, k):
        """rerank / select: (key desc, position asc); ids[b][p] the id of position p."""
        B = len(raw)
        s, i, p = np.empty((B, k), np.float32), np.empty((B, k), np.int32), np.empty((B, k), np.int32)
        for b, row in enumerate(raw):
            order = self.rank(row, list(range(len(row))), k)
            s[b, : len(order)] = [row[j] for j in order]
            i[b, : len(order)] = [ids[b][j] for j in order]
            p[b, : len(order)] = order
            for a in (s, i, p):
                self.pad(a[b], len(order))
        return {"scores": s, "ids": i, "pos": p}

    def rerank(self, rows, cand, k):
        w = self.w
        raw = []
        for b, row in enumerate(rows):
            out = []
            for c in cand[b].tolist():
                loc = c - w.id_base
                out.append(row[loc] if c >= 0 and 0 <= loc < w.n else (-np.inf if c < 0 else self.outside(row)))
            raw.append(np.asarray(out, np.float32))
        if k == 0:
            return {"scores": np.stack(raw)}
        return self.select(raw, [c.tolist() for c in cand], k)

    def filtered(self, rows, lists, k):
        w = self.w
        sub, ids = [], []
        for row, al in zip(rows, lists):
            if not self.keep_empty():
                al = [i for i in al if np.isfinite(row[i % w.n])]
            sub.append([row[i % w.n] for i in al])
            ids.append(al)
        return self.topk(sub, ids, k, w.id_base)

    def grouped(self, rows, step):
        w = self.w
        _, gof, G = w.groupings[step["g"]]
        k, r = step["k"], step["r"]
        members = {}
        for i, g in enumerate(gof.tolist()):
            if g >= 0:
                members.setdefault(g, []).append(i)
        B = len(rows)
        s = np.full((B, k), -np.inf, np.float32)
        gi = np.full((B, k), -1, np.int32)
        ci = np.full((B, k, r), -1, np.int32)
        cs = np.full((B, k, r), -np.inf, np.float32)
        for b, row in enumerate(rows):
            ks = self.keys(row)
            best = {g: max(ks[i] for i in m) for g, m in members.items()}
            for j, g in enumerate(sorted(best, key=lambda g: (-best[g], self.tie(g)))[:k]):
                m = members[g]
                order = self.rank([row[i] for i in m], m, r, tie=self.chunk_tie)
                gi[b, j] = g
                ci[b, j, : len(order)] = [m[x] + w.id_base for x in order]
                cs[b, j, : len(order)] = [row[m[x]] for x in order]
                s[b, j] = cs[b, j, 0]
        return {"scores": s, "groups": gi, "ids": ci, "chunk_scores": cs}

    def invalid(self, step):
        """The header's argument checks."""
        faithful = step["on"] == "search_f32"
        bad = step.get("k", 1) < 1 or not 1 <= step.get("r", 1) <= 8 or not 1 <= step["lq"] <= wk.LQ_MAX \
            or step["ws_delta"] < 0 or step["ws_offset"] % 16 != 0 or (faithful and step["null_status"]) \
            or (faithful and not step["k"] <= step["cap"] <= wk.BAND_CAP) \
            or (step["on"] == "search_filtered_batch" and step["B"] != len(self.w.batches[step["fb"]]))
        return {"rc": wk.EINVAL if bad else 0}

    # ----- the call
    def call(self, i, step):
        w, ep = self.w, step["ep"]
        if ep == "set_options":
            self.opts = dict(zip(wk.OPT_NAMES, step["values"]))
            return {"rc": 0}
        if ep == "invalid":
            return self.invalid(step)
        out = {"rc": 0}
        k = step.get("k")
        ids = list(range(w.n))
        if ep in ("select_topk", "topk_rows", "merge_topk", "group_topk_rows"):
            if ep == "select_topk":
                M, cid = wk.select_inputs(w, self.pool, step)
                pos = list(range(M.shape[1]))
                out.update(self.select(list(M), [pos if cid is None else cid[b].tolist() for b in range(len(M))], k))
            elif ep == "topk_rows":
                M = wk.topk_inputs(w, self.pool, step)[:, : w.n]
                out["scores"], out["ids"] = self.topk(list(M), ids, k, w.id_base)
            elif ep == "merge_topk":
                _, in_s, in_i = wk.merge_inputs(w, self.pool, step)
                rows, idl = [], []
                for b in range(in_s.shape[1]):
                    keep = in_i[:, b].reshape(-1) >= 0
                    rows.append(in_s[:, b].reshape(-1)[keep])
                    idl.append(in_i[:, b].reshape(-1)[keep].tolist())
                out["scores"], out["ids"] = self.topk(rows, idl, k, 0)
            else:
                out.update(self.grouped(list(wk.topk_inputs(w, self.pool, step)[:, : w.n]), step))
            return out
        if ep == "search_f32_split":                           # begin, the call between, finish
            rows = self.rows(step)
            out["between"] = self.call(i, step["between"])
            if self.mutant == "finish_takes_between":
                rows = (self.rows(step["between"]) * step["B"])[: step["B"]]
        else:
            rows = self.rows(step)
        if ep == "score":
            out["scores"] = np.stack(rows)
        elif ep in ("search", "search_f32", "search_f32_split"):
            kk = k
            drop = self.mutant == "reuse_and_fused" and ep == "search_f32" and self.opts["BAND_REUSE"] \
                and self.opts["BAND_FUSED"]
            s, ix = self.topk(rows, ids, k + 1 if drop else k, w.id_base)
            if drop:                                            # the k-th doc is lost, the next one moves up
                s, ix = np.delete(s, kk - 1, axis=1), np.delete(ix, kk - 1, axis=1)
            out["scores"], out["ids"] = s, ix
            if ep != "search":
                out["status"] = np.full(len(rows), -1, np.int32)
        elif ep in ("rerank", "rerank_ws", "rerank_f32"):
            out.update(self.rerank(rows, wk.candidates(w, step), k))
        elif ep in ("search_filtered", "search_filtered_f32"):
            al = self.allowed(w.filters[step["f"]])
            out["scores"], out["ids"] = self.filtered(rows, [al] * len(rows), k)
            if ep == "search_filtered_f32":
                out["status"] = np.full(len(rows), -1 if len(al) else 0, np.int32)
        elif ep == "search_filtered_batch":
            lists = [ids if f is None else self.allowed(w.filters[f]) for f in w.batches[step["fb"]][: len(rows)]]
            out["scores"], out["ids"] = self.filtered(rows, lists, k)
        elif ep in ("search_grouped", "search_grouped_f32"):
            out.update(self.grouped(rows, step))
            if ep == "search_grouped_f32":
                any_member = bool((w.groupings[step["g"]][1] >= 0).any())
                out["status"] = np.full(len(rows), -1 if any_member else 0, np.int32)
        elif ep == "retrieve":
            s, ix = self.topk(rows, ids, k, w.id_base)
            if step["how"] == "cancel":
                out["scores"], out["ids"] = s, ix
                return out
            lex = wk.lexical_ids(w, step) if step["kb"] else np.zeros((len(rows), 0), np.int32)
            cand = np.full((len(rows), step["C"]), -1, np.int32)
            for b in range(len(rows)):
                acc = {}
                for lst in (lex[b].tolist(), ix[b].tolist()):
                    for rank, cid in enumerate([c for c in lst if c >= 0], 1):
                        acc[cid] = acc.get(cid, 0) + 1 / (wk.RRF_K + rank)
                fused = [cid for cid, _ in sorted(acc.items(), key=lambda t: -t[1])][: step["C"]]
                cand[b, : len(fused)] = fused
            out.update(self.rerank(rows, cand, step["final_k"]))
            if step["how"] == "finish_host":
                out.update({"host_" + name: out[name] for name in ("scores", "ids", "pos")})
        else:
            raise ValueError(ep)
        return out


def _mutant(name, **hooks):
    return type(name, (Brute,), dict(mutant=name, **hooks))


def _last_word_ignored(self, flt):
    full = 32 * (self.w.n // 32)
    return [i for i in Brute.allowed(self, flt) if i < full]


def _bits_past_n(self, flt):
    return [i for i in range(32 * len(flt.words)) if (int(flt.words[i >> 5]) >> (i & 31)) & 1]


def _poison_pad(self, arr, start):
    arr[start:] = np.nan if arr.dtype == np.float32 else wk.POISON_I


# name -> (the mutant, the entry points whose code it changes: the failing step must be one of them)
_SELECTS = ("search", "search_f32", "search_f32_split", "search_filtered", "search_filtered_f32",
            "search_filtered_batch", "search_grouped", "search_grouped_f32", "topk_rows", "merge_topk",
            "group_topk_rows", "retrieve")
_FILTERED = ("search_filtered", "search_filtered_f32", "search_filtered_batch")
MUTANTS = {
    "ties_to_higher_id": (_mutant("ties_to_higher_id", tie=lambda self, i: -i),
                          _SELECTS + ("rerank", "rerank_ws", "rerank_f32", "select_topk")),
    "last_filter_word_ignored": (_mutant("last_filter_word_ignored", allowed=_last_word_ignored), _FILTERED),
    "filter_bits_past_n": (_mutant("filter_bits_past_n", allowed=_bits_past_n), _FILTERED),
    "padding_not_written": (_mutant("padding_not_written", pad=_poison_pad),
                            _SELECTS + ("rerank", "rerank_ws", "rerank_f32", "select_topk")),
    "stale_split": (_mutant("stale_split"), None),             # any call that takes queries
    "reuse_and_fused": (_mutant("reuse_and_fused"), ("search_f32",)),
    "group_chunk_ties_descending": (_mutant("group_chunk_ties_descending", chunk_tie=lambda self, i: -i),
                                    ("search_grouped", "search_grouped_f32", "group_topk_rows")),
    "outside_candidate_is_doc_0": (_mutant("outside_candidate_is_doc_0", outside=lambda self, row: row[0]),
                                   ("rerank", "rerank_ws", "rerank_f32", "retrieve")),
    "signed_zeros_equal": (_mutant("signed_zeros_equal",
                                   keys=lambda self, row: Brute.keys(self, np.asarray(row, np.float32) + np.float32(0))),
                           ("select_topk", "topk_rows", "merge_topk", "group_topk_rows")),
    "finish_takes_between": (_mutant("finish_takes_between"), ("search_f32_split",)),
    "empty_doc_dropped_by_filter": (_mutant("empty_doc_dropped_by_filter", keep_empty=lambda self: False), _FILTERED),
}


# ---------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def walks():
    return [wk.generate(*key) for key in ws.committed()]


@pytest.fixture(scope="module")
def pools():
    return {(kind, ld): wk.synthetic_pool(kind, ld) for kind in ex.KINDS for ld in wk.LDS}


# ---------------------------------------------------------------------------- determinism
def test_committed_transcripts_hash(walks):
    keys = ws.committed() + ws.committed_large()
    first, again = ([wk.generate(*key) for key in keys] for _ in range(2))
    assert wk.transcripts_hash(again) == wk.transcripts_hash(first), "two runs of the generator differ"
    assert wk.transcripts_hash(first) == ws.TRANSCRIPTS_SHA256, \
        "the committed walks changed: update _walk_seeds.TRANSCRIPTS_SHA256 together with the seed counts"


def test_key_topk_is_oracle_topk_and_partition_agrees():
    rng = np.random.default_rng(5)
    S = (rng.integers(-40, 40, (3, 9000)) / 8).astype(np.float32)      # mass ties, no signed zeros
    S[:, ::97] = -np.inf
    from oracle import oracle as orc
    for k in (1, 10, 1100):
        s, pos, ids = wk.topk_keys(S, k, 5)                             # the partition path (n > 8192)
        es, ei = orc.topk(S, k, 5)
        assert np.array_equal(ids, ei) and np.array_equal(s, es.astype(np.float32))
    s, pos, ids = wk.topk_keys(S[:, :300], 400, 0)                      # oracle.topk on the keys, padded
    es, ei = orc.topk(S[:, :300], 400, 0)
    assert np.array_equal(ids, ei) and np.array_equal(s, es.astype(np.float32))
    z = np.array([[0.0, -0.0, -0.0, 0.0, -1.0, 1.0]], np.float32)
    assert wk.topk_keys(z, 6)[1].tolist() == [[5, 0, 3, 1, 2, 4]]       # -0.0 below +0.0, ties to the lower index


# ---------------------------------------------------------------------------- coverage
def _steps(walks):
    for w in walks:
        for st in w.steps:
            yield w, st
            if "between" in st:
                yield w, dict(st["between"], opts=st["opts"])


def coverage(walks):
    """cell -> visits; every cell the condition names is present (0 when unvisited)."""
    c = Counter()
    for kind in ex.KINDS:
        for ld in wk.LDS:
            for ep in wk.entry_points(kind) + ("set_options", "invalid"):
                c["triple", ep, kind, ld] = 0
            for b in wk.score_batches(kind, ld):
                c["B", wk.scan_family(kind, ld), b] = 0
    for name, _, vals in wk.OPTIONS:
        for v in vals:
            for ep in wk.READS[name]:
                c["option", name, v, ep] = 0
    for a, b in itertools.combinations(wk.BAND_OPTIONS, 2):
        for va in wk.OPTIONS[wk.OPT_INDEX[a]][2]:
            for vb in wk.OPTIONS[wk.OPT_INDEX[b]][2]:
                c["band pair", a, va, b, vb] = 0
    for cls in ("<n", "=n", ">n", ">1024"):
        c["k", cls] = 0
    for ep in ("search_filtered", "search_filtered_f32", "search_filtered_batch"):
        for cls in wk.FILTER_CLASSES:
            c["filter", ep, cls] = 0
    for n in wk.N_EDGES + ("N",):
        c["n", n] = 0
    for w in walks:
        if w.n == w.N:
            c["n", "N"] += 1                                    # the whole pool's size, whatever the ld
        elif ("n", w.n) in c:
            c["n", w.n] += 1
    for w, st in _steps(walks):
        ep = st["ep"]
        if ("triple", ep, w.kind, w.ld) in c:
            c["triple", ep, w.kind, w.ld] += 1
        opts = dict(zip(wk.OPT_NAMES, st["opts"]))
        for name in wk.OPT_NAMES:
            if ep in wk.READS[name]:
                c["option", name, opts[name], ep] += 1
        if ep == "search_f32":
            for a, b in itertools.combinations(wk.BAND_OPTIONS, 2):
                c["band pair", a, opts[a], b, opts[b]] += 1
        if ep in wk.SCAN_EPS:                                   # only the calls that run the family's scan
            c["B", wk.scan_family(w.kind, w.ld), st["B"]] += 1
        if "k" in st and ep not in ("invalid", "retrieve", "rerank", "rerank_ws", "rerank_f32", "select_topk"):
            c["k", wk.k_class(st["k"], w.n)] += 1
        if ep in ("search_filtered", "search_filtered_f32"):
            c["filter", ep, w.filters[st["f"]].cls] += 1
        if ep == "search_filtered_batch":
            for f in set(w.batches[st["fb"]]):
                c["filter", ep, "all" if f is None else w.filters[f].cls] += 1
    return c


def test_coverage_condition(walks):
    c = coverage(walks)
    low = sorted((str(cell), v) for cell, v in c.items() if v < LEAST)
    table = "\n".join(f"{v:5d}  {cell}" for cell, v in sorted((str(k), v) for k, v in c.items()))
    assert not low, f"{len(low)} cells visited fewer than {LEAST} times: {low[:40]}\n{table}"
    steps = [st for w in walks for st in w.steps]
    share = sum(st["ep"] == "invalid" for st in steps) / len(steps)
    assert 0.05 <= share <= 0.10, f"invalid steps are {share:.3f} of {len(steps)} steps"
    # no drawn step is dropped as "not applicable": every step of every walk is
    # legal for its pool, and the model answers each of them
    for w in walks:
        assert 8 <= len(w.steps) <= 12
        legal = set(wk.entry_points(w.kind, w.large)) | {"set_options", "invalid"}
        assert all(st["ep"] in legal for st in w.steps), w.name


def large_coverage(walks):
    """The dispatch paths that exist only from 65,536 docs on, per index kind:
    the steps that LAUNCH each (the dispatch's own conjunctions, restated in
    _walk.large_paths) and, beside them, the steps only the path's own option
    keeps out of it: cell -> visits."""
    c = Counter()
    for kind in ex.KINDS:
        c[kind, "block-max top-k", "on"] = c[kind, "block-max top-k", "off: sampled filter"] = 0
        for v in (0, 1, 2):
            c[kind, "dynamic tail (B >= 33)", str(v)] = 0
        c[kind, "sampled filter on signed zeros", "on"] = 0
        if kind == "fp32":
            for cell in ("band block skip", "fused phase-1 collect", "folded keys"):
                c[kind, cell, "on"] = c[kind, cell, "off"] = 0
            c[kind, "default option vector, B <= 8", "on"] = 0
    for w, st in _steps(walks):
        for path, pos in wk.large_paths(w, st):
            if (w.kind, path, pos) in c:
                c[w.kind, path, pos] += 1
    return c


def _large_ok(seeds):
    walks = [wk.generate(kind, 128, seed, True) for kind in ex.KINDS for seed in range(seeds[kind])]
    c = large_coverage(walks)
    ok = min(c.values()) >= 1 and min(seeds.values()) >= len(wk.THEMES)      # every path, every theme per kind
    return ok and all({w.n for w in walks if w.kind == kind} == set(wk.LARGE_N) for kind in ex.KINDS), c


def test_large_walks_reach_the_large_size_paths():
    ok, c = _large_ok(ws.LARGE_SEEDS)
    assert ok, sorted(c.items(), key=str)
    for key in ws.committed_large():
        w = wk.generate(*key)
        assert w.n in wk.LARGE_N and {st["ep"] for st in w.steps} <= wk.LARGE_EPS | {"set_options"}
    for kind in ex.KINDS:                                       # one seed fewer for any kind leaves a cell short
        assert not _large_ok(dict(ws.LARGE_SEEDS, **{kind: ws.LARGE_SEEDS[kind] - 1}))[0], kind


def test_seed_counts_are_minimal():
    """One seed fewer for any kind leaves a cell short."""
    for kind in ex.KINDS:
        fewer = dict(ws.SEEDS, **{kind: ws.SEEDS[kind] - 1})
        c = coverage([wk.generate(*key) for key in ws.committed(fewer)])
        assert any(v < LEAST for v in c.values()), f"{kind}: {fewer[kind]} seeds would do"


# ---------------------------------------------------------------------------- sensitivity
def test_honest_backend_passes_every_walk(walks, pools):
    for w in walks:
        wk.play(w, pools[w.kind, w.ld], Brute())


def test_honest_backend_passes_on_a_real_pool():
    pool = wk.exact_pool("fp32", 128)
    for key in ws.committed():
        if key[:2] == ("fp32", 128):
            wk.play(wk.generate(*key), pool, Brute())


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(walks, pools, name):
    cls, eps = MUTANTS[name]
    caught = []
    for w in walks:
        try:
            wk.play(w, pools[w.kind, w.ld], cls())
        except wk.WalkFailure as e:
            st = w.steps[e.index]
            if "the call between begin and finish" in str(e):
                st = st["between"]
            ep = st["ep"]
            assert ("q0" in st) if eps is None else (ep in eps), \
                f"mutant {name} was blamed on step {e.index} ({ep}), which does not run the mutated code:\n{e}"
            assert f"fails at step {e.index}" in str(e) and wk.render(e.index, w.steps[e.index]) in str(e)
            caught.append((w.name, e.index, ep))
            if len(caught) == 3:
                break
    assert caught, f"no committed walk fails through mutant {name}"


def test_failure_message_names_walk_step_and_bits(walks, pools):
    cls, _ = MUTANTS["ties_to_higher_id"]
    for w in walks:
        try:
            wk.play(w, pools[w.kind, w.ld], cls())
        except wk.WalkFailure as e:
            text = str(e)
            assert f"walk {w.name} fails at step {e.index}" in text and wk.header(w) in text
            assert text.count("\n") == e.index + 2                      # the transcript up to the failing step
            assert "first at (row " in text and "got " in text and "want " in text
            return
    pytest.fail("no walk failed")
