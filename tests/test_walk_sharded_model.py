"""CPU: the sharded walks of tests/_walk_sharded.py pinned -- the committed seed
list yields the same transcripts on every run, visits every cell of the
coverage table at least 3 times, skips no step it drew, and can SEE bugs: a
brute-force backend that REALLY shards (per-rank tuple sorts on the reference
row, a k-way merge, the union's k-th, a dictionary lookup for the prescored
select; written independently of the model, which knows no shards) passes
every committed walk, and each mutant of it fails at least one at a step that
runs the mutated code.

Two mutants must NOT fail, and that is what they pin:
  options_of_the_neighbour   rank r runs rank r + 1's option vector: options
                             are rank-local and promise identical results.
  union_kth_own_shard        a faithful rank bounds its band by the k-th of its
                             OWN list only.  The k-th largest of any subset of
                             the corpus is a lower bound of the global k-th, so
                             the results cannot change (cbv2_search_f32_begin's
                             paragraph: "any such lower bound keeps the result
                             exact"); the all-gather of fk only narrows the
                             band.  Its failing counterpart is
                             union_kth_of_shard_maxima, a bound that is too
                             high (the largest of the shards' own k-ths, -inf
                             padding skipped).
The coverage table counts, as tests/test_walk_model.py does, marginals and
pairs of its dimensions -- (step kind, kind, ld), (family, G), (family, k
class), (family, kb), (G, cut class), (G, step kind), (cut class, step kind),
(k class, step kind), (kb, step kind), (family, B) -- and the conditions named
one by one (G * k and G * kb on both sides of 8192, some shard n == 0 / n == 1,
every shard n < k, a non-empty shard whose docs are all empty -- on fp32 with k
on both sides of n --, misses > 0, ...), not the full product (22,400 cells, three
visits each, would be 30 times the committed steps).
"""
import struct
from collections import Counter

import numpy as np
import pytest

import _exact as ex
import _walk as wk
import _walk_sharded as sw

LEAST = 3
NEG = float("-inf")


def _key(x):
    """The order-preserving integer key of a float32 (-0.0 below +0.0)."""
    bits = struct.unpack("<I", struct.pack("<f", x))[0]
    return (~bits & 0xFFFFFFFF) if bits >> 31 else (bits | 0x80000000)


def _keys(row):
    bits = np.asarray(row, np.float32).view(np.uint32)
    return np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000)).tolist()


class Brute:
    """G ranks, each answering from its own docs of the reference row."""
    mutant = None

    def start(self, w, pool):
        self.w, self.pool = w, pool
        self.opts = [None] * w.G
        self.stats = [[0, 0] for _ in range(w.G)]

    def finish(self):
        pass

    def same(self, got, want):
        got = np.ascontiguousarray(got)
        return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()

    def host(self, got):
        return got

    def untouched(self, arr):
        return arr is None

    # ----- one rank's work
    def rows(self, step):
        w = self.w
        return [self.pool.ref[(step["q0"] + b) % w.Bp, step["lq"] - 1][w.sel].tolist() for b in range(step["B"])]

    def local_topk(self, row, r, k):
        """rank r's list: [(score, global id)] best first, at most k."""
        a, e = self.w.shard(r)
        ks = _keys(row[a:e])
        order = sorted(range(e - a), key=lambda j: (-ks[j], j))[:k]
        return [(row[a + j], a + j + self.w.id_base) for j in order]

    def stage2(self, row, k):
        """every rank's send list for one row: G lists of k (score, id), -inf / -1 padded."""
        w = self.w
        lists = [self.local_topk(row, r, k) for r in range(w.G)]
        if w.kind == "fp32":                                     # the band keeps what can reach the bound lb
            kth = lambda xs: sorted((_key(s) for s, _ in xs), reverse=True)[k - 1] if len(xs) >= k else _key(NEG)  # noqa: E731
            union = kth([x for lst in lists for x in lst])
            for r in range(w.G):
                lb = union
                if self.mutant == "union_kth_own_shard":
                    lb = kth(lists[r])
                elif self.mutant == "union_kth_of_shard_maxima":
                    lb = max(min((_key(s) for s, _ in lst), default=_key(NEG)) for lst in lists)
                lists[r] = [x for x in lists[r] if _key(x[0]) >= lb]
        out = []
        for r, lst in enumerate(lists):
            a, e = w.shard(r)
            pad_id = w.id_base + a if self.mutant == "empty_shard_emits_id_base" and e == a else -1
            out.append(lst + [(NEG, pad_id)] * (k - len(lst)))
        return out

    def merge(self, lists, k, lex=False):
        """the k-way merge of the G gathered lists (the same entries on every rank) -> (scores [k], ids [k])."""
        ent = [(s, i, g, j) for g, lst in enumerate(lists) for j, (s, i) in enumerate(lst) if i >= 0]
        if lex and self.mutant == "lex_merge_ignores_scores":
            ent.sort(key=lambda t: t[1])
        elif self.mutant == "merge_ties_by_shard_order":         # the heads popped round-robin among equal scores
            ent.sort(key=lambda t: (-_key(t[0]), t[3], t[2]))
        else:
            ent.sort(key=lambda t: (-_key(t[0]), t[1]))
        ent = ent[:k]
        s = np.full(k, -np.inf, np.float32)
        i = np.full(k, -1, np.int32)
        s[: len(ent)] = [t[0] for t in ent]
        i[: len(ent)] = np.asarray([t[1] for t in ent], np.int64).astype(np.int32)
        return s, i

    def on_rank(self, merged, k, r):
        """what rank r writes of a merged stage-2 list."""
        s, i = merged[0].copy(), merged[1].copy()
        if self.mutant == "pads_after_own_shard":
            a, e = self.w.shard(r)
            s[min(k, e - a):], i[min(k, e - a):] = -np.inf, -1
        return s, i

    def lex_lists(self, step, kb_parse):
        """[rank][row] -> [(score, id)]: what the ranks were handed, as the exchange reads the send blocks."""
        w, B, kb = self.w, step["B"], step["kb"]
        glob = sw.lex_global(w, step)
        out = []
        for r in range(w.G):
            ids, s = sw.lex_rank(w, step, r, glob)
            if kb_parse != kb:                                   # the block written for kb, read with another width
                flat = np.concatenate([s.ravel().astype(np.float64), ids.ravel().astype(np.float64),
                                       np.full(2 * B * kb_parse, -1.0)])
                s = flat[: B * kb_parse].reshape(B, kb_parse)
                ids = flat[B * kb_parse: 2 * B * kb_parse].reshape(B, kb_parse).astype(np.int64)
            out.append([[(float(s[b, j]), int(ids[b, j])) for j in range(ids.shape[1])] for b in range(B)])
        return out

    def search(self, step, rows):
        """-> per rank {"scores", "ids", ["lex"]}, and the gathered lists."""
        w, B, k, kb = self.w, step["B"], step["k"], step["kb"]
        s2 = [self.stage2(row, k) for row in rows]               # [row][rank]
        kbx = step.get("kb_local", kb) if self.mutant == "local_kb_reused" else kb
        lex = self.lex_lists(step, kbx) if kb > 0 else None
        res = []
        merged = [self.merge(s2[b], k) for b in range(B)]
        lexm = [self.merge([lex[g][b] for g in range(w.G)], kb, lex=True)[1] for b in range(B)] if kb > 0 else None
        for r in range(w.G):
            o = {"scores": np.empty((B, k), np.float32), "ids": np.empty((B, k), np.int32)}
            if kb > 0:
                o["lex"] = np.stack(lexm)
            for b in range(B):
                o["scores"][b], o["ids"][b] = self.on_rank(merged[b], k, r)
            self.stats[r][0] += sw.gathers(w)
            res.append(o)
        return res, s2, lex

    def select(self, raw, cand, k):
        B = len(raw)
        s, i, p = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int32), np.full((B, k), -1, np.int32)
        for b, row in enumerate(raw):
            ks = _keys(row)
            order = sorted(range(len(row)), key=lambda j: (-ks[j], j))[:k]
            s[b, : len(order)] = [row[j] for j in order]
            i[b, : len(order)] = [cand[b][j] for j in order]
            p[b, : len(order)] = order
        return s, i, p

    def rerank(self, step, rows):
        """every rank scores what it owns, the maximum over the ranks, the select."""
        w = self.w
        cand = wk.candidates(w, step).tolist()
        raw = []
        for b, row in enumerate(rows):
            per_rank = []
            for r in range(w.G):
                a, e = w.shard(r)
                per_rank.append([row[c - w.id_base] if c >= 0 and a <= c - w.id_base < e else NEG for c in cand[b]])
            raw.append([max(col, key=_key) for col in zip(*per_rank)])
        s, i, p = self.select(raw, cand, step["k"])
        for r in range(w.G):
            self.stats[r][1] += 1
        return {"scores": s, "ids": i, "pos": p}

    def lookup(self, step, rows, s2, lex, cand):
        """the prescored select: the gathered (id, score) entries in a dictionary."""
        w, raw, misses = self.w, [], 0
        for b, row in enumerate(rows):
            tab = {}
            for g in range(w.G):
                for j, (s, i) in enumerate(s2[b][g]):
                    if i < 0:
                        continue
                    if self.mutant == "prescored_prefers_non_owner":
                        other = s2[b][(g + 1) % w.G][j]
                        s = other[0] if other[1] >= 0 else s
                    tab[i] = s
                for _, i in (lex[g][b] if lex else ()):
                    if i >= 0:
                        tab.setdefault(i, row[i - w.id_base])   # the owner's prescore: its rerank of the doc
            raw.append([tab.get(c, NEG) if c >= 0 else NEG for c in cand[b]])
            missing = [c for c in cand[b] if c >= 0 and c not in tab]
            misses += len(set(missing)) if self.mutant == "misses_per_distinct_id" else len(missing)
        return raw, misses

    # ----- the call
    def invalid(self, step):
        bad = step["k"] < 1 or step["B"] < 1 or not 1 <= step["lq"] <= wk.LQ_MAX or step["kb"] < 0 \
            or step["ws_delta"] < 0 or (step["on"] == "prescored" and (not 1 <= step["C"] <= 1024 or step["final_k"] < 1))
        return {"rc": wk.EINVAL if bad else 0}

    def call(self, i, step):
        w, ep = self.w, step["ep"]
        before = [tuple(s) for s in self.stats]
        if ep == "set_options":
            nb = self.mutant == "options_of_the_neighbour"
            self.opts = [step["values"][(r + 1) % w.G if nb else r] for r in range(w.G)]
            res = [{"rc": 0} for _ in range(w.G)]
        elif ep == "invalid":
            res = [self.invalid(step) for _ in range(w.G)]
        else:
            rows = self.rows(step)
            if ep == "rerank_sharded":
                o = self.rerank(step, rows)
                res = [dict(o, rc=0) for _ in range(w.G)]
            else:
                res, s2, lex = self.search(step, rows)
                for o in res:
                    o["rc"] = 0
                if ep == "prescored":
                    if "between" in step:
                        btw = self.rerank(step["between"], self.rows(step["between"]))
                        for o in res:
                            o.update({"btw_" + nm: btw[nm] for nm in btw})
                    cand = sw.prescored_candidates(w, self.pool, step)[0].tolist()
                    raw, misses = self.lookup(step, rows, s2, lex, cand)
                    s, ids, p = self.select(raw, cand, step["final_k"])
                    for o in res:
                        o.update(pre_scores=s, pre_ids=ids, pre_pos=p, misses=np.asarray([misses], np.int32))
                elif ep == "retrieve_sharded":
                    out = []
                    for r, o in enumerate(res):
                        C = step["C"]
                        lexm = o["lex"] if step["kb"] > 0 else np.zeros((len(rows), 0), np.int32)
                        cand = sw.fused(lexm, o["ids"], C).tolist()
                        if C <= 1024:
                            raw, _ = self.lookup(step, rows, s2, lex, cand)
                        else:
                            raw = [[row[c - w.id_base] if 0 <= c - w.id_base < w.n else NEG for c in cand[b]]
                                   for b, row in enumerate(rows)]
                            self.stats[r][1] += 1
                        s, ids, p = self.select(raw, cand, step["final_k"])
                        o = {"rc": 0, "scores": s, "ids": ids, "pos": p}
                        if step["how"] == "finish_host":
                            o.update(host_scores=s, host_ids=ids, host_pos=p)
                        out.append(o)
                    res = out
        for r, o in enumerate(res):
            o["comm"] = (self.stats[r][0] - before[r][0], self.stats[r][1] - before[r][1])
        return res


def _mutant(name):
    return type(name, (Brute,), dict(mutant=name))


_SEARCHES = ("search_sharded", "search_split", "prescored", "retrieve_sharded")
# name -> the step kinds that run the mutated code (the failing step must be one of them)
MUTANTS = {
    "merge_ties_by_shard_order": _SEARCHES,
    "empty_shard_emits_id_base": _SEARCHES,
    "union_kth_of_shard_maxima": _SEARCHES,
    "lex_merge_ignores_scores": _SEARCHES,
    "prescored_prefers_non_owner": ("prescored", "retrieve_sharded"),
    "misses_per_distinct_id": ("prescored",),
    "pads_after_own_shard": _SEARCHES,
    "local_kb_reused": ("search_split", "prescored"),
}
HARMLESS = ("options_of_the_neighbour", "union_kth_own_shard")


# ---------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def walks():
    return [sw.generate(*key) for key in sw.committed()]


@pytest.fixture(scope="module")
def pools():
    return {(kind, ld): wk.synthetic_pool(kind, ld) for kind in ex.KINDS for ld in wk.LDS}


def test_committed_transcripts_hash(walks):
    again = [sw.generate(*key) for key in sw.committed()]
    assert sw.transcripts_hash(again) == sw.transcripts_hash(walks), "two runs of the generator differ"
    assert sw.transcripts_hash(walks) == sw.TRANSCRIPTS_SHA256, \
        "the committed sharded walks changed: update _walk_sharded.TRANSCRIPTS_SHA256 together with SEEDS"


def test_cut_classes_are_what_they_say():
    rng = np.random.default_rng(1)
    for G in sw.GS:
        for n in (1, 2, 7, 600):
            for cls in sw.legal_cuts(G, n):
                sizes = np.diff(sw.make_cuts(cls, G, n, rng))
                assert sizes.sum() == n and len(sizes) == G
                if G == 1:
                    continue
                if cls == "first_empty":
                    assert sizes[0] == 0
                elif cls == "last_empty":
                    assert sizes[-1] == 0
                elif cls == "middle_empty":
                    assert sizes[G // 2] == 0
                elif cls == "one_doc":
                    assert sizes[1] == 1
                elif cls == "empty_docs":
                    assert 1 <= sizes[1] <= 3
                elif cls == "one_owner":
                    assert sorted(sizes)[-1] == n and (sizes == 0).sum() == G - 1
                elif cls == "small_first":
                    assert 1 <= sizes[0] <= 5
                elif cls == "even":
                    assert sizes.max() - sizes.min() <= 1


def test_stage1_lists_tie_across_shards_and_have_a_zero_tail(walks):
    ties = zeros = 0
    for w in walks:
        for st in w.steps:
            if st["ep"] in sw.STEP_EPS and st.get("kb", 0) > 1 and w.G > 1:
                for ids, s in sw.lex_global(w, st):
                    owner = np.searchsorted(w.cuts, ids - w.id_base, side="right")
                    same = s[1:] == s[:-1]
                    ties += int((same & (owner[1:] != owner[:-1])).sum())
                    zeros += int((s == 0).sum())
    assert ties > 100 and zeros > 100


# ---------------------------------------------------------------------------- coverage
_SEARCH_STEPS = ("search_sharded", "search_split", "prescored", "retrieve_sharded")   # the steps that draw k and kb


def _searches(walks):
    for w in walks:
        for st in w.steps:
            if st["ep"] in sw.STEP_EPS and st["ep"] != "rerank_sharded":
                yield w, st


def coverage(walks, pools):
    c = Counter()
    fams = sorted({wk.scan_family(k, ld) for k, ld in sw.CASES})
    for kind, ld in sw.CASES:
        for ep in sw.STEP_EPS + ("set_options", "invalid"):
            c["triple", ep, kind, ld] = 0
        for b in wk.score_batches(kind, ld):
            c["B", wk.scan_family(kind, ld), b] = 0
    for fam in fams:
        for G in sw.GS:
            c["family G", fam, G] = 0
    for G in sw.GS:
        for cls in sw.legal_cuts(G, 600):
            c["G cut", G, cls] = 0
        for ep in sw.STEP_EPS:
            c["G step", G, ep] = 0
    for cls in ("<n", "=n", ">n", ">1024"):
        c["k", cls] = 0
        for fam in fams:
            c["family k", fam, cls] = 0
        for ep in _SEARCH_STEPS:
            c["k step", cls, ep] = 0
    for cls in sw.CUT_CLASSES:
        for ep in sw.STEP_EPS:
            c["cut step", cls, ep] = 0
    for kb in sw.KBS:
        for fam in fams:
            c["family kb", fam, kb] = 0
        for ep in _SEARCH_STEPS:
            c["kb step", kb, ep] = 0
    for v in (1, 2, 1024, 1025, 1100):
        c["k value", v] = 0
    for kb in sw.KBS:
        c["kb", kb] = 0
    for what in sw.INVALID_KINDS:
        c["invalid", what] = 0
    for i in range(3):
        c["id_base", i] = 0
    for cell in (("merge", "G*k <= 8192"), ("merge", "G*k > 8192"), ("lex merge", "G*kb <= 8192"),
                 ("lex merge", "G*kb > 8192"), ("shards", "some n == 0"), ("shards", "every n < k"),
                 ("shards", "some n == 1"), ("split", "local kb larger"), ("split", "Q = NULL"), ("split", "with Q"),
                 ("prescored", "strays"), ("prescored", "plain"), ("prescored", "between"), ("prescored", "kb = 0"),
                 ("prescored", "misses > 0"), ("retrieve", "finish"), ("retrieve", "finish_host"),
                 ("retrieve", "C > 1024"), ("retrieve", "begin kb larger"), ("lq", "!= 32"), ("n < G",),
                 ("shards", "a non-empty shard of empty docs only"), ("fp32, a shard of empty docs only", "k < n"),
                 ("fp32, a shard of empty docs only", "k >= n")):
        c[cell] = 0
    for w in walks:
        c["family G", wk.scan_family(w.kind, w.ld), w.G] += 1
        c["G cut", w.G, w.cut_class] += 1
        c["id_base", 0 if w.id_base == 0 else (1 if w.id_base == 1000 else 2)] += 1
        c["n < G",] += w.n < w.G
        sizes = np.diff(w.cuts)
        for st in w.steps:
            ep = st["ep"]
            c["triple", ep, w.kind, w.ld] += 1
            if ep in sw.STEP_EPS:
                c["G step", w.G, ep] += 1
                c["cut step", w.cut_class, ep] += 1
                c["B", wk.scan_family(w.kind, w.ld), st["B"]] += 1
                c["lq", "!= 32"] += st["lq"] != 32
            if ep == "invalid":
                c["invalid", st["what"]] += 1
    for w, st in _searches(walks):
        sizes, k, kb, ep = np.diff(w.cuts), st["k"], st["kb"], st["ep"]
        c["k", wk.k_class(k, w.n)] += 1
        c["family k", wk.scan_family(w.kind, w.ld), wk.k_class(k, w.n)] += 1
        c["k step", wk.k_class(k, w.n), ep] += 1
        c["family kb", wk.scan_family(w.kind, w.ld), kb] += 1
        c["kb step", kb, ep] += 1
        if w.cut_class == "empty_docs":                          # the fp32 bound over a shard of (-inf, valid id) lists
            c["shards", "a non-empty shard of empty docs only"] += 1
            if w.kind == "fp32":
                c["fp32, a shard of empty docs only", "k < n" if k < w.n else "k >= n"] += 1
        if ep == "prescored" and st["strays"]:                   # counted on the model's answer
            c["prescored", "misses > 0"] += int(sw.expected(w, pools[w.kind, w.ld], st)["misses"][0] > 0)
        if ("k value", k) in c:
            c["k value", k] += 1
        if ("kb", kb) in c:
            c["kb", kb] += 1
        c["merge", "G*k <= 8192" if w.G * k <= sw.MERGE_MAX else "G*k > 8192"] += 1
        if kb:
            c["lex merge", "G*kb <= 8192" if w.G * kb <= sw.MERGE_MAX else "G*kb > 8192"] += 1
        c["shards", "some n == 0"] += bool((sizes == 0).any())
        c["shards", "some n == 1"] += bool((sizes == 1).any())
        c["shards", "every n < k"] += bool((sizes < k).all())
        if "kb_local" in st:
            c["split", "local kb larger"] += st["kb_local"] > kb
            c["split", "with Q" if st["with_q"] else "Q = NULL"] += 1
        if ep == "prescored":
            c["prescored", "strays" if st["strays"] else "plain"] += 1
            c["prescored", "between"] += "between" in st
            c["prescored", "kb = 0"] += kb == 0
        if ep == "retrieve_sharded":
            c["retrieve", st["how"]] += 1
            c["retrieve", "C > 1024"] += st["C"] > 1024
            c["retrieve", "begin kb larger"] += st["kb_begin"] > kb
    return c


def test_coverage_condition(walks, pools):
    c = coverage(walks, pools)
    low = sorted((str(cell), v) for cell, v in c.items() if v < LEAST)
    table = "\n".join(f"{v:5d}  {cell}" for cell, v in sorted((str(k), v) for k, v in c.items()))
    assert not low, f"{len(low)} cells visited fewer than {LEAST} times: {low[:40]}\n{table}"
    # no drawn step is dropped as "not applicable": every step kind is legal for every walk
    for w in walks:
        assert 7 <= len(w.steps) <= 9 and w.steps[0]["ep"] == "set_options"
        assert all(st["ep"] in sw.STEP_EPS + ("set_options", "invalid") for st in w.steps), w.name
        assert all(len(st["opts"]) == w.G and len(set(st["opts"])) > (w.G > 1) for st in w.steps), "ranks differ"


def test_seed_count_is_minimal(pools):
    """One seed fewer per (kind, ld) leaves a cell short."""
    walks = [sw.generate(*key) for key in sw.committed(sw.SEEDS - 1)]
    low = [cell for cell, v in coverage(walks, pools).items() if v < LEAST]
    assert low, f"{sw.SEEDS - 1} seeds would do"
    assert not [cell for cell, v in coverage([sw.generate(*key) for key in sw.committed()], pools).items() if v < LEAST]


def test_the_old_seed_lists_are_untouched():
    import _walk_seeds as ws
    assert ws.SEEDS == {"bf16": 45, "mxfp8": 36, "fp32": 50} and ws.LARGE_SEEDS == {"bf16": 14, "mxfp8": 17, "fp32": 14}
    assert ws.TRANSCRIPTS_SHA256 == "c7c1e13e99c58959520f4cbb893bfa2bd6b4d40601632d73b4cf8c3c22dfc27e"


# ---------------------------------------------------------------------------- sensitivity
def test_honest_backend_passes_every_walk(walks, pools):
    for w in walks:
        sw.play(w, pools[w.kind, w.ld], Brute())


def test_honest_backend_passes_on_a_real_pool():
    pool = wk.exact_pool("fp32", 128)
    for key in sw.committed():
        if key[:2] == ("fp32", 128):
            sw.play(sw.generate(*key), pool, Brute())


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(walks, pools, name):
    caught = []
    for w in walks:
        try:
            sw.play(w, pools[w.kind, w.ld], _mutant(name)())
        except sw.ShardedFailure as e:
            ep = w.steps[e.index]["ep"]
            assert ep in MUTANTS[name], \
                f"mutant {name} was blamed on step {e.index} ({ep}), which does not run the mutated code:\n{e}"
            assert f"fails at step {e.index} on rank {e.rank}" in str(e) and sw.render(e.index, w.steps[e.index]) in str(e)
            caught.append((w.name, e.index, ep))
            if len(caught) == 3:
                break
    assert caught, f"no committed sharded walk fails through mutant {name}"


@pytest.mark.parametrize("name", HARMLESS)
def test_harmless_mutant_passes(walks, pools, name):
    """Over the walks that run the mutated code: every faithful walk / every walk of ld = 128."""
    for w in walks:
        if w.kind == "fp32" if name == "union_kth_own_shard" else w.ld == 128:
            sw.play(w, pools[w.kind, w.ld], _mutant(name)())


def test_failure_message_names_walk_step_rank_and_bits(walks, pools):
    for w in walks:
        try:
            sw.play(w, pools[w.kind, w.ld], _mutant("merge_ties_by_shard_order")())
        except sw.ShardedFailure as e:
            text = str(e)
            assert f"walk {w.name} fails at step {e.index} on rank {e.rank}" in text and sw.header(w) in text
            assert text.count("\n") == e.index + 2
            assert "first at (row " in text and "got " in text and "want " in text
            return
    pytest.fail("no walk failed")
