"""CPU: the big-batch walks of tests/_bigbatch.py pinned -- the batch-size table
is what the restated dispatch gives, the walks visit every (entry point, B
class) cell and every side of every gate, the model's one-period shortcut
equals the row-by-row answer, and the walks can SEE the bugs they are for: the
brute-force backend of tests/test_walk_model.py passes every walk, and each of
four mutants of it fails one, at a step that runs the mutated code.

The backend answers one period of a step's rows by sorting Python tuples (as in
tests/test_walk_model.py) and lays the rows out by its own row map, which the
mutants bend.
"""
import numpy as np
import pytest

import _bigbatch as bb
import _exact as ex
import _walk as wk
from test_walk_model import Brute

TWO32 = 1 << 32


class BigBrute(Brute):
    """Brute for steps of more rows than the pool has queries: the first P rows
    answered by Brute, row b of the output taken from row ``source(b)``."""
    name = None

    def source(self, B):
        return np.arange(B) % self.w.Bp

    def rank(self, scores, ids, k, tie=None):
        if len(scores) <= 8192 or tie is not None or type(self).tie is not Brute.tie:
            return Brute.rank(self, scores, ids, k, tie)
        ks = np.asarray(self.keys(scores), np.int64)           # long rows: a stable sort on (key desc, id asc)
        return np.lexsort((np.asarray(ids, np.int64), -ks))[:k].tolist()

    def invalid(self, step):
        if step["what"].startswith("B"):
            return {"rc": wk.EINVAL if step["B"] > 65535 and step["on"] in bb.BOUNDED[self.w.kind] else 0}
        return Brute.invalid(self, step)

    def after(self, step, out):
        return out

    def call(self, i, step):
        sub = wk.one_period(self.w, step)
        if sub is None:
            return Brute.call(self, i, step)
        per = Brute.call(self, i, sub)                         # (the call between comes back through this method)
        src = self.source(step["B"])
        out = {name: x if name in ("rc", "between") else np.ascontiguousarray(np.asarray(x)[src]) for name, x in per.items()}
        return self.after(step, out)


class Wrap16(BigBrute):
    """A row index kept in 16 bits."""
    name, eps = "row index wrapped at 2^16", bb.SELECTIONS + bb.UNBOUNDED_SCANS
    plays = staticmethod(lambda w: any(st.get("B", 0) > 65536 for st in w.steps))

    def source(self, B):
        return (np.arange(B) & 0xFFFF) % self.w.Bp


class Past2048(BigBrute):
    """A launch that covers 2048 rows (64 groups of 32) and leaves the rest."""
    name, eps = "rows past 2048 left unwritten", None
    plays = staticmethod(lambda w: w.cls == "gate")

    def after(self, step, out):
        for name, x in out.items():
            if name not in ("rc", "between") and len(x) > 2048:
                x[2048:] = np.nan if x.dtype == np.float32 else wk.POISON_I
        return out


class Truncated(BigBrute):
    """The offset b * n of a score row kept in 32 bits: the row of scores a
    selection reads starts at (b * n) mod 2^32 of the [B][n] matrix."""
    name, eps = "b * n truncated to 32 bits", ("search",)
    plays = staticmethod(lambda w: w.n * 65534 >= TWO32)

    def after(self, step, out):
        w, n = self.w, self.w.n
        if step["ep"] != "search" or (step["B"] - 1) * n < TWO32:
            return out
        for b in range(-(-TWO32 // n), step["B"]):
            r, c = divmod((b * n) % TWO32, n)
            rows = [self.pool.ref[(step["q0"] + x) % w.Bp, step["lq"] - 1][w.sel] for x in (r, r + 1)]
            s, i = self.topk([np.concatenate([rows[0][c:], rows[1][:c]])], list(range(n)), step["k"], w.id_base)
            out["scores"][b], out["ids"][b] = s[0], i[0]
        return out


class SharedTail(BigBrute):
    """One tail counter for all query groups from the 64th on: each tail task
    is taken by one of them, and the docs past the static part are scored for
    none of the others' rows (here: for none of them)."""
    name, eps = "a tail counter shared by groups 64 and above", ("score",)
    plays = staticmethod(lambda w: w.cls == "gate" and w.kind != "fp32")

    def after(self, step, out):
        w = self.w
        if step["ep"] != "score" or w.kind == "fp32" or step["B"] <= 16:
            return out
        p = bb.plan(w.kind, w.ld, w.n, step["B"], self.opts["DYNAMIC_TAIL"])
        if p["dynamic_tail"] and p["groups"] > 64:
            out["scores"][64 * p["qpb"]:, p["static_docs"]:] = np.nan
        return out


MUTANTS = (Wrap16, Past2048, Truncated, SharedTail)


# ---------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def walks():
    return bb.all_walks()


@pytest.fixture(scope="module")
def pools():
    return {(kind, ld): wk.synthetic_pool(kind, ld) for kind in ex.KINDS for ld in wk.LDS}


# ---------------------------------------------------------------------------- the table
def test_batch_size_table_is_the_dispatch():
    for kind in ex.KINDS:
        q = 64 if kind == "mxfp8" else 32
        for ld in wk.LDS:
            assert bb.gate_edges(kind, ld) == [64 * q, 64 * q + 1], (kind, ld)
            assert bb.over_target(kind, ld) == q * bb.CUS + 1
            bb.check_gates_flip(kind, ld, 300)
            for B in (255, 256, 2048, 2049, 4096, 4097, 8193, 16385, 65535):
                assert bb.scan_shape(kind, ld, B)[0] == (32 if kind == "mxfp8" and ld == 128 and B == 257 else q)
        assert bb.gate_edges(kind, 128, slices=1) == [512 * q, 512 * q + 1]
    assert bb.scan_shape("mxfp8", 128, 257)[:2] == (32, 2)     # 9 groups of 4 x 8 beat 5 of 8 x 8
    assert bb.scan_shape("bf16", 128, 1024)[0] == 32           # no scan picks a 16-query workgroup there
    assert bb.over_target("bf16", 128, cus=304) == 32 * 304 + 1


def test_walks_are_deterministic(walks):
    assert wk.transcripts_hash(bb.all_walks()) == wk.transcripts_hash(walks)
    for w in walks:
        assert w.steps[0]["ep"] == "set_options" and w.n <= 600 or w.cls == "large-n"
        for _, _, st in bb.steps_of([w]):
            if "B" in st and st["ep"] != "invalid":
                assert st["tile"] == 1
                assert st["lq"] <= (4 if st["B"] >= 65535 else 32)
                assert st.get("k", 1) <= 104 or not dict(zip(wk.OPT_NAMES, st["opts"]))["FUSED_TOPK"]
        for row in w.batches:
            assert all(row[b] == bb.CYCLE[b % 5] for b in range(len(row))) and w.Bp % 5 == 0


# ---------------------------------------------------------------------------- coverage
def test_every_cell_and_every_gate_side_is_visited(walks):
    c = bb.coverage(walks)
    missing = sorted(cell for cell in bb.required_cells() if not c[cell])
    assert not missing, f"cells no walk visits: {missing}\n{sorted(c.items(), key=str)}"
    g = bb.gate_steps(walks)
    for kind, ld, cls in bb.cases():
        for gate in bb.required_gates(kind, ld, cls):
            assert g[(kind, ld) + gate] >= 1, (kind, ld, gate)
    # classes 256 / gate / cu: every (kind, ld, entry point, B) under both positions of the switches it reads
    both = {}
    for w, _, st in bb.steps_of([w for w in walks if w.cls in ("256", "gate", "cu")]):
        if "B" in st and st["ep"] != "invalid":
            o = dict(zip(wk.OPT_NAMES, st["opts"]))
            for nm in ("FUSED_TOPK", "TOPK_BMAX", "BAND_DOC_MAJOR", "RESCORE_SPLIT"):
                if st["ep"] in wk.READS[nm]:
                    both.setdefault((w.kind, w.ld, st["ep"], st["B"], nm), set()).add(o[nm])
    assert both and all(len(v) == 2 for v in both.values()), [key for key, v in both.items() if len(v) != 2][:10]
    # the switches that read B, on both sides, in a step that reads them
    seen = set()
    for w, _, st in bb.steps_of(walks):
        if "B" in st and st["ep"] != "invalid":
            o = dict(zip(wk.OPT_NAMES, st["opts"]))
            cls = bb.b_class(w.kind, w.ld, st["B"], n=w.n)
            seen |= {(nm, o[nm], cls) for nm in ("DYNAMIC_TAIL", "FUSED_TOPK", "TOPK_BMAX", "BAND_DOC_MAJOR", "RESCORE_SPLIT")
                     if st["ep"] in wk.READS[nm]}
    for cls in ("256", "gate", "cu", "max"):
        for nm, vals in (("DYNAMIC_TAIL", (0, 1, 2)), ("FUSED_TOPK", (0, 1)), ("TOPK_BMAX", (0, 1)),
                         ("BAND_DOC_MAJOR", (0, 3)), ("RESCORE_SPLIT", (0, 1))):
            for v in vals:
                assert (nm, v, cls) in seen, (nm, v, cls)
    assert {("TOPK_BMAX", 0, "large-n"), ("TOPK_BMAX", 1, "large-n"), ("FUSED_TOPK", 1, "large-n")} <= seen


# ---------------------------------------------------------------------------- the model's shortcut
def test_tiled_expectation_equals_row_by_row_at_257(pools):
    """One period repeated = every row answered on its own, byte for byte."""
    def same(x, y, where):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), where
            for name in x:
                same(x[name], y[name], where + (name,))
        elif isinstance(x, tuple):
            assert x[0] == y[0] and x[2] == y[2] and np.array_equal(x[1], y[1]), where
        elif isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), where
        else:
            assert x == y, where

    for kind in ex.KINDS:
        w = bb.class_walk(kind, 128, "256")
        pool = pools[kind, 128]
        checked = set()
        for st in w.steps:
            if st.get("B") == 257:
                tiled = wk.expected(w, pool, st)
                assert len(tiled["scores"]) == 257
                same(tiled, wk.expected(w, pool, st, tiled=False), (kind, st["ep"]))
                checked.add(st["ep"])
        assert checked == set(wk.entry_points(kind)), (kind, checked)


# ---------------------------------------------------------------------------- sensitivity
def _light(walks):
    return [w for w in walks if w.cls != "large-n"]            # 70003-doc rows: the model's partition path, pinned by
                                                               # test_walk_model.test_key_topk_is_oracle_topk_...


def test_honest_backend_passes_every_walk(walks, pools):
    for w in _light(walks):
        wk.play(w, pools[w.kind, w.ld], BigBrute())
    w = bb.truncation_walk()
    wk.play(w, pools[w.kind, w.ld], BigBrute())


def test_honest_backend_passes_a_large_n_walk(pools):
    w = bb.large_n_walk("bf16")
    wk.play(w, pools["bf16", 128], BigBrute())


@pytest.mark.parametrize("cls", MUTANTS, ids=[m.__name__ for m in MUTANTS])
def test_mutant_is_caught(walks, pools, cls):
    caught = []
    for w in [w for w in _light(walks) + [bb.truncation_walk()] if cls.plays(w)]:   # the walks that run the mutated code
        try:
            wk.play(w, pools[w.kind, w.ld], cls())
        except wk.WalkFailure as e:
            st = w.steps[e.index]
            if "the call between begin and finish" in str(e):
                st = st["between"]
            assert cls.eps is None or st["ep"] in cls.eps, \
                f"mutant '{cls.name}' was blamed on step {e.index} ({st['ep']}), which does not run the mutated code:\n{e}"
            assert f"fails at step {e.index}" in str(e) and wk.render(e.index, w.steps[e.index]) in str(e)
            caught.append((w.name, e.index, st["ep"]))
            if len(caught) == 2:
                break
    assert caught, f"no big-batch walk fails through mutant '{cls.name}'"
