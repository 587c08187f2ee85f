"""The one-round-trip retrieve's exact CPU pipeline (test infrastructure).

On a GridCorpus (tests/_grid.py) every MaxSim score is exact in fp32, so the
bf16, the fp32-faithful and the MXFP8 index share ONE expectation, computed
here without the library: ``g.topk(k)`` (stage 2) -> ``orc.rrf`` over the
stage-1 list and the ColBERT list, ids < 0 stripped as cbv2_rrf_fuse
documents, cut to ``[:C]`` and padded with -1 (LRC:960-978, :916) ->
``g.exact_scores`` of the C candidates (-inf for an id < 0, an id at or past N
and an empty doc) -> ``orc.rerank_select`` (score desc, position asc;
LRC:789-798).  Output: scores, ids, positions ``[B][final_k]``, rows past C
padded with -inf / -1 / -1.

Two corpora, each checked by assertions on the CPU when it is built:
* ``corpus_a`` "ranked-all": 256 docs, 8 queries, three docs emptied, used
  with k = N -- so NEGATIVE finite scores (their bits have the top bit set,
  like a call's tag), -inf scores and exact ties pass through every stage;
* ``corpus_b`` "top-k": 4000 docs, 40 queries, a positive top-100 with ties.

``stage1_lists`` builds the stage-1 id lists by hand, one row of each kind
(ROW_KINDS); ``Runner`` drives a OneTripRetriever against the pipeline.
"""
import ctypes
from functools import lru_cache

import numpy as np

from _grid import GridCorpus
from oracle import oracle as orc

RRF_K = 60
ROW_KINDS = ("planted", "empty", "negative", "past_n", "absent", "tail", "all_pad", "repeat")
INT32_MAX = 2 ** 31 - 1


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


class Corpus:
    """A GridCorpus with its whole ranking (scores desc, id asc) per query."""

    def __init__(self, g: GridCorpus, name: str):
        self.g, self.name, self.N, self.B = g, name, g.N, g.B
        self.rank_s, self.rank_i = g.topk(g.N)          # [B, N]: every doc, -inf (empty docs) last
        self.empty = np.nonzero(g.doclens == 0)[0]
        self._topk = {}

    def topk(self, k: int):
        """g.topk(k), padded with -inf / -1 past N (as the search pads)."""
        if k not in self._topk:
            kk = min(k, self.N)
            s = np.full((self.B, k), -np.inf)
            i = np.full((self.B, k), -1, np.int64)
            s[:, :kk], i[:, :kk] = self.g.topk(kk)
            self._topk[k] = (s, i)
        return self._topk[k]

    def row_stats(self, b: int, k: int):
        """(negative finite scores, -inf scores, exact adjacent ties) in row b's top-k."""
        s = self.topk(k)[0][b]
        fin = s[np.isfinite(s)]
        return int((fin < 0).sum()), int(np.isneginf(s).sum()), int((np.diff(fin) == 0).sum())


@lru_cache(maxsize=None)
def corpus_a() -> Corpus:
    g = GridCorpus(256, 8, seed=5)
    planted = set(g.planted_flat.tolist())
    emptied = [d for d in range(g.N) if d not in planted and g.doclens[d] > 0][:3]
    g.doclens[emptied] = 0
    g.masks = orc.codebook_masks(g.codes, g.doclens)
    c = Corpus(g, "A")
    for b in range(c.B):                     # what the corpus is for, before any GPU call
        neg, ninf, ties = c.row_stats(b, c.N)
        assert neg >= 10 and ninf >= 3 and ties >= 20, f"corpus A row {b}: {neg} negative, {ninf} -inf, {ties} ties"
    return c


@lru_cache(maxsize=None)
def corpus_b() -> Corpus:
    c = Corpus(GridCorpus(4000, 40, seed=11), "B")
    s = c.topk(100)[0]
    assert (s > 0).all(), "corpus B: the top-100 scores should all be positive"
    ties = (np.diff(s[:8], axis=1) == 0).mean()
    assert 0.03 <= ties <= 0.2, f"corpus B: {ties:.3f} of adjacent top-100 pairs tie (B = 8)"
    assert len(c.empty) >= 1, "corpus B should hold an empty doc"
    return c


def stage1_lists(c: Corpus, rows, kb: int, k: int, rot: int = 0, low_ids: bool = False, seed: int = 0):
    """Stage-1 id lists [len(rows), kb] int32, row r of kind ROW_KINDS[(r + rot) % 8]:
    planted hits | ids of empty docs | ids with the lowest (corpus A: negative)
    scores | ids at or past N | ids absent from the ColBERT top-k | a -1 tail |
    all -1 | one id repeated.  Each row's other slots are distinct random ids
    (``low_ids``: from 1..400, so stale ids of every small value lie in the
    buffer's words, both halves)."""
    out = np.full((len(rows), kb), -1, np.int32)
    if kb == 0:
        return out
    rng = np.random.default_rng([seed, kb, k, rot, len(rows)])
    for r, b in enumerate(rows):
        kind = ROW_KINDS[(r + rot) % len(ROW_KINDS)]
        fill = rng.permutation(np.arange(1, min(c.N, 401)) if low_ids else c.N)
        top = set(c.topk(k)[1][b].tolist())
        if kind == "planted":
            head = c.g.planted[b]
        elif kind == "empty":
            head = c.empty
        elif kind == "negative":
            fin = c.rank_i[b][np.isfinite(c.rank_s[b])]
            head = fin[-min(12, kb):][::-1]
        elif kind == "past_n":
            head = np.array([c.N, c.N + 7, INT32_MAX, 2 * c.N])
        elif kind == "absent":
            head = np.array([d for d in fill if d not in top][:max(1, kb // 2)], np.int64)
        else:
            head = np.zeros(0, np.int64)
        row = list(dict.fromkeys([int(x) for x in head] + [int(x) for x in fill]))[:kb]
        row += [-1] * (kb - len(row))
        if kind == "tail":
            row[(kb + 1) // 2:] = [-1] * (kb - (kb + 1) // 2)
        elif kind == "all_pad":
            row = [-1] * kb
        elif kind == "repeat" and kb >= 3:
            row[kb // 2] = row[0]             # the reference's dict adds both ranks
        out[r] = row
    return out


def pipeline(c: Corpus, rows, lex, k: int, C: int, final_k: int, cand_out=None):
    """-> (scores float32 [B, final_k], ids int32, positions int32) of queries
    ``rows``; cand_out (a list): the fused candidate rows [C] are appended to it."""
    B = len(rows)
    out_s = np.full((B, final_k), -np.inf, np.float32)
    out_i = np.full((B, final_k), -1, np.int32)
    out_p = np.full((B, final_k), -1, np.int32)
    ei = c.topk(k)[1]
    for r, b in enumerate(rows):
        l1 = [] if lex is None else [int(x) for x in lex[r] if x >= 0]
        l2 = [int(x) for x in ei[b] if x >= 0]
        fused = [cid for cid, _ in orc.rrf(l1, l2, k=RRF_K)[:C]]
        fused += [-1] * (C - len(fused))
        if cand_out is not None:
            cand_out.append(fused)
        sc = c.g.exact_scores([b], np.array([fused]))[0]
        for j, (p, s, _) in enumerate(orc.rerank_select(sc, final_k)):
            out_s[r, j], out_i[r, j], out_p[r, j] = s, fused[p], p
    return out_s, out_i, out_p


# ---------------------------------------------------------------------- the GPU side
def pool_stats():
    """cbv2_retrieve_pool_stats: (created, idle, final-words calls, host-rerank calls)."""
    from hybrid_rag_colbertv2_amd import _lib
    st = (ctypes.c_int64 * 4)()
    _lib.lib().cbv2_retrieve_pool_stats(st, 4)
    return tuple(int(x) for x in st)


def make_index(c: Corpus, kind: str, dev):
    """(index, device queries) of corpus c as a bf16 / fp32-faithful / MXFP8 shard."""
    import torch
    from hybrid_rag_colbertv2_amd.index import ColbertIndex
    dl = c.g.doclens_on(dev)
    if kind == "fp32":
        return ColbertIndex.faithful_f32(c.g.tokens_on(dev, torch.float32), dl), torch.from_numpy(c.g.Q).to(dev)
    t = c.g.tokens_on(dev)
    ix = ColbertIndex.mxfp8(t, dl) if kind == "mxfp8" else ColbertIndex(t, dl)
    return ix, torch.from_numpy(c.g.Q).to(dev, torch.bfloat16)


class Runner:
    """One corpus as one shard: OneTripRetriever calls against ``pipeline``."""

    def __init__(self, c: Corpus, kind: str, dev):
        self.c, self.kind, self.dev = c, kind, dev
        self.index, self.Q = make_index(c, kind, dev)
        self._ones, self._want, self.cands = {}, {}, {}

    def retriever(self, k, kb_cap, C, final_k):
        from hybrid_rag_colbertv2_amd.hybrid import OneTripRetriever
        key = (k, kb_cap, C, final_k)
        if key not in self._ones:
            self._ones[key] = OneTripRetriever(self.index, colbert_k=k, fused=C, final_k=final_k, rrf_k=RRF_K,
                                               lexical_k=kb_cap)
        return self._ones[key]

    def want(self, shape, b0, B, rot=0, low_ids=False):
        """(stage-1 lists, pipeline result) of queries b0, b0 + 1, ... (B of
        them, cycling through the corpus's queries); computed once, shared."""
        k, _, kb_ret, C, final_k = shape
        key = (shape, b0, B, rot, low_ids)
        if key not in self._want:
            rows = [(b0 + r) % self.c.B for r in range(B)]
            lex = stage1_lists(self.c, rows, kb_ret, k, rot=rot, low_ids=low_ids) if kb_ret > 0 else None
            cand = []
            res = pipeline(self.c, rows, lex, k, C, final_k, cand_out=cand)
            for x in res + ((lex,) if lex is not None else ()):
                x.setflags(write=False)
            self._want[key] = (lex, res)
            self.cands[key] = np.array(cand, np.int32)      # [B, C]: the fused candidates
        return self._want[key]

    def call(self, shape, b0, B, mode="callable", host=False, rot=0, low_ids=False):
        """One call of shape (k, kb_cap, kb_returned, C, final_k) on B queries
        from b0 on; mode "callable" / "array" (host ids; a callable where
        kb_cap != kb_returned).  -> list of problems (empty: equal to the oracle)."""
        import torch
        k, kb_cap, kb_ret, C, final_k = shape
        lex, want = self.want(shape, b0, B, rot, low_ids)
        rows = torch.tensor([(b0 + r) % self.c.B for r in range(B)], device=self.dev)
        Q = self.Q.index_select(0, rows).contiguous()
        if lex is None:
            none = (np.zeros((B, 0), np.int32), np.zeros((B, 0), np.float32))
            lexical = (lambda: none) if mode == "callable" else None
        elif mode == "array" and kb_cap == kb_ret:
            lexical = lex
        else:
            lexical = lambda: (lex, np.zeros(lex.shape, np.float32))   # noqa: E731
        one = self.retriever(k, kb_cap if (lexical is None or callable(lexical)) else kb_ret, C, final_k)
        got = one(Q, lexical, host=host)
        bad = []
        if host:
            dev_out = [x.cpu().numpy() for x in one._dev_out[1:]]
            for g, d, name in zip(got, dev_out, ("scores", "ids", "positions")):
                if not np.array_equal(bits(g) if name == "scores" else g, bits(d) if name == "scores" else d):
                    bad.append(f"host {name} differ from the device outputs")
        else:
            got = [x.cpu().numpy() for x in got]
        for g, w, name in zip(got, want, ("scores", "ids", "positions")):
            gg, ww = (bits(g), bits(w)) if name == "scores" else (np.asarray(g), w)
            if not np.array_equal(gg, ww):
                r = int(np.argwhere(gg != ww)[0][0])
                bad.append(f"{name} differ from the oracle in {int((gg != ww).sum())} places; row {r}: got "
                           f"{np.asarray(g)[r].tolist()[:12]} want {w[r].tolist()[:12]}")
        return bad
