"""GPU: the committed walks of tests/_walk.py played through the C ABI and
compared with the exact model after every step, bit for bit.

What the other GPU tests cannot see and a walk can: option VECTORS (all 17
handle options drawn together and changed on a live handle between calls),
state that outlives a call (one handle, one workspace that keeps what the
previous call left, one query buffer whose contents change at the same
address, filters / filter batches / groupings reused across option changes)
and B, lq, k and n varied together over the edge lists.  The corpora are exact
(tests/_exact.py), so there is no tolerance anywhere.

Buffers of a walk: ONE persistent workspace, filled with 0xA5 at the walk's
start and then left as the calls leave it (every fourth walk re-poisons it
before each step instead), each call given its first *_workspace_size bytes
under the options in force; ONE query buffer overwritten in place; outputs
filled with NaN / -7 before every call.  After a mismatch (never after a
fault) the failing step alone is replayed on a fresh index and a fresh zeroed
workspace; the message says whether it passes there ("state-dependent") or
fails again ("call-dependent").

CBV2_WALK_SEEDS="kind:ld:seed,..." (":large" appended for a large walk) makes
test_small_walks / test_large_walks play those walks of their (kind, ld) in
place of the committed ones.

REGRESSIONS lists the walks that found a bug, by name.

Run time, measured on an MI355X.  The twelve pools (tests/_exact.cached_corpus,
shared with tests/test_gpu_exact_scores.py) cost 0.7-1.9 s each on that box and
fall to whichever test of a session first needs them: in the suite's order the
other file runs first, and its slowest test is
test_score_equals_exact_reference[fp32-1024], 1.83-1.98 s, all but 0.01 s of
it the pool.
  this file alone (box clock 2026-10-21T03:12Z, 37 tests, 27.5 s):
    test_small_walks   45 / 36 / 50 walks each, the pool included: bf16 2.54
                       (the first GPU work of the process), 1.40, 1.15, 1.93 s
                       at ld = 128 ... 1024; MXFP8 1.53, 1.35, 1.17, 2.07 s;
                       fp32 1.73, 1.64, 1.43, 2.40 s -- the pool plus 0.3-0.9 s
                       of walks (2 ms per step, the model's numpy included), so
                       run alone the 1024-slot cases exceed the other file's
                       slowest test by the walks' own time
    test_large_walks   two walks each (LARGE_PART): 0.03-0.77 s (one test per
                       kind took 7.9 s for 19 faithful walks at 70,003 docs,
                       four walks per test up to 3.4 s, hence two)
    test_regression_walks  under 0.01 s each
  after tests/test_gpu_exact_scores.py in one session (the earlier seed list,
  2 ms per step as now): every test_small_walks case 0.24-0.54 s.
"""
import os
import time

import numpy as np
import pytest
import torch

import _exact as ex
import _padding as pad
import _walk as wk
import _walk_seeds as ws
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocFilter, DocGroups, FilterBatch, _stream_ptr, quantize_mxfp8

pytestmark = pytest.mark.gpu

WS_SMALL, WS_LARGE = 96 << 20, 256 << 20
Q_BYTES = 65 * 33 * 128 * 4                     # 65 queries of 33 tokens (the invalid lq = 33), f32
HOST_BYTES = 4 << 20
# The walks that found a bug, written out (the generator may change; these steps stay):
#   host words of a spent launch   cbv2_retrieve_finish_host of 3 queries under CBV2_OPT_RESCORE_SPLIT = 0 (first seen
#       at step 10 of a generated bf16 / 128 walk, these options and arguments): the pre-armed rerank takes no tagged
#       candidates on the one-pair-per-wave path, so it ran on whatever the workspace held and its select stored
#       final words under the call's tag; the host read those (-inf from a poisoned workspace, doc 0's score from a
#       zeroed one) while the device outputs were right.  Both finish forms and both faithful / bf16 shards.
_SPENT = (2, 0, 0, 1, 0, 0, 0, 0, 0, 64, 1, 1, 0, 2, 0, 1, 2)
_RETRIEVE = dict(ep="retrieve", ds=182449841, B=3, lq=16, q0=57, k=10, kb=10, C=1, final_k=1)
REGRESSIONS = tuple(
    (kind, 128, 16, [dict(ep="set_options", values=_SPENT), dict(_RETRIEVE, how="finish_host"),
                     dict(_RETRIEVE, ds=7, q0=3, C=20, final_k=7, how="finish_host"), dict(_RETRIEVE, how="finish")],
     "host words of a spent launch") for kind in ("bf16", "fp32"))


class PoolDev:
    """A pool on the device, laid out as its index kind stores it, for gathers.
    ``padding`` ("nan" / "inf", tests/_padding.py): the padding rows of the
    device arrays are overwritten once, after construction; the bounds stay
    those of the clean split."""

    def __init__(self, pool, dev, padding=None):
        c = pool.corpus
        self.Q = torch.from_numpy(c.queries_f32()).to(dev)                   # [B, 32, 128] f32
        x = torch.from_numpy(c.docs_f32()).to(dev)
        self.doclens = torch.from_numpy(c.doclens.astype(np.int32)).to(dev)
        self.bounds = None
        if pool.kind == "fp32":
            ix = ColbertIndex.faithful_f32(x, self.doclens)
            self.tokens, self.extra, self.bounds = ix.tokens, ix.residual, ix.bounds
            torch.cuda.synchronize()
            ix.close()
        elif pool.kind == "mxfp8":
            self.tokens, self.extra = quantize_mxfp8(x)
        else:
            self.tokens, self.extra = x.to(torch.bfloat16), None
        if padding is not None:
            self.tokens, self.extra = pad.poison(pool.kind, self.tokens, self.extra, self.doclens, padding)
        torch.cuda.synchronize()

    def index(self, sel, id_base):
        s = torch.from_numpy(np.asarray(sel, np.int64)).to(self.tokens.device)
        tok, dl = self.tokens.index_select(0, s), self.doclens.index_select(0, s)
        if self.bounds is not None:
            return ColbertIndex(tok, dl, id_base=id_base, residual=self.extra.index_select(0, s), bounds=self.bounds)
        if self.extra is not None:
            return ColbertIndex(tok, dl, id_base=id_base, scales=self.extra.index_select(0, s))
        return ColbertIndex(tok, dl, id_base=id_base)


_pool_devs = {}


def pool_dev(kind, ld, dev, padding=None):
    if (kind, ld, padding) not in _pool_devs:
        _pool_devs[kind, ld, padding] = PoolDev(wk.exact_pool(kind, ld), dev, padding)
    return _pool_devs[kind, ld, padding]


class Buffers:
    """q_bytes / host_bytes: the query buffer and the pinned host buffer of
    walks with larger batches than 65 (tests/test_gpu_bigbatch.py)."""

    def __init__(self, dev, ws_bytes, q_bytes=Q_BYTES, host_bytes=HOST_BYTES):
        self.ws = [torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.q = torch.zeros((q_bytes,), dtype=torch.uint8, device=dev)
        self.host = torch.empty((host_bytes,), dtype=torch.uint8, pin_memory=True)
        assert all(t.data_ptr() % 256 == 0 for t in self.ws + [self.q])
        self.poison()

    def poison(self, which=(0, 1)):
        for j in which:
            self.ws[j].fill_(0xA5)


class Gpu:
    """Plays a walk's steps through the C ABI.  ``padding``: on a pool whose
    padding rows hold that mode's non-finite values, and with the query buffer
    past each step's B * lq rows filled with them (tests/_padding.query_tail),
    so that a kernel reading a query row too many meets a NaN and not the
    previous step's finite queries."""

    def __init__(self, dev, bufs, repoison=False, zeroed=False, padding=None):
        self.dev, self.bufs, self.repoison, self.zeroed, self.padding = dev, bufs, repoison, zeroed, padding
        self.L = _lib.lib()
        self.ix = None
        self.qtail = None

    # ----- the player's interface
    def start(self, w, pool, opts=None):
        self.w, self.pool = w, pool
        self.pd = pool_dev(w.kind, w.ld, self.dev, self.padding)
        if self.padding is not None:
            self.qtail = torch.from_numpy(pad.query_tail(w.kind, self.padding, self.bufs.q.numel())).to(self.dev)
        self.ix = self.pd.index(w.sel, w.id_base)
        self.h = self.ix._h
        self.faithful = w.kind == "fp32"
        self.qdt = {"bf16": _lib.DTYPE_BF16, "mxfp8": _lib.DTYPE_MXFP8, "fp32": _lib.DTYPE_F32}[w.kind]
        self.set_options(w.steps[0]["values"] if opts is None else opts)   # the batches' chunk size is read at create
        self.filters = [DocFilter(self.ix, torch.from_numpy(f.words.view(np.int32)).to(self.dev)) for f in w.filters]
        self.all = self.ix.all_docs_filter()
        self.batches = [FilterBatch(self.ix, [self.all if f is None else self.filters[f] for f in row])
                        for row in w.batches]
        self.groups = [DocGroups(self.ix, torch.from_numpy(gof), G) for _, gof, G in w.groupings]
        for f, ff in zip(w.filters, self.filters):
            assert ff.count == int(f.mask.sum()), "cbv2_filter_count"
        if self.zeroed:
            for t in self.bufs.ws:
                t.zero_()
        else:
            self.bufs.poison()
        self.keep = []

    def finish(self):
        torch.cuda.synchronize()
        for hs in (getattr(self, "batches", ()), getattr(self, "filters", ()), getattr(self, "groups", ())):
            for x in hs:
                x.close()
        if self.ix is not None:
            if getattr(self, "all", None) is not None:
                self.all.close()
            self.ix.close()
            self.ix = None

    def same(self, got, want):
        if isinstance(got, np.ndarray):
            return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
        x = torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).to(self.dev)
        return tuple(got.shape) == want.shape and torch.equal(got.contiguous().view(torch.int32), x)

    def host(self, got):
        return got if isinstance(got, np.ndarray) else got.cpu().numpy()

    def untouched(self, arr):
        bits = arr.view(torch.int32)
        want = int(np.float32(np.nan).view(np.int32)) if arr.dtype == torch.float32 else wk.POISON_I
        return bool((bits == want).all())

    def diagnose(self, i, step, want):
        """The failing step alone on a fresh index and a fresh zeroed workspace."""
        torch.cuda.synchronize()
        fresh = Gpu(self.dev, Buffers(self.dev, self.bufs.ws[0].numel(), self.bufs.q.numel(), self.bufs.host.numel()),
                    zeroed=True, padding=self.padding)
        try:
            fresh.start(self.w, self.pool, opts=step["opts"])
            msg = wk.compare(fresh, fresh.call(i, step), want)
        finally:
            fresh.finish()
        return "state-dependent: the step alone on a fresh index and a zeroed workspace passes" if msg is None else \
            f"call-dependent: the step alone on a fresh index and a zeroed workspace fails too ({msg})"

    # ----- pieces
    def set_options(self, values):
        for (name, oid, _), v in zip(wk.OPTIONS, values):
            _lib.check(self.L.cbv2_index_set_option(self.h, oid, int(v)))

    def out(self, shape, dtype=torch.float32):
        t = torch.full(shape, float("nan") if dtype == torch.float32 else wk.POISON_I, dtype=dtype, device=self.dev)
        self.keep.append(t)
        return t

    def dev_arr(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def ws(self, need, which=0):
        buf = self.bufs.ws[which]
        assert need <= buf.numel(), f"the walk's workspace is too small ({need} > {buf.numel()})"
        return buf.data_ptr(), int(need)

    def queries(self, step):
        """The step's queries written in place into the walk's one query buffer -> its pointer."""
        B, lq = step["B"], min(max(step["lq"], 1), wk.LQ_MAX)
        rows = torch.from_numpy((step["q0"] + np.arange(B)) % self.w.Bp).to(self.dev)
        Q = self.pd.Q[:, :lq].index_select(0, rows).contiguous()
        qb = self.bufs.q
        if self.w.kind == "fp32":
            qb[: Q.numel() * 4].view(torch.float32).copy_(Q.reshape(-1))
        elif self.w.kind == "bf16":
            qb[: Q.numel() * 2].view(torch.bfloat16).copy_(Q.to(torch.bfloat16).reshape(-1))
        else:
            n_rows = B * lq
            self.keep.append(Q)
            _lib.check(self.L.cbv2_quantize_mxfp8(Q.data_ptr(), _lib.DTYPE_F32, n_rows, qb.data_ptr(),
                                                  qb.data_ptr() + n_rows * 128, _stream_ptr(self.dev)))
        if self.qtail is not None:
            used = B * lq * {"fp32": 512, "bf16": 256, "mxfp8": 130}[self.w.kind]
            qb[used:].copy_(self.qtail[used:])
        return qb.data_ptr()

    # ----- the call
    def call(self, i, step, which=0):
        if which == 0:
            self.keep = []
            if self.repoison:
                self.bufs.poison()
        got = self._call(step, which)
        torch.cuda.synchronize()
        return got

    def _call(self, step, which):
        L, h, w, st = self.L, self.h, self.w, _stream_ptr(self.dev)
        ep = step["ep"]
        if ep == "set_options":
            self.set_options(step["values"])
            return {"rc": 0}
        inv = step if ep == "invalid" else None
        if inv is not None:
            ep = step["on"]
        B, k = step.get("B"), step.get("k")
        full = self.bufs.ws[which].numel() - 64

        def wsp(need):
            """(pointer, bytes) of the call's workspace; an invalid step's variations applied."""
            if inv is None:
                return self.ws(need, which)
            if inv["what"] == "ws_short":
                assert need > 0
                return self.bufs.ws[which].data_ptr(), int(need) - 1
            return self.bufs.ws[which].data_ptr() + inv["ws_offset"], (int(need) if inv["ws_offset"] else full)

        if ep in ("select_topk", "topk_rows", "merge_topk", "group_topk_rows"):
            kk = max(k, 1)
            if ep == "select_topk":
                M, ids = wk.select_inputs(w, self.pool, step)
                o = {"scores": self.out((B, kk)), "ids": self.out((B, kk), torch.int32), "pos": self.out((B, kk), torch.int32)}
                rc = L.cbv2_select_topk(self.dev_arr(M).data_ptr(), None if ids is None else self.dev_arr(ids).data_ptr(),
                                        B, step["C"], k, o["scores"].data_ptr(), o["ids"].data_ptr(), o["pos"].data_ptr(), st)
            elif ep == "topk_rows":
                M = self.dev_arr(wk.topk_inputs(w, self.pool, step))
                need = int(L.cbv2_topk_workspace_bytes(B, w.n)) if step["sampled"] else 0
                p, nb = self.ws(need, which) if need else (None, 0)
                o = {"scores": self.out((B, kk)), "ids": self.out((B, kk), torch.int32)}
                rc = L.cbv2_topk_rows(M.data_ptr(), B, w.n, M.shape[1], k, w.id_base, p, nb, o["scores"].data_ptr(),
                                      o["ids"].data_ptr(), st)
            elif ep == "merge_topk":
                _, in_s, in_i = wk.merge_inputs(w, self.pool, step)
                o = {"scores": self.out((B, kk)), "ids": self.out((B, kk), torch.int32)}
                rc = L.cbv2_merge_topk(self.dev_arr(in_s).data_ptr(), self.dev_arr(in_i).data_ptr(), step["G"], B, k,
                                       o["scores"].data_ptr(), o["ids"].data_ptr(), st)
            else:
                M = self.dev_arr(wk.topk_inputs(w, self.pool, step))
                g, r = self.groups[step["g"]], step["r"]
                p, nb = self.ws(int(L.cbv2_group_topk_workspace_size(g._h, B, k, r)), which)
                o = self.group_out(B, kk, r)
                rc = L.cbv2_group_topk_rows(g._h, M.data_ptr(), M.shape[1], B, k, r, p, nb, o["scores"].data_ptr(),
                                            o["groups"].data_ptr(), o["ids"].data_ptr(), o["chunk_scores"].data_ptr(), st)
            return dict(o, rc=rc)

        q = self.queries(step)
        lq = step["lq"]
        if ep == "score":
            o = {"scores": self.out((B, w.n))}
            if self.faithful:
                p, nb = wsp(int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SCORE, B, min(max(lq, 1), 32), 0)))
                rc = L.cbv2_score_f32(h, q, B, lq, p, nb, o["scores"].data_ptr(), w.n, st)
            else:
                rc = L.cbv2_score(h, 0, q, self.qdt, B, lq, o["scores"].data_ptr(), w.n, st)
        elif ep == "search":
            o = self.topk_out(B, max(k, 1))
            p, nb = wsp(int(L.cbv2_search_workspace_size(h, B, k, 0)))
            rc = L.cbv2_search(h, 0, q, self.qdt, B, lq, k, p, nb, o["scores"].data_ptr(), o["ids"].data_ptr(), st)
        elif ep == "search_f32":
            o = self.topk_out(B, max(k, 1), status=True)
            p, nb = wsp(int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SEARCH, B, lq, step["cap"])))
            status = None if inv is not None and inv["null_status"] else o["status"].data_ptr()
            rc = L.cbv2_search_f32(h, q, B, lq, k, step["cap"], p, nb, o["scores"].data_ptr(), o["ids"].data_ptr(),
                                   status, st)
        elif ep == "search_f32_split":
            o = self.topk_out(B, k, status=True)
            fk = self.out((B, k))
            p, nb = self.ws(int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SEARCH, B, lq, step["cap"])), 0)
            rc = L.cbv2_search_f32_begin(h, q, B, lq, k, step["cap"], p, nb, fk.data_ptr(), o["scores"].data_ptr(),
                                         o["ids"].data_ptr(), o["status"].data_ptr(), st)
            if rc == 0:
                o["between"] = self._call(step["between"], 1)  # another workspace; overwrites the query buffer
                lb = fk.min(dim=1).values.contiguous()
                self.keep.append(lb)
                rc = L.cbv2_search_f32_finish(h, B, lq, k, step["cap"], p, nb, lb.data_ptr(), o["scores"].data_ptr(),
                                              o["ids"].data_ptr(), o["status"].data_ptr(), st)
        elif ep in ("rerank", "rerank_ws", "rerank_f32"):
            cand = self.dev_arr(wk.candidates(w, step))
            C = step["C"]
            if k:
                o = {"scores": self.out((B, k)), "ids": self.out((B, k), torch.int32), "pos": self.out((B, k), torch.int32)}
                ptrs = [o[x].data_ptr() for x in ("scores", "ids", "pos")]
            else:
                o = {"scores": self.out((B, C))}
                ptrs = [o["scores"].data_ptr(), None, None]
            if ep == "rerank":
                rc = L.cbv2_rerank(h, q, B, lq, cand.data_ptr(), C, k, *ptrs, st)
            elif ep == "rerank_ws":
                p, nb = self.ws(int(L.cbv2_rerank_workspace_bytes(B, C)), which)
                rc = L.cbv2_rerank_ws(h, q, B, lq, cand.data_ptr(), C, k, p, nb, *ptrs, st)
            else:
                p, nb = self.ws(int(L.cbv2_f32_workspace_bytes(h, _lib.F32_RERANK, B, lq, C)), which)
                rc = L.cbv2_rerank_f32(h, q, B, lq, cand.data_ptr(), C, k, p, nb, *ptrs, st)
        elif ep == "search_filtered":
            f = self.filters[step["f"]]
            o = self.topk_out(B, k)
            p, nb = self.ws(int(L.cbv2_search_filtered_workspace_size(h, f._h, B, lq, k, 0)), which)
            rc = L.cbv2_search_filtered(h, f._h, 0, q, self.qdt, B, lq, k, p, nb, o["scores"].data_ptr(),
                                        o["ids"].data_ptr(), st)
        elif ep == "search_filtered_f32":
            f = self.filters[step["f"]]
            o = self.topk_out(B, k, status=True)
            p, nb = self.ws(int(L.cbv2_search_filtered_f32_workspace_size(h, f._h, B, lq, k, step["cap"])), which)
            rc = L.cbv2_search_filtered_f32(h, f._h, q, B, lq, k, step["cap"], p, nb, o["scores"].data_ptr(),
                                            o["ids"].data_ptr(), o["status"].data_ptr(), st)
        elif ep == "search_filtered_batch":
            fb = self.batches[step["fb"]]
            o = self.topk_out(B, k)
            p, nb = wsp(int(L.cbv2_search_filtered_batch_workspace_size(h, fb._h, B, lq, k, 0)))
            rc = L.cbv2_search_filtered_batch(h, fb._h, 0, q, self.qdt, B, lq, k, p, nb, o["scores"].data_ptr(),
                                              o["ids"].data_ptr(), st)
        elif ep == "search_grouped":
            g, r = self.groups[step["g"]], step["r"]
            o = self.group_out(B, k, max(r, 1))
            p, nb = wsp(int(L.cbv2_search_grouped_workspace_size(h, g._h, B, lq, k, r, 0)))
            rc = L.cbv2_search_grouped(h, g._h, 0, q, self.qdt, B, lq, k, r, p, nb, o["scores"].data_ptr(),
                                       o["groups"].data_ptr(), o["ids"].data_ptr(), o["chunk_scores"].data_ptr(), st)
        elif ep == "search_grouped_f32":
            g, r = self.groups[step["g"]], step["r"]
            o = self.group_out(B, k, r)
            o["status"] = self.out((B,), torch.int32)
            p, nb = self.ws(int(L.cbv2_search_grouped_f32_workspace_size(h, g._h, B, lq, k, r, step["cap"])), which)
            rc = L.cbv2_search_grouped_f32(h, g._h, q, B, lq, k, r, step["cap"], p, nb, o["scores"].data_ptr(),
                                           o["groups"].data_ptr(), o["ids"].data_ptr(), o["chunk_scores"].data_ptr(),
                                           o["status"].data_ptr(), st)
        elif ep == "retrieve":
            return self.retrieve(step, q, which)
        else:
            raise ValueError(ep)
        return dict(o, rc=rc)

    def topk_out(self, B, k, status=False):
        o = {"scores": self.out((B, k)), "ids": self.out((B, k), torch.int32)}
        if status:
            o["status"] = self.out((B,), torch.int32)
        return o

    def group_out(self, B, k, r):
        return {"scores": self.out((B, k)), "groups": self.out((B, k), torch.int32),
                "ids": self.out((B, k, r), torch.int32), "chunk_scores": self.out((B, k, r))}

    def retrieve(self, step, q, which):
        L, h, w, st = self.L, self.h, self.w, _stream_ptr(self.dev)
        B, lq, k, kb, C, fk = (step[x] for x in ("B", "lq", "k", "kb", "C", "final_k"))
        p, nb = self.ws(int(L.cbv2_retrieve_workspace_bytes(h, None, B, lq, k, kb, C)), which)
        rc = L.cbv2_retrieve_begin(h, None, q, self.qdt, B, lq, k, kb, C, p, nb, st)
        if rc:
            return {"rc": rc}
        if step["how"] == "cancel":                            # the caller's stage 1 failed: cancel, then a plain search
            rc = L.cbv2_retrieve_cancel(h, p, st)
            torch.cuda.synchronize()
            if rc:
                return {"rc": rc}
            plain = {"ep": "search_f32", "cap": wk.BAND_CAP} if self.faithful else {"ep": "search"}
            o = self._call(dict(step, **plain), which)
            o.pop("status", None)
            return o
        hneed = int(L.cbv2_retrieve_host_bytes(B, k, kb, C))
        assert 0 < hneed <= self.bufs.host.numel()
        lex = np.ascontiguousarray(wk.lexical_ids(w, step)) if kb else None
        o = {"scores": self.out((B, fk)), "ids": self.out((B, fk), torch.int32), "pos": self.out((B, fk), torch.int32)}
        args = (h, None, q, self.qdt, B, lq, k, lex.ctypes.data if kb else None, None, kb, wk.RRF_K, C, fk, p, nb,
                self.bufs.host.data_ptr(), self.bufs.host.numel(), o["scores"].data_ptr(), o["ids"].data_ptr(),
                o["pos"].data_ptr())
        if step["how"] == "finish_host":
            hs = np.full((B, fk), np.nan, np.float32)
            hi, hp = np.full((B, fk), wk.POISON_I, np.int32), np.full((B, fk), wk.POISON_I, np.int32)
            rc = L.cbv2_retrieve_finish_host(*args, hs.ctypes.data, hi.ctypes.data, hp.ctypes.data, st)
            o.update(host_scores=hs, host_ids=hi, host_pos=hp)
        else:
            rc = L.cbv2_retrieve_finish(*args, st)
        return dict(o, rc=rc)


# ---------------------------------------------------------------------------- the tests
_bufs = {}


def _buffers(dev, nbytes):
    if nbytes not in _bufs:
        _bufs[nbytes] = Buffers(dev, nbytes)
    return _bufs[nbytes]


def _chosen():
    """The walks named in CBV2_WALK_SEEDS, or None."""
    names = [c.strip().split(":") for c in os.environ.get("CBV2_WALK_SEEDS", "").split(",") if c.strip()]
    return [(p[0], int(p[1]), int(p[2]), len(p) > 3 and p[3] == "large") for p in names] or None


def _play(dev, keys, ws_bytes, padding=None):
    t0 = time.perf_counter()
    steps = 0
    for j, key in enumerate(keys):
        w = wk.generate(*key)
        wk.play(w, wk.exact_pool(w.kind, w.ld),
                Gpu(dev, _buffers(dev, ws_bytes), repoison=j % 4 == 3, padding=padding))
        steps += len(w.steps)
    print(f"{len(keys)} walks, {steps} steps in {time.perf_counter() - t0:.2f} s")


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The walks' buffers, the pools' device copies and the large walks' gathers (GBs) go back after the module."""
    yield
    _bufs.clear()
    _pool_devs.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


CASES = [(kind, ld) for kind in ex.KINDS for ld in wk.LDS]


@pytest.mark.parametrize("kind,ld", CASES, ids=[f"{k}-{ld}" for k, ld in CASES])
def test_small_walks(dev, kind, ld):
    keys = _chosen() or ws.committed()
    _play(dev, [key for key in keys if key[:2] == (kind, ld) and not key[3]], WS_SMALL)


LARGE_PART = 2                                  # large walks per test: a faithful walk at 70,003 docs takes up to 1.4 s
LARGE_CASES = [(kind, first) for kind in ex.KINDS for first in range(0, ws.LARGE_SEEDS[kind], LARGE_PART)]


@pytest.mark.parametrize("kind,first", LARGE_CASES, ids=[f"{k}-{a}" for k, a in LARGE_CASES])
def test_large_walks(dev, kind, first):
    """n in {65536, 65537, 70003} drawn with replacement from the 600-doc pool:
    the block-max top-k, block skip, the fused phase-1 collect, folded keys, the
    sampled filter's overflow fallback and the dynamic tail under option
    vectors and exact mass ties (every pool doc occurs about 110 times)."""
    chosen = _chosen()
    if chosen is not None:               # the chosen large walks of this kind, with the kind's first part
        keys = [key for key in chosen if key[0] == kind and key[3]] if first == 0 else []
    else:
        keys = [key for key in ws.committed_large() if key[0] == kind and first <= key[2] < first + LARGE_PART]
    _play(dev, keys, WS_LARGE)


@pytest.mark.parametrize("reg", REGRESSIONS, ids=[f"{r[0]}-{r[4].replace(' ', '_')}" for r in REGRESSIONS])
def test_regression_walks(dev, reg):
    w = wk.scripted(*reg)
    wk.play(w, wk.exact_pool(w.kind, w.ld), Gpu(dev, _buffers(dev, WS_SMALL)))
