"""GPU: the committed SHARDED walks of tests/_walk_sharded.py played through the
C ABI on cbv2_comm_loopback_init(G) handles and compared with the exact,
shard-free model on every rank after every step, bit for bit -- and the table
of every compute call on an EMPTY index (n == 0, null array pointers).

What the one-shape tests of tests/test_gpu_loopback.py cannot see and a sharded
walk can: exact corpora (mass ties across shards for the (score desc, global id
asc) rule), long documents, MXFP8 against an exact reference, lq != 32 and B on
both sides of every dispatch threshold, k in {1, 2, n - 1, n, n + 1, 1024,
1025, 1100} and kb in {0, 1, 10, 100, 1025} (G * k and G * kb on both sides of
the merge's 8192), a local call whose kb exceeds the exchange's, shards with
n == 0 / n == 1 / n < k on every rank, a non-empty shard whose docs are all
empty, a first id_base that is not 0, ranks
under DIFFERENT option vectors, misses > 0, and workspaces that keep what the
previous exchange left.  These calls are also the only way to union_kth_kernel,
the strided merge_topk_kernel<true / false> on packed send blocks,
prescored_select_kernel and loopback_max_kernel.

Ranks: one host thread and one stream per rank for every step (as
tests/test_gpu_loopback.py::_run_ranks), joined with a timeout; the threads
only issue the C calls, every buffer is prepared and compared on the main
thread.  The first rank error ends the walk: nothing further is launched.
Buffers: per rank ONE persistent workspace (0xA5 at the walk's start, then left
as the calls leave it; every fourth walk re-poisons it before each step) and a
second one for the ``between`` call; one query buffer overwritten in place; one
pinned host stage per rank; outputs filled with NaN / -7 before every call.
Pre-flight: before a walk's first collective every rank's cbv2_index_kind must
equal the walk's kind -- a rank of another kind would leave its peers in the
loopback's 60-second wait (an empty shard of a faithful corpus once did:
REGRESSIONS).

CBV2_SHARDED_WALK_SEEDS="kind:ld:seed,..." makes test_sharded_walks play those
walks of their (kind, ld) in place of the committed ones.

REGRESSIONS lists what the walks and the table found, by name.

Run time, measured on an MI355X (box clock 2026-10-21T06:00Z) in one session
with tests/test_gpu_exact_scores.py and tests/test_gpu_walk.py (100 tests,
37.2 s), whose slowest case there was
test_score_equals_exact_reference[fp32-1024] at 2.03 s (the pool) and, pools
apart, test_small_walks[bf16-128] at 0.87 s for 45 walks / 454 steps:
  test_sharded_walks    20 walks and 156-167 steps per case, 240 walks and 1926
                        steps in all, mean G 3.5: bf16 0.85, 0.80, 0.67, 0.56 s
                        at ld = 128 ... 1024; MXFP8 0.85, 0.69, 0.62, 0.71 s;
                        fp32 0.64, 0.74, 0.61, 0.71 s -- 4 ms per step (G rank
                        threads, the model's numpy included), every case under
                        half the session's slowest existing case
  test_regression_walks 0.09 s; test_empty_index 0.01 s each.
"""
import ctypes
import os
import threading
import time

import numpy as np
import pytest
import torch

import _exact as ex
import _walk as wk
import _walk_sharded as sw
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocFilter, DocGroups, FilterBatch, _stream_ptr
from oracle import oracle as orc
from test_gpu_walk import Gpu, Q_BYTES, pool_dev, _pool_devs

pytestmark = pytest.mark.gpu

WS_BYTES = 128 << 20
HOST_BYTES = 4 << 20
JOIN_S = 100                                     # above the loopback's own 60 s, so its message arrives first
KIND = {"bf16": (_lib.DTYPE_BF16, 0), "mxfp8": (_lib.DTYPE_MXFP8, 0), "fp32": (_lib.DTYPE_BF16, 1)}
# What this file found:
#   an empty faithful shard is not faithful   cbv2_index_attach_residual(h, NULL, ...) on n == 0 stored the null
#       pointer, and "fp32-faithful" was read from that pointer: cbv2_index_kind reported 0, cbv2_score_f32 /
#       _search_f32 / _begin / _rerank_f32 answered CBV2_ESTATE, and in cbv2_search_sharded_local that rank took the
#       bf16 branch and returned CBV2_EINVAL before the all-gather of fk its peers were waiting in.  The handle now
#       remembers that a residual was attached (and that the means were built).  test_empty_index[fp32-*] is the
#       call-by-call form, the walk below the sharded one: G = 3, the middle shard empty, every sharded call.
_DEFAULTS = tuple(v[0] for _, _, v in wk.OPTIONS)
REGRESSIONS = (
    ("fp32", 128, 1, [dict(ep="set_options", values=(_DEFAULTS,) * 3),
                      dict(ep="search_sharded", ds=11, B=3, lq=32, q0=5, k=10, kb=10),
                      dict(ep="search_split", ds=12, B=9, lq=7, q0=0, k=100, kb=10, kb_local=17, with_q=1),
                      dict(ep="rerank_sharded", ds=13, B=2, lq=16, q0=1, C=50, k=10),
                      dict(ep="retrieve_sharded", ds=14, B=3, lq=32, q0=2, k=10, kb=10, kb_begin=10, C=50, final_k=10,
                           how="finish_host")], "an empty faithful shard is not faithful"),
)


def _regression_walk(reg):
    kind, ld, seed, steps, tag = reg
    w = sw.scripted(kind, ld, seed, steps, tag)
    w.G, w.cut_class = 3, "middle_empty"                       # whatever the seed drew
    w.cuts = sw.make_cuts("middle_empty", 3, w.n, w.rng(1))
    return w


class RankBuffers:
    """The device and host buffers of up to 8 ranks, allocated once per module."""

    def __init__(self, dev, G=8):
        self.ws = [[torch.empty((WS_BYTES,), dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(G)]
        self.q = torch.zeros((Q_BYTES,), dtype=torch.uint8, device=dev)
        self.host = [torch.empty((HOST_BYTES,), dtype=torch.uint8, pin_memory=True) for _ in range(G)]
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(G)]
        assert all(t.data_ptr() % 256 == 0 for pair in self.ws for t in pair)

    def poison(self, G):
        for pair in self.ws[:G]:
            for t in pair:
                t.fill_(0xA5)


class _QueryBufs:
    def __init__(self, q):
        self.q = q


class Ranks:
    """Plays a sharded walk's steps: G indexes, G loopback comms, G threads per step."""

    def __init__(self, dev, bufs, repoison=False):
        self.dev, self.bufs, self.repoison = dev, bufs, repoison
        self.L = _lib.lib()
        self.ix, self.comms, self.dead = [], [], False
        self.helper = Gpu(dev, _QueryBufs(bufs.q))              # its queries(), same(), host(), untouched()

    # ----- the player's interface
    def start(self, w, pool):
        L = self.L
        self.w, self.pool = w, pool
        pd = pool_dev(w.kind, w.ld, self.dev)
        self.helper.w, self.helper.pd, self.helper.keep = w, pd, []
        self.ix = [pd.index(w.sel[a:e], w.id_base + a) for a, e in (w.shard(r) for r in range(w.G))]
        self.h = [ix._h for ix in self.ix]
        self.qdt = {"bf16": _lib.DTYPE_BF16, "mxfp8": _lib.DTYPE_MXFP8, "fp32": _lib.DTYPE_F32}[w.kind]
        for r, h in enumerate(self.h):                           # pre-flight: before any collective
            dt, f = ctypes.c_int32(-1), ctypes.c_int32(-1)
            _lib.check(L.cbv2_index_kind(h, ctypes.byref(dt), ctypes.byref(f)))
            if (dt.value, f.value) != KIND[w.kind]:
                self.finish()                                    # nothing was launched: the indexes go back
            assert (dt.value, f.value) == KIND[w.kind], \
                f"rank {r} (docs {w.shard(r)}): cbv2_index_kind says (dtype {dt.value}, faithful {f.value}), the walk's " \
                f"kind {w.kind} is {KIND[w.kind]}: its peers would wait for it in the first collective\n{sw.header(w)}"
        arr = (ctypes.c_void_p * w.G)()
        _lib.check(L.cbv2_comm_loopback_init(w.G, arr))
        self.comms = [ctypes.c_void_p(arr[r]) for r in range(w.G)]
        assert [L.cbv2_comm_rank(c) for c in self.comms] == list(range(w.G))
        self.bufs.poison(w.G)
        torch.cuda.synchronize()

    def finish(self):
        if not self.dead:
            torch.cuda.synchronize()
        for c in self.comms:
            self.L.cbv2_comm_destroy(c)
        self.comms = []
        for ix in self.ix:
            ix.close()
        self.ix = []

    def same(self, got, want):
        return self.helper.same(got, want)

    def host(self, got):
        return self.helper.host(got)

    def untouched(self, arr):
        return self.helper.untouched(arr)

    # ----- pieces
    def out(self, shape, dtype=torch.float32):
        t = torch.full(shape, float("nan") if dtype == torch.float32 else wk.POISON_I, dtype=dtype, device=self.dev)
        self.keep.append(t)
        return t

    def dev_arr(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def stats(self):
        out = []
        for c in self.comms:
            a = (ctypes.c_int64 * 2)()
            _lib.check(self.L.cbv2_comm_stats(c, a))
            out.append((a[0], a[1]))
        return out

    def run(self, fns):
        """fns[r]() on rank r's own thread -> the return codes.  A thread that does not
        come back ends all GPU work of this walk."""
        G = len(fns)
        rcs, errs = [None] * G, []

        def body(r):
            try:
                rcs[r] = fns[r]()
            except BaseException as e:  # noqa: BLE001 - re-raised on the main thread
                errs.append((r, e))

        torch.cuda.synchronize()                                 # inputs and poison are in before any rank starts
        ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=JOIN_S)
        if any(t.is_alive() for t in ts):
            self.dead = True
            raise RuntimeError(f"rank threads {[r for r, t in enumerate(ts) if t.is_alive()]} did not return")
        if errs:
            self.dead = True
            raise errs[0][1]
        if any(rc not in (0, wk.EINVAL) for rc in rcs):          # a HIP or collective error: launch nothing more
            self.dead = True
            raise RuntimeError(f"return codes {rcs}: {self.L.cbv2_last_error().decode(errors='replace')}")
        for s in self.bufs.streams[:G]:
            s.synchronize()
        return rcs

    # ----- the call
    def call(self, i, step):
        try:
            return self._call(i, step)
        except RuntimeError as e:                                # a rank that hung or a HIP / collective error
            raise RuntimeError(f"{e}\nat step {i} of\n{sw.transcript(self.w, i)}") from None

    def _call(self, i, step):
        w, L = self.w, self.L
        self.keep = []
        if self.repoison:
            self.bufs.poison(w.G)
        ep = step["ep"]
        if ep == "set_options":
            for r, h in enumerate(self.h):
                for (_, oid, _), v in zip(wk.OPTIONS, step["values"][r]):
                    _lib.check(L.cbv2_index_set_option(h, oid, int(v)))
            return [{"rc": 0, "comm": (0, 0)} for _ in range(w.G)]
        before = self.stats()
        outs, fns = [], []
        qstep = dict(step, B=max(step["B"], 1))
        self.helper.keep = []
        q = self.helper.queries(qstep)
        self.keep += self.helper.keep
        pre = None
        if ep == "prescored":
            pre = self.dev_arr(sw.prescored_candidates(w, self.pool, step)[0])
        elif ep == "invalid" and step["on"] == "prescored":
            pre = self.dev_arr(np.zeros((max(step["B"], 1), step["C"]), np.int32))
        glob = sw.lex_global(w, step) if step.get("kb", 0) > 0 else None
        for r in range(w.G):
            o, fn = self.rank_call(r, step, q, glob, pre)
            outs.append(o)
            fns.append(fn)
        rcs = self.run(fns)
        after = self.stats()
        return [dict(o, rc=rc, comm=(a[0] - b[0], a[1] - b[1])) for o, rc, a, b in zip(outs, rcs, after, before)]

    def lex(self, step, r, glob, host):
        ids, s = sw.lex_rank(self.w, step, r, glob)
        if host:
            self.keep += [ids, s]
            return ids.ctypes.data, s.ctypes.data
        return self.dev_arr(ids).data_ptr(), self.dev_arr(s).data_ptr()

    def rank_call(self, r, step, q, glob, pre):
        """-> (rank r's poisoned outputs, the function its thread runs)."""
        L, w, h, c = self.L, self.w, self.h[r], self.comms[r]
        st = self.bufs.streams[r].cuda_stream
        ws0, ws1 = (t.data_ptr() for t in self.bufs.ws[r])
        ep = step["ep"]
        inv = step if ep == "invalid" else None
        if inv is not None:
            ep = step["on"]
        B, lq, k, kb = step["B"], step["lq"], step.get("k"), step.get("kb")
        Bo, ko = max(B, 1), max(k or 1, 1)

        def need(*a):
            nb = int(L.cbv2_sharded_workspace_bytes(h, c, *a))
            assert nb <= WS_BYTES, f"the walk's workspace is too small ({nb})"
            return nb

        def search_outs():
            o = {"scores": self.out((Bo, ko)), "ids": self.out((Bo, ko), torch.int32)}
            if kb and kb > 0:
                o["lex"] = self.out((Bo, kb), torch.int32)
            return o

        def search(o, how):
            li, ls = self.lex(step, r, glob, host=r % 2 == 0) if kb > 0 else (None, None)
            lo = o["lex"].data_ptr() if kb > 0 else None
            if how == "search_sharded":
                nb = need(B, k, kb, 0)
                return lambda: L.cbv2_search_sharded(h, c, 0, q, self.qdt, B, lq, k, li, ls, kb, ws0, nb, o["scores"].data_ptr(),
                                                     o["ids"].data_ptr(), lo, st)
            nl, nb = need(B, k, step["kb_local"], 0), need(B, k, kb, 0)

            def split():
                rc = L.cbv2_search_sharded_local(h, c, 0, q, self.qdt, B, lq, k, step["kb_local"], ws0, nl, st)
                if rc:
                    return rc
                return L.cbv2_search_sharded_exchange(h, c, q if step["with_q"] else None, self.qdt, lq, B, k, li, ls, kb,
                                                      ws0, nb, o["scores"].data_ptr(), o["ids"].data_ptr(), lo, st)
            return split

        def rerank(rs, which, prefix=""):
            cand = self.dev_arr(wk.candidates(w, rs))
            o = {prefix + "scores": self.out((rs["B"], rs["k"])), prefix + "ids": self.out((rs["B"], rs["k"]), torch.int32),
                 prefix + "pos": self.out((rs["B"], rs["k"]), torch.int32)}
            nb = need(rs["B"], 1, 0, rs["C"])
            return o, lambda qq: L.cbv2_rerank_sharded(h, c, qq, rs["B"], rs["lq"], cand.data_ptr(), rs["C"], rs["k"],
                                                      which, nb, o[prefix + "scores"].data_ptr(),
                                                      o[prefix + "ids"].data_ptr(), o[prefix + "pos"].data_ptr(), st)

        if inv is not None:
            o = search_outs()
            if ep == "prescored":
                fk = max(step["final_k"], 1)
                o = {"pre_scores": self.out((Bo, fk)), "pre_ids": self.out((Bo, fk), torch.int32),
                     "pre_pos": self.out((Bo, fk), torch.int32), "misses": self.out((1,), torch.int32)}
                nb = need(B, k, kb, 0)
                return o, lambda: L.cbv2_rerank_sharded_prescored(
                    h, c, B, k, kb, pre.data_ptr(), step["C"], step["final_k"], ws0, nb, o["pre_scores"].data_ptr(),
                    o["pre_ids"].data_ptr(), o["pre_pos"].data_ptr(), o["misses"].data_ptr(), st)
            nb = int(L.cbv2_sharded_workspace_bytes(h, c, B, k, kb, 0))
            nb = nb + step["ws_delta"] if nb else WS_BYTES        # bad sizes have no workspace size: the whole buffer
            li, ls = (self.lex(dict(step, B=Bo), r, sw.lex_global(w, dict(step, B=Bo)), host=True)
                      if kb > 0 else (None, None))
            lo = o["lex"].data_ptr() if kb > 0 else None
            return o, lambda: L.cbv2_search_sharded(h, c, 0, q, self.qdt, B, lq, k, li, ls, kb, ws0, nb,
                                                    o["scores"].data_ptr(), o["ids"].data_ptr(), lo, st)
        if ep in ("search_sharded", "search_split"):
            o = search_outs()
            return o, search(o, ep)
        if ep == "rerank_sharded":
            o, fn = rerank(step, ws0)
            return o, lambda: fn(q)
        if ep == "prescored":
            o = search_outs()
            first = search(o, step["how"])
            fk = step["final_k"]
            o.update(pre_scores=self.out((B, fk)), pre_ids=self.out((B, fk), torch.int32),
                     pre_pos=self.out((B, fk), torch.int32))
            o["misses"] = torch.zeros((1,), dtype=torch.int32, device=self.dev)   # the caller zeroes it
            self.keep.append(o["misses"])
            btw = None
            if "between" in step:                                # its own queries: a buffer of its own, this once
                bs = step["between"]
                if r == 0:
                    rows = torch.from_numpy((bs["q0"] + np.arange(bs["B"])) % w.Bp).to(self.dev)
                    Q = self.helper.pd.Q.index_select(0, rows)[:, : bs["lq"]].contiguous()
                    if w.kind == "bf16":
                        Q = Q.to(torch.bfloat16)
                    elif w.kind == "mxfp8":
                        n_rows = bs["B"] * bs["lq"]
                        buf = torch.zeros((n_rows * 130 + 256,), dtype=torch.uint8, device=self.dev)
                        _lib.check(L.cbv2_quantize_mxfp8(Q.data_ptr(), _lib.DTYPE_F32, n_rows, buf.data_ptr(),
                                                         buf.data_ptr() + n_rows * 128, _stream_ptr(self.dev)))
                        self.keep.append(Q)
                        Q = buf
                    self.keep.append(Q)
                    self.btw_q = Q.data_ptr()
                bo, bfn = rerank(bs, ws1, "btw_")
                o.update(bo)
                bq = self.btw_q
                btw = lambda: bfn(bq)                            # noqa: E731
            nb = need(B, k, kb, 0)

            def chain():
                rc = first()
                if rc == 0 and btw is not None:
                    rc = btw()
                if rc:
                    return rc
                return L.cbv2_rerank_sharded_prescored(h, c, B, k, kb, pre.data_ptr(), step["C"], fk, ws0, nb,
                                                       o["pre_scores"].data_ptr(), o["pre_ids"].data_ptr(),
                                                       o["pre_pos"].data_ptr(), o["misses"].data_ptr(), st)
            return o, chain
        assert ep == "retrieve_sharded"
        C, fk = step["C"], step["final_k"]
        nb = int(L.cbv2_retrieve_workspace_bytes(h, c, B, lq, k, step["kb_begin"], C))
        assert 0 < nb <= WS_BYTES and 0 < int(L.cbv2_retrieve_host_bytes(B, k, step["kb_begin"], C)) <= HOST_BYTES
        li, ls = self.lex(step, r, glob, host=True) if kb > 0 else (None, None)
        o = {"scores": self.out((B, fk)), "ids": self.out((B, fk), torch.int32), "pos": self.out((B, fk), torch.int32)}
        hb = self.bufs.host[r]
        args = (h, c, q, self.qdt, B, lq, k, li, ls, kb, wk.RRF_K, C, fk, ws0, nb, hb.data_ptr(), hb.numel(),
                o["scores"].data_ptr(), o["ids"].data_ptr(), o["pos"].data_ptr())
        if step["how"] == "finish_host":
            o.update(host_scores=np.full((B, fk), np.nan, np.float32), host_ids=np.full((B, fk), wk.POISON_I, np.int32),
                     host_pos=np.full((B, fk), wk.POISON_I, np.int32))
            args += (o["host_scores"].ctypes.data, o["host_ids"].ctypes.data, o["host_pos"].ctypes.data)

        def retrieve():
            rc = L.cbv2_retrieve_begin(h, c, q, self.qdt, B, lq, k, step["kb_begin"], C, ws0, nb, st)
            if rc:
                return rc
            return (L.cbv2_retrieve_finish_host if step["how"] == "finish_host" else L.cbv2_retrieve_finish)(*args, st)
        return o, retrieve


# ---------------------------------------------------------------------------- the tests
_bufs = {}


def _buffers(dev):
    if "b" not in _bufs:
        _bufs["b"] = RankBuffers(dev)
    return _bufs["b"]


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _bufs.clear()
    _pool_devs.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _chosen():
    names = [c.strip().split(":") for c in os.environ.get("CBV2_SHARDED_WALK_SEEDS", "").split(",") if c.strip()]
    return [(p[0], int(p[1]), int(p[2])) for p in names] or None


# ---------------------------------------------------------------------------- the empty index (no collective)
def _all_inf_rerank(cand, k):
    """The rerank of candidates that all score -inf: the tie rule alone (position asc)."""
    B, C = cand.shape
    s, i, p = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int32), np.full((B, k), -1, np.int32)
    for b in range(B):
        for j, (pos, _, _) in enumerate(orc.rerank_select(np.full(C, -np.inf, np.float32), k)):
            i[b, j], p[b, j] = cand[b, pos], pos
    return s, i, p


def _empty_index(kind, ld, dev, id_base):
    tok = torch.empty((0, ld, 128), dtype=torch.uint8 if kind == "mxfp8" else torch.bfloat16, device=dev)
    dl = torch.empty((0,), dtype=torch.int32, device=dev)
    assert tok.data_ptr() == 0 and dl.data_ptr() == 0, "an empty tensor has a null data pointer"
    if kind == "mxfp8":
        return ColbertIndex(tok, dl, id_base=id_base, scales=torch.empty((0, ld, 2), dtype=torch.uint8, device=dev))
    if kind == "fp32":                                          # cbv2_index_attach_residual(h, NULL, 0, 0)
        return ColbertIndex(tok, dl, id_base=id_base, residual=torch.empty_like(tok), bounds=(0.0, 0.0))
    return ColbertIndex(tok, dl, id_base=id_base)


EMPTY_CASES = [(kind, ld) for kind in ex.KINDS for ld in (128, 1024)]


@pytest.mark.parametrize("kind,ld", EMPTY_CASES, ids=[f"{k}-{ld}" for k, ld in EMPTY_CASES])
def test_empty_index(dev, kind, ld):
    """n == 0, null array pointers: every compute call returns 0 and writes what
    the header states for an empty shard -- nothing (scores), the padding
    (-inf / -1, status 0), -inf for every candidate -- and nothing past those
    extents.  One handle, no collective: where an empty faithful shard shows
    without any rank waiting for another."""
    L = _lib.lib()
    ix = _empty_index(kind, ld, dev, id_base=1000)
    h, st = ix._h, _stream_ptr(dev)
    dt, f = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.check(L.cbv2_index_kind(h, ctypes.byref(dt), ctypes.byref(f)))
    assert (dt.value, f.value) == KIND[kind], f"cbv2_index_kind of an empty {kind} index: ({dt.value}, {f.value})"
    assert ix.faithful == (kind == "fp32")
    faithful = kind == "fp32"
    qdt = {"bf16": _lib.DTYPE_BF16, "mxfp8": _lib.DTYPE_MXFP8, "fp32": _lib.DTYPE_F32}[kind]
    ws = torch.full((96 << 20,), 0xA5, dtype=torch.uint8, device=dev)
    wp, host = ws.data_ptr(), torch.empty((1 << 20,), dtype=torch.uint8, pin_memory=True)
    nan_bits, ninf = int(np.float32(np.nan).view(np.int32)), float("-inf")
    keep = []

    def out(shape, dtype=torch.float32):
        t = torch.full(shape, float("nan") if dtype == torch.float32 else wk.POISON_I, dtype=dtype, device=dev)
        keep.append(t)
        return t

    def poisoned(t):
        return bool((t.view(torch.int32) == (nan_bits if t.dtype == torch.float32 else wk.POISON_I)).all())

    def padded(what, s, i, k, *more):
        """[B, k + 1] outputs called with row stride k: the first B * k words hold the padding, the rest the poison."""
        torch.cuda.synchronize()
        B = s.shape[0]
        assert (s.reshape(-1)[: B * k] == ninf).all() and (i.reshape(-1)[: B * k] == -1).all(), f"{what}: padding"
        assert poisoned(s.reshape(-1)[B * k:]) and poisoned(i.reshape(-1)[B * k:]), f"{what}: wrote past [B][k]"
        for m in more:
            assert (m == 0).all(), f"{what}: status {m.tolist()}"

    flt = DocFilter(ix, torch.zeros((0,), dtype=torch.int32, device=dev))
    assert flt.count == 0, "cbv2_filter_create on n == 0"
    grp = DocGroups(ix, torch.zeros((0,), dtype=torch.int32))
    assert grp.count == 0, "cbv2_groups_create on n == 0"
    lq = 7
    for B in (1, 9):
        g = torch.Generator().manual_seed(B)
        Qf = torch.randn(B, lq, 128, generator=g).to(dev)
        if kind == "fp32":
            Q = Qf
        elif kind == "bf16":
            Q = Qf.to(torch.bfloat16)
        else:
            Q = torch.zeros((B * lq * 130 + 256,), dtype=torch.uint8, device=dev)
            _lib.check(L.cbv2_quantize_mxfp8(Qf.data_ptr(), _lib.DTYPE_F32, B * lq, Q.data_ptr(),
                                             Q.data_ptr() + B * lq * 128, st))
        q = Q.data_ptr()
        fb = FilterBatch(ix, [flt] * B)
        # ---- scores: rc 0, nothing written
        sc = out((B, 4))
        if faithful:
            nb = int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SCORE, B, lq, 0))
            _lib.check(L.cbv2_score_f32(h, q, B, lq, wp, nb, sc.data_ptr(), 4, st))
        else:
            _lib.check(L.cbv2_score(h, 0, q, qdt, B, lq, sc.data_ptr(), 4, st))
        torch.cuda.synchronize()
        assert poisoned(sc), "a score call on n == 0 wrote something"
        for k in (1, 100):
            cap = 16384
            # ---- search
            s, i, stt = out((B, k + 1)), out((B, k + 1), torch.int32), out((B + 1,), torch.int32)
            if faithful:
                nb = int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SEARCH, B, lq, cap))
                _lib.check(L.cbv2_search_f32(h, q, B, lq, k, cap, wp, nb, s.data_ptr(), i.data_ptr(), stt.data_ptr(), st))
                padded("cbv2_search_f32", s, i, k, stt[:B])
                assert poisoned(stt[B:])
                # ---- begin / finish
                s, i, stt, fk = out((B, k + 1)), out((B, k + 1), torch.int32), out((B + 1,), torch.int32), out((B, k + 1))
                _lib.check(L.cbv2_search_f32_begin(h, q, B, lq, k, cap, wp, nb, fk.data_ptr(), s.data_ptr(), i.data_ptr(),
                                                   stt.data_ptr(), st))
                torch.cuda.synchronize()
                assert (fk.reshape(-1)[: B * k] == ninf).all() and poisoned(fk.reshape(-1)[B * k:]), "begin: fk all -inf"
                lb = torch.full((B,), ninf, device=dev)
                _lib.check(L.cbv2_search_f32_finish(h, B, lq, k, cap, wp, nb, lb.data_ptr(), s.data_ptr(), i.data_ptr(),
                                                    stt.data_ptr(), st))
                padded("cbv2_search_f32_finish", s, i, k, stt[:B])
            else:
                nb = int(L.cbv2_search_workspace_size(h, B, k, 0))
                _lib.check(L.cbv2_search(h, 0, q, qdt, B, lq, k, wp, nb, s.data_ptr(), i.data_ptr(), st))
                padded("cbv2_search", s, i, k)
            # ---- rerank: every candidate -inf, ids and positions by the tie rule
            C = 50
            cand_h = (np.arange(B * C, dtype=np.int32).reshape(B, C) * 7) % 2000 + 990
            cand_h[:, 3] = -1
            cand_h[:, 5] = cand_h[:, 4]
            cand = torch.from_numpy(cand_h).to(dev)
            es, ei, ep = _all_inf_rerank(cand_h, k)
            calls = [("cbv2_rerank_f32", int(L.cbv2_f32_workspace_bytes(h, _lib.F32_RERANK, B, lq, C)))] if faithful else \
                [("cbv2_rerank", None), ("cbv2_rerank_ws", int(L.cbv2_rerank_workspace_bytes(B, C)))]
            for name, nb in calls:
                s, i, p = out((B, k)), out((B, k), torch.int32), out((B, k), torch.int32)
                outs = (s.data_ptr(), i.data_ptr(), p.data_ptr(), st)
                if nb is None:
                    _lib.check(L.cbv2_rerank(h, q, B, lq, cand.data_ptr(), C, k, *outs))
                else:
                    _lib.check(getattr(L, name)(h, q, B, lq, cand.data_ptr(), C, k, wp, nb, *outs))
                torch.cuda.synchronize()
                assert np.array_equal(s.cpu().numpy(), es) and np.array_equal(i.cpu().numpy(), ei) \
                    and np.array_equal(p.cpu().numpy(), ep), f"{name} on n == 0"
                raw = out((B, C + 1))                                # k = 0: the raw scores, [B][C]
                args = (h, q, B, lq, cand.data_ptr(), C, 0) + (() if nb is None else (wp, nb))
                _lib.check(getattr(L, name)(*args, raw.data_ptr(), None, None, st))
                torch.cuda.synchronize()
                assert (raw.reshape(-1)[: B * C] == ninf).all() and poisoned(raw.reshape(-1)[B * C:]), f"{name}, k = 0"
            # ---- filtered, per-query filtered
            s, i, stt = out((B, k + 1)), out((B, k + 1), torch.int32), out((B + 1,), torch.int32)
            if faithful:
                nb = int(L.cbv2_search_filtered_f32_workspace_size(h, flt._h, B, lq, k, cap))
                _lib.check(L.cbv2_search_filtered_f32(h, flt._h, q, B, lq, k, cap, wp, nb, s.data_ptr(), i.data_ptr(),
                                                      stt.data_ptr(), st))
                padded("cbv2_search_filtered_f32", s, i, k, stt[:B])
            else:
                nb = int(L.cbv2_search_filtered_workspace_size(h, flt._h, B, lq, k, 0))
                _lib.check(L.cbv2_search_filtered(h, flt._h, 0, q, qdt, B, lq, k, wp, nb, s.data_ptr(), i.data_ptr(), st))
                padded("cbv2_search_filtered", s, i, k)
            s, i = out((B, k + 1)), out((B, k + 1), torch.int32)
            nb = int(L.cbv2_search_filtered_batch_workspace_size(h, fb._h, B, lq, k, 0))
            _lib.check(L.cbv2_search_filtered_batch(h, fb._h, 0, q, qdt, B, lq, k, wp, nb, s.data_ptr(), i.data_ptr(), st))
            padded("cbv2_search_filtered_batch", s, i, k)
            # ---- grouped
            r = 3
            s, gi = out((B, k + 1)), out((B, k + 1), torch.int32)
            ci, cs, stt = out((B, k + 1, r), torch.int32), out((B, k + 1, r)), out((B + 1,), torch.int32)
            if faithful:
                nb = int(L.cbv2_search_grouped_f32_workspace_size(h, grp._h, B, lq, k, r, cap))
                _lib.check(L.cbv2_search_grouped_f32(h, grp._h, q, B, lq, k, r, cap, wp, nb, s.data_ptr(), gi.data_ptr(),
                                                     ci.data_ptr(), cs.data_ptr(), stt.data_ptr(), st))
                padded("cbv2_search_grouped_f32", s, gi, k, stt[:B])
            else:
                nb = int(L.cbv2_search_grouped_workspace_size(h, grp._h, B, lq, k, r, 0))
                _lib.check(L.cbv2_search_grouped(h, grp._h, 0, q, qdt, B, lq, k, r, wp, nb, s.data_ptr(), gi.data_ptr(),
                                                 ci.data_ptr(), cs.data_ptr(), st))
                padded("cbv2_search_grouped", s, gi, k)
            padded("the grouped search's chunks", cs, ci, k * r)
            # ---- retrieve: begin, finish_host
            kb, C, fk = 2, 4, 3
            lex = np.tile(np.asarray([[1005, -1]], np.int32), (B, 1))
            es, ei, ep = _all_inf_rerank(np.tile(np.asarray([[1005, -1, -1, -1]], np.int32), (B, 1)), fk)
            nb = int(L.cbv2_retrieve_workspace_bytes(h, None, B, lq, k, kb, C))
            assert 0 < nb <= ws.numel() and int(L.cbv2_retrieve_host_bytes(B, k, kb, C)) <= host.numel()
            s, i, p = out((B, fk)), out((B, fk), torch.int32), out((B, fk), torch.int32)
            hs, hi, hp = np.full((B, fk), np.nan, np.float32), np.full((B, fk), -7, np.int32), np.full((B, fk), -7, np.int32)
            _lib.check(L.cbv2_retrieve_begin(h, None, q, qdt, B, lq, k, kb, C, wp, nb, st))
            _lib.check(L.cbv2_retrieve_finish_host(h, None, q, qdt, B, lq, k, lex.ctypes.data, None, kb, wk.RRF_K, C, fk, wp,
                                                   nb, host.data_ptr(), host.numel(), s.data_ptr(), i.data_ptr(),
                                                   p.data_ptr(), hs.ctypes.data, hi.ctypes.data, hp.ctypes.data, st))
            torch.cuda.synchronize()
            for name, got, want in (("scores", s, es), ("ids", i, ei), ("pos", p, ep)):
                assert np.array_equal(got.cpu().numpy(), want), f"cbv2_retrieve_finish_host on n == 0: {name}"
            assert np.array_equal(hs, es) and np.array_equal(hi, ei) and np.array_equal(hp, ep), "its host results"
        fb.close()
    if kind == "bf16":                                          # the means of no docs are built
        _lib.check(L.cbv2_index_build_means(h, None, 128, None, st))
        Qf = torch.randn(2, lq, 128).to(dev)
        sc = out((2, 4))
        _lib.check(L.cbv2_score(h, _lib.SCORER_REF_MEANPOOL_COSINE, Qf.data_ptr(), _lib.DTYPE_F32, 2, lq, sc.data_ptr(), 4, st))
        torch.cuda.synchronize()
        assert poisoned(sc), "REF_MEANPOOL_COSINE on n == 0 wrote something"
    torch.cuda.synchronize()
    flt.close()
    grp.close()
    ix.close()


# ---------------------------------------------------------------------------- the walks
_stopped = []                                    # a rank hung or a HIP / collective error: no further GPU work here


def _play(dev, walks):
    t0 = time.perf_counter()
    steps = 0
    for j, w in enumerate(walks):
        if _stopped:
            pytest.fail(f"not played: {_stopped[0]} hung or failed on the device earlier in this module")
        backend = Ranks(dev, _buffers(dev), repoison=j % 4 == 3)
        try:
            sw.play(w, wk.exact_pool(w.kind, w.ld), backend)
        finally:
            if backend.dead:
                _stopped.append(w.name)
        steps += len(w.steps)
    print(f"{len(walks)} sharded walks, {steps} steps in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("reg", REGRESSIONS, ids=[f"{r[0]}-{r[4].replace(' ', '_')}" for r in REGRESSIONS])
def test_regression_walks(dev, reg):
    _play(dev, [_regression_walk(reg)])


class _WrongShard(Ranks):
    """The last non-empty shard holds its docs in reverse order."""

    def start(self, w, pool):
        r = max(r for r in range(w.G) if w.shard(r)[1] > w.shard(r)[0])
        a, e = w.shard(r)
        good = w.sel
        w.sel = good.copy()
        w.sel[a:e] = good[a:e][::-1]
        try:
            super().start(w, pool)
        finally:
            w.sel = good


def test_player_sees_a_wrong_shard(dev):
    """The comparison is not vacuous: one shard indexed in another order fails its walk, at a named rank and step."""
    if _stopped:
        pytest.fail(f"not played: {_stopped[0]} hung or failed on the device earlier in this module")
    w = next(w for w in (sw.generate(*key) for key in sw.committed() if key[:2] == ("bf16", 128))
             if w.G > 1 and w.n > 100 and w.cut_class == "even")
    backend = _WrongShard(dev, _buffers(dev))
    try:
        with pytest.raises(sw.ShardedFailure) as e:
            sw.play(w, wk.exact_pool(w.kind, w.ld), backend)
    finally:
        if backend.dead:
            _stopped.append(w.name)
    assert f"walk {w.name} fails at step {e.value.index} on rank {e.value.rank}" in str(e.value)
    assert w.steps[e.value.index]["ep"] in sw.STEP_EPS


@pytest.mark.parametrize("kind,ld", sw.CASES, ids=[f"{k}-{ld}" for k, ld in sw.CASES])
def test_sharded_walks(dev, kind, ld):
    keys = _chosen() or sw.committed()
    _play(dev, [sw.generate(*key) for key in keys if key[:2] == (kind, ld)])
