"""Guard bands: no device entry point reads or writes outside its buffers.

include/colbert_mi355x.h states the exact extent of every buffer a caller hands
over (out_scores f32 [B][k]; a workspace of cbv2_search_workspace_size bytes;
"bits at positions >= n are ignored"; "rows t >= doclens[i] never score").  The
rest of the suite cannot see a violation: it takes outputs and workspaces from
the Python wrappers (torch.empty, rounded-up workspaces, the caching
allocator's slack behind them).  Here every buffer of a call lives inside one
guard-band arena (tests/_arena.py) with exactly the stated extent, at an
address that is aligned as the header asks and no better, and the C ABI is
called directly.  For each case:

  1. where a short workspace is an error, the call with `need - 1` bytes
     returns CBV2_EINVAL and has launched nothing (outputs, workspace and every
     guard untouched);
  2. the real call returns 0; every guard and every input is byte-identical
     afterwards (Arena.verify);
  3. the results equal, bit for bit, the same operation through the ordinary
     Python wrappers on CLONES of the inputs in separate allocations.  The
     guards hold values that win when read (100.0 tokens, full-length doclens,
     allowed filter bits, +inf scores, valid ids), so a guard value that
     reached a result makes the two differ; the wrapper results are what the
     rest of the suite ties to the oracle;
  4. slots the header pads hold exactly -inf / -1, and slots it does not
     mention (columns [n, ld_out) of a score matrix) keep the arena's 0xA5.

cbv2_rerank_ws and cbv2_topk_rows document a short workspace as "take the
other path", not as an error: step 1 runs them with `need - 1` bytes and
requires the same results.

Limits of the method.  A load whose value is masked before use (a padded row,
a clamped doc) is invisible here: only loads that reach a result are caught.
Overruns inside LDS are out of scope.  No sanitizer, debugger or assembly
inspection is involved.  An overrun of more than the arena's 1 MiB head / tail
would fault instead of failing an assertion.
"""
import ctypes
import gc
import re
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from _arena import POISON, Arena
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import (ColbertIndex, _stream_ptr, merge_topk, pack_allow, quantize_mxfp8,
                                            select_topk, topk_rows)

pytestmark = pytest.mark.gpu

N_SMALL = 203            # % 4 = 3, % 32 = 11, % 64 = 11: every tail ragged
N_LONG = 65539           # > the sampled / block-max threshold (65,536); % 4 = 3, % 64 = 3
ID_BASE = 1000
POISON32 = int.from_bytes(bytes([POISON]) * 4, "little", signed=True)
MAXSIM, MEANPOOL = _lib.SCORER_MAXSIM, _lib.SCORER_REF_MEANPOOL_COSINE
NEG_INF = float("-inf")

# ------------------------------------------------------------------ completeness
# Every `int cbv2_*(` declaration of the header is driven through the arena
# below (COVERED) or left out for a stated reason (EXCLUDED).
COVERED = {
    "cbv2_index_create", "cbv2_index_create_mxfp8", "cbv2_index_attach_residual", "cbv2_index_build_means",
    "cbv2_quantize_mxfp8", "cbv2_split_f32", "cbv2_score", "cbv2_score_f32", "cbv2_search", "cbv2_search_f32",
    "cbv2_search_f32_begin", "cbv2_search_f32_finish", "cbv2_rerank", "cbv2_rerank_ws", "cbv2_rerank_f32",
    "cbv2_select_topk", "cbv2_topk_rows", "cbv2_merge_topk", "cbv2_filter_create", "cbv2_search_filtered",
    "cbv2_filter_batch_create", "cbv2_search_filtered_batch",
}
_HOST = "host pointers only: the ASan/UBSan driver of the host code has it (tests/test_asan_host.py)"
_HANDLE = "handle, option or diagnostic call: no caller-owned device buffer"
_HBM = "allocator: hands memory out, takes no caller buffer"
_FILE = "index file / writer: host I/O through pinned staging buffers, sizes from the file header"
_FOLLOWUP = ("follow-up, not part of this work: pooled device-mapped host buffers, a second stream, host threads "
             "or a communicator -- needs an arena over mapped memory and per-rank arenas")
EXCLUDED = {
    "cbv2_abi_version": _HANDLE, "cbv2_index_destroy": _HANDLE, "cbv2_index_time_scans": _HANDLE,
    "cbv2_index_scan_times": _HANDLE, "cbv2_index_band_times": _HANDLE, "cbv2_index_scan_clock": _HANDLE,
    "cbv2_index_set_option": _HANDLE, "cbv2_index_last_scan_plan": _HANDLE, "cbv2_index_kind": _HANDLE,
    "cbv2_filter_destroy": _HANDLE, "cbv2_filter_batch_destroy": _HANDLE,
    "cbv2_retrieve_host_marks": _HANDLE, "cbv2_retrieve_pool_stats": _HANDLE, "cbv2_comm_stats": _HANDLE,
    "cbv2_comm_size": _HANDLE, "cbv2_comm_rank": _HANDLE, "cbv2_comm_destroy": _HANDLE,
    "cbv2_hbm_alloc": _HBM, "cbv2_hbm_free": _HBM,
    "cbv2_rrf_fuse": _HOST, "cbv2_bm25_build": _HOST, "cbv2_bm25_search": _HOST,
    "cbv2_bm25_search_filtered": _HOST, "cbv2_bm25_search_filtered_batch": _HOST, "cbv2_bm25_doc_freq": _HOST,
    "cbv2_bm25_build_shard": _HOST, "cbv2_bm25_destroy": _HOST, "cbv2_stem_en": _HOST,
    "cbv2_index_file_info": _FILE, "cbv2_index_file_info_ld": _FILE, "cbv2_index_file_write_ld": _FILE,
    "cbv2_index_file_write_host_ld": _FILE, "cbv2_index_file_write": _FILE, "cbv2_index_file_read": _FILE,
    "cbv2_index_file_write_host": _FILE, "cbv2_index_file_read_host": _FILE,
    "cbv2_index_writer_open": _FILE, "cbv2_index_writer_open_ld": _FILE, "cbv2_index_writer_append": _FILE,
    "cbv2_index_writer_close": _FILE,
    "cbv2_comm_init": _FOLLOWUP, "cbv2_comm_loopback_init": _FOLLOWUP, "cbv2_search_sharded": _FOLLOWUP,
    "cbv2_search_sharded_local": _FOLLOWUP, "cbv2_search_sharded_exchange": _FOLLOWUP,
    "cbv2_rerank_sharded_prescored": _FOLLOWUP, "cbv2_rerank_sharded": _FOLLOWUP,
    "cbv2_retrieve_cancel": _FOLLOWUP, "cbv2_retrieve_begin": _FOLLOWUP, "cbv2_retrieve_finish": _FOLLOWUP,
    "cbv2_retrieve_finish_host": _FOLLOWUP,
}


def test_header_declarations_are_all_accounted_for():
    declared = set(re.findall(r"^int (cbv2_\w+)\(", open(_lib.HEADER).read(), re.M))
    assert len(declared) > 60
    assert not (COVERED & set(EXCLUDED)), sorted(COVERED & set(EXCLUDED))
    assert declared == COVERED | set(EXCLUDED), sorted(declared ^ (COVERED | set(EXCLUDED)))
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())
    src = open(__file__).read()
    body = src[src.index("# ------------------------------------------------------------------ the arena side"):]
    for name in COVERED:       # "covered" means called below, not merely listed
        assert re.search(rf"\bL\.{name}\(", body), name


# ------------------------------------------------------------------ the arena side
def _L():
    return _lib.lib()


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _first_difference(name, got, want) -> str:
    if got.shape != want.shape:
        return f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    d = (g != w).nonzero()
    at = tuple(d[0].tolist())
    return (f"{name}: {d.shape[0]} of {g.numel()} slots differ, first at {at}: got {got[at].item()!r} "
            f"(bits {g[at].item() & 0xFFFFFFFF:#010x}), the wrappers {want[at].item()!r}")


def _bytes_of(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(-1).view(torch.uint8)


def _rand_unit(gen, dev, *shape):
    x = torch.randn(*shape, device=dev, generator=gen)
    return x / x.norm(dim=-1, keepdim=True)


class Shard:
    """One index inside an arena (tokens, doclens, scales / residual, each with
    guards of at least 8 docs) and clones of its arrays in separate allocations
    for the Python wrappers.  kind: "bf16", "fp8" (MXFP8) or "f32" (bf16 hi +
    residual lo from cbv2_split_f32; opened faithful, or plain on hi alone)."""

    def __init__(self, dev, kind, n, ld, dense, extra=48 << 20):
        L = _L()
        self.dev, self.kind, self.n, self.ld, self.dense = dev, kind, n, ld, dense
        row = 128 if kind == "fp8" else 256
        tok_bytes, g8 = n * ld * row, 8 * ld * row
        cap = tok_bytes * (2 if kind == "f32" else 1) + (n * ld * 2 if kind == "fp8" else 0) + 4 * n + 8 * g8 + extra
        self.A = A = Arena(cap, dev)
        gen = torch.Generator(device=dev).manual_seed(1000 * ld + n)
        dl = torch.randint(0, ld + 1, (n,), device=dev, generator=gen, dtype=torch.int32)
        if dense:
            dl.fill_(ld)
        else:
            dl[0], dl[1], dl[2], dl[n - 1] = 0, 1, ld, ld
        A.take("doclens", 4 * n, "doclens", align=4, skew=4, fill=ld).copy_(_bytes_of(dl))
        tok = A.take("tokens", tok_bytes, "e4m3" if kind == "fp8" else "bf16", align=16, skew=16, guard=g8)
        if kind == "fp8":
            sc = A.take("scales", n * ld * 2, "e8m0", align=4, skew=4, guard=8 * ld * 2)
        if kind == "f32":
            A.take("residual", tok_bytes, "bf16", align=16, skew=16, guard=g8)
            bounds = torch.zeros(2, dtype=torch.float32, device=dev)
        step = max(1, (64 << 20) // (ld * 128 * 4))       # filled in chunks of 64 MiB of fp32
        for a in range(0, n, step):
            c = min(step, n - a)
            x = _rand_unit(gen, dev, c, ld, 128)
            if kind == "bf16":
                tok[a * ld * 256: (a + c) * ld * 256] = _bytes_of(x.bfloat16())
            elif kind == "fp8":
                q, s = quantize_mxfp8(x.bfloat16())
                tok[a * ld * 128: (a + c) * ld * 128] = _bytes_of(q)
                sc[a * ld * 2: (a + c) * ld * 2] = _bytes_of(s)
            else:
                off = a * ld * 256
                _lib.check(L.cbv2_split_f32(x.data_ptr(), c * ld, ld, A.address("doclens") + 4 * a,
                                            A.address("tokens") + off, A.address("residual") + off,
                                            bounds.data_ptr(), _stream_ptr(dev)))
                torch.cuda.synchronize()
            del x
        self.bounds = tuple(bounds.tolist()) if kind == "f32" else None
        # the wrappers' side: clones in separate allocations
        tdt = torch.uint8 if kind == "fp8" else torch.bfloat16
        self.tok_c = A.view("tokens").clone().view(tdt).view(n, ld, 128)
        self.dl_c = A.view("doclens").clone().view(torch.int32)
        self.sc_c = A.view("scales").clone().view(n, ld, 2) if kind == "fp8" else None
        self.lo_c = A.view("residual").clone().view(torch.bfloat16).view(n, ld, 128) if kind == "f32" else None
        self.doclens = dl

    def open(self, plain=False, opts=()):
        """(C handle over the arena views, ColbertIndex over the clones), same options."""
        L, A, h = _L(), self.A, ctypes.c_void_p()
        if self.kind == "fp8":
            _lib.check(L.cbv2_index_create_mxfp8(self.dev.index, A.address("tokens"), A.address("scales"), self.n,
                                                 self.ld, 128, A.address("doclens"), ID_BASE, ctypes.byref(h)))
            ref = ColbertIndex(self.tok_c, self.dl_c, id_base=ID_BASE, scales=self.sc_c)
        else:
            _lib.check(L.cbv2_index_create(self.dev.index, A.address("tokens"), _lib.DTYPE_BF16, self.n, self.ld, 128,
                                           A.address("doclens"), ID_BASE, ctypes.byref(h)))
            if self.kind == "f32" and not plain:
                _lib.check(L.cbv2_index_attach_residual(h, A.address("residual"), self.bounds[0], self.bounds[1]))
                ref = ColbertIndex(self.tok_c, self.dl_c, id_base=ID_BASE, residual=self.lo_c, bounds=self.bounds)
            else:
                ref = ColbertIndex(self.tok_c, self.dl_c, id_base=ID_BASE)
        assert ref.dense_docs == (self.dense and self.ld == 128)
        _lib.check(L.cbv2_index_set_option(h, _lib.OPT_DENSE_DOCS, int(ref.dense_docs)))
        for opt, val in opts:
            _lib.check(L.cbv2_index_set_option(h, opt, val))
            ref.set_option(opt, val)
        return h, ref

    @contextmanager
    def case(self, seed, plain=False, opts=()):
        mark = self.A.mark()
        h, ref = self.open(plain, opts)
        c = Case(self, h, ref, seed)
        try:
            yield c
        finally:
            torch.cuda.synchronize()
            c.close()
            _L().cbv2_index_destroy(h)
            ref.close()
            self.A.release(mark)


class Case:
    """The per-test buffers of one call, taken from the shard's arena."""

    def __init__(self, shard, h, ref, seed):
        self.sh, self.A, self.h, self.ref, self.dev = shard, shard.A, h, ref, shard.dev
        self.L, self.st = _L(), _stream_ptr(shard.dev)
        self.gen = torch.Generator(device=shard.dev).manual_seed(seed)
        self.faithful = ref is not None and ref.faithful
        self._filters, self._batches = [], []

    def close(self):
        for fb in self._batches:
            self.L.cbv2_filter_batch_destroy(fb)
        for f in self._filters:
            self.L.cbv2_filter_destroy(f)

    # inputs: 16-B aligned and no better where the header asks for 16 B, else 4-B aligned and no better
    def put(self, name, t, kind, align=16, **kw):
        v = self.A.take(name, t.numel() * t.element_size(), kind, align=align, skew=align, **kw)
        v.copy_(_bytes_of(t))
        return self.A.address(name)

    def out(self, name, nbytes, align=4, zero=False):
        v = self.A.take(name, nbytes, "out", align=align, skew=align, writable=True)
        if zero:
            v.zero_()
        return self.A.address(name)

    def view(self, name, dtype, *shape):
        return self.A.view(name).view(dtype).view(*shape)

    def queries(self, B, lq, f32=False):
        """-> (device address, ABI dtype, the queries as the wrappers take them)."""
        x = _rand_unit(self.gen, self.dev, B, lq, 128)
        if f32 or self.faithful:
            return self.put("Q", x, "f32"), _lib.DTYPE_F32, x.clone()
        xb = x.bfloat16()
        if self.sh.kind != "fp8":
            return self.put("Q", xb, "bf16"), _lib.DTYPE_BF16, xb.clone()
        # MXFP8: B*lq*128 e4m3 bytes, then B*lq*2 scale bytes, quantized inside the arena
        src = self.put("Qsrc", xb, "bf16", align=4)
        rows = B * lq
        self.A.take("Q", rows * 128 + rows * 2, "e8m0", align=16, skew=16)
        q = self.A.address("Q")
        _lib.check(self.L.cbv2_quantize_mxfp8(src, _lib.DTYPE_BF16, rows, q, q + rows * 128, self.st))
        torch.cuda.synchronize()
        return q, _lib.DTYPE_MXFP8, xb.clone()

    def run(self, fn, outs=(), ws=None, need=None, short="einval"):
        """fn(workspace address, workspace bytes) -> rc, under snapshot / verify."""
        A = self.A
        A.snapshot()
        addr = A.address(ws) if ws is not None else None
        need = A._region(ws).nbytes if (ws is not None and need is None) else need
        if ws is not None and short == "einval" and need > 0:
            rc = fn(addr, need - 1)
            torch.cuda.synchronize()
            assert rc == _lib.ERR_EINVAL, (rc, self.L.cbv2_last_error())
            A.verify()
            for name in (*outs, ws):     # "a call that returns an error has launched nothing"
                assert A.untouched(name), f"{name} written by a call that returned CBV2_EINVAL"
        rc = fn(addr, need if ws is not None else 0)
        torch.cuda.synchronize()
        assert rc == 0, (rc, self.L.cbv2_last_error())
        A.verify()

    def topk_outs(self, B, k, pos=False, prefix="out"):
        names = [f"{prefix}_s", f"{prefix}_i"] + ([f"{prefix}_p"] if pos else [])
        return names, [self.out(nm, B * k * 4) for nm in names]

    def check_topk(self, B, k, want, valid=None, prefix="out"):
        """Outputs [B][k] equal the wrappers' bit for bit; rows pad with -inf / -1 past valid[b]."""
        names = [f"{prefix}_s", f"{prefix}_i", f"{prefix}_p"][: len(want)]
        got = [self.view(nm, torch.float32 if nm.endswith("_s") else torch.int32, B, k) for nm in names]
        for nm, g, w in zip(names, got, want):
            assert _same(g, w), _first_difference(nm, g, w)
        if valid is not None:
            for b, m in enumerate(valid):
                m = min(int(m), k)
                assert (got[0][b, m:] == NEG_INF).all() and all((g[b, m:] == -1).all() for g in got[1:]), (b, m)
                assert not (got[1][b, :m] == -1).any(), (b, m)

    # filters -----------------------------------------------------------------
    def make_filter(self, name, mask):
        """cbv2_filter_create over an exact bitmap (bits past n SET) and an exact buf -> (handle, DocFilter)."""
        L, n = self.L, self.sh.n
        words = pack_allow(mask, n).to(self.dev).view(torch.int32).clone()
        if n % 32:
            tail = (~((1 << (n % 32)) - 1)) & 0xFFFFFFFF
            words[-1] |= tail - (1 << 32) if tail >= (1 << 31) else tail
        allow = self.put(f"{name}_allow", words, "bitmap", align=4)
        need = int(L.cbv2_filter_bytes(n))
        buf = self.out(f"{name}_buf", need, align=16)
        h = ctypes.c_void_p()
        self.run(lambda w, wb: L.cbv2_filter_create(self.h, allow, w, wb, self.st, ctypes.byref(h)),
                 ws=f"{name}_buf")
        self._filters.append(h)
        self.A.freeze(f"{name}_buf")       # the handle borrows it: read-only from here on
        want = torch.from_numpy(np.flatnonzero(mask.cpu().numpy()).astype(np.int32)).to(self.dev)
        assert int(L.cbv2_filter_count(h)) == want.numel()
        assert torch.equal(self.A.view(f"{name}_buf")[: 4 * want.numel()].view(torch.int32), want)
        ref = self.ref.filter(mask=mask.cpu())
        assert ref.count == want.numel() and torch.equal(ref.local_ids, want)
        return h, ref

    def mask(self, m):
        """A bool mask [n] with m allowed docs, the first and the last doc among them when m >= 2."""
        n = self.sh.n
        mask = torch.zeros(n, dtype=torch.bool)
        if m >= n:
            mask[:] = True
        elif m > 0:
            inner = (torch.randperm(n - 2, device=self.dev, generator=self.gen) + 1).cpu()
            if m == 1:
                mask[inner[0]] = True
            else:
                mask[0] = mask[n - 1] = True
                mask[inner[: m - 2]] = True
        assert int(mask.sum()) == min(m, n)
        return mask

    def build_means(self):
        """cbv2_index_build_means from an exact tokens_f32 [n][128][128] into an exact doc_means [n][128]."""
        n = self.sh.n
        x = _rand_unit(self.gen, self.dev, n, 128, 128)
        src = self.put("tokens_f32", x, "f32", guard=8 * 128 * 512)
        dm = self.out("doc_means", n * 128 * 4)
        self.run(lambda w, wb: self.L.cbv2_index_build_means(self.h, src, 128, dm, self.st), outs=["doc_means"])
        self.A.freeze("doc_means")
        self.ref.build_means(x.clone())
        assert _same(self.view("doc_means", torch.float32, n, 128), self.ref.means)


@pytest.fixture(scope="module")
def shards(dev):
    """Shards by (kind, n, ld, dense), built once per module and freed with it."""
    cache = {}

    def get(kind, n=N_SMALL, ld=128, dense=False):
        key = (kind, n, ld, dense)
        if key not in cache:
            cache[key] = Shard(dev, kind, n, ld, dense)
        return cache[key]

    yield get
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _expected_workgroups(qpb, per_cu, B, n, dev):
    """launch_scan16x4's grid on a corpus too small for a dynamic tail."""
    groups = (B + qpb - 1) // qpb
    chunks = max(1, min(per_cu * torch.cuda.get_device_properties(dev).multi_processor_count // groups, n))
    chunk_docs = (n + chunks - 1) // chunks
    return groups * ((n + chunk_docs - 1) // chunk_docs)


# (queries per workgroup, workgroups per CU) of the bf16 doc-interleaved shape each batch size takes
BF16_SHAPE = {3: (4, 2), 5: (8, 2), 9: (16, 2), 17: (32, 1), 33: (16, 2)}    # 33: three groups of 4 x 4
BF16_DENSE_SHAPE = {1: (4, 1), 2: (4, 1), 4: (4, 2)}

SCORE_CASES = (
    [("bf16", N_SMALL, 128, False, B, 32) for B in (1, 2, 3, 5, 9, 17, 33)]
    + [("bf16", N_SMALL, 128, False, 5, 1), ("bf16", N_SMALL, 128, False, 9, 20)]
    + [("bf16", N_SMALL, 128, True, B, 32) for B in (1, 2, 4)]
    + [("fp8", N_SMALL, 128, False, B, 32) for B in (1, 3, 5, 9, 17, 33)]
    + [(kind, N_SMALL, 256, False, B, 32) for kind in ("bf16", "fp8") for B in (1, 3, 9)]
    + [("bf16", 11, 1024, False, 9, 32)]
    + [("f32", N_SMALL, 128, False, B, 32) for B in (1, 9)]
)


@pytest.mark.parametrize("kind,n,ld,dense,B,lq", SCORE_CASES)
def test_score(shards, kind, n, ld, dense, B, lq):
    """cbv2_score / cbv2_score_f32 into ld_out = n + 5: columns [n, ld_out) stay 0xA5, rows start 4-B aligned."""
    sh = shards(kind, n, ld, dense)
    with sh.case(seed=B * 100 + lq) as c:
        L, h = c.L, c.h
        q, qdt, Qr = c.queries(B, lq)
        ldo = n + 5
        o = c.out("out", ((B - 1) * ldo + n) * 4)
        if kind == "f32":
            c.out("ws", int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SCORE, B, lq, 0)), align=16)
            c.run(lambda w, wb: L.cbv2_score_f32(h, q, B, lq, w, wb, o, ldo, c.st), outs=["out"], ws="ws")
        else:
            c.run(lambda w, wb: L.cbv2_score(h, MAXSIM, q, qdt, B, lq, o, ldo, c.st), outs=["out"])
        flat = c.A.view("out").view(torch.int32)
        got = torch.as_strided(flat, (B, n), (ldo, 1))
        assert _same(got, c.ref.score(Qr).view(torch.int32))
        if B > 1:
            assert (torch.as_strided(flat, (B - 1, 5), (ldo, 1), flat.storage_offset() + n) == POISON32).all()
        if kind == "bf16" and ld == 128:
            plan = (ctypes.c_int64 * 4)()
            _lib.check(L.cbv2_index_last_scan_plan(h, plan))
            shape = (BF16_DENSE_SHAPE if dense else BF16_SHAPE).get(B)
            if shape is None:          # the streaming scan plans no doc-interleaved split
                assert list(plan) == [0, 0, 0, 0]
            else:
                assert plan[0] == _expected_workgroups(*shape, B, n, c.dev) and plan[2] == n and plan[3] == 0


def test_score_meanpool(shards):
    """REF_MEANPOOL_COSINE: n = 203 is no multiple of the 64-doc tile, B = 17 none of the 16-query tile."""
    sh = shards("bf16")
    with sh.case(seed=7) as c:
        L, n, B, lq = c.L, sh.n, 17, 7
        c.build_means()
        q, qdt, Qr = c.queries(B, lq, f32=True)
        ldo = n + 5
        o = c.out("out", ((B - 1) * ldo + n) * 4)
        c.run(lambda w, wb: L.cbv2_score(c.h, MEANPOOL, q, qdt, B, lq, o, ldo, c.st), outs=["out"])
        flat = c.A.view("out").view(torch.int32)
        assert _same(torch.as_strided(flat, (B, n), (ldo, 1)), c.ref.score(Qr, "ref_meanpool_cosine").view(torch.int32))
        assert (torch.as_strided(flat, (B - 1, 5), (ldo, 1), flat.storage_offset() + n) == POISON32).all()


@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_quantize_mxfp8(dev, rows, dtype):
    A = Arena(4 << 20, dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    x = (torch.randn(rows, 128, device=dev, generator=gen) * 3).to(dtype)
    A.take("x", x.numel() * x.element_size(), "bf16" if dtype == torch.bfloat16 else "f32", align=4,
           skew=4).copy_(_bytes_of(x))
    A.take("q", rows * 128, "out", align=4, skew=4, writable=True)
    A.take("scales", rows * 2, "out", align=4, skew=4, writable=True)
    A.snapshot()
    dt = _lib.DTYPE_BF16 if dtype == torch.bfloat16 else _lib.DTYPE_F32
    rc = _L().cbv2_quantize_mxfp8(A.address("x"), dt, rows, A.address("q"), A.address("scales"), _stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == 0
    A.verify()
    q, s = quantize_mxfp8(x.clone())
    assert torch.equal(A.view("q").view(rows, 128), q) and torch.equal(A.view("scales").view(rows, 2), s)


@pytest.mark.parametrize("rows,doclens", [(3 * 128, [0, 77, 128]), (5, None)])
def test_split_f32(dev, rows, doclens):
    L, st = _L(), _stream_ptr(dev)
    A = Arena(4 << 20, dev)
    gen = torch.Generator(device=dev).manual_seed(rows)
    x = _rand_unit(gen, dev, rows, 128)
    A.take("x", rows * 512, "f32", align=16, skew=16).copy_(_bytes_of(x))
    dl = None
    if doclens is not None:
        dl = torch.tensor(doclens, dtype=torch.int32, device=dev)
        A.take("doclens", 4 * len(doclens), "doclens", align=4, skew=4, fill=128).copy_(_bytes_of(dl))
    A.take("hi", rows * 256, "out", align=16, skew=16, writable=True)
    A.take("lo", rows * 256, "out", align=16, skew=16, writable=True)
    A.take("bounds", 8, "out", align=4, skew=4, writable=True).zero_()
    A.snapshot()
    rc = L.cbv2_split_f32(A.address("x"), rows, 128, A.address("doclens") if dl is not None else None,
                          A.address("hi"), A.address("lo"), A.address("bounds"), st)
    torch.cuda.synchronize()
    assert rc == 0
    A.verify()
    xc = x.clone()
    hi, lo = torch.empty(rows, 128, dtype=torch.bfloat16, device=dev), torch.empty(rows, 128, dtype=torch.bfloat16,
                                                                                   device=dev)
    bounds = torch.zeros(2, device=dev)
    _lib.check(L.cbv2_split_f32(xc.data_ptr(), rows, 128, dl.clone().data_ptr() if dl is not None else None,
                                hi.data_ptr(), lo.data_ptr(), bounds.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(A.view("hi").view(torch.bfloat16).view(rows, 128), hi)
    assert torch.equal(A.view("lo").view(torch.bfloat16).view(rows, 128), lo)
    assert _same(A.view("bounds").view(torch.float32), bounds)


SEARCH_CASES = [
    # kind, n, B, k, options                          the path
    ("bf16", N_SMALL, 1, 10, ()),                     # exact row select
    ("bf16", N_SMALL, 3, 300, ()),                    # k > n: padding
    ("bf16", 4099, 2, 1500, ()),                      # k > 1024: multi-pass
    ("bf16", N_SMALL, 17, 10, ((_lib.OPT_FUSED_TOPK, 1),)),   # fused scan + top-k, the small fused workspace
    ("f32", N_LONG, 1, 100, ()),                      # the stream folds the block maxima
    ("f32", N_LONG, 3, 100, ()),                      # bmax_topk_kernel, arrival counters at the end of the counters
    ("f32", N_LONG, 9, 100, ()),                      # block-max kernel + select
    ("f32", N_LONG, 3, 100, ((_lib.OPT_TOPK_BMAX, 0),)),      # the sampled filter
    ("fp8", N_LONG, 3, 100, ()),
]


@pytest.mark.parametrize("kind,n,B,k,opts", SEARCH_CASES)
def test_search(shards, kind, n, B, k, opts):
    """cbv2_search with exactly cbv2_search_workspace_size bytes: its [B][n] score matrix (ld = n) ends on the
    workspace's last byte.  The long bf16 corpus is the hi half of the faithful one, opened without the residual."""
    sh = shards(kind, n)
    with sh.case(seed=B * 10 + k, plain=True, opts=opts) as c:
        L, h, lq = c.L, c.h, 32
        q, qdt, Qr = c.queries(B, lq)
        need = int(L.cbv2_search_workspace_size(h, B, k, MAXSIM))
        fused = any(o == _lib.OPT_FUSED_TOPK for o, _ in opts)
        assert (int(L.cbv2_search_fused_slots(h, B, k, MAXSIM)) > 0) == fused
        c.out("ws", need, align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search(h, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st), outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k), valid=[n] * B)


F32_SEARCH_CASES = [
    # n, B, k, cap, options, overflow expected
    (N_LONG, 1, 100, 16384, (), False),
    (N_LONG, 9, 100, 16384, (), False),
    (N_LONG, 2, 100, 100, (), True),                  # cap = k: rows overflow into the full-scan fallback
    (N_LONG, 3, 100, 16384, ((_lib.OPT_BAND_BLOCK_SKIP, 0),), False),
    (N_LONG, 3, 100, 16384, ((_lib.OPT_P1_COLLECT_FUSED, 0),), False),
    (N_LONG, 3, 100, 16384, ((_lib.OPT_BAND_FUSED, 1),), False),
    (N_SMALL, 2, 10, 16384, (), False),
]


@pytest.mark.parametrize("n,B,k,cap,opts,overflow", F32_SEARCH_CASES)
def test_search_f32(shards, n, B, k, cap, opts, overflow):
    sh = shards("f32", n)
    with sh.case(seed=B * 10 + cap % 7, opts=opts) as c:
        L, h, lq = c.L, c.h, 32
        q, _, Qr = c.queries(B, lq)
        c.out("ws", int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SEARCH, B, lq, cap)), align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        st_ = c.out("status", B * 4)
        c.run(lambda w, wb: L.cbv2_search_f32(h, q, B, lq, k, cap, w, wb, os_, oi, st_, c.st),
              outs=names + ["status"], ws="ws")
        c.check_topk(B, k, c.ref._search_f32(Qr, B, lq, k, cap), valid=[n] * B)
        status = c.view("status", torch.int32, B)
        assert torch.equal(status, c.ref.last_band)
        assert bool((status == -1).any()) == overflow


def test_search_f32_begin_finish(shards):
    """The two-call form: fk exactly [B][k]; lb = the row minimum of fk (one shard)."""
    sh = shards("f32", N_LONG)
    with sh.case(seed=41) as c:
        L, h, B, lq, k, cap = c.L, c.h, 3, 32, 100, 16384
        q, _, Qr = c.queries(B, lq)
        c.out("ws", int(L.cbv2_f32_workspace_bytes(h, _lib.F32_SEARCH, B, lq, cap)), align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        st_, fk = c.out("status", B * 4), c.out("fk", B * k * 4)
        lb = c.put("lb", torch.zeros(B, device=c.dev), "f32", align=4)
        c.run(lambda w, wb: L.cbv2_search_f32_begin(h, q, B, lq, k, cap, w, wb, fk, os_, oi, st_, c.st),
              outs=names + ["status", "fk"], ws="ws")
        got_fk = c.view("fk", torch.float32, B, k).clone()
        c.view("lb", torch.float32, B).copy_(got_fk.min(dim=1).values)
        # finish on the same workspace: a short one is still an error, but the workspace now holds begin's state
        c.A.snapshot()
        ws, need = c.A.address("ws"), c.A._region("ws").nbytes
        assert L.cbv2_search_f32_finish(h, B, lq, k, cap, ws, need - 1, lb, os_, oi, st_, c.st) == _lib.ERR_EINVAL
        assert L.cbv2_search_f32_finish(h, B, lq, k, cap, ws, need, lb, os_, oi, st_, c.st) == 0
        torch.cuda.synchronize()
        c.A.verify()
        seen = {}

        def lb_reduce(f):
            seen["fk"] = f.clone()
            return f.min(dim=1).values

        c.check_topk(B, k, c.ref._search_f32_global(Qr, B, lq, k, lb_reduce, cap), valid=[sh.n] * B)
        assert _same(got_fk, seen["fk"])
        assert torch.equal(c.view("status", torch.int32, B), c.ref.last_band)


def _candidates(c, B, C):
    n = c.sh.n
    cand = torch.randint(ID_BASE, ID_BASE + n, (B, C), device=c.dev, generator=c.gen, dtype=torch.int32)
    if C >= 3:
        cand[:, 1] = -1                      # padding
        cand[:, C - 1] = ID_BASE + n + 5     # outside the shard
        cand[0, 0] = ID_BASE + n - 1         # the last doc
    # a stray read of candidate C sees a valid id of a full-length doc
    return c.put("cand", cand, "ids", align=4, fill=ID_BASE + 2), cand.clone()


RERANK_CASES = [(1, 1, 1), (1, 50, 10), (5, 1024, 37), (2, 1025, 10), (33, 50, 10), (3, 50, 0)]


@pytest.mark.parametrize("B,C,k", RERANK_CASES)
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("with_ws", [False, True])
def test_rerank(shards, kind, B, C, k, with_ws):
    """cbv2_rerank and cbv2_rerank_ws (exactly cbv2_rerank_workspace_bytes; one byte short takes cbv2_rerank's path):
    C = 1025 the dynamic-LDS kernel, B = 33 one workgroup per query, k = 0 raw [B][C] with out_ids / out_pos NULL."""
    sh = shards(kind)
    with sh.case(seed=B * 1000 + C) as c:
        L, h, lq = c.L, c.h, 32
        q, _, Qr = c.queries(B, lq)
        cand, cand_c = _candidates(c, B, C)
        want = c.ref.rerank(Qr, cand_c, k)
        if k == 0:
            names, os_, oi, op = ["out_s"], c.out("out_s", B * C * 4), None, None
        else:
            names, (os_, oi, op) = c.topk_outs(B, k, pos=True)

        def check():
            if k == 0:
                assert _same(c.view("out_s", torch.float32, B, C), want)
            else:
                c.check_topk(B, k, want, valid=[C] * B)

        if not with_ws:
            c.run(lambda w, wb: L.cbv2_rerank(h, q, B, lq, cand, C, k, os_, oi, op, c.st), outs=names)
            check()
            return
        c.out("ws", int(L.cbv2_rerank_workspace_bytes(B, C)), align=16)
        for short in (1, 0):
            for nm in names:
                c.A.wipe(nm)
            c.run(lambda w, wb: L.cbv2_rerank_ws(h, q, B, lq, cand, C, k, w, wb - short, os_, oi, op, c.st),
                  outs=names, ws="ws", short="fallback")
            check()


def test_rerank_f32(shards):
    sh = shards("f32")
    with sh.case(seed=5) as c:
        L, h, B, lq, C, k = c.L, c.h, 3, 32, 50, 10
        q, _, Qr = c.queries(B, lq)
        cand, cand_c = _candidates(c, B, C)
        c.out("ws", int(L.cbv2_f32_workspace_bytes(h, _lib.F32_RERANK, B, lq, C)), align=16)
        names, (os_, oi, op) = c.topk_outs(B, k, pos=True)
        c.run(lambda w, wb: L.cbv2_rerank_f32(h, q, B, lq, cand, C, k, w, wb, os_, oi, op, c.st), outs=names, ws="ws")
        c.check_topk(B, k, c.ref.rerank(Qr, cand_c, k), valid=[C] * B)


# ------------------------------------------------------------------ selection calls (no index)
@contextmanager
def _plain_case(dev, capacity, seed):
    class _NoShard:
        pass
    sh = _NoShard()
    sh.dev, sh.A, sh.kind, sh.n = dev, Arena(capacity, dev), "none", 0
    yield Case(sh, None, None, seed)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [1, 1023, 1024, 1025, 4099])
@pytest.mark.parametrize("big_k", [False, True])
@pytest.mark.parametrize("with_ids", [False, True])
def test_select_topk(dev, C, big_k, with_ids):
    """Rank counting in LDS up to C = 1024 (C rounded up to the workgroup), the multi-pass selection beyond;
    k = C + 3 pads; with and without the id map and out_pos."""
    B, k = 3, (C + 3 if big_k else 10)
    with _plain_case(dev, 4 << 20, C) as c:
        L = c.L
        sc = (torch.randn(B, C, device=dev, generator=c.gen) * 4).round() / 4      # ties
        s = c.put("scores", sc, "scores", align=4)
        ids = None
        if with_ids:
            ids_t = torch.randperm(B * C, device=dev, generator=c.gen).to(torch.int32).view(B, C) + ID_BASE
            ids = c.put("ids", ids_t, "ids", align=4, fill=ID_BASE)
        names, outs = c.topk_outs(B, k, pos=with_ids)
        os_, oi, op = (*outs, None)[:3]
        c.run(lambda w, wb: L.cbv2_select_topk(s, ids, B, C, k, os_, oi, op, c.st), outs=names)
        want = select_topk(sc.clone(), k, ids=ids_t.clone() if with_ids else None)
        c.check_topk(B, k, want[: len(names)], valid=[C] * B)


@pytest.mark.parametrize("n", [33, 65536, N_LONG, 262147])
@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("align", [16, 4])
@pytest.mark.parametrize("with_ws", [True, False])
@pytest.mark.parametrize("k", [100, 1500])
def test_topk_rows(dev, n, pad, align, with_ws, k):
    """The float4 / scalar split paths of the row selections, keyed on ld & 3 and the base address; the sampled
    filter with exactly cbv2_topk_workspace_bytes, one byte less and none (the exact radix select)."""
    B, ld = 3, n + pad
    with _plain_case(dev, 16 << 20, n + pad + align + k) as c:
        L = c.L
        sc = torch.randn(B, n, device=dev, generator=c.gen)
        flat = torch.full(((B - 1) * ld + n,), float("inf"), device=dev)      # the columns between rows win too
        torch.as_strided(flat, (B, n), (ld, 1)).copy_(sc)
        s = c.put("scores", flat, "scores", align=align)
        need = int(L.cbv2_topk_workspace_bytes(B, n))
        assert (need > 0) == (n >= 65536)
        names, (os_, oi) = c.topk_outs(B, k)
        want = topk_rows(sc.clone(), k, id_base=ID_BASE, sampled=with_ws)
        if with_ws and need:
            c.out("ws", need, align=16)
        for short in ((1, 0) if with_ws and need else (0,)):
            for nm in names:
                c.A.wipe(nm)
            use_ws = "ws" if with_ws and need else None
            c.run(lambda w, wb: L.cbv2_topk_rows(s, B, n, ld, k, ID_BASE, w, wb - short if w else 0, os_, oi, c.st),
                  outs=names, ws=use_ws, short="fallback")
            c.check_topk(B, k, want, valid=[n] * B)


@pytest.mark.parametrize("G,B,k", [(3, 2, 100), (9, 2, 1000)])
def test_merge_topk(dev, G, B, k):
    """G*k <= 8192 keys staged in LDS, more searched in place; every list ends in a padded suffix."""
    with _plain_case(dev, 4 << 20, G) as c:
        L = c.L
        sc = torch.full((G, B, k), NEG_INF, device=dev)
        ids = torch.full((G, B, k), -1, dtype=torch.int32, device=dev)
        uniq = torch.randperm(G * B * k, device=dev, generator=c.gen).to(torch.int32).view(G, B, k) + ID_BASE
        for g in range(G):
            for b in range(B):
                m = (0, k, k // 3)[(g + b) % 3] if g < 3 else int(torch.randint(0, k + 1, (1,), device=dev,
                                                                                 generator=c.gen))
                # a shard's list: score descending, then id ascending (the tie rule); no -0.0
                vals = (torch.randn(m, device=dev, generator=c.gen) * 8).round() / 8 + 0.0
                o = uniq[g, b, :m].argsort()
                vals, idl = vals[o], uniq[g, b, :m][o]
                o = vals.argsort(descending=True, stable=True)
                sc[g, b, :m], ids[g, b, :m] = vals[o], idl[o]
        s, i = c.put("in_s", sc, "scores", align=4), c.put("in_i", ids, "ids", align=4, fill=ID_BASE)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_merge_topk(s, i, G, B, k, os_, oi, c.st), outs=names)
        valid = [int((ids[:, b] >= 0).sum()) for b in range(B)]
        c.check_topk(B, k, merge_topk(sc.clone(), ids.clone(), k), valid=valid)


# ------------------------------------------------------------------ filters
@pytest.mark.parametrize("n", [N_SMALL, N_LONG])
@pytest.mark.parametrize("density", [0.0, 0.03, 1.0])
def test_filter_create(shards, n, density):
    """Bitmaps of exactly ceil(n / 32) words whose bits past n are SET; buf of exactly cbv2_filter_bytes(n)."""
    sh = shards("bf16" if n == N_SMALL else "f32", n)
    with sh.case(seed=int(density * 100), plain=True) as c:
        m = {0.0: 0, 1.0: n}.get(density, max(2, int(density * n)))
        h, ref = c.make_filter("f", c.mask(m))
        assert ref.count == m


FILTERED_CASES = (
    # kind, n, ld, scorer, path, B, m, k
    [("bf16", N_SMALL, 128, MAXSIM, _lib.FILTER_SUBSET, B, 40, k) for B in (1, 3, 17) for k in (10, 64)]
    + [("f32", N_SMALL, 128, MAXSIM, _lib.FILTER_SUBSET, 2, 40, k) for k in (10, 64)]
    + [("fp8", N_SMALL, 128, MAXSIM, _lib.FILTER_DENSE, 3, 40, k) for k in (10, 64)]
    + [("bf16", N_SMALL, 256, MAXSIM, _lib.FILTER_DENSE, 3, 40, 10)]
    + [("bf16", N_SMALL, 128, MEANPOOL, _lib.FILTER_DENSE, 3, 40, 10)]
    + [("f32", N_LONG, 128, MAXSIM, _lib.FILTER_SUBSET, 3, 2000, 10)]
    + [("bf16", N_SMALL, 128, MAXSIM, _lib.FILTER_SUBSET, 3, 0, 10)]
)


@pytest.mark.parametrize("kind,n,ld,scorer,path,B,m,k", FILTERED_CASES)
def test_search_filtered(shards, kind, n, ld, scorer, path, B, m, k):
    sh = shards(kind, n, ld)
    plain = kind == "f32" and n == N_LONG          # the long corpus serves as the bf16 index here
    with sh.case(seed=B * 100 + k + m, plain=plain, opts=((_lib.OPT_FILTER_PATH, path),)) as c:
        L, h = c.L, c.h
        lq = 7 if scorer == MEANPOOL else 32
        if scorer == MEANPOOL:
            c.build_means()
        f, fref = c.make_filter("f", c.mask(m))
        q, qdt, Qr = c.queries(B, lq, f32=scorer == MEANPOOL)
        c.out("ws", int(L.cbv2_search_filtered_workspace_size(h, f, B, lq, k, scorer)), align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered(h, f, scorer, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        want = c.ref.search(Qr, k, scorer="maxsim" if scorer == MAXSIM else "ref_meanpool_cosine", filter=fref)
        c.check_topk(B, k, want, valid=[m] * B)


BATCH_COUNTS = (0, 1, 40, N_SMALL)       # and the 40-doc handle once more
BATCH_CASES = [
    # kind, path, chunk docs, all rows empty
    ("bf16", _lib.FILTER_SUBSET, 0, False),
    ("bf16", _lib.FILTER_SUBSET, 16, False),
    ("f32", _lib.FILTER_SUBSET, 0, False),
    ("fp8", _lib.FILTER_DENSE, 0, False),
    ("bf16", _lib.FILTER_SUBSET, 0, True),
]


@pytest.mark.parametrize("kind,path,chunk,empty", BATCH_CASES)
def test_search_filtered_batch(shards, kind, path, chunk, empty):
    """B = 5 per-query filters with 0, 1, 40, 203 and (a repeated handle) 40 docs; the table in exactly
    cbv2_filter_batch_bytes(B); k = 64 pads the short rows."""
    sh = shards(kind)
    opts = ((_lib.OPT_FILTER_PATH, path), (_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk))
    with sh.case(seed=chunk + len(kind), opts=opts) as c:
        L, h, B, lq, k = c.L, c.h, 5, 32, 64
        counts = (0, 0) if empty else BATCH_COUNTS
        made = [c.make_filter(f"f{j}", c.mask(m)) for j, m in enumerate(counts)]
        order = [0, 1, 0, 1, 0] if empty else [0, 1, 2, 3, 2]
        handles = (ctypes.c_void_p * B)(*[made[j][0].value for j in order])
        c.out("table", int(L.cbv2_filter_batch_bytes(B)), align=16)
        fb = ctypes.c_void_p()
        c.run(lambda w, wb: L.cbv2_filter_batch_create(h, handles, B, w, wb, c.st, ctypes.byref(fb)), ws="table")
        c._batches.append(fb)
        c.A.freeze("table")
        fbref = c.ref.filter_batch([made[j][1] for j in order])
        m_b = [counts[j] for j in order]
        assert int(L.cbv2_filter_batch_max_count(fb)) == max(m_b) == fbref.max_count
        assert int(L.cbv2_filter_batch_pairs(fb)) == sum(m_b) == fbref.pairs
        q, qdt, Qr = c.queries(B, lq)
        c.out("ws", int(L.cbv2_search_filtered_batch_workspace_size(h, fb, B, lq, k, MAXSIM)), align=16)
        names, (os_, oi) = c.topk_outs(B, k)
        c.run(lambda w, wb: L.cbv2_search_filtered_batch(h, fb, MAXSIM, q, qdt, B, lq, k, w, wb, os_, oi, c.st),
              outs=names, ws="ws")
        c.check_topk(B, k, c.ref.search(Qr, k, filters=fbref), valid=m_b)
