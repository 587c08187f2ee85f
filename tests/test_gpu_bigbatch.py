"""GPU: the big-batch walks of tests/_bigbatch.py (B = 255 ... 65535, and the
calls that go on past it) played through the C ABI with the backend of
tests/test_gpu_walk.py and compared with the exact model after every step, bit
for bit: workspaces 0xA5-poisoned, outputs NaN / -7-poisoned, no tolerance.

Beside the results, every step whose last launch is the index kind's plain
scan (cbv2_score on bf16 / MXFP8, cbv2_search, cbv2_search_f32) has its work
split read back through cbv2_index_last_scan_plan and compared with
_bigbatch.plan -- workgroups, chunk, static part and the dynamic-tail flag --
and a case fails unless it made that assertion on both sides of each of its
gates (the counter ring at 64 / 65 groups under CBV2_OPT_DYNAMIC_TAIL 0, 1
and 2, the one-slice ring at 512 / 513 groups, groups = / > resident
workgroups), with the B of the last computed from the device's CU count.
Every workspace size is checked against _bigbatch.WS_BUDGET (2 GiB).

After a mismatch (never after a fault) the failing step alone is replayed on a
fresh index and a zeroed workspace (Gpu.diagnose).

REGRESSIONS lists the walks that found a bug, by name.

Run time per case, measured on an MI355X (36 tests, 37 s; the pools of
tests/_exact.cached_corpus fall to the first case of each (kind, ld), the 256
class, when this file runs alone):
  256      0.92-2.64 s, all but 0.2-0.5 s of it the pool (95-98 steps)
  gate     0.14-0.22 s bf16 / MXFP8, 0.41-1.44 s fp32 (61-67 steps)
  cu       0.56 s bf16, 0.78 s MXFP8, 3.04 s fp32
  max      0.76 s bf16, 0.69 s MXFP8, 1.72 s fp32 (three walks: n = 63 / 64 / 65, B = 65535, 65536, 70001)
  large-n  0.39 s bf16, 0.26 s MXFP8, 4.68 s fp32 (the 70003-doc gather of tokens and residual)
  the other three tests: under 0.1 s
"""
import ctypes
import time

import pytest
import torch

import _bigbatch as bb
import _walk as wk
import test_gpu_walk as gw
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import _stream_ptr

pytestmark = pytest.mark.gpu

WS_BYTES = bb.WS_BUDGET                          # the budget itself: whatever passes the check fits
Q_BYTES = 288 << 20                              # 16385 fp32 queries of 32 tokens; 70001 of 4
HOST_BYTES = 16 << 20
# The walks that found a bug, written out as (kind, ld, class, tag): none so far.
REGRESSIONS = ()


class PlanGpu(gw.Gpu):
    """Gpu, with the workspace budget and the scan plan asserted."""

    def __init__(self, dev, bufs, cus, asserted):
        super().__init__(dev, bufs)
        self.cus, self.asserted = cus, asserted

    def ws(self, need, which=0):
        assert need < bb.WS_BUDGET, f"a workspace of {need} bytes is over the budget"
        return super().ws(need, which)

    def call(self, i, step, which=0):
        got = super().call(i, step, which)
        w, ep = self.w, step["ep"]
        if which == 0 and ep in bb.PLAN_EPS and not (ep == "score" and w.kind == "fp32") and got["rc"] == 0:
            dt = dict(zip(wk.OPT_NAMES, step["opts"]))["DYNAMIC_TAIL"]
            want = bb.plan(w.kind, w.ld, w.n, step["B"], dt, self.cus)
            plan = self.ix.last_scan_plan()
            assert plan == {key: want[key] for key in plan}, \
                f"walk {w.name} step {i} ({wk.render(i, step)}): the scan's plan is {plan}, the dispatch restated " \
                f"in tests/_bigbatch.py gives {want} on {self.cus} CUs"
            self.asserted |= bb.gates_of(w.kind, w.ld, step["B"], dt, self.cus)
        return got


_bufs = []


def _buffers(dev):
    if not _bufs:
        _bufs.append(gw.Buffers(dev, WS_BYTES, Q_BYTES, HOST_BYTES))
    return _bufs[0]


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    _bufs.clear()
    gw._pool_devs.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def _play(dev, walks, cus, asserted):
    for w in walks:
        t0 = time.perf_counter()
        gpu = PlanGpu(dev, _buffers(dev), cus, asserted)
        wk.play(w, wk.exact_pool(w.kind, w.ld), gpu)           # (an exception of a call -- a fault -- leaves at once)
        print(f"walk {w.name}: n={w.n}, {len(w.steps)} steps in {time.perf_counter() - t0:.2f} s")


CASES = bb.cases()


@pytest.mark.parametrize("kind,ld,cls", CASES, ids=[f"{k}-{ld}-{c}" for k, ld, c in CASES])
def test_big_batch_walks(dev, kind, ld, cls):
    cus = _cus(dev)
    if cls in ("gate", "cu"):
        bb.check_gates_flip(kind, ld, 300, cus)
    asserted = set()
    _play(dev, bb.case_walks(kind, ld, cls, cus), cus, asserted)
    missing = bb.required_gates(kind, ld, cls, cus) - asserted
    assert not missing, f"no plan assertion was made at {sorted(missing)}"


def test_size_functions_that_report_the_bound(dev):
    """The two size functions that answer 0 past 65535 (the header's "Batch sizes"), on a faithful index."""
    L = _lib.lib()
    w = bb.max_walks("fp32")[0]
    ix = gw.pool_dev("fp32", 128, dev).index(w.sel, w.id_base)
    try:
        from hybrid_rag_colbertv2_amd.index import DocGroups
        _, gof, G = w.groupings[0]
        g = DocGroups(ix, torch.from_numpy(gof), G)
        assert int(L.cbv2_search_grouped_f32_workspace_size(ix._h, g._h, 65535, 4, 10, 2, 64)) > 0
        assert int(L.cbv2_search_grouped_f32_workspace_size(ix._h, g._h, 65536, 4, 10, 2, 64)) == 0
        assert int(L.cbv2_filter_batch_bytes(65535)) > 0 and int(L.cbv2_filter_batch_bytes(65536)) == 0
        g.close()
    finally:
        ix.close()


def test_filter_batch_create_rejects_65536(dev):
    """cbv2_filter_batch_create is bounded at 65535: EINVAL, no handle, the table's buffer untouched."""
    L = _lib.lib()
    w = bb.max_walks("bf16")[0]
    pd = gw.pool_dev("bf16", 128, dev)
    ix = pd.index(w.sel, w.id_base)
    try:
        allf = ix.all_docs_filter()
        assert int(L.cbv2_filter_batch_bytes(65536)) == 0 and int(L.cbv2_filter_batch_bytes(65535)) > 0
        buf = torch.full((int(L.cbv2_filter_batch_bytes(65535)) + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        arr = (ctypes.c_void_p * 65536)(*([allf._h.value] * 65536))
        h = ctypes.c_void_p()
        rc = L.cbv2_filter_batch_create(ix._h, arr, 65536, buf.data_ptr(), buf.numel(), _stream_ptr(dev), ctypes.byref(h))
        torch.cuda.synchronize()
        assert rc == _lib.ERR_EINVAL and not h.value
        assert bool((buf == 0xA5).all()), "a rejected cbv2_filter_batch_create wrote into its buffer"
        allf.close()
    finally:
        ix.close()


def test_regression_walks(dev):
    cus = _cus(dev)
    for kind, ld, cls, tag in REGRESSIONS:
        walks = [w for w in bb.case_walks(kind, ld, cls, cus) if w.tag == tag]
        assert walks, (kind, ld, cls, tag)
        _play(dev, walks, cus, set())
