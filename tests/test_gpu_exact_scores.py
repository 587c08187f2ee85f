"""GPU: every scan, rescoring and rerank dispatch against the exact corpora of
tests/_exact.py, bit for bit.

The other GPU tests pin path X to cbv2_score / cbv2_score_f32's bits; the base
scores themselves were compared with an independent reference only within a
tolerance, or exactly on a codebook corpus whose residual is zero and whose
scale bytes are all equal.  Here every scoring row, the first padding row,
every query token, both residual terms and both scale bytes of a token change
the reference (tests/test_exact_corpus.py), and the kernels must return its
bits: torch.equal on the device, -inf of the empty docs included.

Batch sizes, from the dispatch in csrc/colbert_mi355x.hip (one B inside every
branch, both neighbours of every threshold and of every query-group boundary):
  bf16, ld 128    scan_maxsim: B <= kDirectMaxB = 2 the streaming scans (Q1 /
                  Q2), or with CBV2_OPT_DENSE_DOCS the one-workgroup 4 x 1
                  shape (kOneWgMaxB = 2); then pick_shape(kBf16Shapes): 3-4
                  4 x 1, 5-8 4 x 2, 9-16 4 x 4 (non-temporal), 17-32 and 49-64
                  8 x 4 (32 queries per group), 33-48 and 65-72 4 x 4 in 3 / 5
                  groups of 16.
  MXFP8, ld 128   scan_f8: B <= kF8DirectMaxB = 2 the streaming scan (dense
                  docs: 4 x 1); pick_shape(kF8Shapes): 3-4 4 x 1, 5-8 4 x 2,
                  9-16 4 x 4, 17-24 and 33-40 4 x 2 in 3 / 5 groups of 8, 25-32
                  4 x 8, 41-48 and 65-80 4 x 4, 49-64 8 x 8.
  long documents  scan_maxsim_long: 1, 2 streaming, 3-8 (kLongDirectMaxB) the
                  direct scan in groups of 2, >= 9 8 x 4 in groups of 32;
                  scan_f8_long: <= 2 streaming, 3-8 (kF8SmallMaxB) 4 x 2, >= 9
                  8 x 8 in groups of 64 (64 / 65 at ld = 256).
  fp32-faithful   launch_rescore: one pair per workgroup of 4 waves, or of 2
                  once gx * B > 3 x CUs (128-slot docs: from B = 2 here), the
                  row grid-strided once 4096 / B < n (rescore_grid: B >= 7 at
                  n = 600, >= 14 at 300); CBV2_OPT_RESCORE_SPLIT = 0:
                  rescore_x3_kernel, one candidate per wave step while B * n <=
                  kRsSmallPairs = 4096 (B <= 6 / 13 / 20 at n = 600 / 300 /
                  200).  cbv2_search_f32: kBandPairMaxB = 8.
  rerank          kRrSplitMaxB = 32: B = 3 the candidate-parallel kernels,
                  B = 40 one workgroup per query; kSmallMax = 1024: C = 1100
                  the dynamic-LDS form.
The dynamic tail stays off at these corpus sizes.

MXFP8 exponent window: docs {0, -1, -2}, queries {0, -1} (tests/_exact.py).
Observed on an MI355X: every MXFP8 shape, ld and lq returned the reference's
bits with that window -- the block-scaled fp8 MFMA lost no low bit of these
products (multiples of 2^-11 below 16), so the window was not narrowed.

test_comparison_catches_mutated_indexes plays the CPU mutants through the GPU
(an index that scores one row more or fewer, loses its residual, or swaps a
token's scale bytes) and requires the comparison to notice.
"""
import numpy as np
import pytest
import torch

import _exact as ex
import _exact_shapes as shapes
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import ColbertIndex, _stream_ptr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LDS, SIZE, _score_batches = shapes.LDS, shapes.SIZE, shapes.score_batches
CASES = [(kind, ld) for kind in ex.KINDS for ld in LDS]


def _sweep_batches(kind, ld):
    """One B of every dispatch branch -> [(B, dense docs, rescore split)]."""
    if kind == "fp32":
        bs = [1, 2, 7, 33] if ld == 128 else [1, 14, 21]
        return [(b, 0, s) for b in bs for s in (1, 0)]
    if ld != 128:
        return [(b, 0, 1) for b in ((1, 2, 8, 9) if kind == "bf16" else (2, 8, 9))]
    bs = [1, 2, 4, 8, 16, 32, 40] if kind == "bf16" else [1, 4, 8, 16, 24, 32, 48, 64]
    return [(b, 0, 1) for b in bs] + [(1, 1, 1), (2, 1, 1), (4, 1, 1)]


class _Case:
    def __init__(self, kind, ld, dev):
        n, b = SIZE[ld]
        self.kind, self.ld, self.dev = kind, ld, dev
        self.c = c = ex.cached_corpus(kind, ld, n, b, seed=1)     # shared with tests/test_gpu_walk.py
        self.ref = torch.from_numpy(c.ref.astype(np.float32)).to(dev)           # [B, 32, N]
        self.Q = torch.from_numpy(c.queries_f32()).to(dev)
        self.ix = self.build(c.docs_f32(), c.doclens)

    def build(self, X, doclens, id_base=0):
        x, dl = torch.from_numpy(X).to(self.dev), torch.from_numpy(doclens).to(self.dev)
        if self.kind == "fp32":
            ix = ColbertIndex.faithful_f32(x, dl, id_base=id_base)
            assert ix.faithful
        elif self.kind == "mxfp8":
            ix = ColbertIndex.mxfp8(x, dl, id_base=id_base)
            assert ix.fp8
        else:
            ix = ColbertIndex(x.to(torch.bfloat16), dl, id_base=id_base)
        return ix

    def tripled(self):
        """Three copies of the corpus in one index: a mass tie at every place."""
        return self.build(np.tile(self.c.docs_f32(), (3, 1, 1)), np.tile(self.c.doclens, 3))

    def queries(self, B, lq=ex.LQ):
        q = self.Q[:B, :lq].contiguous()
        return q if self.kind == "fp32" else q.to(torch.bfloat16)

    def want(self, B, lq=ex.LQ):
        return self.ref[:B, lq - 1]

    def check(self, got, want, what, B, lq=ex.LQ, docs=None):
        """got == want bit for bit, or a message that names the first differing
        (query, doc), its length, its planted slots and both bit patterns."""
        if got.shape == want.shape and torch.equal(got, want):
            return
        assert got.shape == want.shape, (what, got.shape, want.shape)
        pytest.fail(ex.difference_message(self.c, self.kind, self.ld, what, B, lq, got.cpu().numpy(),
                                          want.cpu().numpy(), None if docs is None else docs.cpu().numpy()))

    def options(self, dense=0, split=1):
        self.ix.set_option(_lib.OPT_DENSE_DOCS, dense)
        if self.kind == "fp32":
            self.ix.set_option(_lib.OPT_RESCORE_SPLIT, split)


_cases = {}


@pytest.fixture
def case(request, dev):
    key = request.param
    if key not in _cases:
        torch.cuda.empty_cache()
        _cases[key] = _Case(*key, dev)
    yield _cases[key]
    _cases[key].options()


def _ids(cases):
    return [f"{k}-{ld}" for k, ld in cases]


# ---------------------------------------------------------------------------- score
# The sweeps take the case, so that tests/test_gpu_nonfinite_padding.py plays them on indexes whose padding rows
# hold NaN / Inf encodings.
def sweep_score(case):
    for B in _score_batches(case.kind, case.ld):
        for dense in ((0, 1) if B <= 4 else (0,)):
            for split in ((1, 0) if case.kind == "fp32" else (1,)):
                case.options(dense, split)
                got = case.ix.score(case.queries(B))
                case.check(got, case.want(B), f"score (dense docs {dense}, rescore split {split})", B)


def sweep_query_lengths(case):
    for B, dense, split in _sweep_batches(case.kind, case.ld):
        case.options(dense, split)
        for lq in range(1, ex.LQ + 1):
            got = case.ix.score(case.queries(B, lq))
            case.check(got, case.want(B, lq), f"score (dense docs {dense}, rescore split {split})", B, lq)


@pytest.mark.parametrize("case", CASES, indirect=True, ids=_ids(CASES))
def test_score_equals_exact_reference(case):
    sweep_score(case)


@pytest.mark.parametrize("case", CASES, indirect=True, ids=_ids(CASES))
def test_every_query_length_equals_exact_reference(case):
    sweep_query_lengths(case)


SMALL = [(kind, 128) for kind in ex.KINDS]


@pytest.mark.parametrize("case", SMALL, indirect=True, ids=_ids(SMALL))
def test_comparison_catches_mutated_indexes(case):
    """The mutants of tests/test_exact_corpus.py, played through the GPU by
    mutating the INDEX: the comparison above must notice each of them."""
    c, B = case.c, case.c.B
    Q, want = case.queries(B), case.want(B)
    i = torch.arange(c.N, device=case.dev)
    qb = torch.from_numpy(c.qb).to(case.dev)
    # one more scoring row: the first padding row is read
    short = torch.from_numpy(c.doclens < c.ld).to(case.dev)
    ix = case.build(c.docs_f32(), np.minimum(c.doclens + 1, c.ld).astype(np.int32))
    got = ix.score(Q)
    assert (got[qb, i] > want[qb, i])[short].all()
    with pytest.raises(pytest.fail.Exception, match=r"first at query \d+, doc \d+ \(doclens \d+, planted slots"):
        case.check(got, want, "score of an index that reads one padding row", B)
    ix.close()
    # one scoring row fewer: a doc planted in its last row loses that token's maximum
    last = (c.slots[:, 0] >= 0) & (c.slots[:, 0] == c.doclens - 1)
    assert last.sum() >= 20
    ix = case.build(c.docs_f32(), np.maximum(c.doclens - 1, 0).astype(np.int32))
    got = ix.score(Q)
    assert (got[qb, i] < want[qb, i])[torch.from_numpy(last).to(case.dev)].all()
    ix.close()
    full = torch.from_numpy(c.doclens > 0).to(case.dev)
    if case.kind == "fp32":                               # the residual lost: an index of hi alone
        ix = case.build((c.dhi / float(ex.ONE)).astype(np.float32), c.doclens)
        differs = (ix.score(Q) != want).any(dim=0)
        assert differs[full].float().mean() > 0.9 and not differs[~full].any()
        ix.close()
    if case.kind == "mxfp8":                              # the two scale bytes of every token swapped
        ix = ColbertIndex(case.ix.tokens, case.ix.doclens, scales=case.ix.scales.flip(-1).contiguous())
        differs = (ix.score(Q) != want).any(dim=0)
        assert differs[full].float().mean() > 0.9 and not differs[~full].any()
        ix.close()


# ---------------------------------------------------------------------------- faithful search / rerank
def _topk(ref_rows, k):
    """(score desc, position asc) of float32 rows -> (scores, positions) [B, k] on the host."""
    s, p = orc.topk(ref_rows.astype(np.float64), k)
    return s.astype(np.float32), p


FP32 = [("fp32", ld) for ld in LDS]


def sweep_faithful_search(case):
    c, ix, dev = case.c, case.ix, case.dev
    k = 10
    for split in (1, 0):
        case.options(0, split)
        for B in (1, 8, 9, 33):
            ws, wi = _topk(c.scores(B=B), k)
            s, i = ix.search(case.queries(B), k)
            assert (ix.last_band >= k).all(), ("the band held the search", ix.last_band)
            assert torch.equal(i.cpu(), torch.from_numpy(wi).to(torch.int32)), (case.ld, B, split)
            case.check(s, torch.from_numpy(ws).to(dev), f"search_f32 (rescore split {split})", B, docs=i)
    # forced fallback: three copies of the corpus tie at the k-th place, so every band holds >= 12 > cap = 10
    ix3 = case.tripled()
    for split in (1, 0):
        ix3.set_option(_lib.OPT_RESCORE_SPLIT, split)
        for B in (1, 9):
            ws, wi = _topk(np.tile(c.scores(B=B), (1, 3)), k)
            s, i = ix3._search_f32(case.queries(B), B, ex.LQ, k, cap=k)
            assert (ix3.last_band == -1).all(), ("every row fell back to the full scan", ix3.last_band)
            assert torch.equal(i.cpu(), torch.from_numpy(wi).to(torch.int32)), (case.ld, B, split)
            case.check(s, torch.from_numpy(ws).to(dev), f"search_f32 fallback (rescore split {split})", B,
                       docs=i % c.N)
    ix3.close()


@pytest.mark.parametrize("case", FP32, indirect=True, ids=_ids(FP32))
def test_faithful_search_returns_reference_bits(case):
    sweep_faithful_search(case)


def _candidates(c, B, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, c.N, (B, C), generator=g, dtype=torch.int32)
    cand[:, ::11] = -1                                    # negative ids score -inf
    cand[:, 3::13] = c.N + 7                              # outside the shard
    cand[:, 5::17] = -(c.N + 3)
    if C > 4:
        cand[:, 1] = cand[:, 2]                           # a duplicate: tie -> lower position
    return cand.to(dev)


def _want_rerank(case, cand, B):
    inside = (cand >= 0) & (cand < case.c.N)
    w = torch.gather(case.want(B), 1, cand.clamp(0, case.c.N - 1).long())
    return torch.where(inside, w, torch.full_like(w, float("-inf")))


def _check_select(case, out, want_raw, cand, k, what, B):
    ws, wp = _topk(want_raw.cpu().numpy(), k)
    s, i, p = out
    assert torch.equal(p.cpu(), torch.from_numpy(wp).to(torch.int32)), (what, case.kind, case.ld, B)
    finite = torch.from_numpy(np.isfinite(ws)).to(case.dev)               # the ids of the candidates that scored
    assert torch.equal(i[finite], torch.gather(cand, 1, p.long())[finite]), (what, case.kind, case.ld, B)
    case.check(s, torch.from_numpy(ws).to(case.dev), what, B, docs=i)


def rerank_shapes(case):
    return ((3, 60), (40, 60)) + (((3, 1100),) if case.ld == 128 else ())


def sweep_faithful_rerank(case, shapes=None):
    for split in (1, 0):
        case.options(0, split)
        for B, C in shapes or rerank_shapes(case):
            cand = _candidates(case.c, B, C, 100 * B + C, case.dev)
            want = _want_rerank(case, cand, B)
            Q = case.queries(B)
            case.check(case.ix.rerank(Q, cand, 0), want, f"rerank_f32 raw (C {C}, rescore split {split})", B,
                       docs=cand)
            _check_select(case, case.ix.rerank(Q, cand, 10), want, cand, 10,
                          f"rerank_f32 k=10 (C {C}, rescore split {split})", B)


@pytest.mark.parametrize("case", FP32, indirect=True, ids=_ids(FP32))
def test_faithful_rerank_returns_reference_bits(case):
    sweep_faithful_rerank(case)


# ---------------------------------------------------------------------------- bf16 / MXFP8 rerank
def _rerank_call(ix, Q, cand, k, with_ws):
    """cbv2_rerank (no workspace) or cbv2_rerank_ws -> raw scores (k == 0) or (scores, ids, positions)."""
    _keep, qptr, _, B, lq = ix._prep_query(Q, "maxsim")
    C = int(cand.shape[1])
    L = _lib.lib()
    out = [torch.empty((B, k or C), dtype=t, device=ix.device) for t in (torch.float32, torch.int32, torch.int32)]
    ptrs = [o.data_ptr() for o in out] if k else [out[0].data_ptr(), None, None]
    if with_ws:
        need = int(L.cbv2_rerank_workspace_bytes(B, C))
        ws = torch.empty((need,), dtype=torch.uint8, device=ix.device)
        _lib.check(L.cbv2_rerank_ws(ix._h, qptr, B, lq, cand.data_ptr(), C, k, ws.data_ptr(), need, *ptrs,
                                    _stream_ptr(ix.device)))
    else:
        _lib.check(L.cbv2_rerank(ix._h, qptr, B, lq, cand.data_ptr(), C, k, *ptrs, _stream_ptr(ix.device)))
    torch.cuda.current_stream(ix.device).synchronize()    # _keep and ws stay alive until the kernels ran
    return out[0] if k == 0 else out


RERANK = [(kind, ld) for kind in ("bf16", "mxfp8") for ld in LDS]


def sweep_rerank(case, shapes=None):
    for B, C in shapes or rerank_shapes(case):
        cand = _candidates(case.c, B, C, 100 * B + C, case.dev)
        want = _want_rerank(case, cand, B)
        Q = case.queries(B)
        for with_ws in (False, True):
            what = f"rerank (C {C}, {'with' if with_ws else 'no'} workspace)"
            case.check(_rerank_call(case.ix, Q, cand, 0, with_ws), want, what + " raw", B, docs=cand)
            k = C if C <= 60 else 20                      # k > 0: the select kernels / one workgroup per query
            _check_select(case, _rerank_call(case.ix, Q, cand, k, with_ws), want, cand, k, what + f" k={k}", B)


@pytest.mark.parametrize("case", RERANK, indirect=True, ids=_ids(RERANK))
def test_rerank_returns_reference_bits(case):
    sweep_rerank(case)
