"""GPU: every index path past byte offsets 2^31 and 2^32 of its token arrays, bit
for bit, and every caller-given row stride past 2^31 elements.

The filtered, per-query-filtered, grouped and long-document paths, the two new
certified bands and the rerank gathers each form a token address of their own
(an id read through a list, a candidate id minus id_base, a band entry, a
group's order position, a per-doc stride that depends on ld).  An ``int *
stride`` or a 32-bit offset there is right for the first 2 or 4 GiB of an index
and silently reads another doc beyond it; the suite's corpora for these paths
stop at 0.6 GB.  Here the index is full size but sparse (tests/_highoffset.py):
n_total = 2^32 / docbytes + W docs, all filler (doclens 0, every token element
2.0) except the W docs of an exact-arithmetic corpus in three runs -- at doc 0,
astride byte 2^31 and astride byte 2^32.  A scan costs what a scan of 33k-263k
mostly empty docs costs; every expected value is the integer reference's
(tests/_exact.py) placed at its doc, or the oracle's selection of those rows
(oracle/oracle.py topk, tests/_groups.py oracle); every comparison is on bits.
No expected value comes from a second call into the library, and there is no
tolerance anywhere.

test_comparison_catches_wrapped_addresses turns three of the indexes into the
index a kernel with a wrapped address would see (the tokens of every doc at or
past a boundary replaced by those at offset & 0x7fffffff / & 0xffffffff), and
requires the score comparison to report exactly those docs, with the wrapped
twin's bits, and to pass again after the restore.  Docs of the mid and high
run BELOW their boundary keep their offset under the mask, so no wrapped
address can change them; tests/test_highoffset_layout.py pins that every doc at
or past one does change, for query 0 alone.

Ids near INT32_MAX: cbv2_index_create requires id_base + n <= 2^31 - 1, so the
largest id_base it accepts is 2^31 - 1 - n_total and the last doc's global id
is 2^31 - 2 (not 2^31 - 1: that one it refuses).

Row strides (the last section): one 9.7 GB buffer of 9 rows whose stride is
2^28 + 4 (rows 16-B aligned: the float4 paths) or 2^28 + 3 (the scalar paths),
so row 8 starts past element 2^31 and byte 2^33; cbv2_topk_rows,
cbv2_group_topk_rows, cbv2_score and cbv2_score_f32 must write / read exactly
[b, :n] of it.

Out of scope: the MXFP8 SCALE rows.  They reach byte 2^31 only at 8.4M docs
(137 GB of tokens); that boundary stays untested.

Measured on an MI355X (records, not thresholds):
  wall time    the 68 tests of this file 29.5 s, of which about 13 s build the
               12 corpora on the host; the slowest test 2.9 s including the
               build of its index, every test call below 0.6 s.
  peak HBM     torch.cuda.max_memory_allocated() 9.08 GiB (the row-stride
               buffer; the largest index, faithful, is 2 x 4.0 GiB).
  dynamic tail cbv2_index_last_scan_plan after each score of (a), with
               CBV2_OPT_DYNAMIC_TAIL 1 and 2 alike (never with 0): the tail ran
               for bf16 ld 128 at B = 4, 8, 16, 32, 40 (not at B = 1, 2: the
               streaming scans), ld 256 and 512 at B = 9 only, ld 1024 never;
               MXFP8 ld 128 at B = 4, 8, 16, 24, 32, 48, 64 (not at B = 1),
               ld 256 and 512 at B = 8 and 9, ld 1024 at B = 9.  The faithful
               score (cbv2_score_f32) is a rescoring launch, not a scan: it
               leaves no plan, and its three option values run the same code.
"""
import ctypes
import gc

import numpy as np
import pytest
import torch

import _exact as ex
import _groups as gr
import _highoffset as ho
from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.index import BAND_CAP, ColbertIndex, DocGroups, _stream_ptr
from oracle import oracle as orc
from test_gpu_exact_scores import SIZE, _rerank_call

pytestmark = pytest.mark.gpu

assert SIZE == ho.SIZE                                   # the corpus sizes of the exact-score tests
EDGE = [(kind, ld) for kind in ex.KINDS for ld in (128, 1024)]
ALL = [(kind, ld) for kind in ex.KINDS for ld in ho.LDS]
SEARCH_B = (1, 8, 17)                                    # 17: past kDirectMaxB / the fused top-k's B > 16
SEARCH_BMAX, SEARCH_KMAX = 17, 1100
_DEFAULTS = ((_lib.OPT_DYNAMIC_TAIL, 1), (_lib.OPT_DENSE_DOCS, 0), (_lib.OPT_TOPK_BMAX, 1), (_lib.OPT_FUSED_TOPK, 0),
             (_lib.OPT_FILTER_PATH, 0), (_lib.OPT_FILTER_BATCH_CHUNK_DOCS, 0))
_DEFAULTS_F32 = ((_lib.OPT_RESCORE_SPLIT, 1), (_lib.OPT_BAND_DOC_MAJOR, 0), (_lib.OPT_BAND_FUSED, 0),
                 (_lib.OPT_P1_COLLECT_FUSED, 1), (_lib.OPT_FILTER_BAND, 0), (_lib.OPT_GROUP_BAND, 0))
TAIL_SEEN = {}                                           # (kind, ld, B, option value) -> the dynamic tail ran


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int32))


def _f32(x):
    return torch.from_numpy(np.array(x, np.float32))      # a copy: the layouts' rows are read-only


class _Big:
    """The sparse full-size index of one layout, and the host-side expectations."""

    def __init__(self, kind, ld, dev, near_max=False):
        self.kind, self.ld, self.dev = kind, ld, dev
        self.lay = lay = ho.layout(kind, ld)
        self.c, self.n = lay.c, lay.n_total
        self.id_base = (1 << 31) - 1 - self.n if near_max else 0
        c, n = self.c, self.n
        self.Q = torch.from_numpy(c.queries_f32()).to(dev)
        x = torch.from_numpy(c.docs_f32()).to(dev)
        dl = torch.from_numpy(c.doclens).to(dev)
        # the W real docs through the normal constructors; kept as the copy of the true docs
        if kind == "fp32":
            self.small = ColbertIndex.faithful_f32(x, dl)
        elif kind == "mxfp8":
            self.small = ColbertIndex.mxfp8(x, dl)
        else:
            self.small = ColbertIndex(x.to(torch.bfloat16), dl)
        del x
        self.at = torch.from_numpy(lay.doc_of).to(dev)                     # int64 [W]: corpus doc -> global doc
        doclens = torch.zeros(n, dtype=torch.int32, device=dev)
        doclens[self.at] = dl
        residual = scales = None
        if kind == "mxfp8":
            tokens = torch.empty((n, ld, 128), dtype=torch.uint8, device=dev).fill_(0x40)      # e4m3 2.0
            scales = torch.empty((n, ld, 2), dtype=torch.uint8, device=dev).fill_(127)         # 2^0
        else:
            tokens = torch.empty((n, ld, 128), dtype=torch.bfloat16, device=dev).fill_(2.0)    # 0x4000
            if kind == "fp32":
                residual = torch.zeros((n, ld, 128), dtype=torch.bfloat16, device=dev)
        assert tokens.numel() * tokens.element_size() > 1 << 32
        self.ix = ColbertIndex(tokens, doclens, id_base=self.id_base, scales=scales, residual=residual,
                               bounds=self.small.bounds)
        self.restore()
        assert not self.ix.dense_docs
        self._top = {}

    def arrays(self):
        """[(big array, the W true docs' array)] for tokens and, where present, scales / residual."""
        out = [(self.ix.tokens, self.small.tokens)]
        if self.kind == "mxfp8":
            out.append((self.ix.scales, self.small.scales))
        if self.kind == "fp32":
            out.append((self.ix.residual, self.small.residual))
        return out

    def restore(self):
        for big, true in self.arrays():
            big[self.at] = true

    def close(self):
        self.ix._last_filter_batch = None                 # the batch refers back to the index
        self.ix.close()
        self.small.close()
        self.ix = self.small = None

    def defaults(self):
        for opt, v in _DEFAULTS + (_DEFAULTS_F32 if self.kind == "fp32" else ()):
            self.ix.set_option(opt, v)

    # ------------------------------------------------------------------ inputs / expectations
    def queries(self, B, lq=ex.LQ):
        q = self.Q[:B, :lq].contiguous()
        return q if self.kind == "fp32" else q.to(torch.bfloat16)

    def rows(self, B, lq=ex.LQ):
        """float32 [B, n] on the host: the exact score matrix of the big index."""
        return self.lay.expected_rows(lq)[:B]

    def top(self, B, k):
        """The oracle's top-k of rows(B): (scores f32 [B, k], global ids int64 [B, k]); one
        selection of SEARCH_BMAX rows and SEARCH_KMAX places serves every smaller call."""
        if "full" not in self._top:
            self._top["full"] = orc.topk(self.rows(SEARCH_BMAX), SEARCH_KMAX)
        s, i = self._top["full"]
        assert B <= s.shape[0] and k <= s.shape[1]
        return s[:B, :k].astype(np.float32), np.where(i[:B, :k] >= 0, i[:B, :k] + self.id_base, -1)

    def local(self, ids):
        """Global ids (tensor or array) -> local docs on the host (whatever lies outside stays outside)."""
        ids = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        return np.where(ids >= 0, ids.astype(np.int64) - self.id_base, -1)

    def check(self, got, want, what, B, lq=ex.LQ, docs=None):
        """got == want on bits, or the message of tests/_exact.py naming the first
        differing (query, doc), its run and boundary, its length and both patterns."""
        want = want if isinstance(want, torch.Tensor) else _f32(want)
        want = want.to(self.dev)
        assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
        if torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)):
            return
        pytest.fail(ex.difference_message(self.c, self.kind, self.ld, what, B, lq, got.cpu().numpy(),
                                          want.cpu().numpy(), None if docs is None else self.local(docs),
                                          corpus_at=self.lay.corpus_at, place=self.lay.place))

    def check_ids(self, got, want, what):
        want = _i32(want)
        assert torch.equal(got.cpu(), want), (what, self.kind, self.ld, "first difference at",
                                              (got.cpu() != want).nonzero()[0].tolist())


_live = {}


def _drop_big():
    for old in list(_live):
        _live.pop(old).close()
    gc.collect()
    torch.cuda.empty_cache()


def _big(key, dev):
    """At most one big index alive: the one of ``key`` = (kind, ld[, near_max])."""
    if key not in _live:
        _drop_big()
        _live[key] = _Big(key[0], key[1], dev, *key[2:])
    return _live[key]


@pytest.fixture(scope="module", autouse=True)
def _release():
    """Nothing of this file stays in HBM or host memory for the modules that run after it."""
    if torch.cuda.is_available():
        torch.cuda.reset_peak_memory_stats()             # the peak this file prints is its own
    yield
    _drop_big()
    ho._layouts.clear()


@pytest.fixture
def big(request, dev):
    b = _big(request.param, dev)
    b.defaults()
    yield b
    b.defaults()


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def _param(cases):
    return pytest.mark.parametrize("big", cases, indirect=True, ids=_ids(cases))


# ---------------------------------------------------------------------------- (a) score
def _score_sweep(big, note=None):
    """The comparison of (a): every dispatch branch's B, both query lengths, the three work splits."""
    for B in ho.score_batches(big.kind, big.ld):
        for lq in ho.SCORE_LQS:
            for tail in (0, 1, 2):
                big.ix.set_option(_lib.OPT_DYNAMIC_TAIL, tail)
                got = big.ix.score(big.queries(B, lq))
                if note is not None and big.kind != "fp32":
                    note[(big.kind, big.ld, B, tail)] = big.ix.last_scan_plan()["dynamic_tail"]
                big.check(got, big.rows(B, lq), f"score (dynamic tail {tail})", B, lq)


@_param(ALL)
def test_score_past_2gib_and_4gib(big):
    _score_sweep(big, TAIL_SEEN)
    ran = sorted(k for k, v in TAIL_SEEN.items() if v and k[:2] == (big.kind, big.ld))
    print(f"\n[high offsets] {big.kind} ld={big.ld} n={big.n}: dynamic tail ran for (B, option) "
          f"{[k[2:] for k in ran] or 'none'}; peak {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


# ---------------------------------------------------------------------------- (b) search
@_param(ALL)
def test_search_past_2gib_and_4gib(big):
    W = big.lay.W
    for B in SEARCH_B:
        Q = big.queries(B)
        for k in (100, 1100, W + 37):
            ws, wi = big.top(B, k)                        # past the docs that score: -inf filler, lowest ids first
            modes = [(bmax, 0) for bmax in (0, 1)] + ([(1, 1)] if big.kind == "bf16" and B > 16 else [])
            for bmax, fused in modes:
                big.ix.set_option(_lib.OPT_TOPK_BMAX, bmax)
                big.ix.set_option(_lib.OPT_FUSED_TOPK, fused)
                s, i = big.ix.search(Q, k)
                what = f"search k={k} (block-max {bmax}, fused top-k {fused})"
                big.check_ids(i, wi, what + f" B={B}")
                big.check(s, ws, what, B, docs=i)


# ---------------------------------------------------------------------------- (c) faithful search
FP32_EDGE = [("fp32", 128), ("fp32", 1024)]


@_param(FP32_EDGE)
def test_faithful_search_past_2gib_and_4gib(big):
    ix, k = big.ix, 10
    configs = [dict(split=s, fused=f, p1=p, major=0) for s in (1, 0) for f in (0, 1) for p in (0, 1)]
    for B in (2, 8, 9, 17):
        Q = big.queries(B)
        ws, wi = big.top(B, k)
        for cfg in configs + ([dict(split=1, fused=0, p1=1, major=m) for m in (1, 2, 3, 4)] if B > 8 else []):
            ix.set_option(_lib.OPT_RESCORE_SPLIT, cfg["split"])
            ix.set_option(_lib.OPT_BAND_FUSED, cfg["fused"])
            ix.set_option(_lib.OPT_P1_COLLECT_FUSED, cfg["p1"])
            ix.set_option(_lib.OPT_BAND_DOC_MAJOR, cfg["major"])
            s, i = ix.search(Q, k)
            # certified: filler scores -inf on hi as well, so a band holds at most the corpus's docs
            assert ((ix.last_band >= k) & (ix.last_band <= big.lay.W)).all(), (cfg, B, ix.last_band)
            big.check_ids(i, wi, f"search_f32 {cfg} B={B}")
            big.check(s, ws, f"search_f32 {cfg}", B, docs=i)
        big.defaults()
        # begin / finish with lb = the row minimum of fk
        s, i = ix.search(Q, k, lb_reduce=lambda fk: fk.min(dim=1).values)
        assert (ix.last_band >= k).all(), (B, ix.last_band)
        big.check_ids(i, wi, f"search_f32 begin / finish B={B}")
        big.check(s, ws, "search_f32 begin / finish", B, docs=i)
    # the on-device fallback.  k past the number of docs that score: the k-th place is -inf, every one of
    # the n_total docs ties for it, so no band of cap = k < n_total entries can hold the row.
    live = int((big.c.doclens > 0).sum())
    k = live + 5
    for split in (1, 0):
        ix.set_option(_lib.OPT_RESCORE_SPLIT, split)
        for B in (2, 9):
            ws, wi = big.top(B, k)
            s, i = ix._search_f32(big.queries(B), B, ex.LQ, k, cap=k)
            assert (ix.last_band == -1).all(), ("every row fell back to the full scan", split, B, ix.last_band)
            big.check_ids(i, wi, f"search_f32 fallback B={B} split={split}")
            big.check(s, ws, f"search_f32 fallback (rescore split {split})", B, docs=i)


# ---------------------------------------------------------------------------- (d) rerank
def _candidates(big, B, C, seed):
    """Global candidate ids from all three runs, filler, outside the shard, -1 and duplicates."""
    lay, rng = big.lay, np.random.default_rng(seed)
    cand = lay.doc_of[rng.integers(0, lay.W, size=(B, C))]                   # the three runs
    cand[:, 4::7] = rng.integers(0, lay.n_total, size=cand[:, 4::7].shape)  # (mostly) filler, anywhere in the index
    cand[:, 6::19] = lay.d32 - 1 - rng.integers(0, 4, size=cand[:, 6::19].shape)
    cand = cand + big.id_base
    cand[:, ::11] = -1
    cand[:, 3::13] = big.id_base + lay.n_total + 7 if big.id_base == 0 else big.id_base - 7      # outside the shard
    cand[:, 5::17] = big.id_base - 3 if big.id_base else -(lay.n_total + 3)
    cand[:, 1] = cand[:, 2]                                                  # a duplicate: tie -> lower position
    return cand


def _rerank_checks(big, B, C, k):
    cand = _candidates(big, B, C, 100 * B + C)
    loc = cand - big.id_base
    inside = (cand >= 0) & (loc >= 0) & (loc < big.n)
    raw = np.where(inside, np.take_along_axis(big.rows(B), np.clip(loc, 0, big.n - 1), axis=1), -np.inf)
    raw = raw.astype(np.float32)
    assert np.isfinite(raw).sum() > B * C // 3 and inside.sum() < inside.size
    ws, wp = orc.topk(raw, k)
    ws = ws.astype(np.float32)
    cand_t, Q = _i32(cand).to(big.dev), big.queries(B)
    if big.kind == "fp32":
        calls = [("rerank_f32", lambda kk: big.ix.rerank(Q, cand_t, kk))]
    else:
        calls = [("rerank", lambda kk: _rerank_call(big.ix, Q, cand_t, kk, False)),
                 ("rerank_ws", lambda kk: _rerank_call(big.ix, Q, cand_t, kk, True))]
    for name, call in calls:
        what = f"{name} (C {C}"
        big.check(call(0), raw, what + ") raw", B, docs=cand)
        s, i, p = call(k)
        big.check_ids(p, wp, what + f", k {k}) positions B={B}")
        fin = np.isfinite(ws)
        assert np.array_equal(i.cpu().numpy()[fin], np.take_along_axis(cand, np.clip(wp, 0, None), axis=1)[fin]), what
        big.check(s, ws, what + f", k {k})", B, docs=i)


@_param(EDGE)
def test_rerank_past_2gib_and_4gib(big):
    for B in (3, 40):
        for C, k in ((50, 50), (50, 10), (1100, 20)):
            _rerank_checks(big, B, C, k)


# ---------------------------------------------------------------------------- (e) filtered search
def _allowed(big, seed, runs=(0, 1, 2), share=0.5, filler=300):
    """Ascending local ids: about ``share`` of each run of ``runs`` plus ``filler`` filler docs."""
    lay, rng = big.lay, np.random.default_rng([seed, big.ld])
    mask = np.zeros(lay.n_total, bool)
    mask[lay.doc_of[(rng.random(lay.W) < share) & np.isin(lay.run_of, runs)]] = True
    if filler:
        spots = np.concatenate([rng.integers(0, lay.n_total, size=filler - 40),
                                lay.d31 + rng.integers(-150, 150, size=20), lay.d32 + rng.integers(-150, 150, size=20)])
        mask[spots[lay.corpus_at[spots] < 0]] = True
    return np.flatnonzero(mask)


def _filter_ref(big, rows, E, k):
    rs, ri = orc.topk(rows[:, E], k)
    ids = np.where(ri >= 0, big.id_base + E[np.clip(ri, 0, None)], -1) if len(E) else np.full(ri.shape, -1)
    return rs.astype(np.float32), ids


def _filtered_checks(big, Bs, ks, paths=(1, 2)):
    ix = big.ix
    E = _allowed(big, 5)
    assert all(((big.lay.run_of == r) & np.isin(big.lay.doc_of, E)).sum() >= big.lay.sizes[r] // 4 for r in range(3))
    flt = ix.filter(ids=(E + big.id_base).tolist())
    assert flt.count == len(E)
    for B in Bs:
        Q = big.queries(B)
        for k in ks + ((len(E) + 3,) if big.kind != "fp32" else ()):      # past m: -inf / -1 padding
            ws, wi = _filter_ref(big, big.rows(B), E, k)
            for path in paths:
                ix.set_option(_lib.OPT_FILTER_PATH, path)
                for band in ((1, 2) if big.kind == "fp32" else (0,)):
                    what = f"filtered search k={k} (path {path}, band {band})"
                    if big.kind == "fp32":
                        ix.set_option(_lib.OPT_FILTER_BAND, band)
                    s, i = ix.search(Q, k, filter=flt)
                    if big.kind == "fp32":                # the status of the header: the band's size, or -1
                        st = ix.last_band
                        if path == 1 and band == 1:
                            assert ((st >= k) & (st <= len(E))).all(), (what, B, st)
                        else:
                            assert (st == -1).all(), (what, B, st)
                    big.check_ids(i, wi, what + f" B={B}")
                    big.check(s, ws, what, B, docs=i)
    flt.close()


@_param(ALL)
def test_filtered_search_past_2gib_and_4gib(big):
    _filtered_checks(big, (1, 2, 8, 40), (10, 100))


# ---------------------------------------------------------------------------- (f) filter batch
@_param(EDGE)
def test_filter_batch_past_2gib_and_4gib(big):
    ix = big.ix
    Es = [_allowed(big, 20 + j, share=0.3 + 0.1 * j, filler=60 + 40 * j) for j in range(6)]
    Es.append(np.zeros(0, np.int64))                                       # an empty filter
    Es.append(_allowed(big, 31, runs=(2,), share=0.7, filler=0))           # only docs of the high run
    assert len(Es[7]) > 10 and (Es[7] >= big.lay.starts[2]).all()
    assert len({e.tobytes() for e in Es}) == 8
    flts = [ix.filter(ids=(E + big.id_base).tolist()) for E in Es]
    use = [0, 1, 2, 3, 4, 5, 6, 7, 0, 0, 3, 5, 7]                          # some shared between queries
    B = len(use)
    Q = big.queries(B)
    for chunk in (0, 64):                                                  # 64: a row splits into several work items
        ix.set_option(_lib.OPT_FILTER_BATCH_CHUNK_DOCS, chunk)
        batch = ix.filter_batch([flts[j] for j in use])
        for k in (10, 100):
            want = [_filter_ref(big, big.rows(B)[b:b + 1], Es[j], k) for b, j in enumerate(use)]
            ws, wi = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
            s, i = ix.search(Q, k, filters=batch)
            big.check_ids(i, wi, f"filter batch k={k} chunk docs {chunk}")
            big.check(s, ws, f"filter batch k={k} (chunk docs {chunk})", B, docs=i)
        torch.cuda.synchronize()
        batch.close()
    for f in flts:
        f.close()


# ---------------------------------------------------------------------------- (g) grouped search
def _grouping(big, G=37):
    """group_of over all n_total docs: G groups that each mix low, mid and high
    docs (the j-th doc of every run is in group j % G) and a few hundred filler
    docs; group G made only of filler; every other filler doc in no group."""
    lay, rng = big.lay, np.random.default_rng([9, big.ld])
    g = np.full(lay.n_total, -1, np.int32)
    for r in range(3):
        docs = lay.starts[r] + np.arange(lay.sizes[r])
        g[docs] = np.arange(lay.sizes[r]) % G
    spots = np.concatenate([rng.integers(0, lay.n_total, size=300), lay.d32 + rng.integers(-150, 150, size=40)])
    spots = np.unique(spots[lay.corpus_at[spots] < 0])
    g[spots[:-20]] = rng.integers(0, G, size=len(spots) - 20)
    g[spots[-20:]] = G
    for j in range(G):
        members = lay.corpus_at[np.flatnonzero(g == j)]
        assert set(lay.run_of[members[members >= 0]].tolist()) == {0, 1, 2} and (members < 0).any()
    return g, G + 1


def _check_grouped(big, got, want, what, B):
    ws, wg, wi, wc = want
    s, g, i, c = got
    big.check_ids(g, wg, what + " groups")
    big.check_ids(i.reshape(B, -1), wi.reshape(B, -1), what + " chunk ids")
    big.check(c.reshape(B, -1), wc.reshape(B, -1), what + " chunk scores", B, docs=i.reshape(B, -1))
    big.check(s, ws, what + " group scores", B, docs=i[:, :, 0])


FALLBACKS = []                    # (ld, B, k, r, rows that fell back) of the calls with cap = k r


def _grouped_checks(big, Bs, rs=(1, 3)):
    ix = big.ix
    g, G = _grouping(big)
    grp = ix.groups(group_of=torch.from_numpy(g), G=G)
    for B in Bs:
        Q = big.queries(B)
        for r in rs:
            for k in (10, G + 2):                         # G + 2: the all-filler group last, then padding
                want = gr.oracle(big.rows(B), g, G, k, r, id_base=big.id_base)
                if big.kind != "fp32":
                    _check_grouped(big, ix.search_grouped(Q, k, grp, r), want, f"search_grouped k={k} r={r}", B)
                    continue
                for band, cap in ((2, BAND_CAP), (1, BAND_CAP), (1, k * r)):
                    ix.set_option(_lib.OPT_GROUP_BAND, band)
                    got = ix.search_grouped(Q, k, grp, r, cap=cap)
                    st = ix.last_band
                    what = f"search_grouped_f32 k={k} r={r} (band {band}, cap {cap})"
                    if band == 2 or k >= G:               # the band needs G' > k
                        assert (st == -1).all(), (what, B, st)
                    elif cap == BAND_CAP:
                        assert ((st >= k) & (st <= big.lay.W)).all(), (what, B, st)
                    else:
                        assert ((st == -1) | ((st >= k) & (st <= cap))).all(), (what, B, st)
                        FALLBACKS.append((big.ld, B, k, r, int((st == -1).sum())))
                    _check_grouped(big, got, want, what, B)
    grp.close()


@_param(EDGE)
def test_grouped_search_past_2gib_and_4gib(big):
    del FALLBACKS[:]
    _grouped_checks(big, (2, 9))
    if big.kind == "fp32":                                # cap = k r: some row of some call overflowed it
        assert any(f[-1] > 0 for f in FALLBACKS), FALLBACKS


# ---------------------------------------------------------------------------- (h) ids near INT32_MAX
NEAR_MAX = [("bf16", 128, True), ("fp32", 128, True)]


@_param(NEAR_MAX)
def test_ids_near_int32_max(big, dev):
    assert big.id_base + big.n == (1 << 31) - 1
    with pytest.raises(ValueError, match="global ids must fit int32"):                     # one more and the last id would not fit the contract
        ColbertIndex(big.ix.tokens, big.ix.doclens, id_base=big.id_base + 1,
                     residual=big.ix.residual, bounds=big.ix.bounds)
    B, k = 8, big.lay.W + 37                              # the -inf filler: ids from id_base upwards
    ws, wi = big.top(B, k)
    assert wi[wi >= 0].min() == big.id_base and wi.max() > (1 << 31) - 1 - big.lay.W
    if big.kind == "fp32":
        k = 10
        ws, wi = big.top(B, k)
    s, i = big.ix.search(big.queries(B), k)
    big.check_ids(i, wi, "search near INT32_MAX")
    big.check(s, ws, "search near INT32_MAX", B, docs=i)
    _rerank_checks(big, 3, 50, 10)
    _filtered_checks(big, (2,), (10,), paths=(1,))
    _grouped_checks(big, (2,), rs=(3,))


# ---------------------------------------------------------------------------- (i) the comparison sees a wrapped address
TWINS = [("bf16", 128), ("mxfp8", 128), ("fp32", 1024)]


@_param(TWINS)
def test_comparison_catches_wrapped_addresses(big):
    lay = big.lay
    docs, twin = lay.wrapped_twin()                                        # corpus docs, float64 [B, 32, len]
    dst = torch.from_numpy(lay.doc_of[docs]).to(big.dev)
    src = torch.from_numpy(lay.wrapped_source()).to(big.dev)
    live = lay.c.doclens[docs] > 0
    try:
        for arr, _ in big.arrays():                                        # in place: the wrapped location's bytes
            arr[dst] = arr[src]
        B = max(ho.score_batches(big.kind, big.ld))
        got = big.ix.score(big.queries(B))
        want = _f32(big.rows(B)).to(big.dev)
        differs = (got.view(torch.int32) != want.view(torch.int32)).any(dim=0).nonzero().flatten().cpu().numpy()
        assert np.array_equal(differs, np.sort(lay.doc_of[docs][live])), \
            "the comparison must differ in exactly the docs at or past a boundary that hold tokens"
        one = (got[:1].view(torch.int32) != want[:1].view(torch.int32)).any(dim=0).nonzero().flatten().cpu().numpy()
        assert np.array_equal(one, differs), "query 0 alone shows every one of them"
        # and what the kernel scored is the twin, bit for bit
        big.check(got[:, dst], twin[:B, ex.LQ - 1].astype(np.float32), "score of the wrapped twin", B,
                  docs=dst[None].expand(B, -1))
        with pytest.raises(pytest.fail.Exception, match=r"first at query \d+, doc \d+ \(doclens \d+, planted slots"
                                                        r".*(mid|high) run, \d+ docs at or past byte offset 2\^3[12]"):
            _score_sweep(big)
    finally:
        big.restore()
    _score_sweep(big)


# ---------------------------------------------------------------------------- row strides past 2^31 elements
ROWS, N_ROW = 9, 70001
STRIDES = ((1 << 28) + 4, (1 << 28) + 3)                 # rows 16-B aligned (float4 paths) / not (scalar paths)
GUARD = 4096
POISON = -1515870811                                     # int32 of the bytes A5 A5 A5 A5


@pytest.fixture(scope="module")
def wide(dev):
    """One buffer of 9 rows of 2^28 + 4 floats (9.7 GB), filled with the byte 0xA5."""
    _drop_big()
    buf = torch.empty(ROWS * STRIDES[0] * 4, dtype=torch.uint8, device=dev)
    yield buf.view(torch.float32)
    print(f"\n[high offsets] peak torch.cuda.max_memory_allocated() {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
    del buf
    torch.cuda.empty_cache()


def _place(wide, ld, x):
    """Poison the buffer, write x [B, n] at [b, :n] of stride ld -> the strided view."""
    wide.view(torch.uint8).fill_(0xA5)
    B, n = x.shape
    assert (B - 1) * ld > 1 << 31 and (B - 1) * ld + n <= wide.numel()
    view = torch.as_strided(wide, (B, n), (ld, 1))
    view.copy_(x)
    return view


def _guards_intact(wide, ld, B, n, what):
    w = wide.view(torch.int32)
    for b in range(B):
        a = b * ld
        before = w[max(a - GUARD, 0): a]
        if b > 0:                                         # row 0 starts the buffer
            assert (before == POISON).all(), (what, "before row", b)
        assert (w[a + n: a + n + GUARD] == POISON).all(), (what, "after column n of row", b)


def _row_contents(dev):
    g = torch.Generator(device=dev).manual_seed(N_ROW)
    x = torch.randn(ROWS, N_ROW, device=dev, generator=g)
    x[3:6] = torch.randint(-3, 4, (3, N_ROW), device=dev, generator=g).float()      # heavy integer ties
    x[6:9] *= 1e-3
    x[6:9, ::50000] = 100.0                                                          # a spike
    return x


@pytest.mark.parametrize("ld", STRIDES)
def test_topk_rows_with_a_row_stride_past_2_31(dev, wide, ld):
    x = _row_contents(dev)
    xs = _place(wide, ld, x)
    L = _lib.lib()
    want = {k: orc.topk(x.cpu().numpy(), k) for k in (100, 1100)}
    for sampled in (True, False):
        need = int(L.cbv2_topk_workspace_bytes(ROWS, N_ROW)) if sampled else 0
        assert need > 0 or not sampled
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
        for k in (100, 1100):
            out_s = torch.empty((ROWS, k), dtype=torch.float32, device=dev)
            out_i = torch.empty((ROWS, k), dtype=torch.int32, device=dev)
            _lib.check(L.cbv2_topk_rows(xs.data_ptr(), ROWS, N_ROW, ld, k, 0, ws.data_ptr() if need else None, need,
                                        out_s.data_ptr(), out_i.data_ptr(), _stream_ptr(dev)))
            what = f"cbv2_topk_rows ld={ld} k={k} {'sampled' if sampled else 'radix'}"
            assert torch.equal(out_i.cpu(), _i32(want[k][1])), what
            assert torch.equal(out_s.cpu().view(torch.int32), _f32(want[k][0]).view(torch.int32)), what
            assert torch.equal(xs, x), what + ": the rows were written"
            _guards_intact(wide, ld, ROWS, N_ROW, what)


class _ShapeIndex:
    """An index handle of n chunks that is never scanned: cbv2_groups_create needs its n, id_base and device."""

    def __init__(self, dev, n):
        self.device, self.n, self.id_base = dev, n, 0
        self._tok = torch.zeros(256, dtype=torch.uint8, device=dev)
        self._dl = torch.zeros(n, dtype=torch.int32, device=dev)
        h = ctypes.c_void_p()
        _lib.check(_lib.lib().cbv2_index_create(dev.index or 0, self._tok.data_ptr(), _lib.DTYPE_BF16, n, 128, 128,
                                                self._dl.data_ptr(), 0, ctypes.byref(h)))
        self._h = h

    def close(self):
        _lib.lib().cbv2_index_destroy(self._h)


@pytest.mark.parametrize("ld", STRIDES)
def test_group_topk_rows_with_a_row_stride_past_2_31(dev, wide, ld):
    x = _row_contents(dev)
    xs = _place(wide, ld, x)
    rng = np.random.default_rng(3)
    g = (np.arange(N_ROW) % 501).astype(np.int32)
    g[rng.random(N_ROW) < 0.2] = -1
    shape = _ShapeIndex(dev, N_ROW)
    grp = DocGroups(shape, torch.from_numpy(g), 501)
    L = _lib.lib()
    for k, r in ((100, 1), (501, 3)):
        need = int(L.cbv2_group_topk_workspace_size(grp._h, ROWS, k, r))
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        outs = [torch.empty(s, dtype=t, device=dev) for s, t in (((ROWS, k), torch.float32), ((ROWS, k), torch.int32),
                                                                 ((ROWS, k, r), torch.int32), ((ROWS, k, r), torch.float32))]
        _lib.check(L.cbv2_group_topk_rows(grp._h, xs.data_ptr(), ld, ROWS, k, r, ws.data_ptr(), ws.numel(),
                                          *[o.data_ptr() for o in outs], _stream_ptr(dev)))
        want = gr.oracle(x.cpu().numpy(), g, 501, k, r)
        what = f"cbv2_group_topk_rows ld={ld} k={k} r={r}"
        for name, o, w in zip(("scores", "groups", "ids", "chunk scores"), outs, want):
            assert gr.same_bits(o.cpu().numpy(), w), (what, name)
        assert torch.equal(xs, x), what
        _guards_intact(wide, ld, ROWS, N_ROW, what)
    grp.close()
    shape.close()


@pytest.mark.parametrize("kind", ex.KINDS)
def test_score_with_a_row_stride_past_2_31(dev, wide, kind):
    c = ho.layout(kind, 128).c                                             # 600 exact docs
    x, dl = torch.from_numpy(c.docs_f32()).to(dev), torch.from_numpy(c.doclens).to(dev)
    ix = {"fp32": ColbertIndex.faithful_f32, "mxfp8": ColbertIndex.mxfp8,
          "bf16": lambda t, d: ColbertIndex(t.to(torch.bfloat16), d)}[kind](x, dl)
    B, n = ROWS, c.N
    Q = torch.from_numpy(c.queries_f32()).to(dev)[:B].contiguous()
    want = torch.from_numpy(c.scores(B=B)).to(dev)
    L = _lib.lib()
    for ld in STRIDES:
        wide.view(torch.uint8).fill_(0xA5)
        if kind == "fp32":
            ws = ix._f32_ws(_lib.F32_SCORE, B, ex.LQ, 0)
            _lib.check(L.cbv2_score_f32(ix._h, Q.data_ptr(), B, ex.LQ, ws.data_ptr(), ws.numel() * 4, wide.data_ptr(),
                                        ld, _stream_ptr(dev)))
        else:
            keep, qptr, qdt, _, lq = ix._prep_query(Q, "maxsim")
            _lib.check(L.cbv2_score(ix._h, _lib.SCORERS["maxsim"], qptr, qdt, B, lq, wide.data_ptr(), ld,
                                    _stream_ptr(dev)))
        torch.cuda.synchronize()
        got = torch.as_strided(wide, (B, n), (ld, 1))
        assert (B - 1) * ld > 1 << 31
        assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), (kind, ld)
        _guards_intact(wide, ld, B, n, f"cbv2_score {kind} ld_out={ld}")
    ix.close()
