"""GPU: non-finite padding rows never reach a score, on any path.

The header promises that rows t >= doclens[i] of a doc never score and that no
value outside the stated extents influences a result; the handle borrows the
caller's arrays, so an uncleared or 0xFF-filled allocation puts NaN and Inf
encodings into padding rows (and, for MXFP8, into their scale bytes).  Every
MaxSim kernel masks a partly filled 16-row tile additively (the accumulator of
a padding row starts at -inf, the MFMA adds the row's products on top, an fmaxf
chain folds the rows), which is right only as long as every later max drops
the NaN that non-finite padding makes of that accumulator.  The exact corpora
elsewhere hold a finite winning row in their padding and the guard-band arena
avoids NaN on purpose, so nothing else in the suite would see such a leak.

Here the padding rows of the pools of tests/test_gpu_exact_scores.py are
overwritten on the device (tests/_padding.py: modes "nan" and "inf", several
patterns per tile) and the handle is built from the poisoned arrays with the raw
ColbertIndex(tokens, doclens, residual= / bounds= / scales=) constructors, the
bounds those of the clean split.  The reference is a function of the scoring
rows only (tests/test_nonfinite_padding_model.py), so every call must return
the same bits as on clean padding, the -inf of the empty docs included:
  test_dispatch_sweep     the sweeps of tests/test_gpu_exact_scores.py: score at
                          every batch size of the dispatch table (dense docs on
                          at B <= 4, both rescore splits), every query length
                          1 .. 32 at one B per branch, the faithful search with
                          its band and with the forced cap = k fallback, and the
                          rerank set B = 3 / 40 x C = 50 / 1100 with and without
                          workspace (bf16, MXFP8) and through cbv2_rerank_f32.
  test_small_walks /      a stratified subset of the committed walks of
  test_large_walks        tests/test_gpu_walk.py (tests/_walk_seeds.PADDING_SEEDS)
                          on poisoned pools; the player also fills the query
                          buffer past each step's B * lq rows with the mode's
                          values.
  test_split_* / test_means_*   the preparation kernels read a poisoned f32
                          source matrix: cbv2_split_f32 (directly and through
                          IndexBuilder in two batches) and
                          cbv2_index_build_means give the clean bits on every
                          scoring row, bound and mean.
No score, query row or score matrix is made non-finite.

Result on an MI355X: all 60 cases pass in both modes; no path leaked.

Run time, measured on an MI355X, this file alone (60 tests, 24.5 s, of which the
twelve pools take 14.4 s: they fall to whichever test of a session first needs
them, in the suite's order tests/test_gpu_exact_scores.py):
  test_dispatch_sweep   0.02-0.10 s per case after its pool (0.7-2.0 s of setup
                        on the "nan" case of each (kind, ld), run alone)
  test_small_walks      3-11 walks, 26-115 steps, 0.07-0.31 s per case
  test_large_walks      two walks each: bf16 0.27 s, MXFP8 0.31-0.33 s, fp32
                        0.54-0.57 s
  test_split_f32_of_a_poisoned_matrix  0.03-0.09 s, test_means_of_a_poisoned_matrix 0.03 s
"""
import pytest
import torch

import _exact as ex
import _padding as pad
import _walk_seeds as ws
import test_gpu_exact_scores as es
import test_gpu_walk as gw
from hybrid_rag_colbertv2_amd import index as index_mod
from hybrid_rag_colbertv2_amd.index import ColbertIndex, IndexBuilder

pytestmark = pytest.mark.gpu

MODES = pad.MODES
RERANK_SHAPES = tuple((B, C) for B in (3, 40) for C in (50, 1100))


def _clean(kind, ld, dev):
    """The clean case of tests/test_gpu_exact_scores.py: its pool, reference and index are built once per session."""
    if (kind, ld) not in es._cases:
        torch.cuda.empty_cache()
        es._cases[kind, ld] = es._Case(kind, ld, dev)
    return es._cases[kind, ld]


def _second(ix):
    return ix.residual if ix.faithful else ix.scales


def _raw_index(kind, tokens, second, doclens, bounds):
    if kind == "fp32":
        return ColbertIndex(tokens, doclens, residual=second, bounds=bounds)
    if kind == "mxfp8":
        return ColbertIndex(tokens, doclens, scales=second)
    return ColbertIndex(tokens, doclens)


def _scoring(doclens, ld):
    return torch.arange(ld, device=doclens.device)[None, :] < doclens[:, None]


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class _Poisoned(es._Case):
    """A case of tests/test_gpu_exact_scores.py on the same pool, reference and
    queries, its index built from poisoned clones of the clean index's device
    arrays."""

    def __init__(self, clean, mode):
        self.kind, self.ld, self.dev, self.c, self.ref, self.Q = clean.kind, clean.ld, clean.dev, clean.c, clean.ref, clean.Q
        self.mode = mode
        cix = clean.ix
        self.tokens, self.second = pad.poison(self.kind, cix.tokens, _second(cix), cix.doclens, mode)
        self.doclens, self.bounds = cix.doclens, cix.bounds
        keep = _scoring(cix.doclens, self.ld)
        for new, old in ((self.tokens, cix.tokens), (self.second, _second(cix))):
            if old is not None:                      # the scoring rows bit for bit, every padding row changed
                assert torch.equal(_bits(new)[keep], _bits(old)[keep])
                assert (_bits(new)[~keep] != _bits(old)[~keep]).any(dim=1).all()
        if self.kind != "mxfp8" and mode == "nan":
            assert torch.isnan(self.tokens[~keep].float()).all()
        self.ix = _raw_index(self.kind, self.tokens, self.second, self.doclens, self.bounds)
        assert self.ix.faithful == (self.kind == "fp32") and self.ix.fp8 == (self.kind == "mxfp8")

    def tripled(self):
        rep = [None if x is None else x.repeat(3, 1, 1) for x in (self.tokens, self.second)]
        return _raw_index(self.kind, rep[0], rep[1], self.doclens.repeat(3), self.bounds)

    def check(self, got, want, what, B, lq=ex.LQ, docs=None):
        super().check(got, want, f"[padding rows poisoned: {self.mode}] {what}", B, lq, docs)


_poisoned = {}


@pytest.fixture
def poisoned(request, dev):
    kind, ld, mode = request.param
    if request.param not in _poisoned:
        _poisoned[request.param] = _Poisoned(_clean(kind, ld, dev), mode)
    yield _poisoned[request.param]
    _poisoned[request.param].options()


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    for case in _poisoned.values():
        case.ix.close()
    _poisoned.clear()
    gw._bufs.clear()
    gw._pool_devs.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


CASES = [(kind, ld, mode) for kind, ld in es.CASES for mode in MODES]
IDS = [f"{k}-{ld}-{m}" for k, ld, m in CASES]


# ---------------------------------------------------------------------------- the dispatch sweep
@pytest.mark.parametrize("poisoned", CASES, indirect=True, ids=IDS)
def test_dispatch_sweep(poisoned):
    case = poisoned
    es.sweep_score(case)
    es.sweep_query_lengths(case)
    if case.kind == "fp32":
        es.sweep_faithful_search(case)
        es.sweep_faithful_rerank(case, RERANK_SHAPES)
    else:
        es.sweep_rerank(case, RERANK_SHAPES)


# ---------------------------------------------------------------------------- the walks
@pytest.mark.parametrize("kind,ld,mode", CASES, ids=IDS)
def test_small_walks(dev, kind, ld, mode):
    gw._play(dev, ws.padding_walks(kind, ld, mode), gw.WS_SMALL, padding=mode)


LARGE = [(kind, mode) for kind in ex.KINDS for mode in MODES]


@pytest.mark.parametrize("kind,mode", LARGE, ids=[f"{k}-{m}" for k, m in LARGE])
def test_large_walks(dev, kind, mode):
    """The block-max select, block skip, folded keys and the dynamic tail at 65,536+ docs gathered from the poisoned pool."""
    keys = [key for key in ws.committed_large() if key[0] == kind and key[2] < ws.PADDING_LARGE]
    assert len(keys) == ws.PADDING_LARGE
    gw._play(dev, keys, gw.WS_LARGE, padding=mode)


# ---------------------------------------------------------------------------- the preparation kernels
SPLIT = [("fp32", ld, mode) for ld in (128, 256) for mode in MODES]


def _check_split(ix, clean, what):
    keep = _scoring(clean.ix.doclens, clean.ld)
    assert ix.bounds == clean.ix.bounds, (what, ix.bounds, clean.ix.bounds)
    assert torch.equal(_bits(ix.tokens)[keep], _bits(clean.ix.tokens)[keep]), f"{what}: hi scoring rows"
    assert torch.equal(_bits(ix.residual)[keep], _bits(clean.ix.residual)[keep]), f"{what}: lo scoring rows"


@pytest.mark.parametrize("kind,ld,mode", SPLIT, ids=[f"{ld}-{m}" for _, ld, m in SPLIT])
def test_split_f32_of_a_poisoned_matrix(dev, monkeypatch, kind, ld, mode):
    clean = _clean(kind, ld, dev)
    c, dl = clean.c, clean.ix.doclens
    x = pad.poison_f32(torch.from_numpy(c.docs_f32()).to(dev), dl, mode)
    keep = _scoring(dl, ld)
    assert (torch.isnan(x[~keep]).all() if mode == "nan" else not torch.isfinite(x[~keep]).all())
    ix = ColbertIndex.faithful_f32(x, dl)
    _check_split(ix, clean, "cbv2_split_f32")
    assert not torch.isfinite(ix.tokens[~keep].float()).all()            # the padding is split too, and is non-finite
    B = 9
    clean.check(ix.score(clean.queries(B)), clean.want(B), f"score of the split of a poisoned matrix ({mode})", B)
    ix.close()
    # the same through IndexBuilder in two batches (the bounds accumulate): its packer zeroes padding, so the
    # batches are handed to it packed, padding as poisoned
    monkeypatch.setattr(index_mod, "_as_batch", lambda embs, device, dtype, ld=None: embs)
    b = IndexBuilder(c.N, dev, "fp32", ld=ld)
    cut = c.N // 2 + 1
    assert b.append((x[:cut], dl[:cut])) == cut and b.append((x[cut:], dl[cut:])) == c.N - cut
    ix = b.finish()
    _check_split(ix, clean, "IndexBuilder, two batches")
    clean.check(ix.score(clean.queries(B)), clean.want(B), f"score of a built index ({mode})", B)
    ix.close()


@pytest.mark.parametrize("mode", MODES)
def test_means_of_a_poisoned_matrix(dev, mode):
    n, B, lq = 130, 17, 7
    clean = _clean("bf16", 128, dev)
    c = clean.c
    dl = clean.ix.doclens[:n].contiguous()
    assert (dl < 128).sum() > n // 2                                      # most docs have padding rows
    x = torch.from_numpy(c.docs_f32()[:n]).to(dev)
    Q = clean.Q[:B, :lq].contiguous()
    ix = ColbertIndex(clean.ix.tokens[:n].contiguous(), dl)
    ix.build_means(x)
    want_means, want = ix.means.clone(), ix.score(Q, scorer="ref_meanpool_cosine").clone()
    assert torch.isfinite(want).all()
    tok, _ = pad.poison("bf16", clean.ix.tokens[:n].contiguous(), None, dl, mode)
    px = ColbertIndex(tok, dl)
    px.build_means(pad.poison_f32(x, dl, mode))
    assert torch.equal(_bits(px.means), _bits(want_means)), "cbv2_index_build_means read a padding row"
    got = px.score(Q, scorer="ref_meanpool_cosine")
    assert torch.equal(_bits(got.contiguous()), _bits(want.contiguous()))
    ix.close()
    px.close()
