"""CPU: the sparse full-size layouts of tests/_highoffset.py are what
tests/test_gpu_high_offsets.py needs them to be -- the runs straddle byte
offsets 2^31 and 2^32, each side of each boundary holds an empty, a 1-token, a
full and a ragged doc, and the index a kernel with a wrapped address would see
(the wrapped twin) scores differently from the true one in EVERY doc at or past
a boundary, for query 0 alone already.  (A doc below its boundary keeps its
offset under the 31- / 32-bit mask: its twin is the doc itself.)
"""
import numpy as np
import pytest

import _exact as ex
import _highoffset as ho

CASES = [(kind, ld) for kind in ex.KINDS for ld in ho.LDS]


@pytest.fixture(scope="module", params=CASES, ids=[f"{k}-{ld}" for k, ld in CASES])
def lay(request):
    return ho.layout(*request.param)


def test_runs_straddle_their_boundaries(lay):
    assert lay.docbytes == lay.ld * (128 if lay.kind == "mxfp8" else 256)
    assert lay.d31 * lay.docbytes == 1 << 31 and lay.d32 * lay.docbytes == 1 << 32
    assert lay.n_total == lay.d32 + lay.W and lay.n_total * lay.docbytes > 1 << 32
    assert sum(lay.sizes) == lay.W and min(lay.sizes) >= lay.W // 3 and lay.starts[0] == 0
    for r, k in ((1, 31), (2, 32)):
        first, last = lay.starts[r], lay.starts[r] + lay.sizes[r] - 1
        assert first * lay.docbytes < 1 << k <= last * lay.docbytes + lay.docbytes
        assert last < lay.n_total
    assert lay.starts[0] + lay.sizes[0] <= lay.starts[1] and lay.starts[1] + lay.sizes[1] <= lay.starts[2]
    # a bijection of the corpus onto the three runs
    assert np.array_equal(np.sort(lay.doc_of), lay.pos_doc)
    assert np.array_equal(lay.corpus_at[lay.doc_of], np.arange(lay.W))
    assert (lay.corpus_at >= 0).sum() == lay.W
    assert np.array_equal(lay.doclens[lay.doc_of], lay.c.doclens) and (lay.doclens > 0).sum() == (lay.c.doclens > 0).sum()


def test_every_side_of_every_boundary_holds_the_edge_lengths(lay):
    dl = lay.c.doclens
    for r, bnd in ((1, lay.d31), (2, lay.d32)):
        for past in (False, True):
            side = dl[(lay.run_of == r) & ((lay.doc_of >= bnd) == past)]
            assert len(side) >= 4
            assert (side == 0).any() and (side == 1).any() and (side == lay.ld).any() and (side % 16 != 0).any(), \
                (ho.RUNS[r], past, sorted(side.tolist()))
    # the base plan's special lengths all survive the amendment
    assert set(ex.special_doclens(lay.ld)) <= set(dl.tolist())


def test_expected_rows_are_the_reference_in_place(lay):
    for lq in ho.SCORE_LQS:
        rows = lay.expected_rows(lq)
        assert rows.shape == (lay.B, lay.n_total) and rows.dtype == np.float32
        assert np.array_equal(rows[:, lay.doc_of].astype(np.float64), lay.c.ref[:, lq - 1])
        filler = np.ones(lay.n_total, bool)
        filler[lay.doc_of] = False
        assert np.isneginf(rows[:, filler]).all()
        assert np.array_equal(np.isfinite(rows[0]), lay.doclens > 0)


def test_wrapped_twin_differs_in_every_wrapped_doc(lay):
    """The twin condition, for B = 1 (query 0 alone) and every B the GPU file scores."""
    docs, twin = lay.wrapped_twin()
    # every doc at or past a boundary, and none below: a wrapped read of the mid run lands in the low run
    past = ((lay.run_of == 1) & (lay.doc_of >= lay.d31)) | ((lay.run_of == 2) & (lay.doc_of >= lay.d32))
    assert np.array_equal(docs, np.flatnonzero(past)) and len(docs) >= lay.W // 3 - 2
    src = lay.wrapped_source()
    assert np.array_equal(src, lay.doc_of[docs] - np.where(lay.run_of[docs] == 1, lay.d31, lay.d32))
    assert (lay.corpus_at[src] >= 0).all() and (lay.run_of[lay.corpus_at[src]] == 0).all()
    live = lay.c.doclens[docs] > 0
    assert live.sum() >= len(docs) - ho.EXTRA - 1
    true = lay.c.ref[:, :, docs]
    assert np.isneginf(twin[:, :, ~live]).all()
    for lq in ho.SCORE_LQS:
        for B in sorted({1, *ho.score_batches(lay.kind, lay.ld)}):
            differs = (twin[:B, lq - 1] != true[:B, lq - 1]).any(axis=0)
            assert differs[live].all(), (lay.kind, lay.ld, lq, B, docs[live & ~differs].tolist())
