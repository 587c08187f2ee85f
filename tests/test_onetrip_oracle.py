"""CPU: the one-trip tests' exact pipeline (tests/_onetrip_oracle.py) itself.

* the two corpora are what the GPU tests need them to be (negative scores,
  -inf and ties pass through corpus A ranked whole; corpus B's top-100 is
  positive with ties) -- their own assertions run when they are built;
* the hand-built stage-1 lists hold a row of every kind;
* the pipeline's fusion (orc.rrf on the lists with ids < 0 stripped, [:C], -1
  padded) equals the native host fusion cbv2_rrf_fuse on the raw lists,
  repeated ids, out-of-range ids and all-padding rows included;
* the select orders negative and -inf scores and -1 padding as (score desc,
  position asc), and rows past C are -inf / -1 / -1."""
import numpy as np

import _onetrip_oracle as oto
from hybrid_rag_colbertv2_amd.hybrid import rrf_fuse


def test_corpora_and_stage1_rows():
    a, b = oto.corpus_a(), oto.corpus_b()
    assert len(a.empty) == 3 and not set(a.empty.tolist()) & set(a.g.planted_flat.tolist())
    rows = list(range(8))
    lex = oto.stage1_lists(a, rows, 16, a.N)
    assert lex.shape == (8, 16) and lex.dtype == np.int32
    top = a.topk(a.N)[1]
    assert set(a.g.planted[0].tolist()) <= set(lex[0].tolist())                       # planted
    assert set(a.empty.tolist()) <= set(lex[1].tolist())                              # empty docs
    sc = a.g.exact_scores([2], lex[2:3])[0]
    assert (sc[:10] < 0).all() and np.isfinite(sc[:10]).all()                         # negative scores
    assert (lex[3] >= a.N).sum() >= 3 and lex[3].max() == oto.INT32_MAX               # at or past N
    assert (lex[5][8:] == -1).all() and (lex[5][:8] >= 0).all()                       # a -1 tail
    assert (lex[6] == -1).all()                                                       # all -1
    assert lex[7][8] == lex[7][0] and len(set(lex[7].tolist())) == 15                 # one id repeated
    lexb = oto.stage1_lists(b, [4], 100, 100, rot=4)                                  # absent from the top-k
    assert not set(lexb[0][:50].tolist()) & set(b.topk(100)[1][4].tolist())
    assert top.shape == (8, 256)
    low = oto.stage1_lists(b, rows, 100, 100, low_ids=True)
    assert ((low[4] >= 1) & (low[4] <= 400)).all()          # the fill: small ids only
    assert ((low >= 1) & (low <= 400)).mean() > 0.6


def test_pipeline_fusion_equals_native_rrf_and_select_rules():
    for c, k, kb, C, fk in ((oto.corpus_a(), 256, 16, 300, 300), (oto.corpus_b(), 20, 16, 64, 64),
                            (oto.corpus_b(), 100, 100, 50, 60), (oto.corpus_b(), 1, 1, 1, 1)):
        rows = list(range(8))
        lex = oto.stage1_lists(c, rows, kb, k)
        cand = []
        s, i, p = oto.pipeline(c, rows, lex, k, C, fk, cand_out=cand)
        cand = np.array(cand, np.int32)
        ids2 = c.topk(k)[1][rows]
        assert np.array_equal(cand, rrf_fuse(lex, ids2, rrf_k=oto.RRF_K, C=C)), "fusion differs from cbv2_rrf_fuse"
        m = min(C, fk)
        assert (p[:, m:] == -1).all() and (i[:, m:] == -1).all() and np.isneginf(s[:, m:]).all()
        for r, b in enumerate(rows):
            sc = c.g.exact_scores([b], cand[r:r + 1])[0]
            assert sorted(p[r, :m].tolist()) == sorted(set(p[r, :m].tolist())) and (p[r, :m] >= 0).all()
            assert np.array_equal(i[r, :m], cand[r, p[r, :m]])
            assert np.array_equal(oto.bits(s[r, :m]), oto.bits(sc[p[r, :m]]))
            key = list(zip((-sc[p[r, :m]]).tolist(), p[r, :m].tolist()))
            assert key == sorted(key), "not (score desc, position asc)"
            if m == C:
                assert sorted(p[r, :m].tolist()) == list(range(C))
