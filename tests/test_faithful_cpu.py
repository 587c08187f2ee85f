"""CPU: the fp32-faithful index's arithmetic (oracle restatement, no GPU).

The reference keeps fp32 embeddings (local_rag_complete.py:735-746) and scores
them in fp32 (:802-831).  The faithful search scans hi = bf16(x) with bf16(q)
(score T), then rescores every doc with T >= lb - beta(q) (lb: the minimum exact
score of the bf16 top-k; or T >= T_k - 2 beta(q)).  These tests pin
the two facts that make that exact: |T - S| <= beta(q) for every doc, and the
band therefore holds the exact top-k.  (Parity unpinned by reference fixtures:
the reference has no fp32-vs-bf16 case; the exact fp64 MaxSim of the fp32
values is the ground truth.)
"""
import numpy as np
import pytest

from oracle import oracle as orc


def rand_unit(rng, *shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def case(seed, N=600, B=6, lq=32):
    rng = np.random.default_rng(seed)
    docs = rand_unit(rng, N, 128, 128)
    doclens = rng.integers(1, 129, N)
    doclens[:5] = 128
    Q = rand_unit(rng, B, lq, 128)
    # a few near-duplicates of query tokens so the top of the ranking is structured
    for b in range(B):
        docs[10 * b, :lq] = Q[b] + 0.05 * rand_unit(rng, lq, 128)
        doclens[10 * b] = 128
    return docs, doclens, Q


def test_split_reconstructs_and_matches_bf16_cast():
    import torch
    docs, doclens, _ = case(0, N=60)
    hi, lo, (E, M) = orc.split_f32(docs, doclens)
    np.testing.assert_array_equal(hi, torch.from_numpy(docs).bfloat16().float().numpy())
    err = np.abs(docs.astype(np.float64) - hi - lo)
    assert err.max() <= 2.0 ** -16 * np.abs(docs).max()
    assert 0 < E <= 2.0 ** -8 * 1.001 and 0.99 < M < 1.01


def test_bf16_scan_within_beta_of_exact():
    docs, doclens, Q = case(1)
    hi, _, (E, M) = orc.split_f32(docs, doclens)
    S = orc.maxsim(Q, docs, doclens)                                   # exact fp64 on the fp32 values
    T = orc.maxsim(orc.bf16_round(Q), hi, doclens)                     # the bf16 scan (exact products)
    beta = orc.band_beta(Q, E, M)
    dev = np.abs(T - S).max(axis=1)
    assert (dev <= beta).all(), (dev, beta)
    # the bound is what the certificate pays for: bf16 alone misses the 1e-3 tolerance
    assert dev.max() > 1e-4


def test_band_contains_exact_topk():
    docs, doclens, Q = case(2, N=1500)
    hi, _, (E, M) = orc.split_f32(docs, doclens)
    S = orc.maxsim(Q, docs, doclens)
    T = orc.maxsim(orc.bf16_round(Q), hi, doclens)
    beta = orc.band_beta(Q, E, M)
    k = 50
    _, ids_exact = orc.topk(S, k)
    for b in range(Q.shape[0]):
        tk = np.sort(T[b])[::-1][k - 1]
        band = set(np.nonzero(T[b] >= tk - 2 * beta[b])[0].tolist())
        assert set(ids_exact[b].tolist()) <= band
        assert len(band) < len(T[b])          # the band is a real filter on this data


def test_maxsim_additive_over_query_token_blocks():
    """The identity the long-query path (ColbertIndex._query_blocks) rests on:
    MaxSim sums over query tokens (LRC:807-812), so a query's score is the sum
    of its 32-token blocks' scores -- checked on the oracle in float64, with
    ragged and empty docs."""
    import numpy as np
    from oracle import oracle as orc
    g = np.random.default_rng(4)
    Q = g.standard_normal((3, 70, 128))
    docs = g.standard_normal((50, 128, 128))
    doclens = g.integers(0, 129, 50)
    full = orc.maxsim(Q, docs, doclens)
    parts = sum(orc.maxsim(Q[:, a:a + 32], docs, doclens) for a in range(0, 70, 32))
    fin = np.isfinite(full)
    assert (np.isneginf(full) == np.isneginf(parts)).all()
    np.testing.assert_allclose(parts[fin], full[fin], rtol=0, atol=1e-9)


def test_lower_bound_band_contains_exact_topk_and_is_narrower():
    """The two-pass band of cbv2_search_f32 (CBV2_OPT_BAND_LOWER_BOUND): lb =
    the minimum exact score of the k docs the bf16 scan ranks first is a lower
    bound of the exact k-th score, so every exact top-k doc has T >= lb - beta;
    that band is no wider than T >= T_k - 2 beta (lb >= T_k - beta)."""
    for seed, k in ((3, 10), (4, 50), (5, 100)):
        docs, doclens, Q = case(seed, N=1500)
        hi, _, (E, M) = orc.split_f32(docs, doclens)
        S = orc.maxsim(Q, docs, doclens)
        T = orc.maxsim(orc.bf16_round(Q), hi, doclens)
        beta = orc.band_beta(Q, E, M)
        _, tk = orc.topk(T, k)                                  # the bf16 scan's top-k (ids)
        lb = np.array([S[b, tk[b]].min() for b in range(len(Q))])
        _, ek = orc.topk(S, k)                                  # the exact top-k
        Tk = orc.topk(T, k)[0][:, -1]
        for b in range(len(Q)):
            band_lb = T[b] >= lb[b] - beta[b]
            band_plain = T[b] >= Tk[b] - 2 * beta[b]
            assert band_lb[ek[b]].all(), (seed, b)
            assert lb[b] >= Tk[b] - beta[b] - 1e-12
            assert band_lb.sum() <= band_plain.sum()


def _exact_topk_in(band, ids):
    return bool(band[ids].all())


@pytest.mark.parametrize("lq", [32, 7])
def test_adversarial_residuals_approach_the_bound(lq):
    """Docs whose residuals are aligned with a bf16-exact query
    (tests/_adversarial.py): |T - F| reaches 0.82 .. 0.88 beta (random unit
    vectors: 0.03), the bf16 top-k is the anti-aligned decoys and the exact
    top-k the aligned hidden docs, 1.35 .. 1.50 beta below T_k and 0.525 ..
    0.64 beta below lb.  The documented bands hold the exact top-k; the same
    bands with beta / 2, and the one-pass band T_k - beta, do not."""
    import _adversarial as adv
    k = 10
    c = adv.adversarial_case(lq, N=600, B=4, lq=lq, K=k)
    r = adv.check_preconditions(c, k)
    T, F, beta, Tk, lb = r["T"], r["F"], r["beta"], r["Tk"], r["lb"]
    S = orc.maxsim(c.Q, c.docs, c.doclens)
    fin = np.isfinite(S)
    assert np.abs(F[fin] - S[fin]).max() <= 1e-4          # only lo's own rounding and nothing else is dropped
    assert (np.abs(T[fin] - S[fin]).reshape(-1) <= np.repeat(beta, T.shape[1])[fin.reshape(-1)]).all()
    _, ek = orc.topk(S, k)
    for b in range(len(c.Q)):
        assert set(ek[b].tolist()) == set(c.hidden[b].tolist())
        assert not set(ek[b].tolist()) & set(orc.topk(T[b:b + 1], k)[1][0].tolist())
        assert _exact_topk_in(T[b] >= lb[b] - beta[b], ek[b])
        assert _exact_topk_in(T[b] >= Tk[b] - 2 * beta[b], ek[b])
        assert (T[b] >= lb[b] - beta[b]).sum() == 2 * k == (T[b] >= Tk[b] - 2 * beta[b]).sum()
        # the test discriminates: half of beta, or one beta in the one-pass band, loses exact top-k docs
        assert not _exact_topk_in(T[b] >= lb[b] - beta[b] / 2, ek[b])
        assert not _exact_topk_in(T[b] >= Tk[b] - 2 * (beta[b] / 2), ek[b])
        assert not _exact_topk_in(T[b] >= Tk[b] - beta[b], ek[b])


@pytest.mark.parametrize("lq", [32, 7])
def test_query_residuals_aligned_with_docs_stay_within_beta(lq):
    """The eq * M term: fp32 queries whose residual q - bf16(q) is 0.49 ulp per
    element with the sign of bf16(q), against docs that are copies of bf16(q)
    in a bf16-exact corpus (E = 0: beta is this term and the slack).  |T - S|
    <= beta for every doc; measured here, the copies reach |T - S| / beta =
    0.89 at lq = 32 and at lq = 7 (the rest is the slack term), the random
    fillers 0.22 .. 0.24 (the residual is nearly parallel to the query itself,
    so every doc's T - S is about -T / 181)."""
    import _adversarial as adv
    rng = np.random.default_rng(500 + lq)
    docs, doclens, _ = case(100 + lq, N=300, lq=lq)
    docs = orc.bf16_round(docs)                      # a bf16-exact corpus: E = 0, beta is the eq * M term and the slack
    qh = orc.bf16_round(rand_unit(rng, 4, lq, 128))
    Q = np.stack([adv.with_residual(qh[b], qh[b], 1.0) for b in range(4)])
    assert np.array_equal(orc.bf16_round(Q), qh)
    for b in range(4):
        docs[20 * b + 3, :lq] = qh[b]
        doclens[20 * b + 3] = 128
    hi, _, (E, M) = orc.split_f32(docs, doclens)
    assert E == 0
    S = orc.maxsim(Q, docs, doclens)
    T = orc.maxsim(qh, hi, doclens)
    beta = orc.band_beta(Q, E, M)
    ratio = np.abs(T - S) / beta[:, None]
    assert (ratio <= 1).all(), ratio.max()
    planted = np.array([ratio[b, 20 * b + 3] for b in range(4)])
    print("query-side |T - S| / beta:", planted, "fillers:", np.delete(ratio, [3, 23, 43, 63], axis=1).max())
    assert (planted >= 0.8).all(), planted        # the eq * M term is exercised, not idle


def test_beta_holds_for_non_unit_norms():
    """Token norms spread over 2^-6 .. 2^6, one outlier row (2^6 * 1.5) setting
    M, query norms over 2^-2 .. 2^2: |T - S| <= beta still holds for every
    doc.  (E and M are maxima over the corpus, so the bound is loose here:
    max |T - S| / beta = 0.024.)"""
    rng = np.random.default_rng(9)
    docs, doclens, Q = case(9, N=400, B=4)
    docs *= np.exp2(rng.uniform(-6, 6, docs.shape[:2])).astype(np.float32)[..., None]
    docs[7, 3] *= np.float32(96.0 / np.linalg.norm(docs[7, 3]))
    doclens[7] = 128
    Q = Q * np.exp2(rng.uniform(-2, 2, Q.shape[:2])).astype(np.float32)[..., None]
    hi, _, (E, M) = orc.split_f32(docs, doclens)
    assert 95.0 < M < 97.0 and E > 0.1
    S = orc.maxsim(Q, docs, doclens)
    T = orc.maxsim(orc.bf16_round(Q), hi, doclens)
    beta = orc.band_beta(Q, E, M)
    ratio = np.abs(T - S) / beta[:, None]
    print("non-unit norms |T - S| / beta:", ratio.max())
    assert (ratio <= 1).all() and ratio.max() > 0
