"""Adversarial corpora for the faithful search's band certificate (numpy, no GPU).

The faithful search is exact because |T - F| <= beta(q) for every doc (T: the
bf16 scan's score, F: the faithful score; include/colbert_mi355x.h under
cbv2_search_f32).  On random unit vectors the residuals x - bf16(x) are
uncorrelated with the query and |T - F| / beta stays near 0.03, so a beta 30
times too small passes every test built on such data.  ``adversarial_case``
builds docs whose residuals are ALIGNED with a bf16-exact query:

* a planted doc's token i is the query's token i (hi = q_i), each element
  moved by 0.49 ulp(bf16) with the sign of the query element (aligned: F > T)
  or the opposite sign (anti-aligned: F < T); where such a move would change
  hi (an exact power of two moved toward zero: the binade below has half the
  ulp) the move is halved until hi stays put;
* per query, K DECOYS are anti-aligned and have the highest T (decoy j's hi is
  stepped toward zero, one bf16 ulp per element, until T has dropped by
  ``decoy_step * j`` beta: no ties);
* K HIDDEN docs are aligned, their hi stepped toward zero until T sits
  ``(hidden_gap + 0.01 j) beta`` below lb, the least faithful score of the
  query's decoys (computed here, so the placement does not depend on how
  well a particular query's residuals align).

So the bf16 scan ranks the decoys first and the hidden docs well below its
k-th score, while the faithful top-k is exactly the hidden docs: a search
finds them only if its band reaches as far down as the certificate says.

Measured (float64, seeds 0..7, N = 600, K = k = 10, B = 4, hidden_gap = 0.53,
decoy_step = 0.005; beta ~ 0.105 at lq = 32, ~ 0.0224 at lq = 7):

    (F - T) / beta of the planted docs    +0.82 .. +0.88 / -0.88 .. -0.82
    (b) (T_k - T_h) / beta                1.35 .. 1.50    (asserted in [1.30, 1.55))
    (b) (lb  - T_h) / beta                0.525 .. 0.64   (asserted in [0.50, 0.70))
    (c) min F(hidden) - max F(other)      >= 0.155 beta   (asserted >= 0.10)
    (d) max |T - F| / beta                0.82 .. 0.88    (asserted in [0.8, 1])
    (e) fillers                           T < T_k - 220 beta  (asserted < T_k - 2 beta)

(The B = 12 corpora of the GPU tests, where E is a maximum over more queries:
(b) 1.34 .. 1.49 and 0.52 .. 0.63, (c) >= 0.15, (d) 0.817 .. 0.86.)

Every hidden doc thus lies below ``lb - beta / 2`` and below ``T_k - beta``:
halving beta (in either band), or a one-pass band of T_k - beta, loses all of
them, and so does any beta below 0.52 (two-pass) / 0.67 (one-pass) of its value,
while the documented bands ``T >= lb - beta`` and ``T >= T_k - 2 beta`` hold
them with >= 0.36 beta / 0.50 beta to spare.  The hidden docs are not pushed
further down so that (c) -- their lead in F -- stays far above fp32
accumulation noise (0.10 beta ~ 0.01 at lq = 32, ~ 0.002 at lq = 7, against
~ 1e-5).

``groups`` > 1 plants that many sets of decoys and hidden docs per query, set
g in the g-th of ``groups`` equal id ranges (one per shard of a sharded
search) with its own lb, its hidden docs another 0.005 g beta lower so no
two tie.
"""
from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc

RESID = 0.49            # residual per element, in bf16 ulps of hi
HIDDEN_GAP = 0.53       # lb - T of hidden doc 0, in beta
DECOY_STEP = 0.005      # T drop between successive decoys, in beta


@dataclass
class Case:
    docs: np.ndarray        # f32 [N, 128, 128]
    doclens: np.ndarray     # int32 [N]
    Q: np.ndarray           # f32 [B, lq, 128], bf16-exact
    decoys: np.ndarray      # int64 [B, groups * K] doc ids (group-major)
    hidden: np.ndarray      # int64 [B, groups * K]
    K: int
    groups: int

    def shard(self, g):
        """Group g's id range as a case of its own (ids local to the range)."""
        n = len(self.docs) // self.groups
        a, K = g * n, self.K
        return Case(self.docs[a:a + n], self.doclens[a:a + n], self.Q, self.decoys[:, g * K:(g + 1) * K] - a,
                    self.hidden[:, g * K:(g + 1) * K] - a, K, 1)


def rand_unit(rng, *shape):
    x = rng.standard_normal(shape).astype(np.float32)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def bf16_ulp(v):
    """ulp of the bf16 binade of each (bf16-exact, nonzero) value, float64."""
    _, e = np.frexp(np.abs(v.astype(np.float64)))          # |v| = f 2^e, f in [0.5, 1)
    return np.where(v != 0, np.exp2(e - 8.0), 0.0)


def step_toward_zero(hi, q, drop, rng):
    """Step elements of hi (bf16-exact f32 [lq, 128]) toward zero, one bf16 ulp
    each and in random order (again from the start if one round is not
    enough), until <q, hi> summed over the rows has dropped by at least
    ``drop``.  Returns the stepped copy."""
    bits = orc.to_bf16_bits(hi).reshape(-1)
    qf = q.astype(np.float64).reshape(-1)
    while drop > 0:
        cur = orc.from_bf16_bits(bits).astype(np.float64)
        nxt = orc.from_bf16_bits(bits - 1).astype(np.float64)     # sign-magnitude: one ulp toward zero
        gain = qf * (cur - nxt)                                   # >= 0: hi has q's signs
        order = rng.permutation(len(bits))
        cum = np.cumsum(gain[order])
        m = int(np.searchsorted(cum, drop)) + 1
        take = order[:m]
        bits = bits.copy()
        bits[take] -= 1
        drop -= cum[min(m, len(cum)) - 1]
    return orc.from_bf16_bits(bits).reshape(hi.shape)


def with_residual(hi, q, sign):
    """f32 tokens hi + sign * sign(q) * RESID ulp(hi), the move halved wherever
    bf16() of the result would not be hi."""
    h = hi.astype(np.float64)
    move = sign * np.sign(q.astype(np.float64)) * RESID * bf16_ulp(hi)
    for _ in range(4):
        x = (h + move).astype(np.float32)
        bad = orc.bf16_round(x) != hi
        if not bad.any():
            return x
        move = np.where(bad, move / 2, move)
    raise AssertionError("a residual changed hi")


def adversarial_case(seed, N=600, B=4, lq=32, K=10, groups=1, hidden_gap=HIDDEN_GAP, decoy_step=DECOY_STEP,
                     filler=True):
    """-> Case (see the module docstring).  filler=False leaves the filler docs
    empty (doclens 0, tokens zero) for a caller that generates its own."""
    rng = np.random.default_rng(seed)
    assert N % groups == 0 and 2 * K * B <= (N // groups) * 4 // 5
    Q = orc.bf16_round(rand_unit(rng, B, lq, 128))
    if filler:
        docs = rand_unit(rng, N, 128, 128)
        doclens = rng.integers(1, 129, N).astype(np.int32)
        doclens[rng.choice(N, max(N // 100, 2), replace=False)] = 0          # a few empty docs
    else:
        docs = np.zeros((N, 128, 128), np.float32)
        doclens = np.zeros(N, np.int32)
    n = N // groups
    decoys = np.empty((B, groups * K), np.int64)
    hidden = np.empty((B, groups * K), np.int64)
    # beta before any doc is stepped, for the decoys' spacing: E from the
    # full-size residual of each query's own tokens, M from the fillers and the queries
    proto = np.stack([with_residual(Q[b], Q[b], 1.0) for b in range(B)])
    _, _, (E0, _) = orc.split_f32(proto)
    M0 = max(orc.split_f32(docs, doclens)[2][1], float(np.linalg.norm(Q.astype(np.float64), axis=-1).max()))
    beta0 = orc.band_beta(Q, E0, M0)
    q64 = Q.astype(np.float64)
    for g in range(groups):
        ids = g * n + rng.permutation(n)[:2 * K * B].reshape(B, 2, K)
        for b in range(B):
            decoys[b, g * K:(g + 1) * K] = ids[b, 0]
            hidden[b, g * K:(g + 1) * K] = ids[b, 1]
            for j in range(K):
                hd = step_toward_zero(Q[b], Q[b], decoy_step * j * beta0[b], rng)
                for d in ids[b, :, j]:
                    docs[d] = rand_unit(rng, 128, 128)                        # rows past lq: random
                    docs[d, :lq] = with_residual(hd, Q[b], -1.0)              # (the hidden doc's: replaced below)
                    doclens[d] = 128
    # the decoys carry the largest residuals (the hidden docs' hi is stepped
    # further toward zero: smaller ulps), so E, M and beta are final here; each
    # group's lb is the least faithful score of its decoys
    _, _, (E, M) = orc.split_f32(docs, doclens)
    beta = orc.band_beta(Q, E, M)
    for g in range(groups):
        for b in range(B):
            dec = decoys[b, g * K:(g + 1) * K]
            lb = min(float((q64[b] * docs[d, :lq].astype(np.float64)).sum()) for d in dec)
            tmax = float((q64[b] * q64[b]).sum())
            for j in range(K):
                drop = tmax - lb + (hidden_gap + 0.01 * j + 0.005 * g) * beta[b]
                hh = step_toward_zero(Q[b], Q[b], drop, rng)
                docs[hidden[b, g * K + j], :lq] = with_residual(hh, Q[b], 1.0)
    return Case(docs, doclens, Q, decoys, hidden, K, groups)


def planted_ids(case):
    return np.unique(np.concatenate([case.decoys.reshape(-1), case.hidden.reshape(-1)]))


def check_preconditions(case, k, bounds=None, docs_subset=None, verbose=False):
    """Assert conditions (a)-(e) of the module docstring on a one-group case, in
    float64 from oracle.split_f32 / maxsim / band_beta, and return the measured
    quantities.  bounds: (E, M) of the index under test (default: the split's
    own).  docs_subset (sorted ids): score only these docs -- the caller checks
    the others' condition (e) itself, against the returned ``T_k - 2 beta``."""
    assert case.groups == 1 and k == case.K
    ids = np.arange(len(case.docs)) if docs_subset is None else np.asarray(docs_subset)
    docs, doclens = case.docs[ids], case.doclens[ids]
    hi, lo, own = orc.split_f32(docs, doclens)
    E, M = own if bounds is None else bounds
    assert E >= own[0] * (1 - 1e-6) and (docs_subset is not None or M >= own[1] * (1 - 1e-6)), (E, M, own)
    Qh = orc.bf16_round(case.Q)
    assert np.array_equal(Qh, case.Q), "queries must be bf16-exact"
    T = orc.maxsim(Qh, hi, doclens)
    F = orc.maxsim(case.Q, hi.astype(np.float64) + lo.astype(np.float64), doclens)
    beta = orc.band_beta(case.Q, E, M)
    pos = {int(d): p for p, d in enumerate(ids)}
    Tk = np.empty(len(case.Q))
    lb = np.empty(len(case.Q))
    out = {"T": T, "F": F, "beta": beta, "Tk": Tk, "lb": lb, "ids": ids}
    r_tk, r_lb, r_c, r_d, r_e, r_al = [], [], [], [], [], []
    for b in range(len(case.Q)):
        dec = np.array([pos[int(d)] for d in case.decoys[b]])
        hid = np.array([pos[int(d)] for d in case.hidden[b]])
        top = orc.topk(T[b:b + 1], k)[1][0]
        assert set(top.tolist()) == set(dec.tolist()), (b, "(a) the bf16 top-k must be the decoys")
        Tk[b] = T[b, top[-1]]
        lb[b] = F[b, top].min()
        bt = beta[b]
        th = T[b, hid]
        r_tk += ((Tk[b] - th) / bt).tolist()
        r_lb += ((lb[b] - th) / bt).tolist()
        assert (th > Tk[b] - 2 * bt).all() and (th <= Tk[b] - 1.3 * bt).all(), (b, "(b) T_k window", r_tk[-k:])
        assert (th > Tk[b] - 1.55 * bt).all(), (b, "(b) T_k window", r_tk[-k:])
        assert (th > lb[b] - bt).all() and (th <= lb[b] - 0.5 * bt).all(), (b, "(b) lb window", r_lb[-k:])
        assert (th > lb[b] - 0.7 * bt).all(), (b, "(b) lb window", r_lb[-k:])
        other = np.ones(T.shape[1], bool)
        other[hid] = False
        r_c.append((F[b, hid].min() - F[b, other].max()) / bt)
        assert r_c[-1] >= 0.10, (b, "(c) the hidden docs' lead in F", r_c[-1])
        fin = np.isfinite(T[b])
        r_d.append(np.abs(T[b, fin] - F[b, fin]).max() / bt)
        assert 0.8 <= r_d[-1] <= 1.0, (b, "(d) tightness", r_d[-1])
        r_al += ((F[b, hid] - T[b, hid]) / bt).tolist() + ((F[b, dec] - T[b, dec]) / bt).tolist()
        fill = other.copy()
        fill[dec] = False
        r_e.append((Tk[b] - T[b, fill & fin].max()) / bt if (fill & fin).any() else np.inf)
        assert r_e[-1] > 2.0, (b, "(e) fillers below the band", r_e[-1])
    out["ratios"] = {"Tk_minus_Th": (min(r_tk), max(r_tk)), "lb_minus_Th": (min(r_lb), max(r_lb)),
                     "c_margin": min(r_c), "d_tightness": (min(r_d), max(r_d)),
                     "aligned": (min(x for x in r_al if x > 0), max(r_al)),
                     "anti": (min(r_al), max(x for x in r_al if x < 0)), "e_fillers": min(r_e)}
    if verbose:
        print(out["ratios"])
    return out
