"""Groupings and the numpy oracle of the grouped search (tests/test_group_host.py,
tests/test_gpu_group.py).

The oracle works on score BITS: the order-preserving uint32 key of a float
(larger float <=> larger key; the key the kernels and every top-k of the
library rank by), so its group scores, group order, chunk order and every tie
are exact, and a result can be compared bit for bit.
"""
from __future__ import annotations

import numpy as np


# ------------------------------------------------------------------ groupings
def groupings(n: int, seed: int = 0):
    """name -> (group_of int32 [n], G): the cases both test files walk."""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n, dtype=np.int64)
    out = {}
    G = max(1, min(n, 7 if n < 200 else 37))
    out["runs"] = ((i * G // max(n, 1)).astype(np.int32), G)               # contiguous id ranges
    out["interleaved"] = ((i % G).astype(np.int32), G)                       # i % G: a gather
    out["one_group"] = (np.zeros(n, dtype=np.int32), 1)                      # one group holding everything
    out["singletons"] = (i.astype(np.int32), max(n, 1))                      # G' = n
    g = (i % G).astype(np.int32)
    g[rng.random(n) < 0.3] = -1                                              # 30 % of the chunks in no group
    out["holes"] = (g, G)
    # memberless groups in the middle and at the end: only even indices below G - 3 are used
    Gm = 2 * G + 5
    out["memberless"] = ((2 * (i % G)).astype(np.int32), Gm)
    # random sizes, shuffled ids: groups smaller than r beside large ones
    cuts = np.sort(rng.integers(0, n + 1, size=max(1, min(n, 50))))
    g = np.searchsorted(cuts, i, side="right").astype(np.int32)
    out["ragged"] = (g[rng.permutation(n)] if n else g, int(g.max()) + 1 if n else 1)
    return out


def build_reference(group_of: np.ndarray, G: int):
    """numpy's answer to cbv2_groups_build_host: (order, offsets, labels, out3)."""
    group_of = np.asarray(group_of, dtype=np.int64)
    members = np.flatnonzero(group_of >= 0)
    order = members[np.argsort(group_of[members], kind="stable")]             # ascending id inside a group
    counts = np.bincount(group_of[members], minlength=G)
    labels = np.flatnonzero(counts)
    offsets = np.concatenate([[0], np.cumsum(counts[labels])])
    out3 = (int(members.size), int(labels.size), int(counts.max()) if members.size else 0)
    return order.astype(np.int32), offsets.astype(np.int32), labels.astype(np.int32), out3


# ------------------------------------------------------------------ the oracle
def f2u(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def u2f(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _rank_keys(keys: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """score descending, then lower index first, as one descending uint64."""
    return (keys.astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)


def oracle(scores: np.ndarray, group_of: np.ndarray, G: int, k: int, r: int, id_base: int = 0):
    """(out_scores f32 [B, k], out_groups int32 [B, k], out_ids int32 [B, k, r],
    out_chunk_scores f32 [B, k, r]) of the contract in include/colbert_mi355x.h.
    ``scores`` [B, >= n]: columns at or past n = len(group_of) are ignored."""
    n = len(group_of)
    S = np.ascontiguousarray(np.asarray(scores, dtype=np.float32)[:, :n])
    B = S.shape[0]
    order, offsets, labels, (_, Gp, _) = build_reference(group_of, G)
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_g = np.full((B, k), -1, dtype=np.int32)
    out_i = np.full((B, k, r), -1, dtype=np.int32)
    out_c = np.full((B, k, r), -np.inf, dtype=np.float32)
    if Gp == 0:
        return out_s, out_g, out_i, out_c
    keys = f2u(S)                                                            # [B, n]
    gkeys = np.maximum.reduceat(keys[:, order], offsets[:-1].astype(np.int64), axis=1)   # [B, G']
    kk = min(k, Gp)
    pos = np.arange(Gp, dtype=np.uint32)
    for b in range(B):
        top = np.argsort(_rank_keys(gkeys[b], pos))[::-1][:kk]               # rank keys are distinct
        out_s[b, :kk] = u2f(gkeys[b, top])
        out_g[b, :kk] = labels[top]
        for j, p in enumerate(top):
            ids = order[offsets[p]: offsets[p + 1]]
            rk = _rank_keys(keys[b, ids], ids)
            best = ids[np.argsort(rk)[::-1][:r]]
            out_i[b, j, : best.size] = best + id_base
            out_c[b, j, : best.size] = S[b, best]
    return out_s, out_g, out_i, out_c


def same_bits(got, want) -> bool:
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(
        (got.view(np.uint32) == want.view(np.uint32)).all())
