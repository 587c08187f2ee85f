"""The numpy model of the sharded grouped search (tests/test_group_sharded_model.py,
tests/test_gpu_group_sharded.py): the protocol of DESIGN.md 3.9 on score BITS.

Every rank runs the unsharded ``oracle`` of tests/_groups.py on its own slice;
the two merges work on the order-preserving keys, so the model's answer can be
compared bit for bit with the unsharded oracle of the whole corpus and with
the kernels.
"""
from __future__ import annotations

import numpy as np

from _groups import f2u, oracle, u2f


def _key(hi: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """hi descending, then lower index first, as one descending uint64."""
    return (hi.astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)


# ------------------------------------------------------------------ the merges
def merge_group_topk(in_s: np.ndarray, in_g: np.ndarray, k: int):
    """[G, B, k] (score, group) lists (group < 0: padding) -> the maximum per
    group, then the top k by (score key desc, group asc): ([B, k], [B, k])."""
    in_s, in_g = np.asarray(in_s, np.float32), np.asarray(in_g, np.int32)
    B = in_s.shape[1]
    out_s = np.full((B, k), -np.inf, np.float32)
    out_g = np.full((B, k), -1, np.int32)
    keys = f2u(in_s)
    for b in range(B):
        best = {}
        for g, s in zip(in_g[:, b].reshape(-1).tolist(), keys[:, b].reshape(-1).tolist()):
            if g >= 0 and s > best.get(g, -1):
                best[g] = s
        ranked = sorted(best.items(), key=lambda e: (-e[1], e[0]))[:k]
        for j, (g, s) in enumerate(ranked):
            out_s[b, j] = u2f(np.uint32(s))
            out_g[b, j] = g
    return out_s, out_g


def merge_group_chunks(in_i: np.ndarray, in_c: np.ndarray):
    """[G, B, k, r] (chunk id, score) lists (id < 0: padding) -> per (b, j) the
    best r by (score key desc, id asc): ([B, k, r], [B, k, r])."""
    in_i, in_c = np.asarray(in_i, np.int32), np.asarray(in_c, np.float32)
    _, B, k, r = in_i.shape
    out_i = np.full((B, k, r), -1, np.int32)
    out_c = np.full((B, k, r), -np.inf, np.float32)
    keys = f2u(in_c)
    for b in range(B):
        for j in range(k):
            pairs = {(s, i) for i, s in zip(in_i[:, b, j].reshape(-1).tolist(), keys[:, b, j].reshape(-1).tolist())
                     if i >= 0}
            for t, (s, i) in enumerate(sorted(pairs, key=lambda e: (-e[0], e[1]))[:r]):
                out_i[b, j, t] = i
                out_c[b, j, t] = u2f(np.uint32(s))
    return out_i, out_c


# ------------------------------------------------------------------ the local stages
def local_chunks(scores: np.ndarray, group_of: np.ndarray, G: int, sel: np.ndarray, r: int, id_base: int = 0):
    """Round 2 on one rank: for each selected group sel[b, j] (-1: padding) the
    best r chunks of that group among the rank's own (-1 / -inf where it has none)."""
    S = np.asarray(scores, np.float32)
    B, k = sel.shape
    out_i = np.full((B, k, r), -1, np.int32)
    out_c = np.full((B, k, r), -np.inf, np.float32)
    group_of = np.asarray(group_of)
    for b in range(B):
        for j in range(k):
            g = int(sel[b, j])
            if g < 0 or g >= G:
                continue
            ids = np.flatnonzero(group_of == g)
            if ids.size == 0:
                continue
            best = ids[np.argsort(_key(f2u(S[b, ids]), ids))[::-1][:r]]
            out_i[b, j, : best.size] = best + id_base
            out_c[b, j, : best.size] = S[b, best]
    return out_i, out_c


def shards(n: int, cuts):
    """cuts: ascending interior cut points (duplicates = empty shards) -> [(a, b)]."""
    edges = [0] + [int(c) for c in cuts] + [n]
    return list(zip(edges[:-1], edges[1:]))


def sharded(scores: np.ndarray, group_of: np.ndarray, G: int, k: int, r: int, cuts):
    """The two-exchange protocol over contiguous shards of the columns."""
    S = np.asarray(scores, np.float32)
    group_of = np.asarray(group_of, np.int32)
    parts = shards(len(group_of), cuts)
    r1 = [oracle(S[:, a:b], group_of[a:b], G, k, 1, id_base=a) for a, b in parts]
    _, sel = merge_group_topk(np.stack([x[0] for x in r1]), np.stack([x[1] for x in r1]), k)
    r2 = [local_chunks(S[:, a:b], group_of[a:b], G, sel, r, id_base=a) for a, b in parts]
    out_i, out_c = merge_group_chunks(np.stack([x[0] for x in r2]), np.stack([x[1] for x in r2]))
    return np.ascontiguousarray(out_c[:, :, 0]), sel, out_i, out_c


def one_exchange(scores: np.ndarray, group_of: np.ndarray, G: int, k: int, r: int, cuts):
    """The WRONG shortcut: round 1 carries each local top-k group's best r chunks,
    and the chunk merge reuses those lists (a rank whose local top-k lacks a
    selected group contributes nothing to it)."""
    S = np.asarray(scores, np.float32)
    group_of = np.asarray(group_of, np.int32)
    parts = shards(len(group_of), cuts)
    r1 = [oracle(S[:, a:b], group_of[a:b], G, k, r, id_base=a) for a, b in parts]
    out_s, sel = merge_group_topk(np.stack([x[0] for x in r1]), np.stack([x[1] for x in r1]), k)
    B = S.shape[0]
    ids = np.full((len(parts), B, k, r), -1, np.int32)
    cs = np.full((len(parts), B, k, r), -np.inf, np.float32)
    for p, (_, lg, li, lc) in enumerate(r1):
        for b in range(B):
            for j in range(k):
                hit = np.flatnonzero(lg[b] == sel[b, j]) if sel[b, j] >= 0 else []
                if len(hit):
                    ids[p, b, j], cs[p, b, j] = li[b, hit[0]], lc[b, hit[0]]
    out_i, out_c = merge_group_chunks(ids, cs)
    return out_s, sel, out_i, out_c


# ------------------------------------------------------------------ cases
def tie_scores(rng, B: int, n: int) -> np.ndarray:
    """Tie-heavy integer scores with +0.0, -0.0 and -inf."""
    S = rng.integers(-3, 4, size=(B, n)).astype(np.float32)
    S[rng.random((B, n)) < 0.1] = -0.0
    S[rng.random((B, n)) < 0.1] = -np.inf
    return S


def cut_cases(n: int, G: int, rng):
    """Cut lists for G shards of n columns: even, with an empty shard, with a
    tiny shard, with a duplicate cut, random."""
    if G == 1:
        return [[]]
    even = [n * (g + 1) // G for g in range(G - 1)]
    out = [even, [0] + even[1:], sorted([min(2, n)] + even[1:]), sorted([even[0]] + even[:-1])]
    out.append(sorted(rng.integers(0, n + 1, size=G - 1).tolist()))
    return out


def planted_fact2():
    """Fact 2: n = 8 in two shards of 4, k = 1, r = 2.  Group 0's best chunk is
    on rank 0 and its runner-up on rank 1, where group 1 outranks group 0 -- so
    group 0 is outside rank 1's local top-1 and a one-exchange protocol never
    sees the runner-up.  -> (scores [1, 8], group_of, G, k, r, cuts)."""
    group_of = np.array([0, 0, 1, 1, 0, 0, 1, 1], np.int32)
    S = np.array([[9.0, 1.0, 2.0, 2.0, 8.0, 0.5, 8.5, 3.0]], np.float32)
    return S, group_of, 2, 1, 2, [4]
