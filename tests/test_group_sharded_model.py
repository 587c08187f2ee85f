"""CPU: the two-exchange protocol of the sharded grouped search (DESIGN.md 3.9,
tests/_groups_sharded.py) equals the unsharded oracle bit for bit, and the
one-exchange shortcut does not.

The matrix: n in {1, 7, 65, 300}, the seven groupings, tie-heavy integer scores
with +-0.0 and -inf, k in {1, 4, 40}, r in {1, 3, 8}, 1 to 8 shards with empty
shards and duplicate cut points.  The numpy twins of the two merges that the
gloo path uses (distributed.merge_group_*_host) are held to the model too.
"""
import numpy as np
import pytest

from _groups import groupings, oracle, same_bits
from _groups_sharded import (cut_cases, merge_group_chunks, merge_group_topk, one_exchange, planted_fact2, sharded,
                             tie_scores)

NAMES = ["runs", "interleaved", "one_group", "singletons", "holes", "memberless", "ragged"]


def _check(got, want, what):
    for name, g, w in zip(("scores", "groups", "ids", "chunk scores"), got, want):
        assert same_bits(g, w), f"{what}: {name} differ from the unsharded oracle"
    assert same_bits(got[0], np.ascontiguousarray(got[3][:, :, 0])), f"{what}: out_scores != chunk_scores[..., 0]"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [1, 7, 65, 300])
def test_protocol_equals_unsharded_oracle(n, name):
    group_of, G = groupings(n)[name]
    rng = np.random.default_rng(1000 * n + NAMES.index(name))
    B = 3
    S = tie_scores(rng, B, n)
    want = {(k, r): oracle(S, group_of, G, k, r) for k in (1, 4, 40) for r in (1, 3, 8)}
    for shards in range(1, 9):
        # one cut list per shard count, the five kinds (even, empty shard, tiny shard,
        # duplicate cut, random) taking turns over shard counts, sizes and groupings
        kinds = cut_cases(n, shards, rng)
        cuts = kinds[(shards + NAMES.index(name) + n) % len(kinds)]
        for (k, r), w in want.items():
            _check(sharded(S, group_of, G, k, r, cuts), w, f"n={n} {name} k={k} r={r} cuts={cuts}")


def test_planted_runner_up_needs_the_second_exchange():
    """Fact 2 by hand: group 0's runner-up chunk (id 4, score 8) sits on rank 1,
    where group 1 (8.5) pushes group 0 out of the local top-1."""
    S, group_of, G, k, r, cuts = planted_fact2()
    want = oracle(S, group_of, G, k, r)
    assert want[1].tolist() == [[0]] and want[2].tolist() == [[[0, 4]]]
    _check(sharded(S, group_of, G, k, r, cuts), want, "planted")
    short = one_exchange(S, group_of, G, k, r, cuts)
    assert short[1].tolist() == [[0]], "round 1 alone does select the right group"
    assert short[2].tolist() == [[[0, 1]]], "the shortcut reports rank 0's own runner-up (id 1, score 1)"


def test_one_exchange_shortcut_is_wrong_on_normal_scores():
    """Normal scores, n in {65, 300}, k = r = 3, four shards: reusing round 1's
    chunk lists gets (row, slot) entries wrong; the two-exchange protocol none."""
    wrong = 0
    for n in (65, 300):
        for name in NAMES:
            group_of, G = groupings(n)[name]
            rng = np.random.default_rng(77 + n)
            S = rng.standard_normal((8, n)).astype(np.float32)
            cuts = [n // 4, n // 2, 3 * n // 4]
            want = oracle(S, group_of, G, 3, 3)
            _check(sharded(S, group_of, G, 3, 3, cuts), want, f"n={n} {name}")
            short = one_exchange(S, group_of, G, 3, 3, cuts)
            assert same_bits(short[1], want[1]), "the group selection needs one exchange only (Fact 1)"
            wrong += int((short[2] != want[2]).any(axis=-1).sum())
    assert wrong > 0, "the shortcut should lose runner-up chunks somewhere in these cases"


@pytest.mark.parametrize("G,B,k,r", [(1, 1, 1, 1), (2, 5, 7, 3), (8, 3, 40, 8), (3, 2, 100, 1)])
def test_host_twins_equal_the_model(G, B, k, r):
    from hybrid_rag_colbertv2_amd.distributed import merge_group_chunks_host, merge_group_topk_host
    rng = np.random.default_rng(G * 100 + k)
    in_s = tie_scores(rng, G * B, k).reshape(G, B, k)
    in_g = rng.integers(-1, max(2, k // 2), size=(G, B, k)).astype(np.int32)
    in_g[:, 0] = -1 if B > 1 else in_g[:, 0]                 # a row that is all padding
    gs, gg = merge_group_topk(in_s, in_g, k)
    hs, hg = merge_group_topk_host(in_s, in_g, k)
    assert same_bits(hs, gs) and same_bits(hg, gg)
    in_c = tie_scores(rng, G * B * k, r).reshape(G, B, k, r)
    in_i = rng.permutation(G * B * k * r).astype(np.int32).reshape(G, B, k, r)   # a chunk lives on one rank
    in_i[rng.random(in_i.shape) < 0.3] = -1
    mi, mc = merge_group_chunks(in_i, in_c)
    hi, hc = merge_group_chunks_host(in_i, in_c)
    assert same_bits(hi, mi) and same_bits(hc, mc)
