"""CPU, world_size 2 and 4 (gloo): ShardedSearcher.search_grouped over
torch.distributed -- two all-gathers and the two merges -- equals the
unsharded oracle of tests/_groups.py bit for bit on every rank.  The per-shard
compute is injected as oracle-backed CPU objects (test-only) and the merges
are the numpy twins of the HIP merges (distributed.merge_group_*_host); on the
GPU the same method drives the kernels (tests/test_gpu_group_sharded.py).
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _groups import oracle, same_bits
from _groups_sharded import local_chunks
from oracle import oracle as orc


class HostGroups:
    """What the CPU ops need of a DocGroups: this shard's slice of group_of, the corpus-wide G."""
    keyed = False

    def __init__(self, group_of, G, id_base):
        self.group_of, self.G, self.id_base = group_of, G, id_base


class OracleShard:
    """Chunks [a, b) of the corpus.  The scores are columns of the oracle's matrix
    of the whole corpus, so that a chunk's score has the same bits on its rank as
    in the unsharded answer (a BLAS call of another shape may round otherwise);
    the protocol, not the scorer, is under test."""

    def __init__(self, docs, doclens, a, b):
        self.docs, self.doclens, self.a, self.b = docs, doclens, a, b

    def score(self, Q, scorer="maxsim"):
        full = orc.maxsim(Q.numpy(), self.docs, self.doclens).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(full[:, self.a:self.b]))


class HostOps:
    @staticmethod
    def group_topk(scores, k, groups):
        s, g, _, _ = oracle(scores.numpy(), groups.group_of, groups.G, k, 1, id_base=groups.id_base)
        return torch.from_numpy(s), torch.from_numpy(g)

    @staticmethod
    def group_chunks(scores, sel, groups, per_group):
        i, c = local_chunks(scores.numpy(), groups.group_of, groups.G, sel.numpy(), per_group, id_base=groups.id_base)
        return torch.from_numpy(i), torch.from_numpy(c)

    @staticmethod
    def merge_group_topk(S, Gr, k):
        from hybrid_rag_colbertv2_amd.distributed import merge_group_topk_host
        s, g = merge_group_topk_host(S.numpy(), Gr.numpy(), k)
        return torch.from_numpy(s), torch.from_numpy(g)

    @staticmethod
    def merge_group_chunks(I, C):
        from hybrid_rag_colbertv2_amd.distributed import merge_group_chunks_host
        i, c = merge_group_chunks_host(I.numpy(), C.numpy())
        return torch.from_numpy(i), torch.from_numpy(c)


def _data():
    rng = np.random.default_rng(11)
    N, B, G = 151, 3, 23
    docs = orc.bf16_round(rng.standard_normal((N, 16, 128)).astype(np.float32))
    doclens = rng.integers(0, 17, size=N)
    Q = torch.from_numpy(orc.bf16_round(rng.standard_normal((B, 32, 128)).astype(np.float32)))
    group_of = rng.integers(-1, G - 2, size=N).astype(np.int32)         # groups 21, 22: no member anywhere
    group_of[:5] = 20                                                    # a group on the first rank only
    return Q, docs, doclens, group_of, G


def _cuts(world, N):
    """Rank 1 is empty at world 4; sizes differ."""
    return [0, 60, N] if world == 2 else [0, 40, 40, 100, N]


def _worker(rank, world, port, q, k, r):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from hybrid_rag_colbertv2_amd.distributed import ShardedSearcher
        Q, docs, doclens, group_of, G = _data()
        edges = _cuts(world, len(docs))
        a, b = edges[rank], edges[rank + 1]
        ss = ShardedSearcher(OracleShard(docs, doclens, a, b), ops=HostOps())
        out = ss.search_grouped(Q, k, HostGroups(group_of[a:b], G, a), per_group=r)
        q.put((rank, [x.numpy() for x in out]))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,k,r", [(2, 5, 3), (4, 30, 8)])
def test_sharded_grouped_protocol_equals_unsharded(world, k, r):
    """world 4, k = 30: more than the 21 non-empty groups, so the tail is -inf / -1,
    one rank is empty and every rank's lists carry padding."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, world, port, q, k, r)) for rk in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    Q, docs, doclens, group_of, G = _data()
    full = orc.maxsim(Q.numpy(), docs, doclens).astype(np.float32)
    want = oracle(full, group_of, G, k, r)
    for rank, got in res:                     # every rank holds the identical global answer
        for name, g, w in zip(("scores", "groups", "ids", "chunk scores"), got, want):
            assert same_bits(g, w), f"rank {rank}: {name} differ from the unsharded oracle"
        assert same_bits(got[0], np.ascontiguousarray(got[3][:, :, 0]))


def test_keyed_groups_are_refused():
    from hybrid_rag_colbertv2_amd.distributed import ShardedSearcher

    class Keyed(HostGroups):
        keyed = True

    ss = ShardedSearcher(OracleShard(np.zeros((0, 16, 128), np.float32), np.zeros(0, np.int64), 0, 0), ops=HostOps(),
                         world=1)
    with pytest.raises(ValueError, match="group_of"):
        ss.search_grouped(torch.zeros(1, 32, 128), 3, Keyed(np.zeros(0, np.int32), 1, 0))
