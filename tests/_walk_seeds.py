"""The committed walks of tests/_walk.py: seeds 0 .. SEEDS[kind] - 1 of every
(kind, ld), the smallest counts at which every cell of the coverage table of
tests/test_walk_model.py is visited at least 3 times, and the large walks of
tests/test_gpu_walk.py (ld = 128): seeds 0 .. LARGE_SEEDS[kind] - 1, the
smallest counts at which every theme of _walk.THEMES is played and every
dispatch path that exists only from 65,536 docs on is launched, and left out by
its own option alone (the dispatch's conjunctions, _walk.large_paths).  TRANSCRIPTS_SHA256 pins the
transcripts of all of them."""
import _exact as ex
import _walk as wk

SEEDS = {"bf16": 45, "mxfp8": 36, "fp32": 50}
LARGE_SEEDS = {"bf16": 14, "mxfp8": 17, "fp32": 14}
TRANSCRIPTS_SHA256 = "c7c1e13e99c58959520f4cbb893bfa2bd6b4d40601632d73b4cf8c3c22dfc27e"


def committed(seeds=None):
    seeds = SEEDS if seeds is None else seeds
    return [(kind, ld, seed, False) for kind in ex.KINDS for ld in wk.LDS for seed in range(seeds[kind])]


def committed_large():
    return [(kind, 128, seed, True) for kind in ex.KINDS for seed in range(LARGE_SEEDS[kind])]
