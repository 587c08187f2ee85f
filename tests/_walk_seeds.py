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
# tests/test_gpu_nonfinite_padding.py replays seeds 0 .. PADDING_SEEDS[kind, ld] - 1 on pools whose padding rows hold
# NaN / Inf encodings, seed s under padding_mode(s): the smallest prefixes over which, both modes together, every
# entry point of the kind is called on that (kind, ld) and every value of every handle option is in force in a call
# (tests/test_nonfinite_padding_model.py asserts both, and that one seed fewer misses one); and the first
# PADDING_LARGE large walks of every kind under both modes.
PADDING_SEEDS = {("bf16", 128): 6, ("bf16", 256): 12, ("bf16", 512): 16, ("bf16", 1024): 10,
                 ("mxfp8", 128): 11, ("mxfp8", 256): 7, ("mxfp8", 512): 9, ("mxfp8", 1024): 21,
                 ("fp32", 128): 12, ("fp32", 256): 7, ("fp32", 512): 22, ("fp32", 1024): 16}
PADDING_LARGE = 2
PADDING_MODES = ("nan", "inf")


def padding_mode(seed):
    """nan, inf, inf, nan, ...: each mode gets even seeds (an edge n) and odd ones (a uniform n)."""
    return PADDING_MODES[(seed + seed // 2) % 2]


def padding_walks(kind, ld, mode, seeds=None):
    n = (PADDING_SEEDS if seeds is None else seeds)[kind, ld]
    return [(kind, ld, seed, False) for seed in range(n) if padding_mode(seed) == mode]


def committed(seeds=None):
    seeds = SEEDS if seeds is None else seeds
    return [(kind, ld, seed, False) for kind in ex.KINDS for ld in wk.LDS for seed in range(seeds[kind])]


def committed_large():
    return [(kind, 128, seed, True) for kind in ex.KINDS for seed in range(LARGE_SEEDS[kind])]
