"""Pool sizes and batch-size edge lists of the exact-corpus GPU tests (numpy-free,
shared by tests/test_gpu_exact_scores.py and tests/_walk.py)."""

LDS = (128, 256, 512, 1024)
SIZE = {128: (600, 65), 256: (300, 65), 512: (200, 40), 1024: (200, 40)}      # ld -> (docs, queries)


def score_batches(kind, ld):
    """Both neighbours of every dispatch threshold of the index kind's scans
    (the table in tests/test_gpu_exact_scores.py's docstring)."""
    bmax = SIZE[ld][1]
    if kind == "fp32":
        bs = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 16, 17, 20, 21, 31, 32, 33, 64, 65]
    elif ld == 128 and kind == "bf16":
        bs = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 40, 48, 49, 64, 65]
    elif ld == 128:
        bs = [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 64, 65]
    else:
        bs = [1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 64, 65]
    return [b for b in bs if b <= bmax]
