"""CPU: the host side of per-query filters -- cbv2_bm25_search_filtered_batch
against per-query cbv2_bm25_search_filtered / cbv2_bm25_search (ids and score
bits), the argument checks of the filter-batch entry points (no launch: no GPU
is present), and an AddressSanitizer / UBSan build of the new host function
driven by the stand-alone program tests/asan/asan_filter_batch_driver.cpp (the
sanitizer runs in that program only; nothing is loaded into Python under it)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.bm25 import NativeBM25

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-rag-colbertv2_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcolbert_mi355x.so not built")
    return _lib.lib()


def corpus(seed, N, V=50, B=7):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 30, N)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    terms = rng.integers(0, V, int(off[-1])).astype(np.int32)
    qlens = rng.integers(1, 6, B)
    qlens[1] = 0                                   # a query with no term: the row is padding only
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    qt = rng.integers(0, V, int(qoff[-1])).astype(np.int32)
    return terms, off, qt, qoff, V


@pytest.mark.parametrize("n_threads", [1, 4])
def test_bm25_filtered_batch_equals_per_query_search(L, n_threads):
    N, B = 501, 7                                  # n is no multiple of 32
    terms, off, qt, qoff, V = corpus(11, N, B=B)
    bm = NativeBM25(terms, off, V)
    rng = np.random.default_rng(5)
    allows = [
        np.zeros(N, bool),                         # empty
        np.arange(N) == N - 1,                     # a single doc, in the partial last word
        rng.random(N) < 0.3,                       # partial
        np.ones(N, bool),                          # full
        None,                                      # unfiltered
        rng.random(N) < 0.02,                      # a handful
        None,
    ]
    for k in (1, 12, 200, N + 3):                  # above several allowed counts (0, 1, ~10, ~150)
        ids, sc = bm.search_batch(qt, qoff, k, allows, n_threads=n_threads)
        assert ids.shape == (B, k) and sc.shape == (B, k)
        for b in range(B):
            q1 = qt[qoff[b]:qoff[b + 1]]
            o1 = np.array([0, len(q1)], np.int64)
            want_i, want_s = bm.search(q1, o1, k, n_threads=1, allow=allows[b])
            assert np.array_equal(ids[b], want_i[0]), (k, b)
            assert np.array_equal(sc[b].view(np.uint32), want_s[0].view(np.uint32)), (k, b)
            if allows[b] is not None:
                got = ids[b][ids[b] >= 0]
                assert allows[b][got].all() and len(got) == min(k, int(allows[b].sum()))


def test_bm25_filtered_batch_takes_packed_words_and_global_ids(L):
    """Packed uint32 words are the same filter; a shard's bitmaps are local, its ids global."""
    N = 200
    terms, off, qt, qoff, V = corpus(3, N, B=4)
    df = NativeBM25.doc_freq(terms, off, V)
    h = 100
    sh = NativeBM25(terms, off[h:], V, id_base=h, stats=(N, int(off[-1]), df))
    masks = [np.arange(100) % 2 == 1, None, np.arange(100) < 7, np.zeros(100, bool)]
    words = [None if m is None else np.packbits(np.concatenate([m, np.zeros(28, bool)]), bitorder="little")
             .view(np.uint32) for m in masks]
    a_i, a_s = sh.search_batch(qt, qoff, 60, masks)
    b_i, b_s = sh.search_batch(qt, qoff, 60, words, n_threads=2)
    assert np.array_equal(a_i, b_i) and np.array_equal(a_s.view(np.uint32), b_s.view(np.uint32))
    for b, m in enumerate(masks):
        got = a_i[b][a_i[b] >= 0]
        assert ((got >= h) & (got < N)).all()
        if m is not None:
            assert m[got - h].all() and len(got) == min(60, int(m.sum()))
    with pytest.raises(ValueError):
        sh.search_batch(qt, qoff, 5, masks[:3])    # one entry per query


def test_filter_batch_validation_errors_without_gpu(L):
    h = ctypes.c_void_p()
    p = ctypes.c_void_p(256)
    assert L.cbv2_filter_batch_bytes(0) == 0 and L.cbv2_filter_batch_bytes(-3) == 0
    assert L.cbv2_filter_batch_bytes(1) >= 4 * 5 and L.cbv2_filter_batch_bytes(256) >= 4 * (4 * 256 + 1)
    arr = (ctypes.c_void_p * 2)(None, None)
    assert L.cbv2_filter_batch_create(None, arr, 2, p, 1 << 20, None, ctypes.byref(h)) == _lib.ERR_EINVAL
    assert b"null index" in L.cbv2_last_error() and not h.value
    assert L.cbv2_filter_batch_create(None, arr, 2, p, 1 << 20, None, None) == _lib.ERR_EINVAL
    assert b"null output" in L.cbv2_last_error()
    # null batch, null outputs, k < 1
    assert L.cbv2_search_filtered_batch(None, None, 0, p, _lib.DTYPE_BF16, 1, 32, 10, p, 1 << 20, p, p,
                                        None) == _lib.ERR_EINVAL
    assert b"null filter batch" in L.cbv2_last_error()
    assert L.cbv2_search_filtered_batch_workspace_size(None, None, 1, 32, 10, 0) == 0
    assert L.cbv2_filter_batch_pairs(None) == -1 and L.cbv2_filter_batch_max_count(None) == -1
    assert L.cbv2_filter_batch_destroy(None) == 0
    with pytest.raises(ValueError):
        _lib.check(L.cbv2_filter_batch_create(None, arr, 2, None, 0, None, ctypes.byref(h)))
    # the host BM25 entry point
    terms, off, qt, qoff, V = corpus(1, 64, B=2)
    bm = NativeBM25(terms, off, V)
    ids = np.empty((2, 3), np.int32)
    none2 = (ctypes.c_void_p * 2)(None, None)
    f = L.cbv2_bm25_search_filtered_batch
    assert f(None, qt.ctypes.data, qoff.ctypes.data, 2, 3, 1, none2, ids.ctypes.data, None) == _lib.ERR_EINVAL
    assert b"null bm25 index" in L.cbv2_last_error()
    assert f(bm._h, qt.ctypes.data, qoff.ctypes.data, 2, 3, 1, None, ids.ctypes.data, None) == _lib.ERR_EINVAL
    assert b"null per-query bitmap" in L.cbv2_last_error()
    assert f(bm._h, qt.ctypes.data, qoff.ctypes.data, 2, 3, 1, none2, None, None) == _lib.ERR_EINVAL
    assert b"bad search arguments" in L.cbv2_last_error()
    assert f(bm._h, qt.ctypes.data, qoff.ctypes.data, 2, 0, 1, none2, ids.ctypes.data, None) == _lib.ERR_EINVAL
    assert b"bad search arguments" in L.cbv2_last_error()
    assert f(bm._h, qt.ctypes.data, qoff.ctypes.data, 2, 3, 1, none2, ids.ctypes.data, None) == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_filtered_batch_bm25_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "asan_filter_batch_driver")
    srcs = [os.path.join(ROOT, "tests", "asan", "asan_filter_batch_driver.cpp"), os.path.join(CSRC, "host_bm25.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), *srcs, "-pthread", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "0 failed checks" in r.stdout
