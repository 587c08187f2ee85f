"""CPU: the host side of filtered search -- the allow bitmap's bit order
(pack_allow), the filtered host BM25 against the oracle's full ranking with the
disallowed docs dropped (ids and scores exact, padding included), and the
argument checks of the filter entry points (no launch: no GPU is present)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.bm25 import NativeBM25
from hybrid_rag_colbertv2_amd.index import pack_allow
from oracle import oracle as orc


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcolbert_mi355x.so not built")
    return _lib.lib()


def ref_words(mask):
    n = len(mask)
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = mask
    return np.packbits(bits, bitorder="little").view(np.uint32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000])
def test_pack_allow_bit_order(n):
    rng = np.random.default_rng(n)
    for mask in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
        want = ref_words(mask)
        got = pack_allow(torch.from_numpy(mask), n)
        assert got.dtype == torch.uint32 and tuple(got.shape) == ((n + 31) // 32,)
        assert np.array_equal(got.numpy(), want)
        # global ids of a shard starting at 1000, as a tensor, an array and a list
        ids = np.flatnonzero(mask) + 1000
        for form in (torch.from_numpy(ids), ids, ids.tolist()):
            assert np.array_equal(pack_allow(form, n, id_base=1000).numpy(), want)


def test_pack_allow_rejects_out_of_range_ids():
    with pytest.raises(ValueError):
        pack_allow([0, 10], 10)
    with pytest.raises(ValueError):
        pack_allow([-1], 10)
    with pytest.raises(ValueError):
        pack_allow([999], 10, id_base=1000)
    with pytest.raises(ValueError):
        pack_allow([1010], 10, id_base=1000)
    with pytest.raises(ValueError):
        pack_allow(torch.zeros(9, dtype=torch.bool), 10)
    assert np.array_equal(pack_allow([1009], 10, id_base=1000).numpy(), np.array([1 << 9], np.uint32))


def bm25_corpus(seed, N, V=50, B=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 30, N)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    terms = rng.integers(0, V, int(off[-1])).astype(np.int32)
    qlens = rng.integers(1, 6, B)
    qlens[0] = 0                                   # a query with no term: the row is padding only
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    qt = rng.integers(0, V, int(qoff[-1])).astype(np.int32)
    if len(qt) > 1:
        qt[-1] = qt[-2]                            # a repeated query term
    return terms, off, qt, qoff, V


@pytest.mark.parametrize("N", [200, 333, 500])
def test_bm25_filtered_equals_full_ranking_restricted(L, N):
    terms, off, qt, qoff, V = bm25_corpus(N, N)
    B = len(qoff) - 1
    bm = NativeBM25(terms, off, V)
    full_i, full_s = orc.bm25_topk(terms, off, qt, qoff, V, k=N)     # every doc ranked, zero scores in id order
    filters = {
        "every third": np.arange(N) % 3 == 0,
        "one": np.arange(N) == N // 2,
        "none": np.zeros(N, bool),
        "all": np.ones(N, bool),
    }
    for name, mask in filters.items():
        m = int(mask.sum())
        for k in sorted({1, max(1, m // 2), m + 7, N + 3}):          # below and above the allowed count
            ids, sc = bm.search(qt, qoff, k, n_threads=2, allow=mask)
            ids_w, sc_w = bm.search(qt, qoff, k, n_threads=1, allow=ref_words(mask))   # packed words: same
            assert np.array_equal(ids, ids_w) and np.array_equal(sc.view(np.uint32), sc_w.view(np.uint32))
            for b in range(B):
                keep = mask[full_i[b]]
                want_i = full_i[b][keep][:k]
                want_s = full_s[b][keep][:k]
                kk = len(want_i)
                assert kk == min(k, m), (name, k)
                assert np.array_equal(ids[b, :kk], want_i), (name, k, b)
                assert np.array_equal(sc[b, :kk].view(np.uint32), want_s.astype(np.float32).view(np.uint32))
                assert (ids[b, kk:] == -1).all() and (sc[b, kk:] == 0).all(), (name, k, b)
                assert mask[ids[b, :kk]].all(), "a returned (or padding) id is not allowed"


def test_bm25_allow_none_is_the_unfiltered_search(L):
    terms, off, qt, qoff, V = bm25_corpus(7, 300)
    bm = NativeBM25(terms, off, V)
    B, k = len(qoff) - 1, 40
    a_i, a_s = bm.search(qt, qoff, k)
    ids = np.empty((B, k), np.int32)
    sc = np.empty((B, k), np.float32)
    assert L.cbv2_bm25_search_filtered(bm._h, qt.ctypes.data, qoff.ctypes.data, B, k, 1, None, ids.ctypes.data,
                                       sc.ctypes.data) == 0
    assert np.array_equal(ids, a_i) and np.array_equal(sc.view(np.uint32), a_s.view(np.uint32))
    f_i, f_s = bm.search(qt, qoff, k, allow=np.ones(300, bool))
    assert np.array_equal(f_i, a_i) and np.array_equal(f_s.view(np.uint32), a_s.view(np.uint32))


def test_bm25_filtered_shard_returns_global_ids(L):
    """The bitmap is over LOCAL docs; a shard's ids come back global."""
    terms, off, qt, qoff, V = bm25_corpus(3, 200)
    df = NativeBM25.doc_freq(terms, off, V)
    h = 100
    sh = NativeBM25(terms, off[h:], V, id_base=h, stats=(200, int(off[-1]), df))
    mask = np.arange(100) % 2 == 1
    ids, _ = sh.search(qt, qoff, 60, allow=mask)
    got = ids[ids >= 0]
    assert ((got >= h) & (got < 200)).all() and mask[got - h].all()
    assert ((ids >= 0).sum(axis=1) == 50).all()


def test_filter_argument_checks_launch_nothing(L):
    h = ctypes.c_void_p()
    assert L.cbv2_filter_bytes(-1) == 0 and L.cbv2_filter_bytes(1) >= 4 and L.cbv2_filter_bytes(20011) >= 4 * 20011
    assert L.cbv2_filter_create(None, None, ctypes.c_void_p(256), 1 << 20, None, ctypes.byref(h)) == _lib.ERR_EINVAL
    assert b"null index" in L.cbv2_last_error() and not h.value
    assert L.cbv2_filter_create(None, None, None, 0, None, None) == _lib.ERR_EINVAL
    assert b"null output" in L.cbv2_last_error()
    assert L.cbv2_search_filtered(None, None, 0, ctypes.c_void_p(256), _lib.DTYPE_BF16, 1, 32, 10,
                                  ctypes.c_void_p(256), 1 << 20, ctypes.c_void_p(256), ctypes.c_void_p(256),
                                  None) == _lib.ERR_EINVAL
    assert b"null filter" in L.cbv2_last_error()
    assert L.cbv2_search_filtered_workspace_size(None, None, 1, 32, 10, 0) == 0
    assert L.cbv2_filter_count(None) == -1
    assert L.cbv2_filter_destroy(None) == 0
    with pytest.raises(ValueError):
        _lib.check(L.cbv2_filter_create(None, None, None, 0, None, ctypes.byref(h)))
