"""CPU: the host side of the filtered faithful search's band -- the ctypes table
binds cbv2_search_filtered_f32 and its workspace-size function, the option's
number, and the argument checks that return before any launch (no GPU is
present, so no index handle: the checks that need none)."""
import ctypes
import os
import re

import pytest

from hybrid_rag_colbertv2_amd import _lib


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcolbert_mi355x.so not built")
    return _lib.lib()


def test_option_numbers():
    assert _lib.OPT_FILTER_BAND == 16
    assert (_lib.FILTER_BAND_AUTO, _lib.FILTER_BAND_ON, _lib.FILTER_BAND_OFF) == (0, 1, 2)
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define CBV2_OPT_FILTER_BAND 16$", text, re.M)
    assert re.search(r"^#define CBV2_ABI_VERSION 2$", text, re.M)      # additive: the ABI version stays


def test_ctypes_table_binds_both_symbols(L):
    for name in ("cbv2_search_filtered_f32", "cbv2_search_filtered_f32_workspace_size"):
        assert name in _lib._SIGS and name in _lib.header_symbols()
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
    assert L.cbv2_search_filtered_f32_workspace_size.restype is ctypes.c_size_t
    assert len(_lib._SIGS["cbv2_search_filtered_f32"][1]) == 13
    assert L.cbv2_abi_version() == 2


def test_workspace_size_is_zero_without_handles_or_shape(L):
    size = L.cbv2_search_filtered_f32_workspace_size
    assert size(None, None, 1, 32, 10, 16384) == 0
    fake = ctypes.c_void_p(256)          # never dereferenced: the other handle is null / the shape is refused first
    assert size(fake, None, 1, 32, 10, 16384) == 0
    assert size(None, fake, 1, 32, 10, 16384) == 0
    for B, lq, k in ((0, 32, 10), (1, 0, 10), (1, 32, 0), (-1, 32, 10)):
        assert size(None, None, B, lq, k, 16384) == 0


def test_argument_checks_launch_nothing(L):
    p = ctypes.c_void_p(256)
    args = (p, 1, 32, 10, 16384, p, 1 << 20, p, p, p, None)
    assert L.cbv2_search_filtered_f32(None, None, *args) == _lib.ERR_EINVAL
    assert b"null filter" in L.cbv2_last_error()
    with pytest.raises(ValueError, match="null filter"):
        _lib.check(L.cbv2_search_filtered_f32(None, None, *args))
    # option 16 is an index option: without a handle the call is refused, not a crash
    assert L.cbv2_index_set_option(None, _lib.OPT_FILTER_BAND, 1) == _lib.ERR_EINVAL
