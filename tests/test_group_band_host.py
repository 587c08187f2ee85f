"""CPU: the host side of the grouped faithful search's band -- the header
declares cbv2_search_grouped_f32, its workspace-size function and option 17,
the ctypes table binds them, and the checks that need no index handle return
before any launch (no GPU is present here)."""
import ctypes
import re

import pytest

from hybrid_rag_colbertv2_amd import _lib


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_header_declares_the_functions_and_the_option():
    text = open(_lib.HEADER).read()
    assert re.search(r"^#define CBV2_OPT_GROUP_BAND 17$", text, re.M)
    assert re.search(r"^#define CBV2_ABI_VERSION 2$", text, re.M)      # additive: the ABI version stays
    assert re.search(r"^size_t cbv2_search_grouped_f32_workspace_size\(const cbv2_index\* index, "
                     r"const cbv2_groups\* groups, int32_t B,\s+int32_t lq, int32_t k, int32_t r, int32_t cap\);",
                     text, re.M)
    # the return type on a line of its own, like the other grouped entry points
    assert re.search(r"^int\ncbv2_search_grouped_f32\(cbv2_index\* index, const cbv2_groups\* groups, const float\* Q,",
                     text, re.M)
    assert _lib.OPT_GROUP_BAND == 17
    assert (_lib.GROUP_BAND_AUTO, _lib.GROUP_BAND_ON, _lib.GROUP_BAND_OFF) == (0, 1, 2)
    for name in ("cbv2_search_grouped_f32", "cbv2_search_grouped_f32_workspace_size"):
        assert name in _lib._SIGS and name in _lib.header_symbols()


def test_ctypes_table_binds_both_symbols(L):
    for name in ("cbv2_search_grouped_f32", "cbv2_search_grouped_f32_workspace_size"):
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
    assert L.cbv2_search_grouped_f32_workspace_size.restype is ctypes.c_size_t
    assert len(_lib._SIGS["cbv2_search_grouped_f32"][1]) == 16
    assert len(_lib._SIGS["cbv2_search_grouped_f32_workspace_size"][1]) == 7


def test_workspace_size_is_zero_without_handles_or_shape(L):
    size = L.cbv2_search_grouped_f32_workspace_size
    assert size(None, None, 1, 32, 10, 3, 16384) == 0
    fake = ctypes.c_void_p(256)          # never dereferenced: the other handle is null
    assert size(fake, None, 1, 32, 10, 3, 16384) == 0
    assert size(None, fake, 1, 32, 10, 3, 16384) == 0
    for B, lq, k, r, cap in ((0, 32, 10, 3, 16384), (-1, 32, 10, 3, 16384), (65536, 32, 10, 3, 16384),
                             (1, 0, 10, 3, 16384), (1, 33, 10, 3, 16384), (1, 32, 0, 3, 16384), (1, 32, 10, 0, 16384),
                             (1, 32, 10, 9, 16384), (1, 32, 10, 3, 9), (1, 32, 10, 3, 16385), (1, 32, 10, 3, -1)):
        assert size(None, None, B, lq, k, r, cap) == 0, (B, lq, k, r, cap)


def test_argument_checks_launch_nothing(L):
    p = ctypes.c_void_p(256)
    args = (p, 1, 32, 10, 3, 16384, p, 1 << 20, p, p, p, p, p, None)
    assert L.cbv2_search_grouped_f32(None, None, *args) == _lib.ERR_EINVAL
    assert b"null groups" in L.cbv2_last_error()
    with pytest.raises(ValueError, match="null groups"):
        _lib.check(L.cbv2_search_grouped_f32(None, None, *args))
    assert L.cbv2_index_set_option(None, _lib.OPT_GROUP_BAND, 1) == _lib.ERR_EINVAL
