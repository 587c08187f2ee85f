"""CPU: the host side of the grouped search -- cbv2_groups_build_host against
numpy, the ctypes table and the header, the argument checks that return before
any launch (no GPU is present, so no index or groups handle: the checks that
need none), the label numbering of ColbertIndex.groups and
ChunkStore.document_keys."""
import ctypes
import os
import re

import numpy as np
import pytest

from hybrid_rag_colbertv2_amd import _lib
from hybrid_rag_colbertv2_amd.hybrid import ChunkStore
from hybrid_rag_colbertv2_amd.index import ColbertIndex, DocGroups, group_labels, group_topk_rows

from _groups import build_reference, groupings

NEW = ("cbv2_groups_bytes", "cbv2_groups_build_host", "cbv2_groups_create", "cbv2_groups_count", "cbv2_groups_destroy",
       "cbv2_group_topk_workspace_size", "cbv2_group_topk_rows", "cbv2_search_grouped_workspace_size",
       "cbv2_search_grouped")
SENTINEL = -7777


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcolbert_mi355x.so not built")
    return _lib.lib()


def _build(L, group_of, G):
    group_of = np.ascontiguousarray(group_of, dtype=np.int32)
    n = group_of.size
    order = np.full(n, SENTINEL, dtype=np.int32)
    offsets = np.full(G + 1, SENTINEL, dtype=np.int32)
    labels = np.full(G, SENTINEL, dtype=np.int32)
    out3 = np.full(3, SENTINEL, dtype=np.int64)
    rc = L.cbv2_groups_build_host(group_of.ctypes.data, n, G, order.ctypes.data, offsets.ctypes.data,
                                  labels.ctypes.data, out3.ctypes.data)
    return rc, order, offsets, labels, out3


@pytest.mark.parametrize("n", [1, 31, 64, 65, 2049, 20011])
def test_build_host_matches_numpy(L, n):
    for name, (group_of, G) in groupings(n).items():
        rc, order, offsets, labels, out3 = _build(L, group_of, G)
        assert rc == 0, (name, L.cbv2_last_error())
        want_order, want_off, want_lab, (members, Gp, largest) = build_reference(group_of, G)
        assert tuple(out3) == (members, Gp, largest), name
        assert (order[:members] == want_order).all(), name
        assert (offsets[: Gp + 1] == want_off).all(), name
        assert (labels[:Gp] == want_lab).all(), name
        # what the arrays mean, stated without the reference: segments partition the members,
        # ascending id inside a segment, every chunk of segment s in group labels[s]
        assert offsets[0] == 0 and offsets[Gp] == members and (np.diff(offsets[: Gp + 1]) >= 1).all(), name
        assert (np.diff(labels[:Gp]) > 0).all(), name
        for s in range(Gp):
            seg = order[offsets[s]: offsets[s + 1]]
            assert (np.diff(seg) > 0).all() and (group_of[seg] == labels[s]).all(), (name, s)
        assert np.array_equal(np.sort(order[:members]), np.flatnonzero(group_of >= 0)), name
        # nothing past the valid prefixes was written
        assert (order[members:] == SENTINEL).all() and (offsets[Gp + 1:] == SENTINEL).all() \
            and (labels[Gp:] == SENTINEL).all(), name


@pytest.mark.parametrize("bad", [-2, "G"])
def test_build_host_rejects_values_outside_the_range(L, bad):
    n, G, at = 2049, 37, 1234
    group_of = (np.arange(n) % G).astype(np.int32)
    group_of[at] = G if bad == "G" else bad
    group_of[at + 100] = -5                                  # a later one: the FIRST position is named
    rc, order, offsets, labels, out3 = _build(L, group_of, G)
    assert rc == _lib.ERR_EINVAL
    msg = L.cbv2_last_error().decode()
    assert re.search(rf"\b{at}\b", msg) and str(int(group_of[at])) in msg, msg
    for a in (order, offsets, labels, out3):                  # nothing was written
        assert (a == SENTINEL).all()
    with pytest.raises(ValueError, match=str(at)):
        _lib.check(rc)


def test_build_host_limits(L):
    one = np.zeros(1, dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    p = one.ctypes.data
    assert L.cbv2_groups_build_host(p, 1, 0, p, p, p, out.ctypes.data) == _lib.ERR_EINVAL       # G >= 1
    assert L.cbv2_groups_build_host(p, 1 << 31, 1, p, p, p, out.ctypes.data) == _lib.ERR_EINVAL  # n <= 2^31 - 1
    assert L.cbv2_groups_build_host(p, -1, 1, p, p, p, out.ctypes.data) == _lib.ERR_EINVAL
    assert L.cbv2_groups_build_host(p, 1, 1, p, None, p, out.ctypes.data) == _lib.ERR_EINVAL
    rc, order, offsets, labels, out3 = _build(L, np.zeros(0, dtype=np.int32), 3)                 # an empty shard
    assert rc == 0 and tuple(out3) == (0, 0, 0) and offsets[0] == 0


def test_ctypes_table_and_header(L):
    header = _lib.header_symbols()
    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name in _lib._SIGS and name in header, name
        assert getattr(L, name).argtypes == _lib._SIGS[name][1], name
    for name in ("cbv2_groups_bytes", "cbv2_group_topk_workspace_size", "cbv2_search_grouped_workspace_size"):
        assert getattr(L, name).restype is ctypes.c_size_t
    assert L.cbv2_groups_count.restype is ctypes.c_int64
    assert len(_lib._SIGS["cbv2_group_topk_rows"][1]) == 13 and len(_lib._SIGS["cbv2_search_grouped"][1]) == 16
    assert re.search(r"^#define CBV2_ABI_VERSION 2$", text, re.M) and L.cbv2_abi_version() == 2   # additive
    # the guard-band table of tests/test_gpu_bounds.py lists the one-line `int cbv2_*(` declarations
    assert not set(re.findall(r"^int (cbv2_\w+)\(", text, re.M)) & set(NEW)


def test_sizes_without_handles_or_shape(L):
    fake = ctypes.c_void_p(256)          # never dereferenced: the other handle is null / the shape is refused first
    assert L.cbv2_group_topk_workspace_size(None, 1, 10, 1) == 0
    for B, k, r in ((0, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 9)):
        assert L.cbv2_group_topk_workspace_size(None, B, k, r) == 0
    size = L.cbv2_search_grouped_workspace_size
    assert size(None, None, 1, 32, 10, 1, 0) == 0
    assert size(fake, None, 1, 32, 10, 1, 0) == 0
    assert size(None, fake, 1, 32, 10, 1, 0) == 0
    assert L.cbv2_groups_count(None) == -1
    # the buffer of a grouping: three int32 arrays, each rounded up to 256 B
    r256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    for n, G in ((0, 1), (1, 1), (65, 7), (20011, 20011)):
        assert L.cbv2_groups_bytes(n, G) == r256(4 * n) + r256(4 * (G + 1)) + r256(4 * G)
    assert L.cbv2_groups_bytes(-1, 1) == 0 and L.cbv2_groups_bytes(1 << 31, 1) == 0 and L.cbv2_groups_bytes(5, 0) == 0


def test_argument_checks_launch_nothing(L):
    p = ctypes.c_void_p(256)
    assert L.cbv2_group_topk_rows(None, p, 8, 1, 10, 1, p, 1 << 20, p, p, p, p, None) == _lib.ERR_EINVAL
    assert b"null groups" in L.cbv2_last_error()
    assert L.cbv2_group_topk_rows(None, p, 8, 1, 10, 1, p, 1 << 20, None, None, None, None, None) == _lib.ERR_EINVAL
    args = (0, p, _lib.DTYPE_BF16, 1, 32, 10, 1, p, 1 << 20)
    assert L.cbv2_search_grouped(None, None, *args, p, p, p, p, None) == _lib.ERR_EINVAL
    assert b"null groups" in L.cbv2_last_error()
    assert L.cbv2_search_grouped(None, p, *args, p, p, p, p, None) == _lib.ERR_EINVAL      # groups given, no index
    assert b"null index" in L.cbv2_last_error()
    assert L.cbv2_search_grouped(None, None, *args, None, None, None, None, None) == _lib.ERR_EINVAL
    h = ctypes.c_void_p(1)
    assert L.cbv2_groups_create(None, p, 1, p, 1 << 20, None, ctypes.byref(h)) == _lib.ERR_EINVAL
    assert h.value is None                                   # the out handle is cleared first
    assert L.cbv2_groups_create(None, p, 1, p, 1 << 20, None, None) == _lib.ERR_EINVAL
    assert L.cbv2_groups_destroy(None) == 0
    with pytest.raises(ValueError, match="null groups"):
        _lib.check(L.cbv2_group_topk_rows(None, p, 8, 1, 10, 1, p, 1 << 20, p, p, p, p, None))


def test_label_numbering():
    gof, labels = group_labels(["b", "a", None, "b", ("t", 1), "a", None, 7])
    assert gof.tolist() == [0, 1, -1, 0, 2, 1, -1, 3] and labels == ["b", "a", ("t", 1), 7]
    assert str(gof.dtype) == "torch.int32"
    gof, labels = group_labels([None, None])
    assert gof.tolist() == [-1, -1] and labels == []
    gof, labels = group_labels([])
    assert gof.numel() == 0 and labels == []
    # the public surface exists (its device side: tests/test_gpu_group.py)
    assert callable(ColbertIndex.groups) and callable(ColbertIndex.search_grouped) and callable(group_topk_rows)
    assert DocGroups.__init__.__code__.co_varnames[:5] == ("self", "index", "group_of", "G", "labels")


def test_document_keys():
    store = ChunkStore([{"chunk_id": 0, "text": "a", "document_id": "doc-x"},
                        {"chunk_id": 1, "text": "b", "document_id": "doc-y"},
                        {"chunk_id": 3, "text": "c", "document_id": "doc-x"},
                        {"chunk_id": 4, "text": "d"}])
    assert store.document_keys(6) == ["doc-x", "doc-y", None, "doc-x", None, None]
    assert store.document_keys(0) == [] and store.document_keys(2) == ["doc-x", "doc-y"]
    gof, labels = group_labels(store.document_keys(6))
    assert gof.tolist() == [0, 1, -1, 0, -1, -1] and labels == ["doc-x", "doc-y"]
    assert store.ids_of_document("doc-x") == [0, 3]          # the filters' view of the same key
