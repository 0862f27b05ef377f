"""Per-query filtered search, host side: the layout of the per-query allow bitmaps (`pack_row_masks`) and the two entry points' NULL
checks, which come before any device call and so hold on a CPU-only host."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_mask, pack_row_masks


def test_layout_is_query_major_rows_of_pack_row_mask():
    m = pack_row_masks(40, allow=[[0], [33], [31, 32], []])
    assert m.dtype == np.uint32 and m.shape == (4, 2) and m.flags["C_CONTIGUOUS"]
    assert m.tolist() == [[1, 0], [0, 2], [0x80000000, 1], [0, 0]]
    e = pack_row_masks(40, exclude=[[], [0, 39]])
    assert e.tolist() == [[0xFFFFFFFF, 0xFF], [0xFFFFFFFE, 0x7F]]              # tail bits stay zero


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_agrees_with_pack_row_mask_row_by_row(n):
    rng = np.random.default_rng(n)
    keeps = [rng.random(n) < p for p in (0.5, 0.01, 1.0, 0.0, 0.3)]
    entries = [keeps[0], np.flatnonzero(keeps[1]), np.flatnonzero(keeps[2]).tolist(), [], iter(np.flatnonzero(keeps[4]).tolist())]
    m = pack_row_masks(n, allow=entries)
    assert m.shape == (5, (n + 31) // 32)
    for i, keep in enumerate(keeps):
        assert np.array_equal(m[i], pack_row_mask(n, allow=keep))
        full = np.unpackbits(m[i].view(np.uint8), bitorder="little")
        assert np.array_equal(full[:n].astype(bool), keep) and not full[n:].any()
    ex = pack_row_masks(n, exclude=[np.flatnonzero(k) for k in keeps])
    for i, keep in enumerate(keeps):
        assert np.array_equal(ex[i], pack_row_mask(n, exclude=np.flatnonzero(keep)))
    assert np.array_equal(pack_row_masks(n, allow=np.stack(keeps)), m)         # a 2-d bool array: one bool row per query
    assert pack_row_masks(n, allow=[]).shape == (0, (n + 31) // 32)


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        pack_row_masks(10)                                                      # the number of queries has to come from somewhere
    with pytest.raises(ValueError):
        pack_row_masks(10, allow=[[1]], exclude=[[2]])
    with pytest.raises(ValueError):
        pack_row_masks(10, allow=3)
    for bad in ([[0], [10]], [[-1]], [[0.5]], [np.ones(9, dtype=bool)]):
        with pytest.raises(ValueError):
            pack_row_masks(10, allow=bad)
    with pytest.raises(ValueError):
        pack_row_masks(10, exclude=[[0], [11]])
    with pytest.raises(ValueError):
        pack_row_masks(-1, allow=[[]])


def test_entry_points_reject_null_arguments_without_a_device():
    """cmr_index_search_masked_each / _dev: a NULL handle or NULL arguments give CMR_ERR_INVALID before any device call."""
    lib = L.lib()
    q = np.zeros((2, 8), np.float32)
    ids = np.zeros((2, 4), np.int64)
    sc = np.zeros((2, 4), np.float32)
    w = np.ones((2, 1), np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    assert lib.cmr_index_search_masked_each(None, p(q), 2, 4, p(w), 1, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert b"NULL" in lib.cmr_last_error()
    assert lib.cmr_index_search_masked_each(None, None, 2, 4, None, 0, None, None, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_index_search_masked_each_dev(None, p(q), 2, 4, p(w), 1, p(ids), p(sc), None, None, None) == L.CMR_ERR_INVALID
    assert b"NULL" in lib.cmr_last_error()
    assert lib.cmr_index_search_masked_each_dev(None, None, 2, 4, None, 0, None, None, None, None, None) == L.CMR_ERR_INVALID


def test_route_bit_is_in_the_header():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "comorag_hip.h")).read()
    assert "#define CMR_ROUTE_FILTERED_EACH (1 << 13)" in hdr and '"combine_filtered"' in hdr
