"""Filtered search, host side: the allow bitmap's layout (`pack_row_mask`) and the two entry points' argument checks, which come before
any device call and so hold on a CPU-only host."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_mask


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def test_bit_layout():
    m = pack_row_mask(40, allow=[0])
    assert m.dtype == np.uint32 and m.tolist() == [1, 0]                    # row 0 -> bit 0 of word 0
    assert pack_row_mask(40, allow=[33]).tolist() == [0, 2]                 # row 33 -> bit 1 of word 1
    assert pack_row_mask(64, allow=[31, 32]).tolist() == [0x80000000, 1]
    assert pack_row_mask(40).tolist() == [0xFFFFFFFF, 0xFF]                 # neither argument: every row, tail bits zero


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_word_count_and_zero_tail(n):
    m = pack_row_mask(n)
    assert m.shape == ((n + 31) // 32,) and m.dtype == np.uint32
    full = np.unpackbits(m.view(np.uint8), bitorder="little")
    assert full[:n].all() and not full[n:].any()
    rng = np.random.default_rng(n)
    keep = rng.random(n) < 0.5
    keep[-1] = True                                                         # the last row's bit is the highest one that may be set
    m = pack_row_mask(n, allow=keep)
    full = np.unpackbits(m.view(np.uint8), bitorder="little")
    assert np.array_equal(full[:n].astype(bool), keep) and not full[n:].any()


@pytest.mark.parametrize("n", [1, 33, 1000])
def test_bool_array_id_list_and_exclude_agree(n):
    rng = np.random.default_rng(100 + n)
    keep = rng.random(n) < 0.3
    ids = np.flatnonzero(keep)
    a = pack_row_mask(n, allow=keep)
    assert np.array_equal(a, pack_row_mask(n, allow=ids))
    assert np.array_equal(a, pack_row_mask(n, allow=ids.tolist()))
    assert np.array_equal(a, pack_row_mask(n, allow=iter(ids.tolist())))
    assert np.array_equal(a, pack_row_mask(n, allow=ids[::-1].astype(np.int32)))      # order and width of the ids do not matter
    ex = pack_row_mask(n, exclude=ids)
    assert np.array_equal(_bits(ex, n), ~keep)                              # the complement ...
    assert np.array_equal(ex | a, pack_row_mask(n)) and not (ex & a).any()  # ... tail bits still zero
    assert np.array_equal(pack_row_mask(n, exclude=[]), pack_row_mask(n))
    assert not pack_row_mask(n, allow=[]).any()


def test_bad_arguments_raise():
    for bad in ([-1], [10], [0, 10], np.array([3, 11])):
        with pytest.raises(ValueError):
            pack_row_mask(10, allow=bad)
        with pytest.raises(ValueError):
            pack_row_mask(10, exclude=bad)
    with pytest.raises(ValueError):
        pack_row_mask(10, allow=[1], exclude=[2])
    with pytest.raises(ValueError):
        pack_row_mask(10, allow=np.ones(9, dtype=bool))
    with pytest.raises(ValueError):
        pack_row_mask(10, allow=[0.5])


def test_filtered_entry_points_reject_null_arguments_without_a_device():
    """cmr_index_search_masked / _dev: a NULL handle or NULL arguments give CMR_ERR_INVALID before any device call."""
    lib = L.lib()
    q = np.zeros((1, 8), np.float32)
    ids = np.zeros((1, 4), np.int64)
    sc = np.zeros((1, 4), np.float32)
    w = np.ones(1, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    assert lib.cmr_index_search_masked(None, p(q), 1, 4, p(w), 1, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert b"NULL" in lib.cmr_last_error()
    assert lib.cmr_index_search_masked(None, None, 1, 4, None, 0, None, None, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_index_search_masked_dev(None, p(q), 1, 4, p(w), 1, p(ids), p(sc), None, None, None) == L.CMR_ERR_INVALID
    assert b"NULL" in lib.cmr_last_error()
    assert lib.cmr_index_search_masked_dev(None, None, 1, 4, None, 0, None, None, None, None, None) == L.CMR_ERR_INVALID
