"""numpy statement of the pre-filter's int8 sampling threshold: which rows a sample of strided panel runs covers, the
k-th largest lower bound among them (tau_s) and the threshold key built from it as the device builds it.
tests/test_prefilter_sample_model.py holds the argument against the input families without a device."""
import numpy as np

from tests import prefilter_tighten_model as tm

PANEL = 32


def sample_rows(n, run, stride, nruns):
    """the real rows of a sample of `nruns` runs of `run` consecutive panels, run g starting at panel g * stride (stride >= run: no row
    twice); a run is cut by the corpus' end, the padding rows of the last panel are no rows"""
    assert stride >= run >= 1
    npanels = (n + PANEL - 1) // PANEL
    rows = []
    for g in range(nruns):
        p0 = g * stride
        p1 = min(p0 + run, npanels)
        if p0 < p1:
            rows.append(np.arange(p0 * PANEL, min(p1 * PANEL, n)))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    assert len(np.unique(rows)) == len(rows)
    return rows


def ord32(f):
    """the order-preserving 32-bit image of fp32 numbers as cmr_make_key takes it (-0 counts as +0)"""
    u = (np.asarray(f, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def make_key(score, row):
    """cmr_make_key: score image in the upper half, 0xFFFFFFFF - row in the lower (of two equal scores the smaller row has the larger key)"""
    return (ord32(score) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(row, np.uint64))


def threshold_key(tau_s, level0_key=0):
    """the key the select step writes: the smallest key with score tau_s, minus 1 (so key > tau <=> score >= tau_s), or the level-0
    key where that is larger; tau_s None (fewer than k records): the level-0 key alone"""
    if tau_s is None:
        return np.uint64(level0_key)
    key = make_key(np.float32(tau_s), 0xFFFFFFFF) - np.uint64(1)
    return max(np.uint64(key), np.uint64(level0_key))


def sample_threshold(lb, rows, k):
    """tau_s: the k-th largest lower bound among the sampled rows (None with fewer than k numbers)"""
    return tm.kth_largest(lb[rows], k)
