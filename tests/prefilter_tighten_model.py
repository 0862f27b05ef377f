"""numpy statement of the pre-filter's threshold tightening: the upper and lower bound of every (row, query) as the
filter kernel evaluates them in fp32, the k-th largest lower bound that replaces a query's sampling threshold, and the rows that
still stand against it.  tests/test_prefilter_tighten_model.py holds the argument against the input families without a device;
tests/test_prefilter_tighten_gpu.py counts with it what the device must at least keep."""
import numpy as np

from tests import prefilter_model as pm

F32 = pm.F32


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays: the product of two fp32 numbers is exact in fp64, the sum is rounded once more on the way to fp32"""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def int_parts(m, hi, lo):
    """[n] the two integer sums of one query (exact: every partial sum is an integer below 2^24 in magnitude for d <= 1024)"""
    mf = np.asarray(m, F32)
    return mf @ np.asarray(hi, F32), mf @ np.asarray(lo, F32)


def bounds(a_r, b_r, I_hi, I_lo, a_q, B_q, c_q):
    """([n] ub, [n] lb) of one query, operation by operation as q8_filter_kernel: ti = fmaf(I_lo, 1 / 254, I_hi), e = fmaf(B_q, b, c_q),
    ub = fmaf(a_r a_q, ti, e), lb = fmaf(a_r a_q, ti, -e)"""
    ti = fma32(I_lo, F32(1.0 / 254.0), I_hi)
    e = fma32(F32(B_q), b_r, F32(c_q))
    s = (np.asarray(a_r, F32) * F32(a_q)).astype(F32)
    return fma32(s, ti, e), fma32(s, ti, -e)


def kth_largest(v, k):
    """the k-th largest of the numbers in v (NaN are not counted); None with fewer than k of them"""
    v = np.asarray(v)
    v = v[v == v]
    if len(v) < k:
        return None
    return np.partition(v, len(v) - k)[len(v) - k]


def standing(ub, tau):
    """[n] bool: the rows the tightening keeps against the threshold tau — !(ub < tau), so a NaN bound stays"""
    return ~(ub < tau) if tau is not None else np.ones(len(ub), bool)
