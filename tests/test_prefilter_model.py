"""The bound of the certified int8 pre-filter, held on the CPU: for every (row, query) of every input family the
scan's score lies within B_q b_r + c_q of the int8 score — so a row whose upper bound is below a threshold cannot reach it."""
import numpy as np
import pytest

from tests import prefilter_model as pm
from tests import value_domain_inputs as vd

N, NQ = 1500, 8


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("family", pm.FAMILIES)
def test_bound_holds_for_every_row_and_query(family, d, dtype):
    X, Q = pm.family(family, N, d, NQ, seed=d)
    Xt, Qt = vd.ROUND[dtype](X), vd.ROUND[dtype](Q)
    a_r, m, b_r, nx = pm.quantise_rows(Xt)
    Mx = nx.max()
    # the scan's score: fp32 accumulation of the rounded operands (any order is within gamma ||q|| ||x|| of the exact dot)
    s32 = (Xt @ Qt.T).astype(np.float32)
    s64 = Xt.astype(np.float64) @ Qt.astype(np.float64).T
    assert np.all(np.abs(Xt.astype(np.float64) - a_r.astype(np.float64)[:, None] * m) <= np.abs(Xt) * (1.0 + 1e-6))      # |e_i| <= |x_i|: b_r <= ||x||, |s^| <= 2 ||Q^|| M_x
    for j in range(NQ):
        a_q, hi, lo, B_q, c_q = pm.quantise_query(Qt[j], Mx, (d + 127) // 128 * 128)
        s_hat = pm.int8_scores(a_r, m, a_q, hi, lo)
        bound = B_q.astype(np.float64) * b_r.astype(np.float64) + float(c_q)
        for s in (s32[:, j].astype(np.float64), s64[:, j]):
            err = np.abs(s_hat.astype(np.float64) - s)
            assert np.all(err <= bound), (family, j, float((err - bound).max()))
        # the comparison as the kernel makes it, in fp32: the upper bound is never below the scan's score
        ub = pm.upper_bounds(s_hat, b_r, B_q, c_q)
        assert np.all(ub >= s32[:, j]), (family, j)
        assert np.all(ub.astype(np.float64) >= s64[:, j] - (d * 2.0 ** -23) * np.linalg.norm(Qt[j].astype(np.float64)) * nx), (family, j)


def test_spike_rows_put_the_whole_score_into_the_error_term():
    """the family is what it claims: the rest of a spike row quantises to zero, and the query of row i scores ||rest|| on it while
    the int8 score is (next to) nothing — the bound has to come from B_q b_r alone"""
    d = 128
    X, Q = pm.spike_family(64, d, 4)
    Xt, Qt = vd.ROUND["bf16"](X), vd.ROUND["bf16"](Q)
    a_r, m, b_r, nx = pm.quantise_rows(Xt)
    assert np.all((m != 0).sum(axis=1) == 1)
    for j in range(4):
        a_q, hi, lo, B_q, c_q = pm.quantise_query(Qt[j], nx.max(), d)
        s = float(Xt[j].astype(np.float64) @ Qt[j].astype(np.float64))
        s_hat = float(pm.int8_scores(a_r, m, a_q, hi, lo)[j])
        assert s > 0.5 * float(b_r[j]) and abs(s_hat) < 0.05 * s
        assert s - s_hat <= float(B_q) * float(b_r[j]) + float(c_q)


def test_zero_rows_and_zero_query_quantise_to_nothing():
    a_r, m, b_r, nx = pm.quantise_rows(np.zeros((3, 128), np.float32))
    assert not a_r.any() and not m.any() and not b_r.any() and not nx.any()
    a_q, hi, lo, B_q, c_q = pm.quantise_query(np.zeros(128, np.float32), 1.0, 128)
    assert a_q == 0 and not hi.any() and not lo.any() and B_q == 0 and 0 < c_q < 2e-7


def test_two_part_query_is_finer_than_one_part():
    rng = np.random.default_rng(5)
    q = vd.ROUND["bf16"](rng.standard_normal((1, 768), dtype=np.float32) / np.sqrt(768))[0]
    a_q, hi, lo, B_q, c_q = pm.quantise_query(q, 1.0, 768)
    one = np.linalg.norm(q.astype(np.float64) - float(a_q) * hi)
    two = np.linalg.norm(q.astype(np.float64) - float(a_q) * (hi + lo / 254.0))
    assert two < one / 50
