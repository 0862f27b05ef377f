"""The threshold tightening of the certified int8 pre-filter, held on the CPU: the lower bound lb = s^ - (B_q b + c_q)
the filter records never exceeds the scan's score, so the k-th largest lb of k distinct rows — of ALL rows or of any subset — is a
threshold below which no row of the top-k, ties included, can have its upper bound."""
import numpy as np
import pytest

from tests import prefilter_model as pm
from tests import prefilter_tighten_model as tm
from tests import value_domain_inputs as vd

N, NQ = 1500, 8
KS = (1, 20, 128)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("family", pm.FAMILIES)
def test_kth_lower_bound_drops_no_row_of_the_top_k(family, d, dtype):
    X, Q = pm.family(family, N, d, NQ, seed=d)
    Xt, Qt = vd.ROUND[dtype](X), vd.ROUND[dtype](Q)
    a_r, m, b_r, nx = pm.quantise_rows(Xt)
    Mx = nx.max()
    s32 = (Xt @ Qt.T).astype(np.float32)
    s64 = Xt.astype(np.float64) @ Qt.astype(np.float64).T
    gamma = d * 2.0 ** -23
    rng = np.random.default_rng(99 + d)
    for j in range(NQ):
        a_q, hi, lo, B_q, c_q = pm.quantise_query(Qt[j], Mx, (d + 127) // 128 * 128)
        ub, lb = tm.bounds(a_r, b_r, *tm.int_parts(m, hi, lo), a_q, B_q, c_q)
        assert np.all(lb == lb) and np.all(ub == ub)
        # the lower bound as the kernel computes it: never above the scan's score, in either statement of that score
        assert np.all(lb <= s32[:, j]), (family, j)
        assert np.all(lb.astype(np.float64) <= s64[:, j] + gamma * np.linalg.norm(Qt[j].astype(np.float64)) * nx), (family, j)
        assert np.all(ub >= s32[:, j]), (family, j)
        half = rng.permutation(N)[:N // 2]
        for k in KS:
            kth_score = np.sort(s32[:, j])[::-1][k - 1]
            top = s32[:, j] >= kth_score                     # the k best and everything tied with the k-th
            for rows in (np.arange(N), half):                # all pairs / what an overflowed list would hold
                tau = tm.kth_largest(lb[rows], k)
                assert tau is not None and tau <= kth_score
                assert np.all(tm.standing(ub, tau)[top]), (family, j, k, len(rows))
            assert tm.kth_largest(lb[half], k) <= tm.kth_largest(lb, k)      # a subset is only looser


def test_selection_counts_numbers_only():
    v = np.array([3.0, np.nan, 1.0, 2.0, np.nan], np.float32)
    assert tm.kth_largest(v, 1) == 3.0 and tm.kth_largest(v, 3) == 1.0 and tm.kth_largest(v, 4) is None
    ub = np.array([0.5, np.nan, 2.0], np.float32)
    assert tm.standing(ub, np.float32(1.0)).tolist() == [False, True, True]
    assert tm.standing(ub, None).all()


def test_fma_matches_a_single_rounding():
    a, b, c = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 - 2.0 ** -23), np.float32(-1.0)
    assert tm.fma32(a, b, c) == np.float32(-(2.0 ** -46))      # a b + c exactly; (a * b) rounded first would give 0
