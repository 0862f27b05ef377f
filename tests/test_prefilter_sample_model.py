"""The int8 sampling threshold of the certified pre-filter, held on the CPU: the k-th largest lower bound tau_s among the
rows of a strided sample never exceeds the k-th best 16-bit score of the whole corpus, no row at or above that k-th best (ties
included) has its upper bound below tau_s, and the threshold key built from tau_s keeps every row that scores tau_s or more."""
import numpy as np
import pytest

from tests import prefilter_model as pm
from tests import prefilter_sample_model as sm
from tests import prefilter_tighten_model as tm
from tests import value_domain_inputs as vd

N, NQ = 1500, 8          # 47 panels, the last one with 28 rows
KS = (1, 20, 128)
NP = (N + 31) // 32
# (run, stride, runs): single panels; runs whose last one ends in the partial panel (panels 40 .. 46); a run the corpus' end cuts
# (panels 45 .. 46 of 45 .. 49); full coverage; more runs than the corpus has room for (waves without a run)
SAMPLES = ((1, 3, 16), (7, 8, 6), (5, 9, 6), (4, 4, 12), (2, 5, 64))


def test_sample_shapes_cover_what_they_claim():
    assert len(sm.sample_rows(N, 1, 3, 16)) == 16 * 32
    assert sm.sample_rows(N, 7, 8, 6)[-1] == N - 1 and len(sm.sample_rows(N, 7, 8, 6)) == 6 * 7 * 32 - 4
    assert sm.sample_rows(N, 5, 9, 6)[-1] == N - 1 and len(sm.sample_rows(N, 5, 9, 6)) == 5 * 5 * 32 + 32 + 28
    assert np.array_equal(sm.sample_rows(N, 4, 4, 12), np.arange(N))
    assert len(sm.sample_rows(N, 2, 5, 64)) == 9 * 64 + 32 + 28        # runs 0 .. 8 whole, run 9 = panels 45, 46; the rest have no run
    assert len(sm.sample_rows(70, 1, 1, 1)) == 32 and len(sm.sample_rows(70, 1, 4, 3)) == 32


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("family", pm.FAMILIES)
def test_sample_threshold_drops_no_row_of_the_top_k(family, d, dtype):
    X, Q = pm.family(family, N, d, NQ, seed=d)
    Xt, Qt = vd.ROUND[dtype](X), vd.ROUND[dtype](Q)
    a_r, m, b_r, nx = pm.quantise_rows(Xt)
    Mx = nx.max()
    s32 = (Xt @ Qt.T).astype(np.float32)
    all_rows = np.arange(N)
    for j in range(NQ):
        a_q, hi, lo, B_q, c_q = pm.quantise_query(Qt[j], Mx, (d + 127) // 128 * 128)
        ub, lb = tm.bounds(a_r, b_r, *tm.int_parts(m, hi, lo), a_q, B_q, c_q)
        score_keys = sm.make_key(s32[:, j], all_rows)
        for k in KS:
            kth_score = np.sort(s32[:, j])[::-1][k - 1]
            top = s32[:, j] >= kth_score                     # the k best and everything tied with the k-th
            for run, stride, nruns in SAMPLES:
                rows = sm.sample_rows(N, run, stride, nruns)
                tau_s = sm.sample_threshold(lb, rows, k)
                if len(rows) < k:
                    assert tau_s is None
                    assert sm.threshold_key(tau_s, 12345) == 12345      # the level-0 key is passed on
                    continue
                assert tau_s is not None and tau_s <= kth_score, (family, j, k, run, stride)
                assert np.all(tm.standing(ub, tau_s)[top]), (family, j, k, run, stride)
                key = sm.threshold_key(tau_s)
                keeps = score_keys > key
                assert np.all(keeps[s32[:, j] >= tau_s]), (family, j, k, run, stride)      # a row tied with tau_s stays
                assert np.all(keeps[top])
                # the key is exactly that threshold: nothing below tau_s passes it
                assert not np.any(keeps[s32[:, j] < tau_s])
                # against a level-0 key: the larger of the two is written
                lvl0 = sm.make_key(np.float32(kth_score), 7)
                assert sm.threshold_key(tau_s, lvl0) == max(key, lvl0)


def test_key_of_a_threshold_at_the_edges():
    rows = np.arange(4)
    for tau in (np.float32(0.0), np.float32(-0.0), np.float32(1.5), np.float32(-2.25), np.float32(-np.inf)):
        key = sm.threshold_key(tau)
        s = np.array([tau, np.nextafter(tau, np.float32(np.inf)), np.float32(3.0), np.float32(0.0) if tau <= 0 else tau], np.float32)
        assert np.all(sm.make_key(s, rows) > key)
        if np.isfinite(tau):
            below = np.full(4, np.nextafter(tau, np.float32(-np.inf)), np.float32)
            if not (tau == 0 and below[0] == 0):
                assert not np.any(sm.make_key(below, rows) > key)
    # +0 and -0 are one score: a threshold of -0 keeps a row scoring +0 and the other way round
    assert sm.make_key(np.float32(0.0), 5) > sm.threshold_key(np.float32(-0.0))
    assert sm.make_key(np.float32(-0.0), 5) > sm.threshold_key(np.float32(0.0))
    # row 0xFFFFFFFE, the largest row id there is, still passes at a tie
    assert sm.make_key(np.float32(1.5), 0xFFFFFFFE) > sm.threshold_key(np.float32(1.5))
