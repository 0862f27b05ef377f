"""CPU tier: the input families of tests/test_value_domain_gpu.py have the properties its assertions rely on (numpy oracle only),
at every size and dtype that file uses — so that none of its tests passes vacuously."""
import numpy as np
import pytest

from oracle import retrieval_np as orc
from tests import value_domain_inputs as vd

ALL = {**vd.SEARCH_ROUTES, **vd.MIN_SCORE_ROUTES, **vd.SCORES_ROUTES, **vd.STREAM_ROUTES, **vd.EXACT_ROUTES}
# (the rejected-append and out-of-range tests draw family P at 64-d with seeds 1000, 13 061, 5, 6, 8)
SHAPES = sorted({(s["dtype"], s["d"], s["n"], s["nq"], s["seed"]) for s in ALL.values()} |
                {("f16", 64, 13_061, 3, 8), ("bf16", 64, 13_061, 3, 8), ("bf16", 64, 1023, 3, 1000), ("f32", 64, 13_084, 3, 13_061), ("f16", 48, 1000, 5, 8)})


def _scores(dtype, X, Q):
    rnd = vd.ROUND[dtype]
    return orc.exact_scores_f64(rnd(X), rnd(Q))


def test_no_size_is_a_multiple_of_the_panel():
    assert all(s["n"] % 32 for s in ALL.values()) and (vd.N_BIG + 31) // 32 == 4098 and vd.N_BIG % 32 == 5
    seeds = [s["seed"] for s in ALL.values()]
    assert len(set(seeds)) == len(seeds)      # every table row draws its own data


@pytest.mark.parametrize("dtype,d,n,nq,seed", SHAPES)
def test_family_p_sign_margin(dtype, d, n, nq, seed):
    X, Q = vd.family_p(n, d, nq, seed=seed)
    S = _scores(dtype, X, Q)
    tol = vd.ERR * 1.01 * 1.01
    assert S.min() > 0.3 and S.min() > 1e4 * tol, S.min()      # the sign is never in doubt: no score within rounding of 0


@pytest.mark.parametrize("dtype,d,n,nq,seed", SHAPES)
def test_family_z_zero_rows_are_the_unique_top_three(dtype, d, n, nq, seed):
    X, Q = vd.family_z(n, d, nq, seed=seed)
    S = _scores(dtype, X, Q)
    z = vd.zero_rows(n)
    assert len(set(z)) == 3 and z == sorted(z)
    assert np.all(S[:, z] == 0) and not np.any(np.signbit(S[:, z]))
    rest = np.delete(S, z, axis=1)
    assert rest.max() < -0.3
    ids, _ = orc.topk_rule(S, 5)
    assert np.all(ids[:, :3] == np.array(z))
    # min_score = -0.5 lets negative rows through besides the three zero rows, more than a list of 20 holds; a bound between the
    # 8th and 9th best score of query 0 lets exactly 8 through there — the threshold-search test uses both
    spec = [s for s in vd.MIN_SCORE_ROUTES.values() if s["seed"] == seed]
    if spec:
        below = spec[0].get("below", vd.MIN_SCORE_BELOW)
        assert below < -0.3 and (S >= below + 1e-4).sum(axis=1).max() > 20, (S >= below).sum(axis=1)      # one query fills its list of 20
        top = np.sort(S[0])[::-1]
        few = float(np.float32(top[7:9].mean()))
        assert top[7] - few > 10 * vd.ERR and few - top[8] > 10 * vd.ERR and (S[0] >= few).sum() == 8


@pytest.mark.parametrize("dtype,d,n,nq,seed", SHAPES)
def test_family_t_blocks(dtype, d, n, nq, seed):
    X, Q = vd.family_t(n, d, nq, seed=seed)
    assert np.all(X == X[0])
    X, Q, n_a = vd.family_t2(n, d, nq, dtype, seed=seed)
    S = _scores(dtype, X, Q)
    assert 0 < n_a < n and n - n_a >= 500 and np.all(X[:n_a] == X[0]) and np.all(X[n_a:] == X[n_a])
    assert np.all(S[:, n_a] - S[:, 0] > 0.2)      # b beats a by far more than any rounding


@pytest.mark.parametrize("dtype,d,n,nq,seed", SHAPES)
def test_family_s_scaling_is_exact(dtype, d, n, nq, seed):
    rnd = vd.ROUND[dtype]
    X0, Q0 = vd.family_s(n, d, nq, dtype, seed=seed)
    assert np.array_equal(rnd(X0), X0) and np.array_equal(rnd(Q0), Q0)
    S0 = orc.exact_scores_f64(X0, Q0)
    for a, b in vd.SCALES:
        Xs, Qs = vd.scaled(X0, a), vd.scaled(Q0, b)
        assert np.array_equal(Xs.astype(np.float64), X0.astype(np.float64) * 2.0 ** a)
        assert np.array_equal(rnd(Xs), Xs) and np.array_equal(rnd(Qs), Qs)
        assert max(np.abs(Xs).max(), np.abs(Qs).max()) < 65504
        if dtype == "f16":      # no subnormal operand on either side of the scaling
            for A in (X0, Q0, Xs, Qs):
                assert np.all((A == 0) | (np.abs(A) >= 2.0 ** -14))
        assert np.array_equal(orc.exact_scores_f64(Xs, Qs), S0 * 2.0 ** (a + b))
    assert np.count_nonzero(X0) > 0.97 * X0.size      # (zeroing the small components left the rows what they were)


def test_family_n_norms_and_exact_certificates():
    X, Q = vd.family_n(13_061, 64, 4, seed=1)
    xn = np.linalg.norm(X.astype(np.float64), axis=1)
    assert xn.min() < 2e-3 and xn.max() > 25 and xn.max() < 32
    assert np.allclose(np.linalg.norm(Q.astype(np.float64), axis=1), [1, 7, 1, 7], rtol=1e-5)
    # the exact search: query 0 certified by the first stage (128 candidates), query 1 by neither stage — with room to spare
    spec = vd.EXACT_ROUTES["exact"]
    X, Q = vd.family_n_exact(spec["n"], spec["d"])
    c1, m1 = vd.reference_certified(X, Q, spec["k"], spec["dtype"], 128)
    c2, m2 = vd.reference_certified(X, Q, spec["k"], spec["dtype"], 4096)
    assert c1[0] and m1[0] > 1.0, (c1, m1)
    assert not c1[1] and not c2[1] and m2[1] < -1.0, (c2, m2)
    S = orc.exact_scores_f64(X, Q[:1])[0]
    top = np.sort(S)[::-1]
    assert top[0] > top[spec["k"] - 1] > top[127] > 0


def test_family_o_values():
    with np.errstate(over="ignore"):
        assert np.isinf(orc.f16_round(np.float32([vd.OVERFLOW["f16"]])))[0] and np.isinf(orc.bf16_round(np.float32([vd.OVERFLOW["bf16"]])))[0]
        assert np.isfinite(orc.f16_round(np.float32([65504.0])))[0] and np.isinf(orc.f16_round(np.float32([65520.0])))[0]
        assert np.isfinite(orc.f16_round(np.float32([65519.996])))[0]
    assert np.isfinite(np.float32(vd.OVERFLOW["bf16"]))
    X, Q = vd.family_o_subnormal(1000, 64)
    Xr = orc.f16_round(X)
    assert np.all((np.abs(Xr) > 2.0 ** -24 * 0.99) & (np.abs(Xr) < 2.0 ** -14))
    S = orc.exact_scores_f64(Xr, orc.f16_round(Q))
    tol = np.stack([vd.row_tol(q, Xr) for q in orc.f16_round(Q)])
    assert np.median(np.abs(S)) > 100 * tol.max()      # a flush to zero would show


def test_row_tolerance_is_the_norm_product():
    q = np.float32([3, 4]); X = np.float32([[0, 0], [1, 0], [6, 8]])
    assert np.allclose(vd.row_tol(q, X), vd.ERR * 5 * np.array([1e-30, 1, 10]))
    assert np.allclose(vd.row_tol(q / 50, X), vd.ERR * np.array([1e-30, 1, 10]))
