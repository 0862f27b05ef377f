"""Seeded input families and the route table of tests/test_value_domain_gpu.py (un-normalised, one-signed, tied and out-of-range
inputs on every search route).  numpy only: tests/test_value_domain_inputs.py checks here, without a device, the properties the GPU
tests rely on, so that none of them passes vacuously."""
import numpy as np

from oracle import retrieval_np as orc

ROUND = {"bf16": orc.bf16_round, "f16": orc.f16_round, "f32": lambda x: np.asarray(x, np.float32)}
ERR = 4e-6      # the project's bound for unit-norm operands; scaled per row by row_tol

# last_route (include/comorag_hip.h), low byte: path | levels << 4 | tau_in_scan << 6 | single 128-panel level << 7; above it query tiles << 8,
# threshold search << 10 and MORE_PASSES
TINY, SMALL, CHAIN, FIN, WIDE, QSPLIT, LARGE_K, SCORES_SINGLE, SCORES, SORTED = range(1, 11)
MORE_PASSES = 1 << 11      # the batch took several corpus passes and last_route describes the first: no test here may see it


def route_code(path, levels=0, tau_in_scan=False, single=False):
    return path | levels << 4 | int(tau_in_scan) << 6 | int(single) << 7


# tag -> what to build and call (seed: the row's own data), and the low byte of last_route the call must leave.  Every n is no multiple of 32; 131 109 rows are
# 4 098 panels with 5 real rows in the last one: the finishing stage needs npanels >= 16 n_cu, i.e. a device of at most 256 CUs.
N_BIG = 131_109
SEARCH_ROUTES = {
    "tiny1": dict(seed=11, dtype="bf16", d=48, n=1000, nq=5, k=20, opts={}, route=route_code(TINY)),
    "tiny1-1wg": dict(seed=12, dtype="f16", d=48, n=1000, nq=5, k=20, opts={"tiny_multi": 0}, route=route_code(TINY)),
    "small": dict(seed=13, dtype="bf16", d=64, n=13_061, nq=3, k=20, opts={}, route=route_code(SMALL)),
    "chain0": dict(seed=14, dtype="bf16", d=64, n=5003, nq=3, k=20, opts={"scan_no_tiny": 1}, route=route_code(CHAIN, 0)),
    "chain1": dict(seed=15, dtype="f16", d=64, n=13_061, nq=3, k=20, opts={"scan_no_tiny": 1}, route=route_code(CHAIN, 1)),
    "chain2": dict(seed=16, dtype="bf16", d=64, n=N_BIG, nq=3, k=20, opts={"scan_no_small": 1, "scan_fin": 0, "sample_single": 0}, route=route_code(CHAIN, 2)),
    "single": dict(seed=17, dtype="bf16", d=64, n=N_BIG, nq=5, k=20, opts={"scan_no_small": 1, "scan_fin": 0}, route=route_code(CHAIN, 1, single=True)),
    "tau-in-scan": dict(seed=18, dtype="bf16", d=64, n=N_BIG, nq=1, k=20, opts={"scan_no_small": 1, "scan_fin": 0}, route=route_code(CHAIN, 1, True, True)),
    "fin1": dict(seed=19, dtype="bf16", d=64, n=N_BIG, nq=1, k=20, opts={"scan_no_small": 1}, route=route_code(FIN), max_cu=256),
    "fin8": dict(seed=20, dtype="bf16", d=64, n=N_BIG, nq=8, k=20, opts={"scan_no_small": 1}, route=route_code(FIN), max_cu=256),
    "two-tile": dict(seed=21, dtype="bf16", d=64, n=5003, nq=40, k=20, opts={}, route=route_code(CHAIN, 0), nqt=2),
    "wide": dict(seed=22, dtype="bf16", d=768, n=8197, nq=70, k=20, opts={"wide_mode": 1}, route=route_code(WIDE, 1)),
    "quad": dict(seed=23, dtype="f16", d=768, n=8197, nq=70, k=20, opts={"wide_mode": 2}, route=route_code(QSPLIT, 1)),
    "quad-f32": dict(seed=24, dtype="f32", d=200, n=8197, nq=70, k=20, opts={}, route=route_code(QSPLIT, 1)),
    "large-k": dict(seed=25, dtype="bf16", d=64, n=5003, nq=3, k=500, opts={}, route=route_code(LARGE_K)),
}
# scores() / sorted_scores(): (dtype, d, n, nq, options, last_route after scores())
SCORES_ROUTES = {
    "scores-1000": dict(seed=26, dtype="bf16", d=48, n=1000, nq=3, opts={}, route=route_code(SCORES_SINGLE)),
    "scores-13061": dict(seed=27, dtype="f16", d=64, n=13_061, nq=3, opts={}, route=route_code(SCORES_SINGLE)),
    "scores-13061-general": dict(seed=28, dtype="bf16", d=64, n=13_061, nq=3, opts={"scan_no_small": 1}, route=route_code(SCORES)),
    "scores-70001": dict(seed=29, dtype="bf16", d=64, n=70_001, nq=4, opts={}, route=route_code(SCORES)),      # 4 x 70 001 scores: beyond the mapped buffer
}
MIN_SCORE_ROUTES = {
    "min-score-5003": dict(seed=30, dtype="bf16", d=64, n=5003, nq=3, k=20, opts={}, route=route_code(CHAIN, 0)),
    "min-score-big": dict(seed=31, dtype="bf16", d=64, n=N_BIG, nq=3, k=20, opts={}, route=route_code(CHAIN, 0)),
    # the wide routes of the threshold search (no sampling level: the plain search's "wide" / "quad" rows have one).  below: at 768-d family
    # Z's negative scores lie in -0.64 +- 0.04, so the bound that lets "far more than k rows" through is -0.62 there, not -0.5
    "min-score-wide": dict(seed=32, dtype="bf16", d=768, n=8197, nq=70, k=20, opts={"wide_mode": 1}, route=route_code(WIDE, 0), below=-0.62),
    "min-score-quad": dict(seed=33, dtype="f16", d=768, n=8197, nq=70, k=20, opts={"wide_mode": 2}, route=route_code(QSPLIT, 0), below=-0.62),
}
MIN_SCORE_BELOW = -0.5      # test_min_score_at_and_below_zero: the bound below zero that fills a list (a row's "below" replaces it)
# the stream paths (search_dev, search_pipelined) and the exact search (its route depends on what stage 1 certifies: asserted in the test)
STREAM_ROUTES = {
    "dev": dict(seed=41, dtype="bf16", d=64, n=13_061, nq=3, k=20, opts={}, route=route_code(SMALL)),
    "pipe": dict(seed=42, dtype="bf16", d=64, n=13_061, nq=3, k=20, opts={}, route=route_code(CHAIN, 1)),
}
EXACT_ROUTES = {
    "exact": dict(seed=43, dtype="bf16", d=64, n=13_061, nq=2, k=10, opts={}, route=None),
}


# ---- tolerance: ERR is stated for unit-norm operands; Cauchy-Schwarz bounds sum |q_i x_i| by the norm product
def row_tol(q, X):
    """[n] tolerance of the scores of one query q against the rows X (both as the index holds them)"""
    qn = max(1.0, float(np.linalg.norm(np.asarray(q, np.float64))))
    return ERR * qn * np.maximum(1e-30, np.linalg.norm(np.asarray(X, np.float64), axis=1))


# ---- family P: one sign
def family_p(n, d, nq, seed=0):
    """rows and queries |g| / ||g||: every score > 0 (with -Q: every score < 0)"""
    rng = np.random.default_rng(7000 + seed)
    X = np.abs(rng.standard_normal((n, d), dtype=np.float32))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = np.abs(rng.standard_normal((nq, d), dtype=np.float32))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return X, Q


# ---- family Z: family P with -Q and three zero rows
def zero_rows(n):
    return [3, n // 2, n - 1]


def family_z(n, d, nq, seed=0):
    X, Q = family_p(n, d, nq, seed)
    X[zero_rows(n)] = 0.0
    return X, -Q


# ---- family T: all rows equal / two blocks
def family_t(n, d, nq, seed=0):
    rng = np.random.default_rng(7100 + seed)
    row = rng.standard_normal(d, dtype=np.float32)
    row /= np.linalg.norm(row)
    Q = rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return np.tile(row, (n, 1)), Q


def family_t2(n, d, nq, dtype, seed=0):
    """first 40 % of the rows equal a, the rest equal b; every query scores b higher (in the index dtype, by far more than rounding)"""
    rng = np.random.default_rng(7200 + seed)
    a = rng.standard_normal(d, dtype=np.float32); a /= np.linalg.norm(a)
    b = rng.standard_normal(d, dtype=np.float32); b /= np.linalg.norm(b)
    Q = b[None, :] + np.float32(0.3 / np.sqrt(d)) * rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    n_a = (2 * n) // 5
    X = np.concatenate([np.tile(a, (n_a, 1)), np.tile(b, (n - n_a, 1))])
    return X, Q, n_a


# ---- family S: power-of-two scaling of operands representable in the index dtype
SCALES = [(5, 3), (-4, 6)]


def family_s(n, d, nq, dtype, seed=0):
    rng = np.random.default_rng(7300 + seed)
    X = rng.standard_normal((n, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    X, Q = ROUND[dtype](X), ROUND[dtype](Q)
    if dtype == "f16":      # subnormals do not scale exactly: 2^-4 x would lose their low bits
        X[np.abs(X) < 2.0 ** -10] = 0.0      # (2^-14 after the scaling by 2^-4)
        Q[np.abs(Q) < 2.0 ** -14] = 0.0
    return X, Q


def scaled(A, e):
    return (A.astype(np.float64) * 2.0 ** e).astype(np.float32)


# ---- family N: mixed norms
def family_n(n, d, nq, seed=0):
    """rows: unit Gaussian directions times 10**U(-3, 1.5); queries of norm 1 (even) and 7 (odd)"""
    rng = np.random.default_rng(7400 + seed)
    X = rng.standard_normal((n, d), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X *= (10.0 ** rng.uniform(-3.0, 1.5, size=(n, 1))).astype(np.float32)
    Q = rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[1::2] *= 7.0
    return X, Q


def family_n_exact(n, d, seed=0):
    """family N for the exact search: query 0 (norm 1) is a plain one — its candidates separate; query 1 (norm 7) points at 5 000
    planted rows of norm ~30 whose scores lie inside its certificate's window, more than the 4 096 candidates of the second stage"""
    X, Q = family_n(n, d, 2, seed)
    rng = np.random.default_rng(7500 + seed)
    u = Q[1] / np.linalg.norm(Q[1])
    at = np.arange(2000, 7000)
    X[at] = 30.0 * (u[None, :] + 1e-4 * rng.standard_normal((len(at), d), dtype=np.float32))
    return X, Q


def exact_bound(q, dim, mx, mdx, dtype):
    """E_q of the exact search's certificate: ||dq|| M_x + ||q|| M_dx + 2 dim 2^-23 ||q~|| M_x"""
    q64 = q.astype(np.float64)
    qt = ROUND[dtype](q[None])[0].astype(np.float64)
    return np.linalg.norm(qt - q64) * mx + np.linalg.norm(q64) * mdx + 2 * dim * 2.0 ** -23 * np.linalg.norm(qt) * mx


def round_stats(X, dtype):
    Xr = ROUND[dtype](X).astype(np.float64)
    return float(np.linalg.norm(Xr, axis=1).max()), float(np.linalg.norm(Xr - X.astype(np.float64), axis=1).max())


def reference_certified(X, Q, k, dtype, kc):
    """per query: does a list of the kc best 16-bit scores certify the top-k (last candidate < k-th - 2 E_q)?  Returns (bool [nq],
    margin [nq] = (k-th - 2 E_q - kc-th) / E_q: far from 0 either way means the device's fp32 arithmetic cannot flip it)"""
    mx, mdx = round_stats(X, dtype)
    S = orc.exact_scores_f64(ROUND[dtype](X), ROUND[dtype](Q))
    out, margin = [], []
    for i in range(len(Q)):
        s = np.sort(S[i])[::-1]
        e = exact_bound(Q[i], X.shape[1], mx, mdx, dtype)
        out.append(bool(s[kc - 1] < s[k - 1] - 2 * e))
        margin.append((s[k - 1] - 2 * e - s[kc - 1]) / max(e, 1e-300))
    return np.array(out), np.array(margin)


# ---- family O: out of range for the index dtype
OVERFLOW = {"f16": 70000.0, "bf16": 3.4e38}


def family_o_subnormal(n, d, seed=0):
    """rows whose components all lie in (2^-24, 2^-14): f16 subnormals; queries of unit norm"""
    rng = np.random.default_rng(7600 + seed)
    X = (rng.uniform(2.0 ** -23, 2.0 ** -14.5, size=(n, d)) * rng.choice([-1.0, 1.0], size=(n, d))).astype(np.float32)
    Q = rng.standard_normal((3, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return X, Q
