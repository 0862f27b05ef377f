"""numpy statement of the certified int8 pre-filter: the row and query quantisers, the int8 score as the device evaluates
it and the bound on its distance from the scan's score.  tests/test_prefilter_model.py holds the bound against the input families
without a device; tests/test_prefilter_gpu.py recomputes the companion's statistics with it."""
import numpy as np

from tests import value_domain_inputs as vd

F32 = np.float32


def up32(d):
    """float64 >= 0 -> the smallest float32 that is not below it"""
    d = np.asarray(d, np.float64)
    f = d.astype(F32)
    return np.where(f.astype(np.float64) < d, np.nextafter(f, F32(np.inf)), f).astype(F32)


def quantise_rows(Xt):
    """stored rows (fp32 values of the index dtype) -> (a [n] fp32, m [n, d] int, b [n] fp32 >= ||x - a m||, ||x|| [n] fp32 rounded up)"""
    Xt = np.asarray(Xt, F32)
    a = (np.abs(Xt).max(axis=1) / F32(127.0)).astype(F32)
    safe = np.where(a > 0, a, F32(1.0))
    m = np.clip(np.rint((Xt / safe[:, None]).astype(F32)), -127, 127).astype(np.int64)
    m[a == 0] = 0
    e = Xt.astype(np.float64) - a.astype(np.float64)[:, None] * m
    return a, m, up32(np.sqrt((e * e).sum(axis=1))), up32(np.sqrt((Xt.astype(np.float64) ** 2).sum(axis=1)))


def quantise_query(qt, Mx, dpad):
    """packed query (fp32 values of the index dtype) -> (a_q, n_hi, n_lo, B_q, c_q)"""
    qt = np.asarray(qt, F32)
    a = F32(np.abs(qt).max() / F32(127.0))
    if a > 0:
        u = (qt / a).astype(F32)
        hi = np.clip(np.rint(u), -127, 127)
        lo = np.clip(np.rint(((u - hi.astype(F32)).astype(F32) * F32(254.0)).astype(F32)), -127, 127)
    else:
        hi = np.zeros_like(qt); lo = np.zeros_like(qt)
    hi, lo = hi.astype(np.int64), lo.astype(np.int64)
    Qh = float(a) * (hi + lo / 254.0)
    f = qt.astype(np.float64) - Qh
    nQ, nf, nq = np.linalg.norm(Qh), np.linalg.norm(f), np.linalg.norm(qt.astype(np.float64))
    gamma = dpad * 2.0 ** -23
    c = (nf + gamma * nq + nQ * 2.0 ** -20) * float(Mx) * (1.0 + 1e-5) + 1e-7
    return a, hi, lo, up32(nQ * (1.0 + 1e-5)), up32(c)


def int8_scores(a_r, m, a_q, hi, lo):
    """[n] the int8 score of every row in the device's fp32 arithmetic: a_r a_q (I_hi + I_lo / 254)"""
    I_hi, I_lo = m @ hi, m @ lo
    t = (I_lo.astype(F32) * F32(1.0 / 254.0) + I_hi.astype(F32)).astype(F32)
    return ((a_r * F32(a_q)).astype(F32) * t).astype(F32)


def upper_bounds(s_hat, b_r, B_q, c_q):
    """[n] what the filter compares with the threshold, in fp32 as the kernel does: s^ + (B_q b_r + c_q)"""
    return (s_hat + (F32(B_q) * b_r + F32(c_q)).astype(F32)).astype(F32)


def spike_family(n, d, nq, seed=0):
    """rows: one large element, the rest below a_r / 2 (they quantise to 0: the whole rest IS the error); queries orthogonal to the
    spike and aligned with the rest of row i"""
    rng = np.random.default_rng(7700 + seed)
    X = (rng.uniform(-0.9, 0.9, size=(n, d)) / 254.0).astype(F32)
    at = rng.integers(0, d, size=n)
    X[np.arange(n), at] = 1.0
    Q = X[:nq].copy()
    Q[np.arange(nq), at[:nq]] = 0.0
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return X, Q


FAMILIES = ("gauss", "one-signed", "equal", "zeros", "norms", "spike")


def family(name, n, d, nq, seed=0):
    """(X, Q) fp32, before rounding to the index dtype"""
    if name == "gauss":
        rng = np.random.default_rng(7800 + seed)
        X = rng.standard_normal((n, d), dtype=F32); X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rng.standard_normal((nq, d), dtype=F32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        return X, Q
    if name == "zeros":      # one-signed rows with three zero rows, negated queries, one of them zero
        X, Q = vd.family_z(n, d, nq, seed)
        Q = Q.copy(); Q[nq // 2] = 0.0
        return X, Q
    return {"one-signed": vd.family_p, "equal": vd.family_t, "norms": vd.family_n, "spike": spike_family}[name](n, d, nq, seed)
