"""Every search route on un-normalised, one-signed, tied and out-of-range inputs (the other GPU files draw unit-norm, two-signed
Gaussian data, where a zero from a padded slot is never a minimum, a maximum or a result).  Inputs and the route table come from
tests/value_domain_inputs.py; tests/test_value_domain_inputs.py checks on the CPU what the assertions here rely on.  Every
route-tagged call is confirmed by the read-only option "last_route"."""
import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc
from tests import value_domain_inputs as vd

pytestmark = pytest.mark.gpu

ROUND = vd.ROUND
ROUTES = {tag: dict(spec, kind="search") for tag, spec in vd.SEARCH_ROUTES.items()}
ROUTES.update({tag: dict(spec, kind="min-score") for tag, spec in vd.MIN_SCORE_ROUTES.items()})
ROUTES.update({tag: dict(spec, kind=tag) for tag, spec in vd.STREAM_ROUTES.items()})
ROUTES.update({tag: dict(spec, kind="exact") for tag, spec in vd.EXACT_ROUTES.items()})
TAGS = list(ROUTES)


def _index(spec, X, **kw):
    from comorag_amd.index import DenseIndex
    if "max_cu" in spec:
        n_cu = L.device_info(0)["n_cu"]
        if (spec["n"] + 31) // 32 < 16 * n_cu:      # plan_pass: the finishing stage needs npanels >= n_cu * 2 * 8
            pytest.skip(f"{n_cu} CUs: {spec['n']} rows are too few panels for the finishing stage on this device")
    idx = DenseIndex(spec["d"], spec["dtype"], options=spec["opts"], keep_f32=spec["kind"] == "exact", **kw)
    if len(X):
        idx.append(X)
    return idx


def _assert_route(idx, spec, ex=None):
    r = idx.get_option("last_route")
    if spec["kind"] == "exact":      # stage 1 asks the chain for 128 candidates; queries it leaves uncertified run again through the large-k search
        assert r & 0xFF in (vd.route_code(vd.CHAIN, 1), vd.route_code(vd.LARGE_K)), hex(r)
        if ex is not None and not ex.all():
            assert r & 0xFF == vd.route_code(vd.LARGE_K), hex(r)
        return
    assert r & 0xFF == spec["route"], f"last_route {r:#x}, expected low byte {spec['route']:#x}"
    if "nqt" in spec:
        assert (r >> 8) & 3 == spec["nqt"], hex(r)
    assert bool(r >> 10 & 1) == (spec["kind"] == "min-score"), hex(r)
    assert not r & vd.MORE_PASSES, f"last_route {r:#x}: the batch was cut into several passes, the route confirmed is only its first"


def _run(idx, spec, Q, k=None, min_score=-1e30):
    """the route's call: (ids, scores, min | None, max | None, exact flags | None), route asserted"""
    k = spec["k"] if k is None else k
    kind = spec["kind"]
    mn = mx = ex = None
    if kind == "search":
        ids, sc, mn, mx = idx.search(Q, k)
    elif kind == "min-score":
        ids, sc = idx.search_min_score(Q, k, min_score)
    elif kind == "exact":
        ids, sc, ex = idx.search_exact(Q, k)
    else:
        import torch
        dev = torch.device("cuda", 0)
        qt = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(dev)
        oi = torch.empty((len(Q), k), dtype=torch.int64, device=dev); os_ = torch.empty((len(Q), k), dtype=torch.float32, device=dev)
        tmn = torch.empty(len(Q), dtype=torch.float32, device=dev); tmx = torch.empty(len(Q), dtype=torch.float32, device=dev)
        if kind == "dev":
            idx.search_dev(qt, k, oi, os_, tmn, tmx)
            torch.cuda.synchronize()
        else:
            idx.sync(idx.search_pipelined(qt, k, oi, os_, tmn, tmx))
        assert idx.query_status() is False
        ids, sc, mn, mx = oi.cpu().numpy(), os_.cpu().numpy(), tmn.cpu().numpy(), tmx.cpu().numpy()
    _assert_route(idx, spec, ex)
    return ids, sc, mn, mx, ex


def _check_minmax(mn, mx, exact, tol):
    """min / max of the device's scores, each within tol[row] of exact[row]: bounded by the rows' own tolerances"""
    for i in range(len(exact)):
        assert (exact[i] - tol[i]).min() <= mn[i] <= exact[i].min() + tol[i][np.argmin(exact[i])], (i, mn[i], exact[i].min())
        assert exact[i].max() - tol[i][np.argmax(exact[i])] <= mx[i] <= (exact[i] + tol[i]).max(), (i, mx[i], exact[i].max())


def _check(spec, X, Q, out, k=None, exact=None, X_tol=None):
    """oracle equivalence under the per-row tolerance ERR * max(1, ||q||) * ||x||; returns the fp64 scores"""
    k = spec["k"] if k is None else k
    ids, sc, mn, mx, ex = out
    rnd = ROUND[spec["dtype"]]
    Xr, Qr = rnd(X), rnd(Q)
    if exact is None:
        exact = orc.exact_scores_f64(Xr, Qr)
    ref_ids, _ = orc.topk_rule(exact, k)
    assert ids.shape == ref_ids.shape and sc.shape == ref_ids.shape
    tol = np.stack([vd.row_tol(Qr[i], Xr if X_tol is None else X_tol) for i in range(len(Q))])
    for i in range(len(Q)):
        if ex is not None and not ex[i]:
            continue
        assert ids[i].min() >= 0 and ids[i].max() < len(X), (i, ids[i].min(), ids[i].max())
        both = np.union1d(ids[i], ref_ids[i])
        orc.assert_topk_equivalent(ids[i], ref_ids[i], exact[i], tol[i][both].max())
        assert np.all(np.abs(sc[i] - exact[i][ids[i]]) <= tol[i][ids[i]]), (i, np.abs(sc[i] - exact[i][ids[i]]).max())
        assert np.all(np.diff(sc[i]) <= 0), "scores not descending"
    if mn is not None:
        _check_minmax(mn, mx, exact, tol)
    return exact


def _raw_search(idx, Q, k):
    """cmr_index_search with the padded tail left in (DenseIndex.search cuts it off)"""
    Q = np.ascontiguousarray(Q, np.float32)
    ids = np.full((len(Q), k), -7, np.int64); sc = np.full((len(Q), k), 7.0, np.float32)
    L.check(L.lib().cmr_index_search(idx._h, Q.ctypes.data, len(Q), k, ids.ctypes.data, sc.ctypes.data, None, None))
    return ids, sc


# ---------------------------------------------------------------------------------------------- P: one sign
@pytest.mark.parametrize("tag", TAGS)
def test_one_signed_scores(tag):
    """every score > 0 (then, with -Q, < 0): a padded slot's 0.0 would be the minimum (the maximum, and in the top-k)"""
    spec = ROUTES[tag]
    X, Q = vd.family_p(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    exact = None
    for sign in (1.0, -1.0):
        out = _run(idx, spec, sign * Q)
        ids, sc, mn, mx, ex = out
        if spec["kind"] == "exact":      # fp32 re-scores of the un-rounded rows; ids promised only where certified
            e32 = orc.exact_scores_f64(X, sign * Q)
            _check(dict(spec, dtype="f32"), X, sign * Q, out, exact=e32)
        else:
            exact = _check(spec, X, sign * Q, out, exact=None if exact is None else -exact)
        assert ids.min() >= 0 and ids.max() < spec["n"]
        assert not np.any(sc == 0.0) and np.all(np.sign(sc) == sign)
        if mn is not None:
            assert np.all(mn > 0) and np.all(mx > 0) if sign > 0 else np.all(mn < 0) and np.all(mx < 0), (mn, mx)
    idx.close()


def test_one_signed_k_above_n():
    spec = ROUTES["tiny1"]
    n, k = 37, 64
    X, Q = vd.family_p(n, spec["d"], spec["nq"], seed=1)
    idx = _index(spec, X)
    for sign in (1.0, -1.0):
        ids, sc = _raw_search(idx, sign * Q, k)
        _assert_route(idx, spec)
        assert np.all(ids[:, n:] == -1) and np.all(np.isneginf(sc[:, n:]))
        assert all(sorted(r.tolist()) == list(range(n)) for r in ids[:, :n]) and not np.any(sc[:, :n] == 0.0)
        _check(spec, X, sign * Q, (ids[:, :n], sc[:, :n], None, None, None), k=k)
    idx.close()


@pytest.mark.parametrize("tag", list(vd.SCORES_ROUTES))
def test_one_signed_all_scores(tag):
    spec = dict(vd.SCORES_ROUTES[tag], kind="scores")
    X, Q = vd.family_p(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    rnd = ROUND[spec["dtype"]]
    exact = orc.exact_scores_f64(rnd(X), rnd(Q))
    tol = np.stack([vd.row_tol(q, rnd(X)) for q in rnd(Q)])
    for sign in (1.0, -1.0):
        s = idx.scores(sign * Q)
        assert idx.get_option("last_route") & 0xFF == spec["route"], hex(idx.get_option("last_route"))
        assert s.shape == exact.shape and np.all(np.abs(s - sign * exact) <= tol) and np.all(np.sign(s) == sign)
        ids, sc, mn, mx = idx.sorted_scores(sign * Q)
        assert idx.get_option("last_route") & 0xFF == vd.route_code(vd.SORTED)
        assert all(np.array_equal(np.sort(r), np.arange(spec["n"])) for r in ids)
        assert np.array_equal(sc, np.take_along_axis(s, ids, 1)) and np.all(np.diff(sc, axis=1) <= 0)
        ties = np.diff(sc, axis=1) == 0
        assert np.all(np.diff(ids, axis=1)[ties] > 0), "equal scores not in ascending row order"
        assert np.array_equal(mn, s.min(1)) and np.array_equal(mx, s.max(1))
    idx.close()


# ---------------------------------------------------------------------------------------------- Z: zero rows, zero query
@pytest.mark.parametrize("tag", TAGS)
def test_zero_rows_lead_negative_scores(tag):
    spec = ROUTES[tag]
    n = spec["n"]
    X, Q = vd.family_z(n, spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    out = _run(idx, spec, Q)
    ids, sc, mn, mx, ex = out
    assert np.all(ids[:, :3] == np.array(vd.zero_rows(n))), ids[:, :3]
    assert np.all(sc[:, :3].view(np.uint32) == 0), "the zero rows' scores must be +0.0, bit for bit"
    assert np.all(sc[:, 3:] < 0)
    if spec["kind"] == "exact":
        _check(dict(spec, dtype="f32"), X, Q, out)
    else:
        _check(spec, X, Q, out)
    if mx is not None:
        assert np.all(mx.view(np.uint32) == 0) and np.all(mn < 0)
    # the zero query: every score is 0 — ids 0..k-1, min == max == 0
    k = spec["k"]
    ids, sc, mn, mx, ex = _run(idx, spec, np.zeros_like(Q))
    assert np.all(ids == np.arange(k)) and np.all(sc.view(np.uint32) == 0)
    if mn is not None:
        assert np.all(mn == 0) and np.all(mx == 0)
    idx.close()


@pytest.mark.parametrize("tag", list(vd.MIN_SCORE_ROUTES))
def test_min_score_at_and_below_zero(tag):
    spec = ROUTES[tag]
    n, k = spec["n"], spec["k"]
    X, Q = vd.family_z(n, spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    for bound in (0.0, -0.0):
        ids, sc, _, _, _ = _run(idx, spec, Q, min_score=bound)
        assert np.all(ids[:, :3] == np.array(vd.zero_rows(n))) and np.all(sc[:, :3].view(np.uint32) == 0)
        assert np.all(ids[:, 3:] == -1) and np.all(np.isneginf(sc[:, 3:]))
    rnd = ROUND[spec["dtype"]]
    exact = orc.exact_scores_f64(rnd(X), rnd(Q))
    tol = np.stack([vd.row_tol(q, rnd(X)) for q in rnd(Q)])
    # -0.5 (the row's "below" at 768-d): far more than k rows pass; and a bound between the 8th and 9th best score of query 0: a list that does not fill
    few = float(np.float32(np.sort(exact[0])[::-1][7:9].mean()))
    branches = set()
    for bound in (spec.get("below", vd.MIN_SCORE_BELOW), few):
        ids, sc, _, _, _ = _run(idx, spec, Q, min_score=bound)
        for i in range(len(Q)):
            may = np.flatnonzero(exact[i] >= bound - tol[i])
            order = may[np.lexsort((may, -exact[i][may]))]
            sure = order[exact[i][order] >= bound + tol[i][order]]      # rows within rounding of the bound may go either way
            got = ids[i][ids[i] >= 0]
            if len(sure) >= k:      # more rows pass than fit: the k best of them
                orc.assert_topk_equivalent(ids[i], order[:k], exact[i], tol[i][np.union1d(ids[i], order[:k])].max())
                branches.add("full")
            else:
                assert set(sure.tolist()) <= set(got.tolist()) <= set(order.tolist())
                assert np.all(ids[i][len(got):] == -1) and np.all(np.isneginf(sc[i][len(got):]))
                branches.add("short")
            assert np.all(np.abs(sc[i][:len(got)] - exact[i][got]) <= tol[i][got]) and np.all(np.diff(sc[i][:len(got)]) <= 0)
    assert branches == {"full", "short"}
    idx.close()


# ---------------------------------------------------------------------------------------------- T: ties
T_KS = {"tiny1": [1, 20, 32, 33, 100], "tiny1-1wg": [1, 20, 32, 33, 100], "small": [1, 20, 32, 33], "chain0": [1, 20, 32, 33, 100],
        "chain1": [1, 20, 32, 33, 100], "chain2": [1, 20, 32, 33, 100], "single": [1, 20, 32], "tau-in-scan": [1, 20, 32], "fin1": [1, 20, 32, 33],
        "fin8": [1, 20, 32, 33], "two-tile": [1, 20, 32, 33, 100], "wide": [1, 20, 32, 33, 100], "quad": [1, 20, 32, 33, 100],
        "quad-f32": [1, 20, 32, 33, 100], "large-k": [500], "min-score-5003": [1, 20, 32, 33, 100], "min-score-big": [1, 20, 32, 33, 100],
        "min-score-wide": [1, 20, 32, 33, 100], "min-score-quad": [1, 20, 32, 33, 100],
        "dev": [1, 20, 32, 33], "pipe": [1, 20, 32, 33, 100], "exact": [1, 10, 32, 33]}


@pytest.mark.parametrize("tag", TAGS)
def test_all_rows_equal(tag):
    """every score ties with every threshold: the result is rows 0..k-1, whatever the sample, the filter or the merge"""
    spec = ROUTES[tag]
    X, Q = vd.family_t(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    for k in T_KS[tag]:
        ids, sc, mn, mx, ex = _run(idx, spec, Q, k=k)
        assert np.all(ids == np.arange(k)), (k, ids[0][:8])
        assert np.all(sc == sc[:, :1])
        if mn is not None:
            assert np.array_equal(mn, mx) and np.array_equal(mn, sc[:, 0])
    idx.close()


@pytest.mark.parametrize("tag", TAGS)
def test_two_blocks_of_equal_rows(tag):
    spec = ROUTES[tag]
    X, Q, n_a = vd.family_t2(spec["n"], spec["d"], spec["nq"], spec["dtype"], seed=spec["seed"])
    idx = _index(spec, X)
    for k in T_KS[tag]:
        ids, sc, mn, mx, ex = _run(idx, spec, Q, k=k)
        assert np.all(ids == n_a + np.arange(k)), (k, ids[0][:8])
        assert np.all(sc == sc[:, :1])
        if mn is not None:
            assert np.array_equal(mx, sc[:, 0]) and np.all(mn < mx)
    idx.close()


@pytest.mark.parametrize("tag", list(vd.SCORES_ROUTES))
def test_all_rows_equal_all_scores(tag):
    spec = dict(vd.SCORES_ROUTES[tag], kind="scores")
    X, Q = vd.family_t(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    s = idx.scores(Q)
    assert idx.get_option("last_route") & 0xFF == spec["route"]
    assert np.all(s == s[:, :1])
    ids, sc, mn, mx = idx.sorted_scores(Q)
    assert idx.get_option("last_route") & 0xFF == vd.route_code(vd.SORTED)
    assert np.all(ids == np.arange(spec["n"])) and np.array_equal(sc, s) and np.array_equal(mn, mx) and np.array_equal(mn, s[:, 0])
    idx.close()


# ---------------------------------------------------------------------------------------------- S: power-of-two scaling
@pytest.mark.parametrize("tag", TAGS)
def test_power_of_two_scaling_is_exact(tag):
    spec = ROUTES[tag]
    rnd = ROUND[spec["dtype"]]
    X0, Q0 = vd.family_s(spec["n"], spec["d"], spec["nq"], spec["dtype"], seed=spec["seed"])
    idx = _index(spec, X0)
    base = _run(idx, spec, Q0)
    idx.close()
    for a, b in vd.SCALES:
        Xs, Qs = vd.scaled(X0, a), vd.scaled(Q0, b)
        assert np.array_equal(rnd(Xs), Xs) and np.array_equal(rnd(Qs), Qs) and np.abs(Xs).max() < 65504 and np.abs(Qs).max() < 65504
        idx = _index(spec, Xs)
        got = _run(idx, spec, Qs)
        idx.close()
        f = np.float32(2.0 ** (a + b))
        assert np.array_equal(got[0], base[0])
        assert np.array_equal(got[1], base[1] * f)
        if base[2] is not None:
            assert np.array_equal(got[2], base[2] * f) and np.array_equal(got[3], base[3] * f)
        if base[4] is not None:
            assert np.array_equal(got[4], base[4])


@pytest.mark.parametrize("tag", list(vd.SCORES_ROUTES))
def test_power_of_two_scaling_is_exact_all_scores(tag):
    spec = dict(vd.SCORES_ROUTES[tag], kind="scores")
    X0, Q0 = vd.family_s(spec["n"], spec["d"], spec["nq"], spec["dtype"], seed=spec["seed"])
    outs = []
    for a, b in [(0, 0)] + vd.SCALES:
        idx = _index(spec, vd.scaled(X0, a))
        s = idx.scores(vd.scaled(Q0, b))
        assert idx.get_option("last_route") & 0xFF == spec["route"]
        ids, sc, mn, mx = idx.sorted_scores(vd.scaled(Q0, b))
        assert idx.get_option("last_route") & 0xFF == vd.route_code(vd.SORTED)
        idx.close()
        f = np.float32(2.0 ** (a + b))
        outs.append((s, ids, sc, mn, mx))
        assert np.array_equal(s, outs[0][0] * f) and np.array_equal(ids, outs[0][1])
        assert all(np.array_equal(x, y * f) for x, y in zip((sc, mn, mx), outs[0][2:]))


# ---------------------------------------------------------------------------------------------- N: mixed norms
@pytest.mark.parametrize("tag", ["chain1", "fin8", "wide", "large-k"])
def test_mixed_norms(tag):
    """row norms from 1e-3 to 30 in one index, queries of norm 1 and 7: the tolerance is ERR times the norm product"""
    spec = ROUTES[tag]
    X, Q = vd.family_n(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    _check(spec, X, Q, _run(idx, spec, Q))
    idx.close()


def test_mixed_norms_sorted():
    spec = dict(vd.SCORES_ROUTES["scores-13061-general"], kind="scores")
    X, Q = vd.family_n(spec["n"], spec["d"], spec["nq"], seed=3)
    idx = _index(spec, X)
    ids, sc, mn, mx = idx.sorted_scores(Q)
    assert idx.get_option("last_route") & 0xFF == vd.route_code(vd.SORTED)
    idx.close()
    _check(spec, X, Q, (ids, sc, mn, mx, None), k=spec["n"])


def test_mixed_norms_exact():
    """the certificate's index-wide maxima at M_x ~ 30: query 0 is certified, query 1 (5 000 rows inside its window) is not — and
    says so; certified ids are the fp64 ranking of the un-rounded rows, re-scored values the fp32 shadow's"""
    spec = ROUTES["exact"]
    k = spec["k"]
    X, Q = vd.family_n_exact(spec["n"], spec["d"])
    idx = _index(spec, X)
    mx_, mdx_ = idx.round_stats()
    rmx, rmdx = vd.round_stats(X, spec["dtype"])
    assert rmx <= mx_ <= rmx * (1 + 1e-6) and rmdx <= mdx_ <= rmdx * (1 + 1e-6) + 1e-30
    out = _run(idx, spec, Q)
    ids, sc, _, _, ex = out
    assert ex.tolist() == [True, False], ex
    assert idx.get_option("last_route") & 0xFF == vd.route_code(vd.LARGE_K)
    e32 = orc.exact_scores_f64(X, Q)
    _check(dict(spec, dtype="f32"), X, Q, out, exact=e32)      # (skips the uncertified query's ids)
    tol1 = vd.row_tol(Q[1], X)
    assert np.all(np.abs(sc[1] - e32[1][ids[1]]) <= tol1[ids[1]]) and np.all(np.diff(sc[1]) <= 0) and len(set(ids[1].tolist())) == k
    idx.close()


# ---------------------------------------------------------------------------------------------- R: a rejected append leaves nothing behind
def _snapshot(idx, Q, tags):
    out = []
    for tag in tags:
        spec = ROUTES[tag]
        for name, v in spec["opts"].items():
            idx.set_option(name, v)
        for sign in (1.0, -1.0):
            out.extend(idx.search(sign * Q, 20))
            _assert_route(idx, spec)
        for name in spec["opts"]:
            idx.set_option(name, 0)
    for sign in (1.0, -1.0):
        out.append(idx.scores(sign * Q))
        out.extend(idx.sorted_scores(sign * Q))
    return out


@pytest.mark.parametrize("n,more,tags", [(1000, 23, ("tiny1", "chain0")), (13_061, 23, ("small", "chain1"))])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_rejected_append_leaves_nothing_behind(n, more, tags, dtype):
    from comorag_amd.index import DenseIndex
    d = 64
    X, Q = vd.family_p(n + more, d, 3, seed=n)
    bad = np.full((37, d), 1e3, np.float32); bad[17, 5] = np.nan
    idx = DenseIndex(d, dtype); idx.append(X[:n])
    stats = idx.round_stats()
    with pytest.raises(L.CmrError) as e:
        idx.append(bad)
    assert e.value.code == L.CMR_ERR_NONFINITE and len(idx) == n and idx.round_stats() == stats
    fresh = DenseIndex(d, dtype); fresh.append(X[:n])
    for a, b in zip(_snapshot(idx, Q, tags), _snapshot(fresh, Q, tags)):
        assert np.array_equal(a, b)
    idx.append(X[n:]); fresh.close()
    fresh = DenseIndex(d, dtype); fresh.append(X)
    assert len(idx) == n + more
    for a, b in zip(_snapshot(idx, Q, tags), _snapshot(fresh, Q, tags)):
        assert np.array_equal(a, b)
    idx.close(); fresh.close()


# ---------------------------------------------------------------------------------------------- O: out of range for the index dtype
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_row_that_overflows_the_index_dtype_is_refused(dtype):
    from comorag_amd.index import DenseIndex
    d, n = 64, 1000
    X, Q = vd.family_p(n, d, 3, seed=5)
    big = X[:5].copy(); big[2, 7] = vd.OVERFLOW[dtype]
    with np.errstate(over="ignore"):
        assert np.isfinite(big).all() and not np.isfinite(ROUND[dtype](big)).all()
    idx = DenseIndex(d, dtype); idx.append(X)
    want = idx.search(Q, 20)
    for rows in (big, -big):
        with pytest.raises(L.CmrError) as e:
            idx.append(rows)
        assert e.value.code == L.CMR_ERR_NONFINITE and len(idx) == n
    got = idx.search(Q, 20)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.all(np.isfinite(idx.scores(Q)))
    idx.close()
    # an fp32 index takes the same rows
    f = DenseIndex(d, "f32"); f.append(X); f.append(big)
    spec = dict(ROUTES["tiny1"], dtype="f32", d=d)
    Xb = np.concatenate([X, big])
    ids, sc, mn, mx = f.search(Q, 20)
    _check(spec, Xb, Q, (ids, sc, mn, mx, None), k=20)
    assert np.all(ids[:, 0] == n + 2)
    f.close()


def test_f16_largest_finite_value_is_accepted():
    from comorag_amd.index import DenseIndex
    d, n = 64, 1000
    X, Q = vd.family_p(n, d, 3, seed=6)
    X[11, 3] = 65504.0; X[12, 3] = -65504.0
    Q[1, 9] = 65504.0
    idx = DenseIndex(d, "f16"); idx.append(X)
    assert len(idx) == n
    out = idx.search(Q, 20)
    _check(dict(ROUTES["tiny1"], dtype="f16", d=d), X, Q, out + (None,), k=20)
    assert np.all(out[0][[0, 2], 0] == 11)      # (query 1 has a 65504 of its own at another component)
    idx.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("tag", ["tiny1", "small", "chain1"])
def test_query_that_overflows_the_index_dtype_is_refused(dtype, tag):
    import torch
    spec = dict(ROUTES[tag], dtype=dtype)
    X, Q = vd.family_p(spec["n"], spec["d"], spec["nq"], seed=8)
    idx = _index(spec, X)
    want = _run(idx, spec, Q)
    bad = Q.copy(); bad[-1, 2] = -vd.OVERFLOW[dtype]
    for call in (lambda: idx.search(bad, 20), lambda: idx.scores(bad), lambda: idx.sorted_scores(bad), lambda: idx.search_min_score(bad, 20, 0.1)):
        with pytest.raises(L.CmrError) as e:
            call()
        assert e.value.code == L.CMR_ERR_NONFINITE
    got = _run(idx, spec, Q)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
    # the stream API cannot raise: query_status() tells afterwards
    idx.search_dev(torch.from_numpy(bad).cuda(), 20); torch.cuda.synchronize()
    assert idx.query_status() is True and idx.query_status() is False
    # a combined call fails exactly like a solo one (the host pre-check keeps such a query out of a batch)
    idx.set_option("combine", 4)
    with pytest.raises(L.CmrError) as e:
        idx.search(bad[-1:], 20)
    assert e.value.code == L.CMR_ERR_NONFINITE
    with pytest.raises(L.CmrError) as e:
        idx.scores(bad[-1:])
    assert e.value.code == L.CMR_ERR_NONFINITE
    got = idx.search(Q, 20)
    assert all(np.array_equal(a, b) for a, b in zip(got, want[:4]))
    idx.close()
    # an fp32 index takes the query
    fspec = dict(spec, dtype="f32")
    f = _index(fspec, X)
    out = _run(f, fspec, bad)
    assert np.all(np.isfinite(out[1])) and out[0].min() >= 0 and out[0].max() < spec["n"]
    if dtype == "f16":      # (3.4e38 times a unit row is no score an fp32 accumulator bounds by ERR: the f16 limit is the fp32 case)
        _check(fspec, X, bad, out)
    f.close()


def _threads(fns, timeout=120.0):
    """every fn on a thread of its own, released by one barrier -> [result or exception]"""
    import threading
    out = [None] * len(fns)
    bar = threading.Barrier(len(fns))

    def work(i):
        try:
            bar.wait()
            out[i] = fns[i]()
        except Exception as e:          # noqa: BLE001
            out[i] = e
    ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
        assert not t.is_alive(), "deadlock: a combined call did not return"
    return out


@pytest.mark.parametrize("dtype,value,accepted", [("f16", 70000.0, False), ("f16", -65520.0, False), ("f16", 65519.996, True),
                                                  ("bf16", 3.4e38, False), ("bf16", -3.3961775e38, False), ("bf16", 3.3961772e38, True),
                                                  ("f32", 3.4e38, True)])
@pytest.mark.parametrize("call", ["search", "scores"])
def test_overflowing_query_fails_alone_in_a_combined_batch(dtype, value, accepted, call):
    """sixteen concurrent callers under a long gather window, one of them with a component at the edge of the index dtype.  The host
    pre-check (combine.h all_finite) must judge it as the packing kernel does: a refused query stays out of the batch and fails
    alone, the other fifteen are batched and get their solo bits; an accepted one (the largest fp32 below the rounding midpoint
    — 65520 for f16, 2^127 (2 - 2^-8) for bf16 — rounds to the largest finite value) joins the batch of sixteen."""
    from comorag_amd.index import DenseIndex
    d, n = 64, 5003
    X, Q = vd.family_p(n, d, 16, seed=9)
    Q[6, 17] = value
    if accepted and dtype != "f32":
        with np.errstate(over="ignore"):
            assert np.isfinite(ROUND[dtype](Q[6:7])).all() and np.float32(value) == Q[6, 17]
    idx = DenseIndex(d, dtype); idx.append(X)
    fn = (lambda i: idx.search(Q[i], 20)) if call == "search" else (lambda i: (idx.scores(Q[i]),))
    solo = []
    for i in range(16):
        if i == 6 and not accepted:
            with pytest.raises(L.CmrError) as e:
                fn(i)
            assert e.value.code == L.CMR_ERR_NONFINITE
            solo.append(None)
        else:
            solo.append(fn(i))
    width = 16 if accepted else 15
    idx.set_option("combine", width)      # the batch fills exactly: nobody waits the window out
    idx.set_option("combine_wait_us", 500_000)
    before = idx.combine_stats()
    got = _threads([lambda i=i: fn(i) for i in range(16)])
    for i in range(16):
        if solo[i] is None:
            assert isinstance(got[i], L.CmrError) and got[i].code == L.CMR_ERR_NONFINITE, repr(got[i])
        else:
            assert not isinstance(got[i], Exception), (i, repr(got[i]))
            assert all(np.array_equal(g, w) for g, w in zip(got[i], solo[i])), i
    now = idx.combine_stats()
    assert (now["batches"] - before["batches"], now["queries"] - before["queries"], now["max_width"]) == (1, width, width)
    idx.close()


def test_f16_subnormal_operands():
    """rows whose components are all f16 subnormals, on both all-scores routes.  Observed on gfx950: the matrix instruction keeps them
    (max |score - fp64 of the f16-rounded operands| = 6.7e-12 at scores of ~8e-5, tolerance 9.4e-10), so the reference
    is the plain oracle on f16_round inputs — a flush to zero would miss it by the whole score."""
    from comorag_amd.index import DenseIndex
    d, n = 64, 1000
    X, Q = vd.family_o_subnormal(n, d)
    Xr, Qr = orc.f16_round(X), orc.f16_round(Q)
    assert np.all((np.abs(Xr) > 0) & (np.abs(Xr) < 2.0 ** -14))
    keep = orc.exact_scores_f64(Xr, Qr)
    tol = np.stack([vd.row_tol(q, Xr) for q in Qr])
    assert np.abs(keep).max() > 100 * tol.max(), "scores too small to tell a flush from rounding"
    for opts, route in (({}, vd.SCORES_SINGLE), ({"scan_no_small": 1}, vd.SCORES)):
        idx = DenseIndex(d, "f16", options=opts); idx.append(X)
        s = idx.scores(Q)
        assert idx.get_option("last_route") & 0xFF == route
        idx.close()
        assert np.all(np.abs(s - keep) <= tol), "the matrix instruction does not keep f16 subnormal operands"
