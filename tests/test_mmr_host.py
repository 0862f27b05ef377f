"""Diversified top-k (cmr_mmr_select, cmr_index_pair_scores, cmr_index_mmr_select*, cmr_index_search_mmr*, cmr_mindex_*; DESIGN.md
§4.20), host side: the symbols are bound and declared, the argument rules answer before the handle is looked at (so they hold on a
host without a device), and the host selection cmr_mmr_select equals the numpy model tests/mmr_model.py bit for bit — on the clustered
near-duplicate inputs of the GPU tests and on hand-made edge cases.  The model itself is held against a hand-computed example."""
import ctypes as C
import os

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc
from tests import mmr_model as mm

NEW = ("cmr_mmr_select", "cmr_index_pair_scores", "cmr_index_mmr_select", "cmr_index_mmr_select_dev", "cmr_index_search_mmr",
       "cmr_index_search_mmr_dev", "cmr_mindex_pair_scores", "cmr_mindex_mmr_select", "cmr_mindex_search_mmr")
NAN, INF = float("nan"), np.float32(np.inf)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _err():
    return L.lib().cmr_last_error().decode()


def host_select(rel, G, ids, k, lam):
    rel = np.ascontiguousarray(np.atleast_2d(rel), np.float32)
    ids = np.ascontiguousarray(np.atleast_2d(ids), np.int64)
    G = np.ascontiguousarray(G, np.float32).reshape(ids.shape + (ids.shape[1],))
    out_i = np.empty((len(ids), k), np.int64)
    out_s = np.empty((len(ids), k), np.float32)
    L.check(L.lib().cmr_mmr_select(_p(rel), _p(G), _p(ids), len(ids), ids.shape[1], k, lam, _p(out_i), _p(out_s)))
    return out_i, out_s


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_every_new_symbol_is_bound_and_declared():
    lib = L.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "comorag_hip.h")).read()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert f"int32_t {name}(" in hdr, name
    assert lib.cmr_abi_version() == 2 == L.ABI_VERSION                   # symbols were only added
    assert "#define CMR_ROUTE_MMR (1 << 15)" in hdr and L.CMR_ROUTE_MMR == 1 << 15


# ---- argument rules on NULL handles: f(handle, nq, F, k, lam, buf) for every entry point that takes a handle
def _calls():
    lib = L.lib()
    return {
        "cmr_index_pair_scores": lambda h, nq, F, k, lam, b: lib.cmr_index_pair_scores(h, b, nq, F, b),
        "cmr_mindex_pair_scores": lambda h, nq, F, k, lam, b: lib.cmr_mindex_pair_scores(h, b, nq, F, b),
        "cmr_index_mmr_select": lambda h, nq, F, k, lam, b: lib.cmr_index_mmr_select(h, b, b, nq, F, k, lam, b, b),
        "cmr_mindex_mmr_select": lambda h, nq, F, k, lam, b: lib.cmr_mindex_mmr_select(h, b, b, nq, F, k, lam, b, b),
        "cmr_index_mmr_select_dev": lambda h, nq, F, k, lam, b: lib.cmr_index_mmr_select_dev(h, b, b, nq, F, k, lam, b, b, None),
        "cmr_index_search_mmr": lambda h, nq, F, k, lam, b: lib.cmr_index_search_mmr(h, b, nq, k, F, lam, b, b),
        "cmr_mindex_search_mmr": lambda h, nq, F, k, lam, b: lib.cmr_mindex_search_mmr(h, b, nq, k, F, lam, b, b),
        "cmr_index_search_mmr_dev": lambda h, nq, F, k, lam, b: lib.cmr_index_search_mmr_dev(h, b, nq, k, F, lam, b, b, None),
    }


def test_the_calls_below_cover_every_new_entry_point():
    assert sorted(list(_calls()) + ["cmr_mmr_select"]) == sorted(NEW)


@pytest.mark.parametrize("name", sorted(_calls()))
def test_arguments_are_checked_before_the_handle(name):
    f = _calls()[name]
    buf = _p(np.zeros(4096, np.float32))
    pair = "pair_scores" in name                                      # (no k, no lambda)
    assert f(None, 1, 8, 4, 0.5, buf) == L.CMR_ERR_INVALID and "NULL index" in _err()
    assert f(None, 1, 8, 4, 0.5, None) == L.CMR_ERR_INVALID and "NULL argument" in _err()
    assert f(None, 0, 8, 4, 0.5, buf) == L.CMR_ERR_INVALID and "nq" in _err() and "NULL" not in _err()
    assert f(None, 1, L.CMR_MAX_K + 1, 4, 0.5, buf) == L.CMR_ERR_UNSUPPORTED and "CMR_MAX_K" in _err()
    assert f(None, 1, 0, 1, 0.5, buf) == L.CMR_ERR_INVALID and "NULL" not in _err()
    assert f(None, 1, L.CMR_MAX_K, 4, 0.5, buf) == L.CMR_ERR_INVALID and "NULL index" in _err()      # the largest F is fine
    if pair:
        return
    for k in (0, -1, 9):
        assert f(None, 1, 8, k, 0.5, buf) == L.CMR_ERR_INVALID and "fetch_k" in _err() and "NULL" not in _err(), k
    for lam in (-0.001, 1.001, NAN, float("inf"), -float("inf")):
        assert f(None, 1, 8, 4, lam, buf) == L.CMR_ERR_INVALID and "lambda" in _err() and "NULL" not in _err(), lam
    for lam in (0.0, 1.0, -0.0):
        assert f(None, 1, 8, 4, lam, buf) == L.CMR_ERR_INVALID and "NULL index" in _err(), lam
    assert f(None, 1, 8, 8, 0.5, buf) == L.CMR_ERR_INVALID and "NULL index" in _err()                # k == F is fine


def test_host_select_checks_its_arguments():
    lib = L.lib()
    rel, G, ids = np.ones((1, 4), np.float32), np.ones((1, 4, 4), np.float32), np.arange(4, dtype=np.int64)[None]
    oi, os_ = np.empty((1, 4), np.int64), np.empty((1, 4), np.float32)
    ok = lambda **kw: lib.cmr_mmr_select(*[kw.get(n, d) for n, d in (("rel", _p(rel)), ("G", _p(G)), ("ids", _p(ids)), ("nq", 1), ("F", 4), ("k", 2),
                                                                      ("lam", 0.5), ("oi", _p(oi)), ("os", _p(os_)))])
    assert ok() == L.CMR_OK
    for name in ("rel", "G", "ids", "oi", "os"):
        assert ok(**{name: None}) == L.CMR_ERR_INVALID, name
    assert ok(nq=0) == ok(k=0) == ok(k=5) == ok(lam=NAN) == ok(lam=1.5) == ok(lam=-0.5) == L.CMR_ERR_INVALID
    big = np.zeros(129 * 129, np.float32)
    assert lib.cmr_mmr_select(_p(big), _p(big), _p(np.zeros(129, np.int64)), 1, 129, 2, 0.5, _p(oi), _p(os_)) == L.CMR_ERR_UNSUPPORTED
    bad = rel.copy(); bad[0, 3] = NAN
    assert ok(rel=_p(bad)) == L.CMR_ERR_INVALID and "NaN" in _err()


# ---- the model against a hand-computed example
def test_model_on_a_hand_computed_example():
    # rows 0 and 1 are near-duplicates (pair 0.95); lam 0.5: pick 0 (rel .9); then 1: .425 - .475 = -.05, 2: .25 - .05 = .2,
    # 3: .15 - .1 = .05 -> 2; then 1: pen max(.95, .1) -> -.05, 3: pen max(.2, 0) -> .05 -> 3; then 1
    rel = np.array([0.9, 0.85, 0.5, 0.3], np.float32)
    G = np.array([[1, .95, .1, .2], [.95, 1, .1, .2], [.1, .1, 1, 0], [.2, .2, 0, 1]], np.float32)
    ids = np.array([10, 11, 12, 13], np.int64)
    got = mm.select_one(rel, G, ids, 4, 0.5)
    assert got[0].tolist() == [10, 12, 13, 11] and got[1].tolist() == rel[[0, 2, 3, 1]].tolist()
    assert mm.select_one(rel, G, ids, 4, 1.0)[0].tolist() == [10, 11, 12, 13]                         # lam 1: relevance order
    assert mm.select_one(rel, G, ids, 3, 0.0)[0].tolist() == [10, 12, 13]                             # lam 0: first by relevance, then least similar (ties: lowest position)
    assert mm.select_one(rel, G, np.array([10, 10, -1, 13]), 4, 0.5)[0].tolist() == [10, 13, -1, -1]  # a repeat and a negative id are void
    assert same(host_select(rel, G, ids, 4, 0.5), (got[0][None], got[1][None]))


# ---- cmr_mmr_select == model, bit for bit
@pytest.mark.parametrize("shape", mm.SHAPES, ids=lambda s: "n%d-d%d-nq%d-F%d-k%d" % s)
def test_host_select_equals_the_model_on_clustered_inputs(shape):
    n, d, nq, F, k = shape
    X, Q = mm.inputs(n, d, nq)
    Xr, Qr = orc.bf16_round(X), orc.bf16_round(Q)
    S = (Qr.astype(np.float64) @ Xr.astype(np.float64).T).astype(np.float32)
    ids, rel = mm.topk(S, F)
    G = np.stack([mm.gram_f64(Xr, ids[i]) for i in range(nq)])
    plain = mm.topk(S, k)
    for lam in (0.0, 0.3, 0.5, 1.0):
        want = mm.select(rel, G, ids, k, lam)
        assert same(host_select(rel, G, ids, k, lam), want), lam
        if lam == 1.0:
            assert same(want, plain)
        if lam == 0.5:      # the inputs do their work: every query's list differs from its plain top-k
            assert all(want[0][i].tolist() != plain[0][i].tolist() for i in range(nq))
    if F == k:              # fetch_k == k: the same set in another order
        assert all(sorted(mm.select(rel, G, ids, k, 0.5)[0][i].tolist()) == sorted(plain[0][i].tolist()) for i in range(nq))


def _rand_case(rng, F):
    rel = rng.standard_normal(F).astype(np.float32)
    A = rng.standard_normal((F, 6)).astype(np.float32)
    return rel, (A @ A.T).astype(np.float32), rng.permutation(1000)[:F].astype(np.int64)


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5, 1.0])
def test_host_select_equals_the_model_on_hand_made_cases(lam):
    rng = np.random.default_rng(77)
    cases = []
    for F in (1, 2, 7, 64, 65, 128):
        rel, G, ids = _rand_case(rng, F)
        for k in sorted({1, (F + 1) // 2, F}):
            cases.append((rel, G, ids, k))
    F = 12
    rel, G, ids = _rand_case(rng, F)
    tied = rel.copy(); tied[[2, 5, 9]] = tied.max() + 1                    # three equal maxima: position 2 first
    cases.append((tied, G, ids, 5))
    cases.append((np.zeros(F, np.float32), np.zeros((F, F), np.float32), ids, F))      # everything ties: position order
    void = ids.copy(); void[[0, 4]] = -1; void[7] = void[3]; void[11] = void[3]
    cases.append((rel, G, void, F))                                        # -1 and repeated ids; fewer non-void positions than k
    cases.append((rel, G, np.full(F, -1, np.int64), 3))                    # nothing to pick
    cases.append((rel, G, np.full(F, 5, np.int64), 3))                     # one distinct id
    z = np.zeros(F, np.float32); z[4] = -0.0; z[1] = -0.0
    cases.append((z, np.zeros((F, F), np.float32), ids, 4))                # -0.0 against +0.0: equal, lowest position wins
    for rel, G, ids, k in cases:
        want = mm.select_one(rel, G, ids, k, lam)
        assert same(host_select(rel, G, ids, k, lam), (want[0][None], want[1][None])), (len(ids), k)
    got = host_select(tied, G, cases[-6][2], 5, lam)
    assert got[0][0, 0] == cases[-6][2][2]
    got = host_select(z, np.zeros((F, F), np.float32), ids, 4, lam)
    assert got[0][0].tolist() == ids[:4].tolist() and np.signbit(got[1][0]).tolist() == [False, True, False, False]
    got = host_select(rel, G, void, F, lam)
    assert (got[0][0] >= 0).sum() == F - 4 and set(got[0][0][:F - 4].tolist()) == set(void[void >= 0].tolist()) and np.all(np.isneginf(got[1][0][F - 4:]))


def test_a_batch_of_queries_is_selected_row_by_row():
    rng = np.random.default_rng(5)
    parts = [_rand_case(rng, 20) for _ in range(7)]
    rel, G, ids = (np.stack([p[i] for p in parts]) for i in range(3))
    assert same(host_select(rel, G, ids, 6, 0.4), mm.select(rel, G, ids, 6, 0.4))
