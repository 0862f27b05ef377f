"""Diversified top-k on the device (cmr_index_pair_scores, cmr_index_mmr_select*, cmr_index_search_mmr*, cmr_mindex_*).
Every comparison is `np.array_equal` on ids and on score bits.  The oracle is tests/mmr_model.py: the selection in float32 numpy, over
pair scores built from calls that existed before the feature (`scores(get_rows(ids))[:, ids]`) and candidates from `search(q, fetch_k)`.
One anchor holds the pair scores against fp64 products of the rounded rows under the tolerance of tests/test_range_search_gpu.py's anchor
(tests/value_domain_inputs.py: row_tol).  Inputs: clustered rows with near-duplicates (mmr_model.inputs); indexes are built once."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc
from tests import mmr_model as mm
from tests import value_domain_inputs as vd

pytestmark = pytest.mark.gpu

NQ_MAX = 65
# tag -> (dtype, n, d): 768-d bf16; f16 with dim no multiple of 16 and n no multiple of 32; a small fp32 index
CASES = {"bf16-1000x768": ("bf16", 1000, 768), "f16-333x40": ("f16", 333, 40), "f32-70x24": ("f32", 70, 24)}
LAMS = (0.0, 0.3, 0.5, 1.0)
BASE = 1_000_000
NEG_INF = np.float32(-np.inf)

_cache = {}


def _rows(tag):
    if ("rows", tag) not in _cache:
        _, n, d = CASES[tag]
        _cache[("rows", tag)] = mm.inputs(n, d, NQ_MAX, seed=len(tag))
    return _cache[("rows", tag)]


def _index(tag, kind="plain", **kw):
    from comorag_amd.index import DenseIndex
    key = ("index", tag, kind)
    if key not in _cache:
        dtype, n, d = CASES[tag]
        idx = DenseIndex(d, dtype, **kw)
        idx.append(_rows(tag)[0])
        if kind == "based":
            idx.set_id_base(BASE)
        _cache[key] = idx
    return _cache[key]


def teardown_module(module):
    for key, v in list(_cache.items()):
        if key[0] == "index":
            v.close()
    _cache.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _padded(ids, sc, F):
    nq, have = ids.shape
    pi, ps = np.full((nq, F), -1, np.int64), np.full((nq, F), NEG_INF, np.float32)
    pi[:, :have], ps[:, :have] = ids, sc
    return pi, ps


def _candidates(idx, Q, F, key=None):
    """search(Q, F) padded to F columns and the model's pair scores of those candidates (cached per key: the reference is computed once)"""
    if key is not None and ("cand",) + key in _cache:
        return _cache[("cand",) + key]
    ids, sc, _, _ = idx.search(Q, F)
    ids, sc = _padded(ids, sc, F)
    out = (ids, sc, mm.gram(idx, ids))
    if key is not None:
        _cache[("cand",) + key] = out
    return out


def _expect(idx, Q, k, F, lam, key=None):
    ids, sc, G = _candidates(idx, Q, F, key)
    want = mm.select(sc, G, ids, k, lam)
    kk = min(k, len(idx))
    return want[0][:, :kk], want[1][:, :kk]


# ---------------------------------------------------------------------------------------------- pair scores
@pytest.mark.parametrize("tag", sorted(CASES))
def test_pair_scores_equal_scores_of_get_rows(tag):
    idx, (X, Q) = _index(tag), _rows(tag)
    ids = idx.search(Q[:4], 33)[0]
    got = idx.pair_scores(ids)
    assert got.shape == (4, 33, 33) and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(mm.gram(idx, ids)))
    assert np.all(np.isfinite(got))
    one = idx.pair_scores(ids[0])                                        # [F] -> [F, F]
    assert one.shape == (33, 33) and np.array_equal(_bits(one), _bits(got[0]))


@pytest.mark.parametrize("F", [1, 31, 32, 33, 128])
def test_pair_scores_at_the_tile_edges(F):
    idx = _index("bf16-1000x768")
    rng = np.random.default_rng(F)
    ids = np.stack([rng.permutation(1000)[:F] for _ in range(3)]).astype(np.int64)
    ids[1, : min(F, 4)] = [3, 17, 500, 999][: min(F, 4)]                 # the bit-equal copies: distinct ids, equal rows
    got = idx.pair_scores(ids)
    assert np.array_equal(_bits(got), _bits(mm.gram(idx, ids))) and np.all(np.isfinite(got))
    if F >= 4:
        assert len(set(_bits(got[1][:4, :4]).ravel().tolist())) == 1      # copies of one row score alike, whichever side they are on


@pytest.mark.parametrize("tag", ["f16-333x40", "f32-70x24"])
def test_pair_scores_with_void_positions(tag):
    idx = _index(tag)
    n = len(idx)
    ids = np.array([[5, -1, 7, 5, n, 9, n + 1000, 7, -5, 0, n - 1, 2 ** 40, 11] + list(range(20, 42)),
                    [-1] * 35,
                    [3] * 35], dtype=np.int64)
    got = idx.pair_scores(ids)
    want = mm.gram(idx, ids)
    assert np.array_equal(_bits(got), _bits(want))
    void = [1, 3, 4, 6, 7, 8, 11]
    assert np.all(np.isneginf(got[0][void, :])) and np.all(np.isneginf(got[0][:, void]))
    live = [p for p in range(35) if p not in void]
    assert np.all(np.isfinite(got[0][np.ix_(live, live)]))
    assert np.all(np.isneginf(got[1])) and np.isfinite(got[2][0, 0]) and np.isneginf(got[2]).sum() == 35 * 35 - 1


def test_pair_scores_with_an_id_base():
    tag = "f16-333x40"
    plain, based = _index(tag), _index(tag, "based")
    local = np.array([[0, 5, 332, 17, 3, 100, 333, -1] + list(range(40, 66))], dtype=np.int64)
    ids = np.where(local >= 0, local + BASE, local)
    got = based.pair_scores(ids)
    assert np.array_equal(_bits(got), _bits(mm.gram(based, ids, base=BASE)))
    assert np.array_equal(_bits(got), _bits(plain.pair_scores(local)))
    assert np.all(np.isneginf(based.pair_scores(local[:, :6])))           # ids below the base are held by nobody


@pytest.mark.parametrize("tag", sorted(CASES))
def test_pair_scores_against_fp64_of_the_rounded_rows(tag):
    idx, (X, Q) = _index(tag), _rows(tag)
    Xr = vd.ROUND[CASES[tag][0]](X)
    ids = idx.search(Q[:2], 33)[0]
    got = idx.pair_scores(ids)
    for i in range(2):
        R = Xr[ids[i]]
        exact = orc.exact_scores_f64(R, R)                                # [s, c]: query s against row c
        for s in range(33):
            assert np.all(np.abs(got[i][s].astype(np.float64) - exact[s]) <= vd.row_tol(R[s], R)), (i, s)


# ---------------------------------------------------------------------------------------------- search_mmr against the model
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("tag", sorted(CASES))
def test_search_mmr_equals_the_model(tag, lam):
    idx, (X, Q) = _index(tag), _rows(tag)
    k, F = 10, 40
    got = idx.search_mmr(Q[:5], k, F, lam)
    assert got[0].shape == (5, k)
    assert same(got, _expect(idx, Q[:5], k, F, lam, key=(tag, 5, F)))


@pytest.mark.parametrize("nq", [1, 3, 65])
@pytest.mark.parametrize("k,F", [(1, 1), (8, 32), (10, 33), (31, 31), (20, 128)])
def test_search_mmr_shapes(k, F, nq):
    tag = "bf16-1000x768"
    idx, (X, Q) = _index(tag), _rows(tag)
    got = idx.search_mmr(Q[:nq], k, F, 0.5)
    assert same(got, _expect(idx, Q[:nq], k, F, 0.5, key=(tag, nq, F)))
    plain = idx.search(Q[:nq], k)
    assert same(idx.search_mmr(Q[:nq], k, F, 1.0), plain[:2])            # lambda 1 is the plain top-k
    if F == k:
        assert np.array_equal(np.sort(got[0], axis=1), np.sort(plain[0], axis=1))      # the same set in MMR order
    if k >= 8 and F > k:      # the inputs do their work: every query's list differs from its plain top-k
        assert all(got[0][i].tolist() != plain[0][i].tolist() for i in range(nq))


def test_lists_differ_from_top_k_on_the_f16_shape_too():
    tag = "f16-333x40"
    idx, (X, Q) = _index(tag), _rows(tag)
    got = idx.search_mmr(Q, 10, 33, 0.5)
    plain = idx.search(Q, 10)
    assert same(got, _expect(idx, Q, 10, 33, 0.5, key=(tag, NQ_MAX, 33)))
    assert all(got[0][i].tolist() != plain[0][i].tolist() for i in range(NQ_MAX))
    assert same(idx.search_mmr(Q, 10, 33, 1.0), plain[:2])
    assert same(idx.search_mmr(Q, 10), _expect(idx, Q, 10, 40, 0.5))      # the default fetch_k = min(128, max(4 k, 20))


def test_route_independence_and_last_route():
    from comorag_amd.index import DenseIndex
    tag = "bf16-1000x768"
    ref, (X, Q) = _index(tag), _rows(tag)
    want = {nq: ref.search_mmr(Q[:nq], 10, 40, 0.5) for nq in (2, 65)}
    routes = set()
    for opts in ({}, {"scan_no_tiny": 1}, {"scan_no_small": 1}, {"scan_no_tiny": 1, "scan_no_small": 1, "scan_fin": 0}):
        idx = DenseIndex(768, "bf16", options=opts)
        try:
            idx.append(X)
            for nq in (2, 65):
                assert same(idx.search_mmr(Q[:nq], 10, 40, 0.5), want[nq]), (opts, nq)
                mmr_route = idx.get_option("last_route")
                assert mmr_route & L.CMR_ROUTE_MMR
                idx.search(Q[:nq], 40)
                assert idx.get_option("last_route") == mmr_route & ~L.CMR_ROUTE_MMR      # ... together with the candidate search's route
                routes.add((nq, mmr_route & 0xF))
        finally:
            idx.close()
    assert len({r for nq, r in routes if nq == 2}) >= 2                   # the options did move the candidate search between routes


# ---------------------------------------------------------------------------------------------- small and empty indexes
def test_small_and_empty_indexes():
    from comorag_amd.index import DenseIndex
    X, Q = mm.inputs(8, 32, 3, seed=1)
    for n in (5, 1):
        idx = DenseIndex(32, "bf16")
        try:
            idx.append(X[:n])
            got = idx.search_mmr(Q, 8, 16, 0.5)
            assert got[0].shape == (3, n)                                # k' = min(k, len)
            assert same(got, _expect(idx, Q, 8, 16, 0.5))
            assert all(sorted(r.tolist()) == list(range(n)) for r in got[0])
            ids = np.empty((3, 8), np.int64); sc = np.empty((3, 8), np.float32)      # the C call pads to k columns
            L.check(L.lib().cmr_index_search_mmr(idx._h, C.c_void_p(Q.ctypes.data), 3, 8, 16, 0.5, C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data)))
            assert np.array_equal(ids[:, :n], got[0]) and np.all(ids[:, n:] == -1) and np.all(np.isneginf(sc[:, n:]))
        finally:
            idx.close()
    idx = DenseIndex(32, "bf16")
    try:
        assert idx.search_mmr(Q, 8, 16, 0.5)[0].shape == (3, 0)
        ids = np.zeros((3, 8), np.int64); sc = np.zeros((3, 8), np.float32)
        L.check(L.lib().cmr_index_search_mmr(idx._h, C.c_void_p(Q.ctypes.data), 3, 8, 16, 0.5, C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data)))
        assert np.all(ids == -1) and np.all(np.isneginf(sc))
        assert np.all(np.isneginf(idx.pair_scores(np.arange(4))))
        sel = idx.mmr_select(np.arange(4), np.ones(4, np.float32), 2)
        assert np.all(sel[0] == -1) and np.all(np.isneginf(sel[1]))
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------- mmr_select over other searches' candidates
def test_mmr_select_of_a_filtered_search():
    tag = "f16-333x40"
    idx, (X, Q) = _index(tag), _rows(tag)
    Qs = Q[:6]
    top = idx.search(Qs, 25)[0]
    exclude = [top[i, ::2] for i in range(6)]                             # every other row of each query's top 25, a list per query
    allow_few = np.arange(0, 333, 29)                                     # 12 rows: fewer than fetch_k, so the candidates come padded
    for kw in ({"exclude": exclude}, {"allow": allow_few}):
        cid, csc, _, _ = idx.search_filtered_ids(Qs, 40, with_minmax=False, **kw)
        got = idx.mmr_select(cid, csc, 10, 0.5)
        assert same(got, idx.search_mmr(Qs, 10, 40, 0.5, **kw))
        assert same(got, mm.select(csc, mm.gram(idx, cid), cid, 10, 0.5))
        if "exclude" in kw:
            assert all(not set(got[0][i].tolist()) & set(exclude[i].tolist()) for i in range(6)) and np.all(got[0] >= 0)
        else:
            assert (cid < 0).any() and set(got[0].ravel().tolist()) <= set(allow_few.tolist())
    with pytest.raises(L.CmrError):
        idx.mmr_select(np.arange(4), np.array([1, np.nan, 0, 0], np.float32), 2)


def test_dev_forms_equal_the_host_forms():
    import torch
    tag = "bf16-1000x768"
    idx, (X, Q) = _index(tag), _rows(tag)
    dev = torch.device("cuda", 0)
    for nq in (3, 65):
        q_t = torch.from_numpy(Q[:nq]).to(dev)
        want = idx.search_mmr(Q[:nq], 10, 40, 0.3)
        ids_t, sc_t = idx.search_mmr_dev(q_t, 10, 40, 0.3)
        torch.cuda.synchronize(dev)
        assert same((ids_t.cpu().numpy(), sc_t.cpu().numpy()), want)
        cid, csc, _, _ = idx.search(Q[:nq], 40)
        oi, os_ = idx.mmr_select_dev(torch.from_numpy(cid.copy()).to(dev), torch.from_numpy(csc.copy()).to(dev), 10, 0.3)
        torch.cuda.synchronize(dev)
        assert same((oi.cpu().numpy(), os_.cpu().numpy()), want)
        assert same(idx.mmr_select(cid, csc, 10, 0.3), want)
    side = torch.cuda.Stream(dev)                                         # ... and on a stream that is not the default one
    with torch.cuda.stream(side):
        q_t = torch.from_numpy(Q[:3]).to(dev)
        ids_t, sc_t = idx.search_mmr_dev(q_t, 10, 40, 0.3)
    side.synchronize()
    assert same((ids_t.cpu().numpy(), sc_t.cpu().numpy()), idx.search_mmr(Q[:3], 10, 40, 0.3))


# ---------------------------------------------------------------------------------------------- after row changes; keep_f32
def test_after_remove_ids_and_update_rows_it_equals_a_fresh_index():
    from comorag_amd.index import DenseIndex
    tag = "f16-333x40"
    X, Q = _rows(tag)
    Qs = Q[:7]
    idx = DenseIndex(40, "f16")
    try:
        idx.append(X)
        gone = np.array([0, 3, 40, 41, 166, 332])
        assert idx.remove_ids(gone) == 6
        final = np.delete(X, gone, axis=0)
        fresh = DenseIndex(40, "f16"); fresh.append(final)
        try:
            assert same(idx.search_mmr(Qs, 10, 33, 0.5), fresh.search_mmr(Qs, 10, 33, 0.5))
            assert same(idx.search_mmr(Qs, 10, 33, 0.5), _expect(fresh, Qs, 10, 33, 0.5))
        finally:
            fresh.close()
        at = np.array([1, 14, 200, len(final) - 1])
        final = final.copy(); final[at] = X[[3, 3, 50, 60]]              # two more copies of row 3, two other rows
        assert idx.update_rows(at, final[at]) == 4
        fresh = DenseIndex(40, "f16"); fresh.append(final)
        try:
            assert same(idx.search_mmr(Qs, 10, 33, 0.5), fresh.search_mmr(Qs, 10, 33, 0.5))
            ids = fresh.search(Qs, 33)[0]
            assert np.array_equal(_bits(idx.pair_scores(ids)), _bits(fresh.pair_scores(ids)))
        finally:
            fresh.close()
    finally:
        idx.close()


def test_keep_f32_returns_the_bits_of_the_plain_index():
    tag = "bf16-1000x768"
    plain, (X, Q) = _index(tag), _rows(tag)
    kept = _index(tag, "keep_f32", keep_f32=True)
    assert same(kept.search_mmr(Q[:5], 10, 40, 0.5), plain.search_mmr(Q[:5], 10, 40, 0.5))
    ids = plain.search(Q[:2], 33)[0]
    assert np.array_equal(_bits(kept.pair_scores(ids)), _bits(plain.pair_scores(ids)))


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("S", [2, 3])
def test_shards_equal_one_index(S):
    from comorag_amd.index import DenseIndex
    from comorag_amd.multi_index import MultiDeviceIndex
    n, d = 3000, 64
    if ("shard-rows",) not in _cache:
        X, Q = mm.inputs(n, d, NQ_MAX, seed=4)
        one = DenseIndex(d, "bf16"); one.append(X)
        _cache[("shard-rows",)] = (X, Q)
        _cache[("index", "shard-one", "plain")] = one
    X, Q = _cache[("shard-rows",)]
    one = _cache[("index", "shard-one", "plain")]
    multi = MultiDeviceIndex(d, "bf16", devices=[0] * S, options={"append_block_rows": 1024})
    try:
        multi.append(X)
        assert sum(1 for r in multi.shard_rows() if r > 0) >= 2           # the rows do lie on several shards
        for nq, k, F in ((3, 10, 40), (65, 8, 33), (2, 20, 128)):
            assert same(multi.search_mmr(Q[:nq], k, F, 0.5), one.search_mmr(Q[:nq], k, F, 0.5)), (nq, k, F)
        assert same(multi.search_mmr(Q[:4], 10, 40, 1.0), one.search(Q[:4], 10)[:2])
        cid, csc, _, _ = one.search(Q[:5], 40)
        cid, csc = cid.copy(), csc.copy()
        cid[0, 3] = -1; cid[1, 5] = cid[1, 2]; cid[2, 7] = n + 5          # padding, a repeat, an id nobody holds
        assert same(multi.mmr_select(cid, csc, 10, 0.3), one.mmr_select(cid, csc, 10, 0.3))
        assert same(one.mmr_select(cid, csc, 10, 0.3), mm.select(csc, mm.gram(one, cid), cid, 10, 0.3))
        for F in (1, 33, 128):
            ids = cid[:, :F] if F <= 40 else np.stack([np.random.default_rng(i).permutation(n)[:F] for i in range(2)]).astype(np.int64)
            assert np.array_equal(_bits(multi.pair_scores(ids)), _bits(one.pair_scores(ids))), F
        ex = [cid[i, :6] for i in range(5)]
        assert same(multi.search_mmr(Q[:5], 10, 40, 0.5, exclude=ex), one.search_mmr(Q[:5], 10, 40, 0.5, exclude=ex))
    finally:
        multi.close()
