"""Per-query filtered search (cmr_index_search_masked_each*): row i of the result is bit for bit what the one-query
`search_filtered(Q[i:i+1], k, mask=masks[i])` returns — ids, score bits, min, max and the -1 / -inf padding, no tolerance.  The oracle
uses only calls that existed before the feature; once per corpus size it is itself held against `search` on a second index of a query's
allowed rows.  Corpora and indexes are built once per module, with the shapes of tests/test_filtered_search_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_mask, pack_row_masks

pytestmark = pytest.mark.gpu

CHAIN, MORE_PASSES, FILTERED, EACH = 3, 1 << 11, 1 << 12, 1 << 13
N_SMALL = 1000                  # no sampling, partial last panel
N_ONE_LEVEL = 8192 + 5          # 257 panels: one sampling level
N_TWO_LEVELS = 131072 + 7       # 4097 panels: in-scan thresholds at nq <= 2, the single 128-panel level at nq <= 8, two levels above
SHAPES = {"bf16": 128, "f16": 96, "f32": 96}      # dim 96 is padded to 128
NQ_MAX = 65

_cache = {}


def _rows(dtype, n):
    """seeded, row-normalised corpus [n, dim] and NQ_MAX queries, half of them planted near corpus rows"""
    key = ("rows", dtype, n)
    if key not in _cache:
        d = SHAPES[dtype]
        rng = np.random.default_rng(1000 * n + d)
        X = rng.standard_normal((n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rng.standard_normal((NQ_MAX, d)).astype(np.float32)
        pick = rng.integers(0, n, NQ_MAX // 2)
        Q[: len(pick)] = X[pick] + 0.05 * Q[: len(pick)]
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        _cache[key] = (X, Q)
    return _cache[key]


def _index(dtype, n):
    from comorag_amd.index import DenseIndex
    key = ("index", dtype, n)
    if key not in _cache:
        idx = DenseIndex(SHAPES[dtype], dtype)
        idx.append(_rows(dtype, n)[0])
        _cache[key] = idx
    return _cache[key]


def teardown_module(module):
    for key, v in list(_cache.items()):
        if key[0] == "index":
            v.close()
    _cache.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_rows_equal_solo(idx, Q, k, keeps, got, what="", base=0):
    """got = (ids [nq,k], scores [nq,k], min, max) of one per-query call; keeps[i] = bool [n] of query i.  The oracle call comes AFTER the
    call under test, on the same index."""
    nq = len(Q)
    assert got[0].shape == (nq, k) and got[1].shape == (nq, k) and got[2].shape == (nq,) and got[3].shape == (nq,), what
    for i in range(nq):
        ids, sc, mn, mx = idx.search_filtered(Q[i:i + 1], k, allow=keeps[i])
        kk = ids.shape[1]
        w = f"{what} query {i} allowed={int(keeps[i].sum())}"
        assert kk == min(k, int(keeps[i].sum())), w
        assert np.array_equal(got[0][i, :kk], ids[0]), w
        assert np.array_equal(_bits(got[1][i, :kk]), _bits(sc[0])), w
        assert (got[0][i, kk:] == -1).all() and np.isneginf(got[1][i, kk:]).all(), w
        assert _bits(got[2][i:i + 1])[0] == _bits(mn)[0] and _bits(got[3][i:i + 1])[0] == _bits(mx)[0], w
        if kk:
            assert keeps[i][got[0][i, :kk] - base].all(), w


def _check(dtype, n, nq, k, keeps, what=""):
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    got = idx.search_filtered_each(Q, k, allow=keeps)
    r = idx.get_option("last_route")
    _assert_rows_equal_solo(idx, Q, k, keeps, got, f"{what} {dtype} n={n} nq={nq} k={k}")
    assert r & 0xF == CHAIN and r & FILTERED and r & EACH, hex(r)
    return r


def _random_keeps(n, nq, p=0.5, seed0=0):
    return [np.random.default_rng(seed0 + 7919 * i).random(n) < p for i in range(nq)]


def _second_index_check(dtype, n, keep, q, k, got_row):
    """`search` on an index of the allowed rows alone, ids mapped back: what the solo oracle itself is defined by"""
    from comorag_amd.index import DenseIndex
    rows = np.flatnonzero(keep)
    ref = DenseIndex(SHAPES[dtype], dtype)
    try:
        ref.append(_rows(dtype, n)[0][rows])
        ids, sc, mn, mx = ref.search(q[None, :], k)
    finally:
        ref.close()
    kk = ids.shape[1]
    assert np.array_equal(got_row[0][:kk], rows[ids[0]]) and np.array_equal(_bits(got_row[1][:kk]), _bits(sc[0]))
    assert _bits(got_row[2:3])[0] == _bits(mn)[0] and _bits(got_row[3:4])[0] == _bits(mx)[0]


@pytest.mark.parametrize("nq", [1, 2, 8, 31, 32, 33, 64, 65])
def test_every_lane_position_and_pass(nq):
    """nq = 33, 64: the second tile's words; nq = 65: the second pass's mask offset; nq = 1, 31, 33: padding lanes that must not load"""
    keeps = _random_keeps(N_SMALL, nq)
    for k in (1, 20, 33, 128):
        r = _check("bf16", N_SMALL, nq, k, keeps)
        assert bool(r & MORE_PASSES) == (nq > 64), hex(r)


def _mixed(n, nq, seed):
    """the issue's mask kinds, dealt round robin to the queries of one call (an offset moves every kind over every lane position)"""
    rng = np.random.default_rng(seed)
    one = np.zeros(n, bool); one[n // 2] = True
    tail = np.zeros(n, bool); tail[n - n % 32:] = True
    kinds = [np.ones(n, bool), np.zeros(n, bool), one, tail, np.arange(n) % 2 == 0, (np.arange(n) // 32) % 2 == 1]
    keeps = []
    for i in range(nq):
        j = i % (len(kinds) + 1)
        keeps.append(rng.random(n) < 0.01 if j == len(kinds) else kinds[j].copy())
    return keeps


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL])
def test_mixed_masks_in_one_batch(dtype, n):
    """all-ones, all-zeros, one row, only the last partial panel, every other row, alternating panels and random 1 % side by side: a
    non-uniform `whole` shortcut or a lane without allowed rows taken as reaching a threshold of -inf shows here"""
    for nq, k in ((8, 20), (33, 33), (64, 128)):
        keeps = _mixed(n, nq, seed=n + nq)
        idx = _index(dtype, n)
        Q = _rows(dtype, n)[1][:nq]
        got = idx.search_filtered_each(Q, k, allow=keeps)
        _assert_rows_equal_solo(idx, Q, k, keeps, got, f"mixed {dtype} n={n} nq={nq} k={k}")
        zero = [i for i in range(nq) if not keeps[i].any()]
        assert zero and (got[0][zero] == -1).all() and np.isneginf(got[1][zero]).all()
        assert np.isposinf(got[2][zero]).all() and np.isneginf(got[3][zero]).all()
    if dtype == "bf16":
        _second_index_check(dtype, n, keeps[4], Q[4], k, (got[0][4], got[1][4], got[2][4], got[3][4]))


@pytest.mark.parametrize("n", [N_ONE_LEVEL, N_TWO_LEVELS])
@pytest.mark.parametrize("nq,k,levels2,tau_in_scan2,single2", [(1, 20, 1, True, True), (2, 20, 1, True, True), (8, 20, 1, False, True),
                                                               (33, 33, 2, False, False), (64, 128, 2, False, False)])
def test_per_query_adversarial_masks(n, nq, k, levels2, tau_in_scan2, single2):
    """query i's mask removes exactly query i's OWN unfiltered top-k: a build whose sampling reads another query's words (or none) takes a
    threshold from a forbidden row and loses allowed rows.  The last query allows only 3k rows: its sample holds fewer than k — no threshold."""
    dtype = "bf16"
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    top = idx.search(Q, k)[0]
    keeps = []
    for i in range(nq):
        keep = np.ones(n, bool)
        keep[top[i]] = False
        keeps.append(keep)
    if nq > 1:
        few = np.zeros(n, bool); few[np.random.default_rng(n + nq).choice(n, 3 * k, replace=False)] = True
        keeps[-1] = few
    r = _check(dtype, n, nq, k, keeps, "adversarial")
    got = idx.search_filtered_each(Q, k, allow=keeps)
    for i in range(nq - (nq > 1)):
        assert not np.isin(got[0][i], top[i]).any()
    if n == N_TWO_LEVELS:
        assert ((r >> 4) & 3, bool(r >> 6 & 1), bool(r >> 7 & 1)) == (levels2, tau_in_scan2, single2), hex(r)
    else:
        assert (r >> 4) & 3 == 1, hex(r)
    if nq == 8:
        _second_index_check(dtype, n, keeps[3], Q[3], k, (got[0][3], got[1][3], got[2][3], got[3][3]))


@pytest.mark.parametrize("n,nq,k", [(N_SMALL, 33, 20), (N_ONE_LEVEL, 65, 33), (N_TWO_LEVELS, 8, 20)])
def test_same_mask_for_every_query_is_the_shared_mask_call(n, nq, k):
    dtype = "bf16"
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    keep = np.random.default_rng(n).random(n) < 0.5
    words = pack_row_mask(n, allow=keep)
    got = idx.search_filtered_each(Q, k, masks=np.tile(words, (nq, 1)))
    want = idx.search_filtered(Q, k, mask=words)
    assert np.array_equal(got[0], want[0]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[1:], want[1:]))
    ones = idx.search_filtered_each(Q, k, masks=np.tile(pack_row_mask(n), (nq, 1)))
    assert idx.get_option("last_route") & EACH
    plain = idx.search(Q, k)
    assert np.array_equal(ones[0], plain[0]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ones[1:], plain[1:]))


def test_ties_come_out_id_ascending_among_each_querys_allowed_rows():
    from comorag_amd.index import DenseIndex
    dtype, n, k = "bf16", 1000, 20
    X, Q = _rows(dtype, n)
    X = X.copy()
    dup = np.array([3, 40, 41, 500, 731, 998, 999])
    X[dup] = X[17]                                   # eight rows with one score per query
    Q = np.concatenate([X[17:18], X[17:18], X[17:18], Q[:5]])
    drops = [[17, 41, 998], [3, 40], [], [17, 3, 40, 41, 500, 731, 998], [999], [17], [500, 731], [41]]
    keeps = []
    for d in drops:
        keep = np.ones(n, bool); keep[d] = False
        keeps.append(keep)
    idx = DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X)
        got = idx.search_filtered_each(Q, k, allow=keeps)
        _assert_rows_equal_solo(idx, Q, k, keeps, got, "ties")
    finally:
        idx.close()
    assert got[0][0, :5].tolist() == [3, 40, 500, 731, 999]          # the query IS the duplicated row: its allowed copies lead, ids ascending
    assert got[0][1, :6].tolist() == [17, 41, 500, 731, 998, 999]
    assert got[0][2, :8].tolist() == [3, 17, 40, 41, 500, 731, 998, 999]
    assert len(np.unique(_bits(got[1][2, :8]))) == 1


def test_id_base_and_block_table_move_the_ids_and_not_the_masks():
    from comorag_amd.index import DenseIndex
    dtype, n, nq, k, base = "f16", 1000, 8, 20, 5000
    X, Q = _rows(dtype, n)
    Q = Q[:nq]
    keeps = _random_keeps(n, nq, seed0=3)
    plain = _index(dtype, n).search_filtered_each(Q, k, allow=keeps)
    idx = DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X)
        idx.set_id_base(base)
        got = idx.search_filtered_each(Q, k, allow=keeps)
        _assert_rows_equal_solo(idx, Q, k, keeps, got, "id base", base=base)
    finally:
        idx.close()
    assert np.array_equal(got[0], plain[0] + base) and np.array_equal(_bits(got[1]), _bits(plain[1]))
    idx = DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X)
        idx.set_id_blocks([0, 600], [100, 9000])          # local rows 0..599 -> 100.., 600.. -> 9000..
        got = idx.search_filtered_each(Q, k, allow=keeps)
    finally:
        idx.close()
    want = np.where(plain[0] < 600, plain[0] + 100, plain[0] - 600 + 9000)
    assert np.array_equal(got[0], want) and np.array_equal(_bits(got[1]), _bits(plain[1]))


@pytest.mark.parametrize("n,nq,k", [(N_SMALL, 8, 20), (N_ONE_LEVEL, 65, 33), (N_TWO_LEVELS, 2, 20)])
def test_dev_form_equals_host_form(n, nq, k):
    import torch
    dtype = "bf16"
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    words = pack_row_masks(n, allow=_random_keeps(n, nq, p=0.3, seed0=n))
    host = idx.search_filtered_each(Q, k, masks=words)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(Q).to(dev)
    m_t = torch.from_numpy(words.view(np.int32)).to(dev)          # 2-d int32, read in place
    mn_t = torch.empty(nq, dtype=torch.float32, device=dev)
    mx_t = torch.empty(nq, dtype=torch.float32, device=dev)
    ids_t, sc_t = idx.search_filtered_each_dev(q_t, k, m_t, out_min=mn_t, out_max=mx_t)
    torch.cuda.synchronize(dev)
    r = idx.get_option("last_route")
    assert r & EACH and bool(r & MORE_PASSES) == (nq > 64)
    assert np.array_equal(ids_t.cpu().numpy(), host[0]) and np.array_equal(_bits(sc_t.cpu().numpy()), _bits(host[1]))
    assert np.array_equal(_bits(mn_t.cpu().numpy()), _bits(host[2])) and np.array_equal(_bits(mx_t.cpu().numpy()), _bits(host[3]))
    assert not idx.query_status()
    with pytest.raises(ValueError):
        idx.search_filtered_each_dev(q_t, k, m_t[0])


def test_other_calls_return_what_they_returned_before():
    import torch
    dtype, n, nq, k = "bf16", N_ONE_LEVEL, 8, 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(Q).to(dev)
    shared = np.random.default_rng(9).random(n) < 0.5

    def others():
        ids_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
        sc_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        idx.sync(idx.search_pipelined(q_t, k, ids_t, sc_t))
        f = idx.search_filtered(Q, k, allow=shared)
        assert idx.get_option("last_route") & FILTERED and not idx.get_option("last_route") & EACH
        return [*f, *idx.search(Q, k), idx.scores(Q), ids_t.cpu().numpy(), sc_t.cpu().numpy()]

    before = others()
    for p_keep in (0.5, 0.01, 0.0):
        idx.search_filtered_each(Q, k, allow=_random_keeps(n, nq, p=p_keep, seed0=5))
    idx.search_filtered_each(_rows(dtype, n)[1], 128, allow=_random_keeps(n, NQ_MAX, seed0=6))
    after = others()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    idx.search(Q, k)
    assert not idx.get_option("last_route") & (FILTERED | EACH)


def test_error_paths():
    dtype, n = "bf16", 1000
    idx = _index(dtype, n)
    Q = np.ascontiguousarray(_rows(dtype, n)[1][:2])
    words = pack_row_masks(n, allow=_random_keeps(n, 2))
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_each(Q, 129, masks=words)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_each(Q, 0, masks=words)
    assert e.value.code == L.CMR_ERR_INVALID
    # the C call itself: a wrong word count and NULL arguments
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    ids = np.zeros((2, 20), np.int64); sc = np.zeros((2, 20), np.float32)
    call = L.lib().cmr_index_search_masked_each
    nw = words.shape[1]
    for bad in (nw - 1, nw + 1, 0):
        assert call(idx._h, p(Q), 2, 20, p(words), bad, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), 2, 20, None, nw, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, None, 2, 20, p(words), nw, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), 2, 20, p(words), nw, None, p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), 2, 20, p(words), nw, p(ids), p(sc), None, None) == L.CMR_OK
    # Python: masks must be [nq, n_words]
    for bad in (words[0], words[:1], words[:, :-1], np.concatenate([words, words])):
        with pytest.raises(ValueError):
            idx.search_filtered_each(Q, 20, masks=bad)
    with pytest.raises(ValueError):
        idx.search_filtered_each(Q, 20, masks=words, allow=[[1], [2]])
    bad_q = Q.copy()
    bad_q[1, 3] = np.nan
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_each(bad_q, 20, masks=words)
    assert e.value.code == L.CMR_ERR_NONFINITE
    got = idx.search_filtered_each(Q, 20, masks=words)          # the flag is re-armed: the next call is served
    for i in range(2):
        want = idx.search_filtered(Q[i:i + 1], 20, mask=words[i])
        assert np.array_equal(got[0][i], want[0][0]) and np.array_equal(_bits(got[1][i]), _bits(want[1][0]))
    assert idx.get_option("combine_filtered") == 0              # a known option, off by default
    with pytest.raises(L.CmrError):
        idx.set_option("combine_filtered", 2)


def test_retrieval_sibling_with_a_pool_per_question():
    from comorag_amd.retrieval import dense_passage_topk, dense_passage_topk_filtered_each
    dtype, n, k = "bf16", 1000, 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:4]
    top_ids, _ = dense_passage_topk(idx, Q, k)
    pools = [np.unique(top_ids[i, : 3 + 2 * i]) for i in range(4)]          # every question's pool holds some of ITS best rows
    ids, sc = dense_passage_topk_filtered_each(idx, Q, k, exclude_rows=pools)
    assert ids.shape == (4, k)
    for i in range(4):
        assert not np.isin(ids[i], pools[i]).any()
    raw = idx.search_filtered_each(Q, k, exclude=pools)
    assert np.array_equal(ids, raw[0])
    assert np.allclose(sc, (raw[1] - raw[2][:, None]) / (raw[3] - raw[2])[:, None]) and (sc <= 1).all() and (sc >= 0).all()
    allow = [np.flatnonzero(~np.isin(np.arange(n), pools[i])) for i in range(4)]
    ids2, sc2 = dense_passage_topk_filtered_each(idx, Q, k, allow_rows=allow)
    assert np.array_equal(ids2, ids) and np.array_equal(sc2, sc)
