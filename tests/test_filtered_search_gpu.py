"""Filtered search (cmr_index_search_masked*): the result is bit for bit what `search` returns on a second index that
holds only the allowed rows, ids mapped back — ids, score bits, min and max, no tolerance.  The oracle uses only calls that existed
before the feature.  Corpora and indexes are built once per module."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_mask

pytestmark = pytest.mark.gpu

CHAIN, FILTERED, MORE_PASSES = 3, 1 << 12, 1 << 11
N_ONE_LEVEL = 8192 + 5          # 257 panels: one sampling level (npanels >= 256)
N_TWO_LEVELS = 131072 + 7       # 4097 panels: two levels (npanels >= 4096) — or the single 128-panel level of a small batch
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


def _oracle(dtype, n, keep, Q, k):
    """`search` on an index of the allowed rows alone, ids mapped back to the original rows"""
    from comorag_amd.index import DenseIndex
    nq = len(Q)
    rows = np.flatnonzero(keep)
    if len(rows) == 0:
        return (np.empty((nq, 0), np.int64), np.empty((nq, 0), np.float32), np.full(nq, np.inf, np.float32), np.full(nq, -np.inf, np.float32))
    ref = DenseIndex(SHAPES[dtype], dtype)
    try:
        ref.append(_rows(dtype, n)[0][rows])
        ids, sc, mn, mx = ref.search(Q, k)
    finally:
        ref.close()
    return rows[ids], sc, mn, mx


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(dtype, n, keep, nq, k, base=0):
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    got = idx.search_filtered(Q, k, allow=keep)
    want = _oracle(dtype, n, keep, Q, k)
    what = f"{dtype} n={n} nq={nq} k={k} allowed={int(keep.sum())}"
    assert got[0].shape == want[0].shape == (nq, min(k, int(keep.sum()))), what
    assert np.array_equal(got[0], want[0] + base), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(_bits(got[3]), _bits(want[3])), what
    return idx.get_option("last_route")


def _masks(n, rng):
    """the simple and sparse masks of the issue's table that make sense at n rows"""
    m = {"all-ones": np.ones(n, bool), "all-zeros": np.zeros(n, bool)}
    one = np.zeros(n, bool); one[n // 2] = True
    m["one-row"] = one
    if n % 32:
        tail = np.zeros(n, bool); tail[n - n % 32:] = True
        m["last-partial-panel"] = tail
    m["every-other-row"] = np.arange(n) % 2 == 0
    m["alternating-panels"] = (np.arange(n) // 32) % 2 == 1
    if n >= 5:
        five = np.zeros(n, bool); five[rng.choice(n, 5, replace=False)] = True
        m["five-rows"] = five
    m["random-0.5"] = rng.random(n) < 0.5
    m["random-0.01"] = rng.random(n) < 0.01
    return m


# (nq, k) pairs that together hold every nq and every k of the table; a list of masks walks through them
COMBOS = [(1, 20), (8, 1), (33, 33), (64, 128), (65, 20), (1, 128), (8, 33), (33, 1), (65, 128), (64, 20)]


@pytest.mark.parametrize("n", [1, 31, 32, 33])
def test_tiny_corpora_every_mask(n):
    rng = np.random.default_rng(n)
    for i, (name, keep) in enumerate(_masks(n, rng).items()):
        for nq, k in (COMBOS[i % len(COMBOS)], (1, 1), (8, 20)):
            r = _check("bf16", n, keep, nq, k)
            assert r & 0xF == CHAIN and r & FILTERED and (r >> 4) & 3 == 0, (name, hex(r))


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_partial_last_panel_every_mask_nq_and_k(dtype):
    n = 1000
    rng = np.random.default_rng(7)
    for i, (name, keep) in enumerate(_masks(n, rng).items()):
        for nq, k in (COMBOS[i % len(COMBOS)], COMBOS[(i + 5) % len(COMBOS)]):
            r = _check(dtype, n, keep, nq, k)
            assert r & 0xF == CHAIN and r & FILTERED, (name, hex(r))
            assert bool(r & MORE_PASSES) == (nq > 64), (name, hex(r))


def _adversarial(dtype, n, nq, k):
    """exactly the unfiltered top-k of every query masked out: the result must be the next k"""
    ids = _index(dtype, n).search(_rows(dtype, n)[1][:nq], k)[0]
    keep = np.ones(n, bool)
    keep[np.unique(ids)] = False
    return keep


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_one_sampling_level(dtype):
    n = N_ONE_LEVEL
    rng = np.random.default_rng(11)
    masks = _masks(n, rng)
    for i, name in enumerate(["all-ones", "random-0.5", "random-0.01", "alternating-panels", "every-other-row", "five-rows", "last-partial-panel", "all-zeros"]):
        nq, k = COMBOS[i % len(COMBOS)]
        r = _check(dtype, n, masks[name], nq, k)
        assert r & 0xF == CHAIN and r & FILTERED and (r >> 4) & 3 == 1, (name, hex(r))      # the sampling level is there
    for nq, k in ((1, 20), (8, 20), (33, 33), (65, 128)):
        _check(dtype, n, _adversarial(dtype, n, nq, k), nq, k)


@pytest.mark.parametrize("nq,k,levels,tau_in_scan,single", [(1, 20, 1, True, True), (8, 20, 1, False, True), (33, 20, 2, False, False), (8, 33, 2, False, False),
                                                            (64, 128, 2, False, False)])
def test_two_level_corpus(nq, k, levels, tau_in_scan, single):
    """4097 panels: one or two queries derive the thresholds inside the main scan, up to eight take the single 128-panel level, everything
    else samples in two levels — every one of them with the mask, or an unmasked row's score becomes the threshold and allowed rows vanish"""
    dtype, n = "bf16", N_TWO_LEVELS
    rng = np.random.default_rng(13)
    few = np.zeros(n, bool); few[rng.choice(n, 3 * k, replace=False)] = True      # a sample holds fewer than k allowed rows: no threshold
    masks = {"all-ones": np.ones(n, bool), "random-0.5": rng.random(n) < 0.5, "random-0.01": rng.random(n) < 0.01, "3k-rows": few,
             "adversarial": _adversarial(dtype, n, nq, k)}
    for name, keep in masks.items():
        r = _check(dtype, n, keep, nq, k)
        assert r & 0xF == CHAIN and r & FILTERED, (name, hex(r))
        assert ((r >> 4) & 3, bool(r >> 6 & 1), bool(r >> 7 & 1)) == (levels, tau_in_scan, single), (name, hex(r))


@pytest.mark.parametrize("dtype,n,nq,k", [("bf16", 1000, 8, 20), ("f32", N_ONE_LEVEL, 33, 33), ("bf16", N_TWO_LEVELS, 1, 20), ("bf16", N_TWO_LEVELS, 65, 128)])
def test_all_ones_mask_is_the_unfiltered_search(dtype, n, nq, k):
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    want = idx.search(Q, k)
    got = idx.search_filtered(Q, k)
    assert np.array_equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(_bits(a), _bits(b))
    assert idx.get_option("last_route") & FILTERED


def test_ties_come_out_id_ascending_among_the_allowed_rows():
    from comorag_amd.index import DenseIndex
    dtype, n, k = "bf16", 1000, 20
    X, Q = _rows(dtype, n)
    X = X.copy()
    dup = np.array([3, 40, 41, 500, 731, 998, 999])
    X[dup] = X[17]                                   # eight rows with one score per query
    Q = np.concatenate([X[17:18], Q[:7]])
    keep = np.ones(n, bool)
    keep[[17, 41, 998]] = False                      # some of the duplicates are masked
    idx, ref = DenseIndex(SHAPES[dtype], dtype), DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X)
        ref.append(X[keep])
        got = idx.search_filtered(Q, k, allow=keep)
        want = ref.search(Q, k)
    finally:
        idx.close(); ref.close()
    assert np.array_equal(got[0], np.flatnonzero(keep)[want[0]]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert got[0][0, :5].tolist() == [3, 40, 500, 731, 999]          # the query IS the duplicated row: its allowed copies lead, ids ascending
    assert len(np.unique(_bits(got[1][0, :5]))) == 1


def test_id_base_moves_the_ids_and_not_the_mask():
    from comorag_amd.index import DenseIndex
    dtype, n, nq, k, base = "f16", 1000, 8, 20, 5000
    X, Q = _rows(dtype, n)
    keep = np.random.default_rng(3).random(n) < 0.5
    idx = DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X)
        idx.set_id_base(base)
        got = idx.search_filtered(Q[:nq], k, allow=keep)
        ex = idx.search_filtered(Q[:nq], k, exclude=np.flatnonzero(~keep))
    finally:
        idx.close()
    want = _oracle(dtype, n, keep, Q[:nq], k)
    assert np.array_equal(got[0], want[0] + base) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(_bits(got[3]), _bits(want[3]))
    assert np.array_equal(ex[0], got[0]) and np.array_equal(_bits(ex[1]), _bits(got[1]))


@pytest.mark.parametrize("n,nq,k,p", [(1000, 8, 20, 0.5), (N_ONE_LEVEL, 65, 33, 0.01), (N_TWO_LEVELS, 1, 20, 0.5)])
def test_dev_form_equals_host_form(n, nq, k, p):
    import torch
    dtype = "bf16"
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    keep = np.random.default_rng(n).random(n) < p
    words = pack_row_mask(n, allow=keep)
    host = idx.search_filtered(Q, k, mask=words, with_minmax=True)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(Q).to(dev)
    m_t = torch.from_numpy(words.view(np.int32)).to(dev)
    mn_t = torch.empty(nq, dtype=torch.float32, device=dev)
    mx_t = torch.empty(nq, dtype=torch.float32, device=dev)
    ids_t, sc_t = idx.search_filtered_dev(q_t, k, m_t, out_min=mn_t, out_max=mx_t)
    torch.cuda.synchronize(dev)
    kk = host[0].shape[1]
    ids, sc = ids_t.cpu().numpy(), sc_t.cpu().numpy()
    assert np.array_equal(ids[:, :kk], host[0]) and np.array_equal(_bits(sc[:, :kk]), _bits(host[1]))
    assert (ids[:, kk:] == -1).all() and np.isneginf(sc[:, kk:]).all()
    assert np.array_equal(_bits(mn_t.cpu().numpy()), _bits(host[2])) and np.array_equal(_bits(mx_t.cpu().numpy()), _bits(host[3]))
    assert not idx.query_status()


def test_short_lists_are_padded_and_an_empty_mask_is_ok():
    """the C call itself: fewer than k allowed rows pad with -1 / -inf; none allowed is CMR_OK, all padding, min +inf, max -inf"""
    dtype, n, nq, k = "bf16", 1000, 3, 20
    idx = _index(dtype, n)
    Q = np.ascontiguousarray(_rows(dtype, n)[1][:nq])
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    for rows in ([5, 64, 65, 300, 999], []):
        words = pack_row_mask(n, allow=rows)
        ids = np.zeros((nq, k), np.int64); sc = np.zeros((nq, k), np.float32)
        mn = np.zeros(nq, np.float32); mx = np.zeros(nq, np.float32)
        assert L.lib().cmr_index_search_masked(idx._h, p(Q), nq, k, p(words), len(words), p(ids), p(sc), p(mn), p(mx)) == L.CMR_OK
        assert (np.sort(ids[:, :len(rows)], axis=1) == np.array(rows, np.int64)).all()
        assert (ids[:, len(rows):] == -1).all() and np.isneginf(sc[:, len(rows):]).all()
        if rows:
            assert np.array_equal(_bits(mn), _bits(sc[:, len(rows) - 1])) and np.array_equal(_bits(mx), _bits(sc[:, 0]))
        else:
            assert np.isposinf(mn).all() and np.isneginf(mx).all()


def test_other_calls_return_what_they_returned_before():
    import torch
    dtype, n, nq, k = "bf16", N_ONE_LEVEL, 8, 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(Q).to(dev)

    def others():
        ids_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
        sc_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        idx.sync(idx.search_pipelined(q_t, k, ids_t, sc_t))
        return [*idx.search(Q, k), idx.scores(Q), ids_t.cpu().numpy(), sc_t.cpu().numpy()]

    before = others()
    rng = np.random.default_rng(5)
    for p_keep in (0.5, 0.01, 0.0):
        idx.search_filtered(Q, k, allow=rng.random(n) < p_keep)
    idx.search_filtered(_rows(dtype, n)[1], 128, allow=rng.random(n) < 0.5)
    after = others()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert not idx.get_option("last_route") & FILTERED


def test_error_paths():
    dtype, n = "bf16", 1000
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:2].copy()
    words = pack_row_mask(n)
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered(Q, 129, mask=words)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED
    for bad in (words[:-1], np.concatenate([words, words[:1]])):
        with pytest.raises(L.CmrError) as e:
            idx.search_filtered(Q, 20, mask=bad)
        assert e.value.code == L.CMR_ERR_INVALID
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered(Q, 0, mask=words)
    assert e.value.code == L.CMR_ERR_INVALID
    bad_q = Q.copy()
    bad_q[1, 3] = np.nan
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered(bad_q, 20, mask=words)
    assert e.value.code == L.CMR_ERR_NONFINITE
    got = idx.search_filtered(Q, 20, mask=words)          # the flag is re-armed: the next call is served
    want = idx.search(Q, 20)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_retrieval_sibling_of_dense_passage_topk():
    from comorag_amd.retrieval import dense_passage_topk, dense_passage_topk_filtered
    dtype, n, k = "bf16", 1000, 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:4]
    top_ids, _ = dense_passage_topk(idx, Q, k)
    pool = np.unique(top_ids[:, :5])                     # rows already in the pool
    ids, sc = dense_passage_topk_filtered(idx, Q, k, exclude_rows=pool)
    assert ids.shape == (4, k) and not np.isin(ids, pool).any()
    raw = idx.search_filtered(Q, k, exclude=pool)
    assert np.array_equal(ids, raw[0])
    assert np.allclose(sc, (raw[1] - raw[2][:, None]) / (raw[3] - raw[2])[:, None]) and (sc <= 1).all() and (sc >= 0).all()
    ids2, _ = dense_passage_topk_filtered(idx, Q, k, allow_rows=np.flatnonzero(~np.isin(np.arange(n), pool)))
    assert np.array_equal(ids2, ids)
