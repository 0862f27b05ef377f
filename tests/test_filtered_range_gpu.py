"""Filtered score-bound searches (range_search_filtered*, range_count_filtered*, search_min_score_filtered*) on one
index and across shards.  No oracle is the code under test:
  (A) the UNFILTERED range_search of the same index with the entries of disallowed rows dropped per list (fm.drop), compared with
      ri.same — lims, ids and the fp32 score words;
  (B) ri.oracle on scores() restricted to a query's allowed rows, which must agree with (A);
  (C) the counts are np.diff(lims);
  (D) for the threshold search, search_filtered / _each / _ids of the same k and allow set with the entries below float32(b) padded
      (fm.pad_below), k = 20 and k = 128.
Cases: tests/range_inputs.py (family C of tests/threshold_inputs.py); masks and helpers: tests/filtered_range_model.py, checked without a
device in tests/test_filtered_range_host.py."""
import ctypes as C
import threading

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_masks
from oracle import retrieval_np as orc
from tests import filtered_ids_model as im
from tests import filtered_range_model as fm
from tests import range_inputs as ri

pytestmark = pytest.mark.gpu

INF = float("inf")
TAGS = ["c64-3-bf16", "c64-40-f16", "c64-40-f32", "c768-bf16", "c200-f32"]
KS = (20, 128)


class Case:
    pass


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c.idx.close()
    _CASES.clear()


def _index(d, dtype, X, **opts):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(d, dtype, options=opts)
    if len(X):
        idx.append(X)
    return idx


def _case(tag):
    """the case's index, its scores S, its attained bound, its mask family with the rows every mask allows, and the unfiltered range
    search of every bound — oracle inputs, computed once and never changed"""
    if tag in _CASES:
        return _CASES[tag]
    c = Case()
    c.tag = tag
    c.dtype, c.d, c.n, c.nq, c.seed = ri.CASES[tag]
    c.X, c.Q, c.q_dup, c.info = ri.make(tag)
    c.idx = _index(c.d, c.dtype, c.X)
    c.S = c.idx.scores(c.Q)
    c.S.setflags(write=False)
    c.tied = c.info["tied"]
    c.b_dup = float(c.S[c.q_dup, c.tied[0]])
    c.bounds = ri.bounds(c.b_dup)
    c.M = fm.family(c.n, c.tied, c.seed)
    c.rows = [fm.rows_of(m, c.n) for m in c.M]
    c.Mq = fm.per_query(c.M, c.nq)
    c.rows_q = [c.rows[i % 7] for i in range(c.nq)]
    c.plain = {b: c.idx.range_search(c.Q, b) for b in c.bounds}
    _CASES[tag] = c
    return c


def _route(idx):
    return idx.get_option("last_route")


def _oracle_b(S, b, rows_q, names=None):
    """(B): ri.oracle per query on the scores of its allowed rows, lists concatenated"""
    parts = [ri.oracle(S[i:i + 1][:, rows], b, ids=rows if names is None else names[rows]) for i, rows in enumerate(rows_q)]
    lims = np.concatenate([[0], np.cumsum([p[0][1] for p in parts])]).astype(np.int64)
    return lims, np.concatenate([p[1] for p in parts]).astype(np.int64), np.concatenate([p[2] for p in parts]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1: range, every case x bound x mask
@pytest.mark.parametrize("tag", TAGS)
def test_range_lists_and_counts_equal_the_oracles(tag):
    c = _case(tag)
    for b in c.bounds:
        for m in range(fm.N_FAMILY):      # one mask for every query
            got = c.idx.range_search_filtered(c.Q, b, c.M[m])
            assert _route(c.idx) & 0xF == fm.ROUTE_RANGE and _route(c.idx) & (fm.FILTERED | fm.FILTERED_EACH | fm.FILTERED_IDS) == fm.FILTERED
            want = fm.drop(c.plain[b], c.rows[m])
            ri.same(got, want, (tag, b, m, "A"))
            ri.same(ri.oracle(c.S[:, c.rows[m]], b, ids=c.rows[m]), want, (tag, b, m, "B agrees with A"))
            assert np.array_equal(c.idx.range_count_filtered(c.Q, b, c.M[m]), np.diff(want[0])), (tag, b, m, "C")
        ri.same(c.idx.range_search_filtered(c.Q, b, c.M[0]), c.plain[b], (tag, b, "all ones, garbage beyond n: the unfiltered call"))
        assert not c.idx.range_search_filtered(c.Q, b, c.M[1])[0].any()
        # a mask per query: query i takes mask i mod 7
        got = c.idx.range_search_filtered(c.Q, b, c.Mq)
        if c.nq > 1:
            assert _route(c.idx) & (fm.FILTERED | fm.FILTERED_EACH | fm.FILTERED_IDS) == fm.FILTERED | fm.FILTERED_EACH
        want = fm.drop(c.plain[b], c.rows_q)
        ri.same(got, want, (tag, b, "each", "A"))
        if b in (c.b_dup, 0.0, -INF, INF):
            ri.same(_oracle_b(c.S, b, c.rows_q), want, (tag, b, "each", "B agrees with A"))
        assert np.array_equal(c.idx.range_count_filtered(c.Q, b, c.Mq), np.diff(want[0])), (tag, b, "each", "C")
    # not vacuous: the attained bound keeps the tied rows a mask allows; -inf is every allowed row; a query that allows nothing sits between
    # neighbours with thousands of hits
    cnt = np.diff(c.idx.range_search_filtered(c.Q, c.b_dup, c.M[7])[0])
    assert cnt[c.q_dup] == np.diff(c.plain[c.b_dup][0])[c.q_dup] - 1
    lst = ri.lists(c.idx.range_search_filtered(c.Q, c.b_dup, c.M[3]))[c.q_dup]
    assert lst[0].tolist() == [c.tied[1]]
    assert np.diff(c.idx.range_search_filtered(c.Q, -INF, c.Mq)[0]).tolist() == [len(r) for r in c.rows_q]
    each0 = np.diff(c.idx.range_search_filtered(c.Q, 0.0, c.Mq)[0])
    assert each0[1] == 0 and each0[0] > ri.TILE and each0[2] > 500


# ---------------------------------------------------------------------------------------------- 2: threshold, every case x bound x mask
@pytest.mark.parametrize("tag", TAGS)
def test_threshold_rows_equal_the_padded_filtered_search(tag):
    c = _case(tag)
    for k in KS:
        shared = [c.idx.search_filtered(c.Q, k, c.M[m], with_minmax=False)[:2] for m in range(fm.N_FAMILY)]
        each = c.idx.search_filtered_each(c.Q, k, c.Mq, with_minmax=False)[:2]
        for b in c.bounds:
            for m in range(fm.N_FAMILY):
                got = c.idx.search_min_score_filtered(c.Q, k, b, c.M[m])
                fm.same_rows(got, fm.pad_below(*shared[m], b, k), (tag, k, b, m))
            r = _route(c.idx)
            assert r & 0xF == fm.ROUTE_CHAIN and r & fm.THRESHOLD and r & (fm.FILTERED | fm.FILTERED_EACH | fm.FILTERED_IDS) == fm.FILTERED
            got = c.idx.search_min_score_filtered(c.Q, k, b, c.Mq)
            fm.same_rows(got, fm.pad_below(*each, b, k), (tag, k, b, "each"))
            if c.nq > 1:
                assert _route(c.idx) & (fm.THRESHOLD | fm.FILTERED | fm.FILTERED_EACH) == fm.THRESHOLD | fm.FILTERED | fm.FILTERED_EACH
    # the first min(k, count) entries of the filtered range list
    for b in (c.b_dup, 0.8, 0.0):
        lims, ids, sc = c.idx.range_search_filtered(c.Q, b, c.Mq)
        t_ids, t_sc = c.idx.search_min_score_filtered(c.Q, 128, b, c.Mq)
        for i in range(c.nq):
            m = min(128, int(lims[i + 1] - lims[i]))
            assert np.array_equal(ids[lims[i]:lims[i] + m], t_ids[i, :m]) and np.all(t_ids[i, m:] == -1), (tag, b, i)
            assert np.array_equal(sc[lims[i]:lims[i] + m].view(np.uint32), t_sc[i, :m].view(np.uint32)), (tag, b, i)


# ---------------------------------------------------------------------------------------------- 3: words forms against id forms
def _exclude_lists(c, k=20):
    """the -1 padded int64 results of an earlier search, as tri_retrieve's pool holds them: query i excludes its own best k, the tail of
    every third row already padding"""
    ex = c.idx.search_min_score(c.Q, k, 0.0)[0].copy()
    ex[::3, k // 2:] = -1
    return ex


@pytest.mark.parametrize("tag", ["c64-3-bf16", "c64-40-f16", "c768-bf16"])
def test_id_forms_equal_the_words_forms(tag):
    c = _case(tag)
    ex = _exclude_lists(c)
    assert (ex == -1).any() and (ex >= 0).any() and ex.dtype == np.int64
    Mx = pack_row_masks(c.n, exclude=[row[row >= 0] for row in ex])
    keep_q = [fm.rows_of(m, c.n) for m in Mx]
    # a shared allow list with duplicates, padding, ids the index does not hold
    allow = np.concatenate([c.rows[6], c.rows[6][:5], [-1, -7, c.n, c.n + 31, 10 ** 12], c.tied]).astype(np.int64)
    Ma = fm.words_of(c.n, np.union1d(c.rows[6], c.tied))
    for b in (c.b_dup, 0.8, 0.0, -0.9, -INF, INF):
        got = c.idx.range_search_filtered_ids(c.Q, b, exclude=ex)
        r = _route(c.idx)
        assert r & 0xF == fm.ROUTE_RANGE and r & fm.FILTERED and r & fm.FILTERED_IDS and r & fm.FILTERED_EACH
        ri.same(got, c.idx.range_search_filtered(c.Q, b, Mx), (tag, b, "exclude, per query: words"))
        ri.same(got, fm.drop(c.plain[b], keep_q), (tag, b, "exclude, per query: A"))
        assert np.array_equal(c.idx.range_count_filtered_ids(c.Q, b, exclude=ex), np.diff(got[0]))
        got = c.idx.range_search_filtered_ids(c.Q, b, allow=allow)
        r = _route(c.idx)
        assert r & fm.FILTERED and r & fm.FILTERED_IDS and not r & fm.FILTERED_EACH
        ri.same(got, c.idx.range_search_filtered(c.Q, b, Ma), (tag, b, "allow, shared: words"))
        ri.same(got, fm.drop(c.plain[b], np.union1d(c.rows[6], c.tied)), (tag, b, "allow, shared: A"))
        assert np.array_equal(c.idx.range_count_filtered_ids(c.Q, b, allow=allow), np.diff(got[0]))
        for k in KS:
            got = c.idx.search_min_score_filtered_ids(c.Q, k, b, exclude=ex)
            r = _route(c.idx)
            assert r & 0xF == fm.ROUTE_CHAIN and r & fm.THRESHOLD and r & fm.FILTERED_IDS and r & fm.FILTERED_EACH
            fm.same_rows(got, c.idx.search_min_score_filtered(c.Q, k, b, Mx), (tag, b, k, "words"))
            fm.same_rows(got, fm.pad_below(*c.idx.search_filtered_ids(c.Q, k, exclude=ex, with_minmax=False)[:2], b, k), (tag, b, k, "D"))
            got = c.idx.search_min_score_filtered_ids(c.Q, k, b, allow=allow)
            fm.same_rows(got, fm.pad_below(*c.idx.search_filtered_ids(c.Q, k, allow=allow, with_minmax=False)[:2], b, k), (tag, b, k, "D, shared"))
    # the empty lists: exclude nothing = the unfiltered call, allow nothing = empty lists
    ri.same(c.idx.range_search_filtered_ids(c.Q, 0.0, exclude=[]), c.plain[0.0])
    assert not c.idx.range_search_filtered_ids(c.Q, -INF, allow=[])[0].any()
    if c.nq > 64:      # per-query lists never hold more than 64 queries' words: two blocks here
        c.idx.range_search_filtered_ids(c.Q, 0.0, exclude=ex)
        assert c.idx.get_option("range_blocks_last") == 2
        c.idx.range_search_filtered(c.Q, 0.0, Mx)
        assert c.idx.get_option("range_blocks_last") == 1


# ---------------------------------------------------------------------------------------------- 4: forced blocks and groups
def test_forced_blocks_and_groups_give_the_same_bits():
    c = _case("c768-bf16")
    idx = _index(c.d, c.dtype, c.X, range_block_queries=7, range_scratch_hits=3000)
    ex = _exclude_lists(c)
    for b in (0.0, c.b_dup, 0.8, -INF):
        for masks in (c.Mq, c.M[5], c.M[4]):
            want = c.idx.range_search_filtered(c.Q, b, masks)
            ri.same(idx.range_search_filtered(c.Q, b, masks), want, (b, masks.shape))
            assert idx.get_option("range_blocks_last") == 10
            assert np.array_equal(idx.range_count_filtered(c.Q, b, masks), np.diff(want[0]))
        want = c.idx.range_search_filtered_ids(c.Q, b, exclude=ex)
        ri.same(idx.range_search_filtered_ids(c.Q, b, exclude=ex), want, (b, "ids"))
        assert idx.get_option("range_blocks_last") == 10
        assert np.array_equal(idx.range_count_filtered_ids(c.Q, b, exclude=ex), np.diff(want[0]))
    # several groups in a block: with the random half every list at 0.0 holds ~2000 hits, one group each
    idx.range_search_filtered(c.Q, 0.0, c.M[5])
    assert idx.get_option("range_groups_last") == c.nq
    idx.range_search_filtered(c.Q, 0.0, c.Mq)
    assert 10 < idx.get_option("range_groups_last") <= c.nq
    idx.close()


# ---------------------------------------------------------------------------------------------- 5: id base
def test_id_base_words_stay_local_ids_shift():
    c = _case("c64-40-f16")
    idx = _index(c.d, c.dtype, c.X)
    idx.set_id_base(1000)
    names = np.arange(c.n, dtype=np.int64) + 1000
    ex = _exclude_lists(c)
    for b in (c.b_dup, 0.0, -INF):
        plain = idx.range_search(c.Q, b)
        ri.same(plain, ri.oracle(c.S, b, names))
        ri.same(idx.range_search_filtered(c.Q, b, c.Mq), fm.drop(plain, [names[r] for r in c.rows_q]), (b, "words are local"))
        ri.same(idx.range_search_filtered(c.Q, b, c.Mq), _oracle_b(c.S, b, c.rows_q, names), (b, "B"))
        # ids go in as they come out: the un-based lists name other rows (or none) now
        got = idx.range_search_filtered_ids(c.Q, b, exclude=ex + 1000 * (ex >= 0))
        want = im.words_of(c.n, c.nq, "exclude", np.arange(c.nq + 1) * ex.shape[1], (ex + 1000 * (ex >= 0)).reshape(-1), base=1000)
        ri.same(got, fm.drop(plain, [names[fm.rows_of(w, c.n)] for w in want]), (b, "ids"))
        ri.same(got, fm.drop(plain, [names[np.setdiff1d(np.arange(c.n), row[row >= 0])] for row in ex]), (b, "ids, by hand"))
        t = idx.search_min_score_filtered_ids(c.Q, 20, b, allow=names[c.rows[5]])
        fm.same_rows(t, fm.pad_below(*idx.search_filtered(c.Q, 20, c.M[5], with_minmax=False)[:2], b, 20), (b, "threshold"))
        assert t[0].max() >= 1000
    idx.close()


# ---------------------------------------------------------------------------------------------- 6: max_total
def test_max_total_is_judged_on_the_filtered_total():
    c = _case("c64-40-f16")
    want = c.idx.range_search_filtered(c.Q, 0.3, c.M[5])
    total, unfiltered = int(want[0][-1]), int(c.plain[0.3][0][-1])
    assert 300 < total < unfiltered - 300
    for idx in (c.idx, _index(c.d, c.dtype, c.X, range_block_queries=16)):
        ri.same(idx.range_search_filtered(c.Q, 0.3, c.M[5], max_total=total), want)          # exactly at the limit, far below the unfiltered total
        for call in (lambda: idx.range_search_filtered(c.Q, 0.3, c.M[5], max_total=total - 1),
                     lambda: idx.range_search_filtered_ids(c.Q, 0.3, allow=c.rows[5], max_total=total - 1)):
            with pytest.raises(L.CmrError) as e:
                call()
            assert e.value.code == L.CMR_ERR_UNSUPPORTED and str(total) in str(e.value) and str(unfiltered) not in str(e.value), str(e.value)
        ri.same(idx.range_search_filtered_ids(c.Q, 0.3, allow=c.rows[5], max_total=total), want)      # and the index still answers
        assert idx.range_count_filtered(c.Q, 0.3, c.M[5]).sum() == total                              # the count has no limit
        if idx is not c.idx:
            idx.close()


# ---------------------------------------------------------------------------------------------- 7: argument errors that need the index
def test_errors_that_need_the_index():
    c = _case("c64-3-bf16")
    lib = L.lib()
    nw = fm.n_words(c.n)
    out = np.zeros((c.nq, 4), np.int64)
    outf = np.zeros((c.nq, 4), np.float32)
    q, h = c.Q, c.idx._h
    for words in (np.zeros(nw - 1, np.uint32), np.zeros(nw + 1, np.uint32), np.zeros((c.nq, nw + 1), np.uint32)):
        for call in (c.idx.range_search_filtered, c.idx.range_count_filtered, lambda q_, b_, w_: c.idx.search_min_score_filtered(q_, 4, b_, w_)):
            with pytest.raises(ValueError):
                call(c.Q, 0.0, words)
    w = np.zeros(nw + 1, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    res = C.c_void_p()
    assert lib.cmr_index_range_search_masked(h, p(q), c.nq, 0.0, 0, p(w), nw + 1, 1, C.byref(res)) == L.CMR_ERR_INVALID and b"n_words" in lib.cmr_last_error()
    assert not res.value
    assert lib.cmr_index_range_count_masked(h, p(q), c.nq, 0.0, p(w), nw - 1, 1, p(out)) == L.CMR_ERR_INVALID and b"n_words" in lib.cmr_last_error()
    assert lib.cmr_index_search_min_score_masked(h, p(q), c.nq, 4, 0.0, p(w), nw + 1, 1, p(out), p(outf)) == L.CMR_ERR_INVALID and b"n_words" in lib.cmr_last_error()
    assert lib.cmr_index_range_count_masked(h, p(q), c.nq, 0.0, p(w), nw, 2, p(out)) == L.CMR_ERR_INVALID and b"n_masks" in lib.cmr_last_error()
    for call in (lambda b, q_=c.Q: c.idx.range_search_filtered(q_, b, c.M[5]), lambda b, q_=c.Q: c.idx.range_count_filtered_ids(q_, b, exclude=[3]),
                 lambda b, q_=c.Q: c.idx.search_min_score_filtered(q_, 20, b, c.M[5]), lambda b, q_=c.Q: c.idx.search_min_score_filtered_ids(q_, 20, b, allow=[3])):
        with pytest.raises(L.CmrError) as e:
            call(float("nan"))
        assert e.value.code == L.CMR_ERR_INVALID
        bad = c.Q.copy(); bad[1, 7] = np.inf
        with pytest.raises(L.CmrError) as e:
            call(0.0, bad)
        assert e.value.code == L.CMR_ERR_NONFINITE
    for call in (lambda: c.idx.search_min_score_filtered(c.Q, 129, 0.0, c.M[5]), lambda: c.idx.search_min_score_filtered_ids(c.Q, 129, 0.0, allow=[3])):
        with pytest.raises(L.CmrError) as e:
            call()
        assert e.value.code == L.CMR_ERR_UNSUPPORTED
    ri.same(c.idx.range_search_filtered(c.Q, 0.0, c.M[5]), fm.drop(c.plain[0.0], c.rows[5]))      # the index still answers


# ---------------------------------------------------------------------------------------------- 8: a few rows, no rows
@pytest.mark.parametrize("n", [0, 31, 33])
def test_few_rows(n):
    d, nq = 64, 3
    X = orc.synthetic_corpus(max(n, 1), d, seed=900 + n)[:n]
    Q = orc.synthetic_queries(nq, d, seed=901 + n)
    idx = _index(d, "bf16", X)
    M = fm.small_family(n, n)
    assert M.shape[1] == fm.n_words(n)
    S = idx.scores(Q) if n else np.empty((nq, 0), np.float32)
    best = float(S[0].max()) if n else 0.5
    Mq = np.ascontiguousarray(M[[4, 1, 3]])      # the random half, nothing, the last row alone
    for b in (-INF, best, 0.0, INF):
        plain = idx.range_search(Q, b)
        for m in range(len(M)):
            rows = fm.rows_of(M[m], n)
            got = idx.range_search_filtered(Q, b, M[m])
            ri.same(got, fm.drop(plain, rows), (n, b, m))
            if n:
                ri.same(got, ri.oracle(S[:, rows], b, ids=rows), (n, b, m, "B"))
            assert np.array_equal(idx.range_count_filtered(Q, b, M[m]), np.diff(got[0]))
            ri.same(idx.range_search_filtered_ids(Q, b, allow=rows), got, (n, b, m, "ids"))
            for k in KS:
                f = idx.search_filtered(Q, k, M[m], with_minmax=False)[:2] if n else (np.empty((nq, 0), np.int64), np.empty((nq, 0), np.float32))
                fm.same_rows(idx.search_min_score_filtered(Q, k, b, M[m]), fm.pad_below(*f, b, k), (n, b, m, k))
                fm.same_rows(idx.search_min_score_filtered_ids(Q, k, b, allow=rows), fm.pad_below(*f, b, k), (n, b, m, k, "ids"))
        ri.same(idx.range_search_filtered(Q, b, Mq), fm.drop(plain, [fm.rows_of(w, n) for w in Mq]), (n, b, "each"))
        ri.same(idx.range_search_filtered(Q, b, M[0]), plain)
    if n:
        assert np.diff(idx.range_search_filtered(Q, -INF, Mq)[0]).tolist() == [len(fm.rows_of(Mq[0], n)), 0, 1]
    idx.close()


# ---------------------------------------------------------------------------------------------- 9: after a removal and an update
def test_after_remove_ids_and_update_rows():
    c = _case("c64-40-f16")
    idx = _index(c.d, c.dtype, c.X)
    rng = np.random.default_rng(4191)
    gone = rng.choice(c.n, size=100, replace=False)
    assert idx.remove_ids(gone) == 100
    n2 = c.n - 100
    upd = rng.choice(n2, size=25, replace=False)
    assert idx.update_rows(upd, np.ascontiguousarray(c.X[rng.choice(c.n, size=25, replace=False)][:, ::-1])) == 25
    S2 = idx.scores(c.Q)
    assert S2.shape == (c.nq, n2) and fm.n_words(n2) != fm.n_words(c.n)
    M2 = np.stack([fm.words_of(n2, np.flatnonzero(rng.random(n2) < p)) for p in (0.5, 0.01, 0.9)] + [np.full(fm.n_words(n2), 0xFFFFFFFF, np.uint32)])
    Mq = fm.per_query(M2, c.nq, mod=4)
    rows_q = [fm.rows_of(w, n2) for w in Mq]
    with pytest.raises(ValueError):
        idx.range_search_filtered(c.Q, 0.0, c.M[5])          # words of the old row count
    for b in (0.8, 0.0, -INF):
        plain = idx.range_search(c.Q, b)
        ri.same(plain, ri.oracle(S2, b))
        got = idx.range_search_filtered(c.Q, b, Mq)
        ri.same(got, fm.drop(plain, rows_q), (b, "A"))
        ri.same(got, _oracle_b(S2, b, rows_q), (b, "B"))
        assert np.array_equal(idx.range_count_filtered(c.Q, b, Mq), np.diff(got[0]))
        ri.same(idx.range_search_filtered_ids(c.Q, b, allow=rows_q), got, (b, "ids"))
        for k in KS:
            fm.same_rows(idx.search_min_score_filtered(c.Q, k, b, Mq), fm.pad_below(*idx.search_filtered_each(c.Q, k, Mq, with_minmax=False)[:2], b, k), (b, k))
    idx.close()


# ---------------------------------------------------------------------------------------------- 10: shards
@pytest.mark.parametrize("S", [1, 2, 4])
def test_shards_equal_one_index(S):
    from comorag_amd.multi_index import MultiDeviceIndex
    c = _case("c64-40-f16")
    multi = MultiDeviceIndex(c.d, c.dtype, devices=[0] * S, options={"append_block_rows": 1024})
    multi.append(c.X)
    assert sum(multi.shard_rows()) == c.n and min(multi.shard_rows()) > 0
    ex = _exclude_lists(c)
    allow = np.concatenate([c.rows[5], [-1, c.n + 5]]).astype(np.int64)
    per_q = [c.rows[(i + 3) % 7] for i in range(c.nq)]      # ... with queries that allow nothing, one row, rows of one shard only
    for b in (c.b_dup, 0.8, 0.0, -INF, INF):
        for kw in (dict(exclude=ex), dict(allow=allow), dict(allow=per_q)):
            want = c.idx.range_search_filtered_ids(c.Q, b, **kw)
            ri.same(multi.range_search_filtered_ids(c.Q, b, **kw), want, (S, b, list(kw)))
            assert np.array_equal(multi.range_count_filtered_ids(c.Q, b, **kw), np.diff(want[0]))
            for k in KS:
                fm.same_rows(multi.search_min_score_filtered_ids(c.Q, k, b, **kw), c.idx.search_min_score_filtered_ids(c.Q, k, b, **kw), (S, b, k, list(kw)))
        ri.same(multi.range_search_filtered_ids(c.Q, b, allow=allow), fm.drop(c.plain[b], c.rows[5]), (S, b, "A"))
    want = c.idx.range_search_filtered_ids(c.Q, 0.3, allow=allow)
    total = int(want[0][-1])
    assert 300 < total < int(c.plain[0.3][0][-1])
    with pytest.raises(L.CmrError) as e:
        multi.range_search_filtered_ids(c.Q, 0.3, allow=allow, max_total=total - 1)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED and str(total) in str(e.value)
    ri.same(multi.range_search_filtered_ids(c.Q, 0.3, allow=allow, max_total=total), want)
    multi.close()


# ---------------------------------------------------------------------------------------------- 11: concurrency
def test_two_threads_with_different_masks():
    c = _case("c768-bf16")
    masks = [c.M[5], c.Mq]
    solo = [c.idx.range_search_filtered(c.Q, 0.0, m) for m in masks]
    ri.same(solo[0], fm.drop(c.plain[0.0], c.rows[5]))
    ri.same(solo[1], fm.drop(c.plain[0.0], c.rows_q))
    got, errs = [None] * 2, []
    start = threading.Barrier(2)

    def run(i):
        try:
            start.wait()
            for _ in range(3):
                got[i] = c.idx.range_search_filtered(c.Q, 0.0, masks[i])
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(2):
        ri.same(got[i], solo[i], i)


# ---------------------------------------------------------------------------------------------- 12: the unfiltered calls are what they were
def test_neighbours_within_with_id_lists():
    from comorag_amd.retrieval import neighbours_within
    c = _case("c64-40-f16")
    plain = neighbours_within(c.idx, c.Q, 0.8)
    assert _route(c.idx) & 0xF == fm.ROUTE_RANGE and not _route(c.idx) & (fm.FILTERED | fm.FILTERED_EACH | fm.FILTERED_IDS)
    for (ids, sc), (wi, ws) in zip(plain, ri.lists(c.plain[0.8])):
        assert np.array_equal(ids, wi) and np.array_equal(sc.view(np.uint32), ws.view(np.uint32))
    for kw, rows in ((dict(allow_ids=c.rows[5]), c.rows[5]), (dict(exclude_ids=c.rows[5]), np.setdiff1d(np.arange(c.n), c.rows[5]))):
        got = neighbours_within(c.idx, c.Q, 0.8, **kw)
        assert _route(c.idx) & 0xF == fm.ROUTE_RANGE and _route(c.idx) & fm.FILTERED_IDS
        for (ids, sc), (wi, ws) in zip(got, ri.lists(fm.drop(c.plain[0.8], rows))):
            assert np.array_equal(ids, wi) and np.array_equal(sc.view(np.uint32), ws.view(np.uint32))
