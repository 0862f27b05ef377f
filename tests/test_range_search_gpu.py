"""Range search (range_search / range_count: every row at or above a score bound, as CSR lists) on one index and across shards.  The
oracle of every comparison is the EXISTING all-scores call: with S = idx.scores(Q), list i is the rows with S[i] >= float32(b) in the
order of np.lexsort((rows, -S[i])), compared with np.array_equal on lims, ids and the score bits.  One anchor holds the lists against
the fp64 scores of the rounded operands under the project's tolerance.  Cases and oracle: tests/range_inputs.py; what they rely on is
checked without a device in tests/test_range_inputs.py."""
import threading

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc
from tests import range_inputs as ri
from tests import threshold_inputs as ti
from tests import value_domain_inputs as vd

pytestmark = pytest.mark.gpu

INF = float("inf")


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
    """the case's index, its scores S (the oracle's input: computed once, never changed) and its attained bound"""
    if tag in _CASES:
        return _CASES[tag]
    c = Case()
    c.tag = tag
    c.dtype, c.d, c.n, c.nq, c.seed = ri.CASES[tag]
    c.X, c.Q, c.q_dup, c.info = ri.make(tag)
    c.idx = _index(c.d, c.dtype, c.X)
    c.S = c.idx.scores(c.Q)
    c.S.setflags(write=False)
    tied = c.info["tied"]
    assert len(set(c.S[c.q_dup, tied].view(np.uint32).tolist())) == 1, "the four bit-equal rows must score alike"
    c.b_dup = float(c.S[c.q_dup, tied[0]])
    _CASES[tag] = c
    return c


def _range(idx, Q, b, **kw):
    got = idx.range_search(Q, b, **kw)
    if hasattr(idx, "get_option"):
        assert idx.get_option("last_route") & 0xF == ri.ROUTE_RANGE, hex(idx.get_option("last_route"))
    return got


# ---------------------------------------------------------------------------------------------- 1: the oracle on every shape
@pytest.mark.parametrize("tag", list(ri.CASES))
def test_lists_equal_the_oracle(tag):
    c = _case(tag)
    tied = c.info["tied"]
    counts = {}
    for b in ri.bounds(c.b_dup):
        got = _range(c.idx, c.Q, b)
        ri.same(got, ri.oracle(c.S, b), (tag, b))
        counts[b] = np.diff(got[0])
    b, b_up, b_down = ti.bounds_around(c.b_dup)[:3]
    # the attained bound keeps the four tied rows — the last four of their list, ascending —, the next fp32 value above drops exactly them
    lst = ri.lists(_range(c.idx, c.Q, b))[c.q_dup]
    assert lst[0][-4:].tolist() == tied and counts[b][c.q_dup] - counts[b_up][c.q_dup] == 4
    assert np.array_equal(counts[b], counts[b_down]) or np.any(c.S == np.float32(b_down))
    assert not counts[INF].any() and not counts[ti.FLT_MAX].any()
    assert counts[-INF].tolist() == [c.n] * c.nq == counts[-ti.FLT_MAX].tolist()
    # not vacuous: empty lists, lists beyond one selection list (128) and beyond one tile (2048 hits)
    assert (counts[0.8] == 0).any() and counts[0.0].min() > ri.TILE and counts[-0.9].min() >= c.n - 1 - ti.MEMBERS[1]
    if c.nq >= 5:
        assert counts[0.8][3] == 151


# ---------------------------------------------------------------------------------------------- 2: the anchor
@pytest.mark.parametrize("tag", ["c64-40-f16", "c768-bf16", "c200-f32"])
def test_lists_hold_the_fp64_sets_within_tolerance(tag):
    c = _case(tag)
    rnd = vd.ROUND[c.dtype]
    Xr, Qr = rnd(c.X), rnd(c.Q)
    exact = orc.exact_scores_f64(Xr, Qr)
    got = ri.lists(_range(c.idx, c.Q, 0.8))
    sizes = []
    for i in range(c.nq):
        tol = vd.row_tol(Qr[i], Xr)
        ids, sc = got[i]
        have = set(ids.tolist())
        assert set(np.flatnonzero(exact[i] >= 0.8 + tol).tolist()) <= have <= set(np.flatnonzero(exact[i] >= 0.8 - tol).tolist()), i
        assert np.all(np.abs(sc.astype(np.float64) - exact[i][ids]) <= tol[ids]) and np.all(sc >= np.float32(0.8))
        assert np.all(np.diff(sc) <= 0) and np.all(np.diff(ids)[np.diff(sc) == 0] > 0)
        sizes.append(len(ids))
    assert max(sizes) == 151 and min(sizes) == 0


# ---------------------------------------------------------------------------------------------- 3: the neighbouring calls
@pytest.mark.parametrize("tag", ["c64-3-bf16", "c64-40-f16", "c768-bf16", "c200-f32"])
def test_agrees_with_threshold_search_complete_ranking_and_counts(tag):
    import torch
    c = _case(tag)
    dev = torch.device("cuda", 0)
    qt = torch.from_numpy(c.Q).to(dev)
    torch.cuda.synchronize()
    for b in (c.b_dup, 0.8, 0.0, INF):
        lims, ids, sc = _range(c.idx, c.Q, b)
        cnt = np.diff(lims)
        t_ids, t_sc = c.idx.search_min_score(c.Q, ti.P_K, b)
        for i in range(c.nq):
            m = min(ti.P_K, int(cnt[i]))
            assert np.array_equal(ids[lims[i]:lims[i] + m], t_ids[i, :m]) and np.all(t_ids[i, m:] == -1), (tag, b, i)
            assert np.array_equal(sc[lims[i]:lims[i] + m].view(np.uint32), t_sc[i, :m].view(np.uint32)), (tag, b, i)
        assert np.array_equal(c.idx.range_count(c.Q, b), cnt)
        assert c.idx.get_option("last_route") & 0xF == ri.ROUTE_RANGE
        out = torch.full((c.nq,), -7, dtype=torch.int64, device=dev)
        c.idx.range_count_dev(qt, b, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), cnt)
    assert c.idx.query_status() is False
    # -inf: list i is row i of the complete ranking
    lims, ids, sc = _range(c.idx, c.Q, -INF)
    s_ids, s_sc = c.idx.sorted_scores(c.Q)[:2]
    assert lims.tolist() == [c.n * i for i in range(c.nq + 1)]
    assert np.array_equal(ids.reshape(c.nq, c.n), s_ids) and np.array_equal(sc.reshape(c.nq, c.n).view(np.uint32), s_sc.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 4: edges
@pytest.mark.parametrize("n", ti.FEW_ROWS)
def test_few_rows(n):
    d, nq = 64, 3
    X = orc.synthetic_corpus(n, d, seed=900 + n)
    Q = orc.synthetic_queries(nq, d, seed=901 + n)
    idx = _index(d, "bf16", X)
    S = idx.scores(Q)
    best = float(S[0].max())
    for b in (-INF, best, float(np.nextafter(np.float32(best), np.float32(INF))), 0.0, INF):
        got = _range(idx, Q, b)
        ri.same(got, ri.oracle(S, b), (n, b))
    assert np.diff(idx.range_search(Q, -INF)[0]).tolist() == [n] * nq and np.diff(idx.range_search(Q, best)[0])[0] >= 1
    assert np.array_equal(idx.range_count(Q, best), np.diff(idx.range_search(Q, best)[0]))
    idx.close()


def test_empty_index_nan_bound_and_nonfinite_query():
    idx = _index(64, "bf16", np.empty((0, 64), np.float32))
    Q = orc.synthetic_queries(3, 64, seed=5)
    lims, ids, sc = idx.range_search(Q, 0.5)
    assert lims.tolist() == [0, 0, 0, 0] and ids.shape == (0,) and sc.shape == (0,) and ids.dtype == np.int64 and sc.dtype == np.float32
    assert idx.range_count(Q, 0.5).tolist() == [0, 0, 0]
    idx.append(orc.synthetic_corpus(100, 64, seed=6))
    for call in (lambda q, b: idx.range_search(q, b), lambda q, b: idx.range_count(q, b)):
        with pytest.raises(L.CmrError) as e:
            call(Q, float("nan"))
        assert e.value.code == L.CMR_ERR_INVALID
        bad = Q.copy(); bad[1, 7] = np.inf
        with pytest.raises(L.CmrError) as e:
            call(bad, 0.0)
        assert e.value.code == L.CMR_ERR_NONFINITE
    ri.same(idx.range_search(Q, 0.0), ri.oracle(idx.scores(Q), 0.0))      # the index still answers
    idx.close()


@pytest.mark.parametrize("tag", ["c64-3-bf16", "c768-bf16"])
def test_id_base_and_block_table(tag):
    c = _case(tag)
    idx = _index(c.d, c.dtype, c.X)
    for base in (ti.ID_BASE, None):
        if base is not None:
            idx.set_id_base(base)
        else:
            idx.set_id_blocks(*ti.id_blocks(c.n))
        names = ti.map_ids(np.arange(c.n), c.n, base)
        for b in (c.b_dup, 0.8, 0.0, -INF):
            ri.same(_range(idx, c.Q, b), ri.oracle(c.S, b, names), (tag, base, b))
    idx.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_negative_zero_score_keeps_its_bits(dtype):
    z = ri.SIGNED_ZERO
    X, Q = ri.family_signed_zero()
    idx = _index(z["d"], dtype, X)
    S = idx.scores(Q)
    # An fp32 index accumulates by fused multiply-adds: the products of -1e-60 keep the sum at -0.0.  The 16-bit MFMA rounds every
    # product to -0.0 first and adds it to an accumulator that starts at +0.0: +0.0 (measured on MI355X, every scan route; no input gives
    # a 16-bit index a -0.0 score).  There the three rows tie at +0.0 and only the tie rule is checked.
    assert S[0, z["neg_row"]] == 0 and np.signbit(S[0, z["neg_row"]]) == (dtype == "f32"), "an fp32 index must give this row -0.0"
    assert np.all(S[0, z["zero_rows"]].view(np.uint32) == 0)
    for b in (0.0, -0.0):
        got = _range(idx, Q, b)
        ri.same(got, ri.oracle(S, b), (dtype, b))
        ids, sc = ri.lists(got)[0]
        assert ids[-3:].tolist() == sorted(z["zero_rows"] + [z["neg_row"]])      # the two zeros are one value: ties by ascending row
        assert np.signbit(sc[-3:]).tolist() == [False, False, dtype == "f32"] and np.all(sc[:-3] > 0)
    assert z["neg_row"] not in ri.lists(_range(idx, Q, 1e-45))[0][0].tolist()
    idx.close()


# ---------------------------------------------------------------------------------------------- 5: forced blocks and groups
def test_forced_blocks_and_groups_give_the_same_bits():
    c = _case("c768-bf16")
    want = _range(c.idx, c.Q, 0.0)
    assert c.idx.get_option("range_blocks_last") == 1 and c.idx.get_option("range_groups_last") == 1
    ri.same(want, ri.oracle(c.S, 0.0))
    idx = _index(c.d, c.dtype, c.X, range_block_queries=7, range_scratch_hits=3000)
    got = _range(idx, c.Q, 0.0)
    ri.same(got, want)
    assert idx.get_option("range_blocks_last") == 10 and idx.get_option("range_groups_last") == c.nq      # every list is above 3000 hits: a group each
    assert idx.get_option("range_block_queries") == 7 and idx.get_option("range_scratch_hits") == 3000
    idx.set_option("range_scratch_hits", 9000)      # two lists a group, the block's seventh alone
    ri.same(_range(idx, c.Q, 0.0), want)
    assert idx.get_option("range_groups_last") == 40
    assert np.array_equal(idx.range_count(c.Q, 0.0), np.diff(want[0]))
    for b in (c.b_dup, 0.8):      # groups that hold empty lists
        ri.same(_range(idx, c.Q, b), ri.oracle(c.S, b))
    idx.close()


# ---------------------------------------------------------------------------------------------- 6: max_total
def test_max_total():
    c = _case("c64-40-f16")
    want = _range(c.idx, c.Q, 0.3)
    total = int(want[0][-1])
    assert total > 1000
    for idx in (c.idx, _index(c.d, c.dtype, c.X, range_block_queries=16)):
        with pytest.raises(L.CmrError) as e:
            idx.range_search(c.Q, 0.3, max_total=total - 1)
        assert e.value.code == L.CMR_ERR_UNSUPPORTED and str(total) in str(e.value), str(e.value)
        ri.same(idx.range_search(c.Q, 0.3, max_total=total), want)      # exactly at the limit; and the index still answers
        ri.same(idx.range_search(c.Q, 0.3), want)
        assert idx.range_count(c.Q, 0.3).sum() == total      # the count has no limit
        if idx is not c.idx:
            idx.close()


# ---------------------------------------------------------------------------------------------- 7: shards
@pytest.mark.parametrize("S", [1, 2, 4])
def test_shards_equal_one_index(S):
    from comorag_amd.multi_index import MultiDeviceIndex
    c = _case("c64-40-f16")
    multi = MultiDeviceIndex(c.d, c.dtype, devices=[0] * S, options={"append_block_rows": 1024})
    multi.append(c.X)
    assert sum(multi.shard_rows()) == c.n and min(multi.shard_rows()) > 0
    one = _index(c.d, c.dtype, c.X)
    bounds = [c.b_dup, 0.8, 0.0, -0.9, -INF, INF]
    for b in bounds:
        want = ri.oracle(c.S, b)
        ri.same(multi.range_search(c.Q, b), want, (S, b))
        assert np.array_equal(multi.range_count(c.Q, b), np.diff(want[0]))
    total = int(ri.oracle(c.S, 0.3)[0][-1])
    with pytest.raises(L.CmrError) as e:
        multi.range_search(c.Q, 0.3, max_total=total - 1)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED and str(total) in str(e.value)
    ri.same(multi.range_search(c.Q, 0.3, max_total=total), ri.oracle(c.S, 0.3))
    # after a removal of a random 10 % and an update of 25 rows both layouts match the oracle on the new contents
    rng = np.random.default_rng(77 + S)
    gone = rng.choice(c.n, size=c.n // 10, replace=False)
    assert multi.remove_ids(gone) == one.remove_ids(gone) == len(gone)
    n2 = c.n - len(gone)
    upd = rng.choice(n2, size=25, replace=False)
    rows = np.ascontiguousarray(c.X[rng.choice(c.n, size=25, replace=False)][:, ::-1])
    assert multi.update_rows(upd, rows) == one.update_rows(upd, rows) == 25
    S2 = one.scores(c.Q)
    assert S2.shape == (c.nq, n2)
    for b in (0.8, 0.0, -INF):
        want = ri.oracle(S2, b)
        ri.same(one.range_search(c.Q, b), want, ("one", b))
        ri.same(multi.range_search(c.Q, b), want, ("multi", S, b))
    one.close(); multi.close()


# ---------------------------------------------------------------------------------------------- 8: concurrency
def test_four_threads_with_different_bounds():
    c = _case("c768-bf16")
    bounds = [c.b_dup, 0.8, 0.0, -0.9]
    solo = [c.idx.range_search(c.Q, b) for b in bounds]
    for s, b in zip(solo, bounds):
        ri.same(s, ri.oracle(c.S, b))
    got, errs = [None] * 4, []
    start = threading.Barrier(4)

    def run(i):
        try:
            start.wait()
            for _ in range(3):
                got[i] = c.idx.range_search(c.Q, bounds[i])
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(4):
        ri.same(got[i], solo[i], bounds[i])


# ---------------------------------------------------------------------------------------------- 9: the synonymy join
def test_retrieve_knn_full_lists_from_a_range_search():
    from comorag_amd.index import DenseIndex
    from comorag_amd.retrieval import neighbours_within, retrieve_knn
    n, d = 5003, 64
    X, Q, info = ti.family_c(n, d, 40, seed=61)
    names = [f"e{i}" for i in range(n)]
    large = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=n, max_neighbours=8)
    rng_ = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=n, max_neighbours=8, full_lists="range")
    assert large == rng_
    sizes = np.array([len(large[m][0]) for m in names])
    assert (sizes > 8).sum() >= 100 and sizes[ti.CENTRES[3]] == 1 + ti.MEMBERS[3] > ti.P_K      # lists the range search served, one above 128
    with pytest.raises(ValueError):
        retrieve_knn(names[:2], names, X[:2], X, min_score=0.8, full_lists="other")
    Xn = X / np.maximum(np.sqrt((X * X).sum(axis=1, keepdims=True, dtype=np.float32)), np.float32(1e-12))
    idx = DenseIndex(d, "f32")
    idx.append(Xn)
    rows = ti.CENTRES + [100]
    for r, (ids, sc) in zip(rows, neighbours_within(idx, Xn[rows], 0.8)):
        assert [names[j] for j in ids] == large[names[r]][0] and sc.tolist() == large[names[r]][1]
    idx.close()
