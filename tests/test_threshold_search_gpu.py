"""The threshold search (search_min_score: the fused top-k with every query's running threshold started at the caller's bound) on
every route and through every entry point — cmr_index_search_min_score, _dev, _pipelined, cmr_mindex_search_min_score,
retrieve_knn(min_score=) — bit for bit.  Two layers: the plain search's 128-deep lists P are checked against the fp64 oracle under the
project's tolerance (the anchor); everything else is np.array_equal against threshold_inputs.cut(P, bound, k): `key > tau  <=>
score >= min_score` is a statement about fp32 bits, so there is no either-way band.  Inputs, the route table and the cut rule come from
tests/threshold_inputs.py; tests/test_threshold_inputs.py checks on the CPU what the assertions here rely on.  Every tagged call is
confirmed by the read-only option "last_route"."""
import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc
from tests import threshold_inputs as ti
from tests import value_domain_inputs as vd

pytestmark = pytest.mark.gpu

TAGS = list(ti.ROUTES)
INF = float("inf")


# ---------------------------------------------------------------------------------------------- shared indexes and their anchors
class Case:
    pass


_CASES, _DATA = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for c in _CASES.values():
        c.idx.close()
    _CASES.clear(); _DATA.clear()


def _index(spec, X, **more):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(spec["d"], spec["dtype"], options={**spec["opts"], **more})
    idx.append(X)
    return idx


def _f64_scores(Xr, Qr, rows=16384):
    """orc.exact_scores_f64 in blocks of rows (the fp64 copy of a large corpus is never whole in memory)"""
    return np.concatenate([orc.exact_scores_f64(Xr[r:r + rows], Qr) for r in range(0, len(Xr), rows)], axis=1)


def _anchor(dtype, X, Q, ids, sc):
    """layer 1: plain-search lists against the fp64 scores of the rounded operands, under vd.ERR scaled by vd.row_tol"""
    rnd = vd.ROUND[dtype]
    Xr, Qr = rnd(X), rnd(Q)
    exact = _f64_scores(Xr, Qr)
    ref_ids, _ = orc.topk_rule(exact, ids.shape[1])
    assert ids.shape == ref_ids.shape == sc.shape
    for i in range(len(Q)):
        assert ids[i].min() >= 0 and ids[i].max() < len(X)
        both = np.union1d(ids[i], ref_ids[i])
        tol = dict(zip(both.tolist(), vd.row_tol(Qr[i], Xr[both])))
        orc.assert_topk_equivalent(ids[i], ref_ids[i], exact[i], max(tol.values()))
        assert all(abs(float(s) - exact[i][r]) <= tol[r] for r, s in zip(ids[i].tolist(), sc[i])), i
        assert np.all(np.diff(sc[i]) <= 0), "scores not descending"
        ties = np.diff(sc[i]) == 0
        assert np.all(np.diff(ids[i])[ties] > 0), "equal scores not in ascending row order"


def _plain(idx, Q, dtype, X):
    """P = idx.search(Q, 128), anchored; a plain search never carries the threshold bit"""
    ids, sc = idx.search(Q, ti.P_K)[:2]
    assert not idx.get_option("last_route") & ti.THRESHOLD
    _anchor(dtype, X, Q, ids, sc)
    return ids, sc


def _case(tag):
    """the route's index on family C, its anchored plain lists and its attained bound — built once, shared, never changed"""
    if tag in _CASES:
        return _CASES[tag]
    c = Case()
    c.tag, c.spec = tag, ti.ROUTES[tag]
    s = c.spec
    c.X, Qall, c.info = ti.family_c(s["n"], s["d"], s["nq"], s["seed"])
    c.Q, c.q_dup = ti.pick_queries(Qall, s["nq"])
    c.idx = _index(s, c.X)
    c.P = _plain(c.idx, c.Q, s["dtype"], c.X)
    if "plain_levels" in s:      # the corpus on which the plain search of these queries samples twice
        assert (c.idx.get_option("last_route") >> 4) & 3 == s["plain_levels"], hex(c.idx.get_option("last_route"))
    # the four bit-equal rows: one score, consecutive in their query's list, ascending rows; that score is the attained bound
    tied = c.info["tied"]
    at = int(np.flatnonzero(c.P[0][c.q_dup] == tied[0])[0])
    assert c.P[0][c.q_dup, at:at + 4].tolist() == tied and len(set(c.P[1][c.q_dup, at:at + 4].view(np.uint32).tolist())) == 1
    c.b_dup = float(c.P[1][c.q_dup, at])
    assert c.P[1][c.q_dup, at - 1] > c.b_dup and (at + 4 == ti.P_K or c.P[1][c.q_dup, at + 4] < c.b_dup)
    _CASES[tag] = c
    return c


def _same(got, want, what=""):
    """bit for bit: ids, and the scores as fp32 words (-inf padding included)"""
    assert got[0].shape == want[0].shape and got[0].dtype == np.int64 and got[1].dtype == np.float32, what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32)), what


def _route(idx, spec):
    bad = ti.route_ok(idx.get_option("last_route"), spec)
    assert bad is None, bad


def _host(idx, spec, Q, k, b):
    out = idx.search_min_score(Q, k, b)
    _route(idx, spec)
    return out


# ---------------------------------------------------------------------------------------------- the exact cut on every route
@pytest.mark.parametrize("tag", TAGS)
def test_exact_cut_on_every_route(tag):
    c = _case(tag)
    idx, spec, Q, qd, tied = c.idx, c.spec, c.Q, c.q_dup, c.info["tied"]
    b, b_up, b_down = ti.bounds_around(c.b_dup)[:3]
    seen = {bound: set() for bound in [b] + ti.FIXED_BOUNDS}
    for k in ti.KS:
        out = {}
        for bound in ti.bounds_around(c.b_dup):
            got = _host(idx, spec, Q, k, bound)
            ids, sc, cnt = ti.cut(*c.P, bound, k)
            _same(got, (ids, sc), (tag, k, bound))
            out[bound] = got
            if k == 20 and bound in seen:
                seen[bound] |= {ti.branch(x, k) for x in cnt}
        assert np.all(out[INF][0] == -1) and np.all(np.isneginf(out[INF][1])) and np.all(out[ti.FLT_MAX][0] == -1)
        _same(out[-INF], (c.P[0][:, :k], c.P[1][:, :k])); _same(out[-ti.FLT_MAX], out[-INF])
        assert not np.isin(out[b_up][0][qd], tied).any(), "the next fp32 value above the attained bound must drop all four tied rows"
        if not np.any(c.P[1] == np.float32(b_down)):
            _same(out[b_down], out[b])
        if k == ti.P_K:      # the attained bound keeps all four: they end their query's list
            n_real = int((out[b][0][qd] >= 0).sum())
            assert 4 <= n_real < k and out[b][0][qd, n_real - 4:n_real].tolist() == tied
            assert int((out[b_up][0][qd] >= 0).sum()) == n_real - 4
    for bound, branches in seen.items():
        assert branches == {"empty", "short", "full"}, (bound, branches)
    if spec["nq"] >= 5:      # more rows pass than the longest list holds
        assert ti.cut(*c.P, 0.8, ti.P_K)[2][3] == ti.P_K and ti.cut(*c.P, -0.9, ti.P_K)[2][:4].tolist() == [ti.P_K] * 4


def test_negative_attained_zero_and_subnormal_bounds():
    """the key's other bit pattern (scores < 0), the two zeros, and the smallest subnormal above them — on narrow-1"""
    spec = ti.ROUTES["narrow-1"]
    X, Q = vd.family_p(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])
    idx = _index(spec, X)
    P = _plain(idx, -Q, spec["dtype"], X)
    b = np.float32(P[1][0, 9])      # the 10th best plain score of query 0
    assert b < 0 and np.all(P[1] < 0)
    for k in ti.KS:
        for bound in (float(b), float(np.nextafter(b, np.float32(INF))), float(np.nextafter(b, np.float32(-INF)))):
            ids, sc, cnt = ti.cut(*P, bound, k)
            _same(_host(idx, spec, -Q, k, bound), (ids, sc), (k, bound))
    assert ti.cut(*P, float(b), 20)[2][0] == 10 and ti.cut(*P, float(np.nextafter(b, np.float32(INF))), 20)[2][0] == 9
    idx.close()
    X, Q = vd.family_z(spec["n"], spec["d"], spec["nq"], seed=spec["seed"])      # three rows score +0.0, every other row < 0
    idx = _index(spec, X)
    P = _plain(idx, Q, spec["dtype"], X)
    assert np.all(P[0][:, :3] == np.array(vd.zero_rows(spec["n"]))) and np.all(P[1][:, :3].view(np.uint32) == 0) and np.all(P[1][:, 3:] < 0)
    for k in ti.KS:
        for bound, want in ((0.0, 3), (-0.0, 3), (1e-45, 0), (-1e-45, 3)):
            ids, sc, cnt = ti.cut(*P, bound, k)
            assert cnt.tolist() == [want] * spec["nq"]
            _same(_host(idx, spec, Q, k, bound), (ids, sc), (k, bound))
    idx.close()


# ---------------------------------------------------------------------------------------------- deep lists, few rows, ids
def _asc(n, n_max):
    if "asc" not in _DATA:
        _DATA["asc"] = ti.family_asc(n_max, 768, 70)
    X, Q = _DATA["asc"]
    return X[:n], Q


@pytest.mark.parametrize("k", [20, 100])
@pytest.mark.parametrize("route", ["wide", "quad"])
def test_deep_lists_without_threshold_help(route, k):
    """ascending scores and a bound of -inf: no sampling level and no bound thins the stream out, every candidate list takes at
    least twice its capacity in rows and compacts on the way; the result is the plain search's, bit for bit"""
    n_cu = L.device_info(0)["n_cu"]
    n = ti.deep_n(k, n_cu)
    X, Q = _asc(n, ti.deep_n(100, n_cu))
    wide = route == "wide"
    spec = dict(ti.ROUTES[route], n=n)
    W, rows = ti.deep_lists(n, n_cu, wide)
    assert rows >= 2 * ti.list_cap(k) and n % 32 == 13
    idx = _index(spec, X) if wide else _index(spec, X, scan_grid=ti.deep_grid(n_cu, 2))
    want = idx.search(Q, k)[:2]
    _anchor(spec["dtype"], X, Q, *want)
    for bound in (-INF, -ti.FLT_MAX):
        _same(_host(idx, spec, Q, k, bound), want, (route, k, bound))
    idx.close()


@pytest.mark.parametrize("n", ti.FEW_ROWS)
def test_few_rows_go_through_the_chain(n):
    """the threshold search never takes the single-launch path: 1 .. 37 rows through pack / scan / merge, k above n"""
    spec = dict(ti.ROUTES["narrow-1"], n=n)
    X = orc.synthetic_corpus(n, spec["d"], seed=900 + n)
    Q = orc.synthetic_queries(spec["nq"], spec["d"], seed=901 + n)
    idx = _index(spec, X)
    P = _plain(idx, Q, spec["dtype"], X)
    assert P[0].shape == (spec["nq"], n)
    best = float(P[1][0, 0])
    for bound in (-INF, best):
        ids, sc, cnt = ti.cut(*P, bound, 64)
        got = _host(idx, spec, Q, 64, bound)
        _same(got, (ids, sc), (n, bound))
        assert np.all(got[0][:, n:] == -1) and np.all(np.isneginf(got[1][:, n:]))
        if bound == -INF:
            assert cnt.tolist() == [n] * spec["nq"]
        else:      # the best score is attained: its row is kept
            assert cnt[0] >= 1 and got[0][0, 0] == P[0][0, 0]
    idx.close()


@pytest.mark.parametrize("tag", ["narrow-1", "wide"])
def test_padding_survives_id_base_and_block_table(tag):
    c = _case(tag)
    n = c.spec["n"]
    idx = _index(c.spec, c.X)
    for base in (ti.ID_BASE, None):
        if base is not None:
            idx.set_id_base(base)
        else:
            idx.set_id_blocks(*ti.id_blocks(n))
        plain = idx.search(c.Q, ti.P_K)[:2]
        _same(plain, (ti.map_ids(c.P[0], n, base), c.P[1]))      # real ids map as the plain search maps them
        padded = 0
        for k in (20, ti.P_K):
            for bound in (c.b_dup, 0.8, -INF, INF):
                ids, sc, cnt = ti.cut(*c.P, bound, k)
                got = _host(idx, c.spec, c.Q, k, bound)
                _same(got, (ti.map_ids(ids, n, base), sc), (tag, base, k, bound))
                assert np.all((got[0] == -1) == (ids == -1)) and not np.any(got[0] == (ti.ID_BASE if base else ti.id_blocks(n)[1][0]) - 1)
                padded += int((got[0] == -1).sum())
        assert padded > 0
    idx.close()


# ---------------------------------------------------------------------------------------------- entry points
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(Q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(_dev())


def _outputs(nq, k, minmax=False):
    """a block's own output tensors, pre-filled with values no search returns"""
    import torch
    o = [torch.full((nq, k), -7, dtype=torch.int64, device=_dev()), torch.full((nq, k), 7.0, dtype=torch.float32, device=_dev())]
    if minmax:
        o += [torch.full((nq,), 7.0, dtype=torch.float32, device=_dev()) for _ in range(2)]
    return o


def _np(ts):
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("tag", TAGS)
def test_dev_calls_queued_back_to_back(tag):
    """search_min_score_dev on a non-default stream: two calls with different bounds and no synchronisation between them share the
    stream's workspace (and its tau); each equals the host call"""
    import torch
    c = _case(tag)
    k, nq = 33, c.spec["nq"]
    want = [_host(c.idx, c.spec, c.Q, k, b) for b in (c.b_dup, -INF)]
    for w, b in zip(want, (c.b_dup, -INF)):
        _same(w, ti.cut(*c.P, b, k)[:2])
    qt, o1, o2 = _up(c.Q), _outputs(nq, k), _outputs(nq, k)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(_dev())
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(_dev()).cuda_stream == s.cuda_stream != torch.cuda.default_stream(_dev()).cuda_stream
        c.idx.search_min_score_dev(qt, k, c.b_dup, *o1)
        _route(c.idx, c.spec)
        c.idx.search_min_score_dev(qt, k, -INF, *o2)
        _route(c.idx, c.spec)
    s.synchronize()
    assert c.idx.query_status() is False
    _same(_np(o1), want[0], tag); _same(_np(o2), want[1], tag)


def _block(kind, spec, Q, k, bound, P):
    """one pipelined block: "thr" | "plain", the route it must take, its queries, and the anchored plain lists of those queries"""
    return dict(kind=kind, spec=spec, Q=np.ascontiguousarray(Q), k=k, bound=bound, P=P)


def _pipeline(idx, blocks):
    """Host references first (each checked against the cut of the block's plain lists), then every block enqueued with its own inputs
    and outputs and ONE synchronisation, on the last handle; every block must equal its host call bit for bit"""
    import torch
    want = []
    for b in blocks:
        if b["kind"] == "thr":
            want.append(_host(idx, b["spec"], b["Q"], b["k"], b["bound"]))
            _same(want[-1], ti.cut(*b["P"], b["bound"], b["k"])[:2])
        else:
            want.append(idx.search(b["Q"], b["k"]))
            _same(want[-1][:2], (b["P"][0][:, :b["k"]], b["P"][1][:, :b["k"]]))
    qs = [_up(b["Q"]) for b in blocks]
    outs = [_outputs(len(b["Q"]), b["k"], minmax=b["kind"] == "plain") for b in blocks]
    torch.cuda.synchronize()
    done = None
    for b, qt, o in zip(blocks, qs, outs):
        if b["kind"] == "thr":
            done = idx.search_min_score_pipelined(qt, b["k"], b["bound"], *o)
            _route(idx, b["spec"])
        else:
            done = idx.search_pipelined(qt, b["k"], *o)
            r = idx.get_option("last_route")
            assert not r & ti.THRESHOLD and ("plain_levels" not in b["spec"] or (r >> 4) & 3 == b["spec"]["plain_levels"]), hex(r)
    idx.sync(done)
    assert idx.query_status() is False
    for i, (b, o, w) in enumerate(zip(blocks, outs, want)):
        got = _np(o)
        _same(got[:2], w[:2], (i, b["kind"], b["bound"]))
        if b["kind"] == "plain":
            assert np.array_equal(got[2], w[2]) and np.array_equal(got[3], w[3]), i


def _rolled(c, i):
    """the route's queries rotated by i, with their plain lists"""
    return np.roll(c.Q, i, axis=0), (np.roll(c.P[0], i, axis=0), np.roll(c.P[1], i, axis=0))


@pytest.mark.parametrize("slots", [2, 3, 4])
@pytest.mark.parametrize("tag", ["narrow-2", "wide"])
def test_pipelined_blocks_with_different_bounds_share_slots(tag, slots):
    c = _case(tag)
    nb, k = 2 * slots + 1, 20
    bounds = ti.pipe_bounds(c.b_dup, nb)
    # 1: threshold blocks only, every slot reused with another bound (block i's queries: the route's, rotated by i)
    idx = _index(c.spec, c.X, pipe_slots=slots)
    _pipeline(idx, [_block("thr", c.spec, _rolled(c, i)[0], k, bounds[i], _rolled(c, i)[1]) for i in range(nb)])
    idx.close()
    # 2: plain blocks in between: every slot serves plain, threshold, plain (or the reverse) in turn
    idx = _index(c.spec, c.X, pipe_slots=slots)
    _pipeline(idx, [_block(("plain", "thr")[ti.alternate(i, slots)], c.spec, _rolled(c, i)[0], k, bounds[i], _rolled(c, i)[1]) for i in range(nb)])
    idx.close()


def test_pipelined_plain_blocks_write_sampling_thresholds_into_the_slot():
    """`big`: the plain blocks run both sampling levels, whose thresholds land in the slot's tau; the threshold block that takes
    the slot next must start from its own bound"""
    c = _case("big")
    slots, k = 3, 20
    nb = 2 * slots + 1
    bounds = ti.pipe_bounds(c.b_dup, nb)
    idx = _index(c.spec, c.X, pipe_slots=slots)
    _pipeline(idx, [_block(("plain", "thr")[ti.alternate(i, slots)], c.spec, c.Q, k, bounds[i], c.P) for i in range(nb)])
    idx.close()


@pytest.mark.parametrize("slots", [2, 3, 4])
def test_pipelined_narrow_and_wide_blocks_alternate(slots):
    """768-d: blocks of 40 queries (narrow kernel, two tiles) and of 70 (wide kernel) through the same slots"""
    c = _case("wide")
    narrow = dict(c.spec, nq=40, path=vd.CHAIN, nqt=2)
    nb, k = 2 * slots + 1, 20
    bounds = ti.pipe_bounds(c.b_dup, nb)
    idx = _index(c.spec, c.X, pipe_slots=slots)
    _pipeline(idx, [_block("thr", c.spec, c.Q, k, bounds[i], c.P) if ti.alternate(i, slots) else
                    _block("thr", narrow, c.Q[:40], k, bounds[i], (c.P[0][:40], c.P[1][:40])) for i in range(nb)])
    idx.close()


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("tag", ["narrow-2", "wide"])
def test_shards_merge_padded_lists(tag, S):
    """MultiDeviceIndex.search_min_score over S logical shards on device 0 == one DenseIndex, padding included"""
    from comorag_amd.multi_index import MultiDeviceIndex
    c = _case(tag)
    spec, tied = c.spec, c.info["tied"]
    multi = MultiDeviceIndex(spec["d"], spec["dtype"], devices=[0] * S, options={"append_block_rows": 1024, **spec["opts"]})
    multi.append(c.X)
    assert sum(multi.shard_rows()) == spec["n"] and min(multi.shard_rows()) > 0
    shards = [multi.shard(s) for s in range(S)]
    idle = 0      # (bound, shard, query) where the shard contributes nothing to a query that has rows
    for k in (20, ti.P_K):
        for bound in ti.bounds_around(c.b_dup):
            ids, sc, cnt = ti.cut(*c.P, bound, k)
            _same(multi.search_min_score(c.Q, k, bound), (ids, sc), (tag, S, k, bound))
            for sh in shards:
                _route(sh, spec)
            if k == ti.P_K and np.isfinite(bound):
                for sh in shards:
                    part = sh.search_min_score(c.Q, k, bound)[0]
                    idle += int(((part[:, 0] < 0) & (cnt > 0)).sum())
    assert idle > 0
    holders = [set(tied) & set(sh.search_min_score(c.Q, ti.P_K, c.b_dup)[0][c.q_dup].tolist()) for sh in shards]
    assert set().union(*holders) == set(tied) and sum(bool(h) for h in holders) >= 2, holders
    multi.close()


def test_nan_bound_and_k_129_are_refused_everywhere():
    from comorag_amd.multi_index import MultiDeviceIndex
    c = _case("narrow-1")
    spec, Q, nq = c.spec, c.Q, c.spec["nq"]
    idx = _index(spec, c.X)
    multi = MultiDeviceIndex(spec["d"], spec["dtype"], devices=[0, 0], options={"append_block_rows": 1024})
    multi.append(c.X)
    qt = _up(Q)
    import torch
    torch.cuda.synchronize()

    def pipelined(k, b, o):
        idx.sync(idx.search_min_score_pipelined(qt, k, b, *o))

    def dev(k, b, o):
        idx.search_min_score_dev(qt, k, b, *o); torch.cuda.synchronize()

    calls = {"host": lambda k, b, o: idx.search_min_score(Q, k, b), "multi": lambda k, b, o: multi.search_min_score(Q, k, b), "dev": dev, "pipelined": pipelined}
    for name, call in calls.items():
        for k, b, code in ((20, float("nan"), L.CMR_ERR_INVALID), (129, 0.5, L.CMR_ERR_UNSUPPORTED)):
            with pytest.raises(L.CmrError) as e:
                call(k, b, _outputs(nq, k))
            assert e.value.code == code, (name, k, b, e.value.code)
        # the same index answers correctly afterwards, through the same entry point
        o = _outputs(nq, 20)
        got = call(20, c.b_dup, o)
        _same(got if got is not None else _np(o), ti.cut(*c.P, c.b_dup, 20)[:2], name)
    assert idx.query_status() is False
    idx.close(); multi.close()


def test_retrieve_knn_branches_return_one_dict():
    """retrieve_knn(min_score=) on family C at 5003 x 64: the synchronous branch, the pipelined branch (blocks of 512 queries) and
    max_neighbours = 8 (most clustered queries re-run through the exact large-k path) return the same dict"""
    from comorag_amd.retrieval import retrieve_knn
    n, d = 5003, 64
    X, Q, info = ti.family_c(n, d, 40, seed=61)
    names = [f"e{i}" for i in range(n)]
    sync = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=n)
    pipe = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=512)
    rerun = retrieve_knn(names, names, X, X, min_score=0.8, query_batch_size=n, max_neighbours=8)
    assert sync == pipe, "the pipelined branch differs from the synchronous one"
    assert sync == rerun, "max_neighbours = 8 (exact re-run) differs"
    # not vacuous: lone rows, clustered rows beyond 8 and beyond 128 neighbours; the lists are the fp64 sets within the project's tolerance
    sizes = np.array([len(sync[m][0]) for m in names])
    assert (sizes == 1).sum() > n - 400 and (sizes > 8).sum() >= 100 and sizes[ti.CENTRES[3]] == 1 + ti.MEMBERS[3] > ti.P_K
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    rows = ti.CENTRES + info["tied"][:1] + [100]
    exact = orc.exact_scores_f64(Xn, Xn[rows])
    for e, r in zip(exact, rows):
        got = {int(m[1:]) for m in sync[names[r]][0]}
        assert set(np.flatnonzero(e >= 0.8 + vd.ERR).tolist()) <= got <= set(np.flatnonzero(e >= 0.8 - vd.ERR).tolist())
        sc = np.array(sync[names[r]][1])
        assert np.all(sc >= np.float32(0.8)) and np.all(np.diff(sc) <= 0)
