"""In-place row update (cmr_index_update_rows, cmr_index_update_rows_dev, cmr_mindex_update_rows).  The oracle is code
that existed before the feature: after `update_rows(ids, rows)` every call must return, bit for bit, what the TWIN — a fresh index
built by appending the final row contents in order — returns.  Every comparison is `np.array_equal` on ids and on score bits, no
tolerance.  Corpora as in tests/test_remove_rows_gpu.py: seeded, row-normalised, half the queries planted; its shapes."""
import threading

import numpy as np
import pytest

from comorag_amd import _lib as L
from tests.prefilter_gpu_helpers import N_MID as PF_MID, N_SMALL as PF_SMALL, _enqueue

pytestmark = pytest.mark.gpu

N_SMALL = 1000                  # no sampling, partial last panel
N_ONE_LEVEL = 8192 + 5          # 257 panels: one sampling level
N_TWO_LEVELS = 131072 + 7       # 4097 panels: two sampling levels at wide batches
SHAPES = {"bf16": 128, "f16": 96, "f32": 96}      # dim 96 is padded to 128
NQ_MAX = 65
BASE = 1_000_000

_cache = {}


def _rows(dtype, n):
    key = (dtype, n)
    if key not in _cache:
        d = SHAPES[dtype]
        rng = np.random.default_rng(1000 * n + d)
        X = rng.standard_normal((n, d)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rng.standard_normal((NQ_MAX, d)).astype(np.float32)
        pick = rng.integers(0, n, NQ_MAX // 2)
        Q[: len(pick)] = X[pick] + 0.05 * Q[: len(pick)]
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        X.setflags(write=False); Q.setflags(write=False)
        _cache[key] = (X, Q)
    return _cache[key]


def teardown_module(module):
    _cache.clear()


def _fresh(dtype, m, seed):
    """m new unit rows, nothing like the corpus' own"""
    R = np.random.default_rng(seed).standard_normal((m, SHAPES[dtype])).astype(np.float32)
    return R / np.linalg.norm(R, axis=1, keepdims=True)


def _index(dtype, X, **kw):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(SHAPES[dtype], dtype, **kw)
    idx.append(X)
    return idx


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """tuples of arrays: integer arrays whole, float arrays by their bits, None against None"""
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        if a is None or b is None:
            assert a is None and b is None, what
        elif a.dtype.kind == "f":
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what
        else:
            assert a.shape == b.shape and np.array_equal(a, b), what


def _check_search(idx, twin, Q, what="", nqs=(1, 8, 65), k=10):
    assert len(idx) == len(twin), what
    for nq in nqs:
        _same(idx.search(Q[:nq], k), twin.search(Q[:nq], k), f"{what} search nq={nq}")


def _check_rows(idx, twin, what=""):
    n = len(twin)
    ids = np.unique(np.concatenate([np.arange(min(n, 70)), np.arange(max(0, n - 70), n), np.arange(0, n, max(1, n // 97))])).astype(np.int64)
    _same((idx.get_rows(ids),), (twin.get_rows(ids),), f"{what} get_rows")


def _snapshot(idx, Q, stats=True):
    return (idx.scores(Q[:3]), idx.get_rows(np.arange(len(idx)))) + ((np.array(idx.round_stats(), np.float32),) if stats else ())


PATTERNS = {
    "row0": lambda n, rng: np.array([0]),
    "last": lambda n, rng: np.array([n - 1]),
    "panel1": lambda n, rng: np.arange(32, 64),
    "every_other": lambda n, rng: np.arange(0, n, 2),
    "random1pct": lambda n, rng: rng.choice(n, max(1, n // 100), replace=False),
    "all": lambda n, rng: np.arange(n),
}
CASES = [(dt, N_SMALL, p) for dt in SHAPES for p in PATTERNS] + \
        [("bf16", n, p) for n in (N_ONE_LEVEL, N_TWO_LEVELS) for p in ("row0", "every_other", "random1pct")]


# ---- 1. update patterns, each against the twin
@pytest.mark.parametrize("dtype,n,pattern", CASES)
def test_pattern_equals_the_twin(dtype, n, pattern):
    X, Q = _rows(dtype, n)
    ids = PATTERNS[pattern](n, np.random.default_rng(7))
    new = _fresh(dtype, len(ids), 99)
    final = X.copy(); final[ids] = new
    idx, twin = _index(dtype, X), _index(dtype, final)
    try:
        assert idx.update_rows(ids, new) == len(ids)
        assert idx.get_option("update_chunks_last") == 1
        _check_search(idx, twin, Q, pattern)
        _check_rows(idx, twin, pattern)
        _same((idx.scores(Q[:2]),), (twin.scores(Q[:2]),), "scores")
    finally:
        idx.close(); twin.close()


# ---- 2. every route after an update
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL, N_TWO_LEVELS])
def test_routes_after_update(n):
    X, Q = _rows("bf16", n)
    rng = np.random.default_rng(n)
    ids = np.unique(np.concatenate([[0, n - 1], rng.choice(n, n // 50, replace=False)]))
    new = _fresh("bf16", len(ids), n + 1)
    new[:8] = 0.5 * new[:8] + Q[:8]                                      # eight of the new rows rank high for the queries the routes take
    new /= np.linalg.norm(new, axis=1, keepdims=True)
    final = X.copy(); final[ids] = new
    idx, twin = _index("bf16", X), _index("bf16", final)
    try:
        assert idx.update_rows(ids, new) == len(ids)
        _check_search(idx, twin, Q)
        _same(idx.search(Q[:3], 200), twin.search(Q[:3], 200), "k = 200")
        _same((idx.scores(Q[:3]),), (twin.scores(Q[:3]),), "scores")
        _same(idx.sorted_scores(Q[:2]), twin.sorted_scores(Q[:2]), "sorted_scores")
        _same(idx.search_min_score(Q[:8], 10, 0.3), twin.search_min_score(Q[:8], 10, 0.3), "min_score")
        top = twin.search(Q[:8], 5, with_minmax=False)[0]
        assert np.isin(top, ids).any(), "updated rows must be among the results the routes are compared on"
        _same(idx.search_filtered_ids(Q[:8], 10, exclude=top), twin.search_filtered_ids(Q[:8], 10, exclude=top), "filtered ids, per query")
        _same(idx.search_filtered_ids(Q[:8], 10, allow=ids), twin.search_filtered_ids(Q[:8], 10, allow=ids), "filtered ids, shared allow list")
        _check_rows(idx, twin)
    finally:
        idx.close(); twin.close()


# ---- 3. the fp32 shadow and the exact search
@pytest.mark.parametrize("dtype,n", [("bf16", N_SMALL), ("f16", N_SMALL), ("bf16", N_ONE_LEVEL)])
def test_shadow_permutation_equals_the_twin_whole(dtype, n):
    """new contents = the old contents of the updated rows, permuted: the same multiset of rows, hence the same maxima — the exact
    search's flags and round_stats() must equal the twin's too"""
    X, Q = _rows(dtype, n)
    rng = np.random.default_rng(5)
    ids = np.unique(np.concatenate([[0, 33, n - 1], rng.choice(n, n // 10, replace=False)]))
    new = X[rng.permutation(ids)]
    final = X.copy(); final[ids] = new
    idx, twin = _index(dtype, X, keep_f32=True), _index(dtype, final, keep_f32=True)
    try:
        assert idx.update_rows(ids, new) == len(ids)
        assert idx.round_stats() == twin.round_stats()
        for nq in (1, 8):
            _same(idx.search_exact(Q[:nq], 10), twin.search_exact(Q[:nq], 10), "search_exact")
        cand = twin.search(Q[:8], 50, with_minmax=False)[0]
        _same(idx.rescore(Q[:8], cand, 10), twin.rescore(Q[:8], cand, 10), "rescore")
        _check_search(idx, twin, Q, nqs=(8,))
        _check_rows(idx, twin)
    finally:
        idx.close(); twin.close()


@pytest.mark.parametrize("dtype,n", [("bf16", N_SMALL), ("f16", N_SMALL), ("bf16", N_ONE_LEVEL)])
def test_shadow_fresh_rows_flags_only_fall(dtype, n):
    """freshly drawn rows: our maxima are folded, the twin's recomputed — ours may be larger, so a flag may go from 1 to 0 against the
    twin and never the other way; ids and score bits are the twin's wherever our flag is 1"""
    X, Q = _rows(dtype, n)
    rng = np.random.default_rng(6)
    ids = np.unique(np.concatenate([[0, 33, n - 1], rng.choice(n, n // 10, replace=False)]))
    new = _fresh(dtype, len(ids), 17)
    final = X.copy(); final[ids] = new
    idx, twin = _index(dtype, X, keep_f32=True), _index(dtype, final, keep_f32=True)
    try:
        assert idx.update_rows(ids, new) == len(ids)
        ours, theirs = idx.round_stats(), twin.round_stats()
        assert ours[0] >= theirs[0] and ours[1] >= theirs[1]
        for nq in (1, 8, 65):
            gi, gs, gx = idx.search_exact(Q[:nq], 10)
            wi, ws, wx = twin.search_exact(Q[:nq], 10)
            assert not np.any(gx & ~wx), "a flag the twin does not give"
            assert gx.any(), "no certified query: the comparison below would be empty"
            _same((gi[gx], gs[gx]), (wi[gx], ws[gx]), "search_exact where certified")
        cand = twin.search(Q[:8], 50, with_minmax=False)[0]
        _same(idx.rescore(Q[:8], cand, 10), twin.rescore(Q[:8], cand, 10), "rescore")
        _check_rows(idx, twin)
    finally:
        idx.close(); twin.close()


# ---- 4. id rules
def test_id_rules_duplicates_and_the_count():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    idx = _index("bf16", X)
    try:
        before = _snapshot(idx, Q, stats=False)
        assert idx.update_rows([], np.zeros((0, 128), np.float32)) == 0
        assert idx.update_rows([-1, -7, n, n + 5, 1 << 40], _fresh("bf16", 5, 1)) == 0
        assert idx.get_option("update_chunks_last") == 0
        _same(_snapshot(idx, Q, stats=False), before, "an update of nothing changes nothing")
        ids = np.array([-1, 5, n, 900, 5, 64, -12, 900, 5, 1 << 40], dtype=np.int64)      # 5 three times, 900 twice: the last wins
        new = _fresh("bf16", len(ids), 2)
        assert idx.update_rows(ids, new) == 3
        final = X.copy(); final[5] = new[8]; final[900] = new[7]; final[64] = new[5]
        twin = _index("bf16", final)
        try:
            _check_search(idx, twin, Q); _check_rows(idx, twin)
            _same((idx.get_rows([5, 64, 900]),), (twin.get_rows([5, 64, 900]),))
        finally:
            twin.close()
        assert idx.update_rows(7, new[0]) == 1 and len(idx) == n                         # a scalar id with a 1-d row
    finally:
        idx.close()


def test_a_bad_row_that_would_not_be_written_is_not_looked_at():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    new = _fresh("bf16", 4, 3)
    bad = new.copy(); bad[0, 3] = np.nan; bad[1, 0] = np.inf
    final = X.copy(); final[10] = new[3]; final[11] = new[2]
    idx, twin = _index("bf16", X), _index("bf16", final)
    try:
        assert idx.update_rows([10, -1, 11, 10], bad) == 2          # row 0 loses to row 3, row 1 belongs to an ignored id
        _check_search(idx, twin, Q, nqs=(8,)); _check_rows(idx, twin)
    finally:
        idx.close(); twin.close()


def test_id_base_and_a_three_block_table():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    rows = np.array([0, 17, 500, n - 1])
    new = _fresh("bf16", len(rows), 4)
    final = X.copy(); final[rows] = new
    idx, twin = _index("bf16", X), _index("bf16", final)
    try:
        idx.set_id_base(BASE); twin.set_id_base(BASE)
        assert idx.update_rows(rows, new) == 0                      # plain row numbers are below the base: not held
        assert idx.update_rows(np.concatenate([rows + BASE, [BASE - 1, BASE + n]]), np.concatenate([new, new[:2]])) == len(rows)
        _check_search(idx, twin, Q)
        assert idx.search(Q[:1], 5)[0].min() >= BASE
        # a user-set table of three blocks: nothing is renumbered, so the update goes through it
        ls, gs = [0, n // 3, 2 * n // 3], [100, 100 + n // 3 + 50, 5_000_000]
        idx.set_id_blocks(ls, gs); twin.close()
        gids = np.array([100, 100 + n // 3 - 1, 100 + n // 3, 100 + n // 3 + 50, 5_000_000 + 7, 5_000_000 + (n - 2 * n // 3), 99])
        held = np.array([0, n // 3 - 1, n // 3, 2 * n // 3 + 7])     # ids 2 (in the gap), 5 (beyond the end) and 6 are held by nobody
        new2 = _fresh("bf16", len(gids), 5)
        final[held] = new2[[0, 1, 3, 4]]
        twin = _index("bf16", final); twin.set_id_blocks(ls, gs)
        assert idx.update_rows(gids, new2) == 4
        _check_search(idx, twin, Q)
        _same((idx.get_rows(gids[[0, 1, 3, 4]]),), (twin.get_rows(gids[[0, 1, 3, 4]]),))
        assert idx.search(Q[:1], 5)[0].min() >= 100
    finally:
        idx.close(); twin.close()


# ---- 5. rejection: all or nothing
@pytest.mark.parametrize("dtype,value", [("bf16", np.nan), ("f16", 70000.0), ("f32", np.inf)])
@pytest.mark.parametrize("stage", [7, 0])
def test_a_refused_row_leaves_the_index_unchanged(dtype, value, stage):
    """stage = 7: the bad value sits in the LAST of several forced chunks (every chunk is checked before the first store);
    stage = 0: the default route of a small update"""
    n = N_SMALL
    X, Q = _rows(dtype, n)
    idx = _index(dtype, X, keep_f32=dtype != "f32")
    try:
        before = _snapshot(idx, Q, stats=dtype != "f32")
        m = 40
        ids = np.arange(3, 3 + 5 * m, 5)
        new = _fresh(dtype, m, 8)
        new[m - 1, SHAPES[dtype] - 1] = value
        if stage:
            idx.set_option("update_stage_rows", stage)
            assert idx.get_option("update_stage_rows") == stage
        with pytest.raises(L.CmrError) as e:
            idx.update_rows(ids, new)
        assert e.value.code == L.CMR_ERR_NONFINITE
        assert idx.get_option("update_chunks_last") == 0
        _same(_snapshot(idx, Q, stats=dtype != "f32"), before, "unchanged")
        new[m - 1, SHAPES[dtype] - 1] = 0.0                          # the same call without the bad value goes through
        assert idx.update_rows(ids, new) == m
        assert (idx.get_option("update_chunks_last") > 1) == bool(stage)
        if dtype == "f32":
            _same((idx.get_rows(ids),), (new,), "an f32 index holds the rows as they came")
    finally:
        idx.close()


# ---- 6. chunking: tiny staging buffers force many chunks, same bits
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL])
@pytest.mark.parametrize("stage", [7, 33])
def test_staging_size_never_changes_the_result(n, stage):
    X, Q = _rows("bf16", n)
    rng = np.random.default_rng(stage)
    ids = rng.permutation(np.unique(np.concatenate([[0, n - 1], rng.choice(n, n // 3, replace=False)])))      # any order of ids
    new = _fresh("bf16", len(ids), stage)
    final = X.copy(); final[ids] = new
    idx, dflt, twin = _index("bf16", X, keep_f32=True), _index("bf16", X, keep_f32=True), _index("bf16", final, keep_f32=True)
    try:
        idx.set_option("update_stage_rows", stage)
        assert idx.update_rows(ids, new) == len(ids) and dflt.update_rows(ids, new) == len(ids)
        assert idx.get_option("update_chunks_last") == -(-len(ids) // stage) > 1
        assert dflt.get_option("update_chunks_last") == 1
        assert idx.round_stats() == dflt.round_stats()
        for other in (dflt, twin):
            _same((idx.scores(Q[:8]),), (other.scores(Q[:8]),), "scores")
            _same((idx.get_rows(np.arange(n)),), (other.get_rows(np.arange(n)),), "rows")
            _check_search(idx, other, Q, nqs=(8,))
        _same(idx.search_exact(Q[:8], 10), dflt.search_exact(Q[:8], 10), "search_exact")
    finally:
        idx.close(); dflt.close(); twin.close()


# ---- 7. the int8 pre-filter catches up from the first updated row
@pytest.mark.parametrize("n", [PF_SMALL, PF_MID])
def test_prefiltered_pipelined_search_after_update(n):
    from comorag_amd.index import DenseIndex
    d = 128
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    ids = np.unique(n // 3 + rng.choice(n - n // 3, max(2, n // 100), replace=False))      # from the first third on
    ids[0] = n // 3
    new = rng.standard_normal((len(ids), d)).astype(np.float32)
    h = min(4, len(ids))
    new[:h] += 3.0 * Q[:h]                                                                # updated rows the queries find
    new /= np.linalg.norm(new, axis=1, keepdims=True)
    final = X.copy(); final[ids] = new

    def pipelined(idx):
        done, _, oi, os_ = _enqueue(idx, Q, 10)
        idx.sync(done)
        return oi.cpu().numpy(), os_.cpu().numpy()

    idx, twin = DenseIndex(d, "bf16", options={"prefilter": 1}), DenseIndex(d, "bf16", options={"prefilter": 1})
    try:
        idx.append(X); twin.append(final)
        pipelined(idx)
        assert idx.get_option("prefilter_active") == 1 and idx.get_option("prefilter_rows") == n
        assert idx.update_rows(ids, new) == len(ids)
        assert idx.get_option("prefilter_rows") == n // 3       # stale from the first updated row on
        got, want = pipelined(idx), pipelined(twin)
        assert idx.get_option("prefilter_active") == 1 and twin.get_option("prefilter_active") == 1
        assert idx.get_option("prefilter_rows") == n
        assert np.isin(got[0], ids).any()
        _same(got, want, "pre-filtered")
    finally:
        idx.close(); twin.close()


# ---- 8. searches of another thread see the index before or after, never in between
def test_searches_race_one_update():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    ids = np.arange(0, n, 2)
    new = _fresh("bf16", len(ids), 21)
    final = X.copy(); final[ids] = new
    idx, after = _index("bf16", X), _index("bf16", final)
    try:
        want_before = [idx.search(Q[i:i + 1], 10) for i in range(NQ_MAX)]
        want_after = [after.search(Q[i:i + 1], 10) for i in range(NQ_MAX)]
        go, updated, errors = threading.Event(), [], []

        def updater():
            go.wait()
            try:
                updated.append(idx.update_rows(ids, new))
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        t = threading.Thread(target=updater)
        t.start()
        results = []
        for i in range(200):
            if i == 40:
                go.set()
            results.append((i % NQ_MAX, idx.search(Q[i % NQ_MAX:i % NQ_MAX + 1], 10)))
        t.join()
        assert not errors and updated == [len(ids)]
        for qi, got in results:
            is_after = all(np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a, b.view(np.uint32) if b.dtype.kind == "f" else b)
                           for a, b in zip(got, want_after[qi]))
            if not is_after:
                _same(got, want_before[qi], "neither the index before nor the index after")
        _same(idx.search(Q[:8], 10), after.search(Q[:8], 10))
    finally:
        idx.close(); after.close()


# ---- 9. MultiDeviceIndex: global ids in, one DenseIndex twin
@pytest.mark.parametrize("S", [1, 2, 4])
def test_multi_device_index_equals_one_twin(S):
    from comorag_amd.multi_index import MultiDeviceIndex
    n = N_SMALL
    X, Q = _rows("bf16", n)
    multi = MultiDeviceIndex(SHAPES["bf16"], "bf16", devices=[0] * S, options={"append_block_rows": 64})
    twin = None

    def compare(cur, what):
        nonlocal twin
        twin = _index("bf16", cur)
        for nq in (1, 65):
            _same(multi.search(Q[:nq], 10), twin.search(Q[:nq], 10), f"{what} search nq={nq}")
        _same((multi.scores(Q[:3]),), (twin.scores(Q[:3]),), f"{what} scores")
        _check_rows(multi, twin, what)
        twin.close(); twin = None

    try:
        for a in range(0, 800, 100):      # several calls: every shard ends up with several blocks
            multi.append(X[a:a + 100])
        cur = X[:800].copy()
        rng = np.random.default_rng(S)
        for step, ids in enumerate((np.array([0]), np.arange(0, 800, 2), np.arange(60, 200), rng.permutation(800)[:37])):
            new = _fresh("bf16", len(ids) + 3, 30 + step)
            listed = np.concatenate([ids[:1], ids, [-1, 800]])      # the first id twice (the later row wins), two ignored ids
            assert multi.update_rows(listed, new) == len(ids)
            cur[ids] = new[1:1 + len(ids)]
            compare(cur, f"step {step}")
        # a refused row on one shard leaves every shard as it was
        bad = _fresh("bf16", 800, 40); bad[799, 5] = np.nan
        with pytest.raises(L.CmrError) as e:
            multi.update_rows(np.arange(800), bad)
        assert e.value.code == L.CMR_ERR_NONFINITE
        compare(cur, "after a refused update")
        # non-trivial tables: remove, append, then update by the NEW global ids
        gone = np.arange(1, 800, 7)
        assert multi.remove_ids(gone) == len(gone)
        keep = np.ones(800, bool); keep[gone] = False
        multi.append(X[800:1000])
        cur = np.concatenate([cur[keep], X[800:1000]])
        assert len(multi) == len(cur)
        ids = rng.permutation(len(cur))[: len(cur) // 2]
        new = _fresh("bf16", len(ids), 50)
        assert multi.update_rows(ids, new) == len(ids)
        cur[ids] = new
        compare(cur, "after remove + append")
    finally:
        multi.close()
        if twin is not None:
            twin.close()


# ---- 10. rows on the device
@pytest.mark.parametrize("dtype", list(SHAPES))
def test_update_rows_dev_equals_the_host_form(dtype):
    import torch
    n = N_ONE_LEVEL
    X, Q = _rows("bf16", n) if dtype == "bf16" else _rows(dtype, N_SMALL)
    n = len(X)
    rng = np.random.default_rng(12)
    ids = rng.permutation(n)[: n // 4]
    ids = np.concatenate([ids, ids[:3], [-1, n]])
    new = _fresh(dtype, len(ids), 13)
    host, dev = _index(dtype, X, keep_f32=dtype != "f32"), _index(dtype, X, keep_f32=dtype != "f32")
    try:
        want = host.update_rows(ids, new)
        got = dev.update_rows_dev(ids, torch.from_numpy(new).to(torch.device("cuda", dev.device)))
        assert got == want == n // 4
        _check_search(dev, host, Q)
        _same((dev.get_rows(np.arange(n)),), (host.get_rows(np.arange(n)),))
        if dtype != "f32":
            assert dev.round_stats() == host.round_stats()
            _same(dev.search_exact(Q[:8], 10), host.search_exact(Q[:8], 10))
        bad = torch.from_numpy(new).to(torch.device("cuda", dev.device)); bad[5, 0] = float("inf")
        with pytest.raises(L.CmrError) as e:
            dev.update_rows_dev(ids, bad)
        assert e.value.code == L.CMR_ERR_NONFINITE
        _same((dev.get_rows(np.arange(n)),), (host.get_rows(np.arange(n)),), "unchanged")
        assert dev.update_rows_dev(np.zeros(0, np.int64), torch.empty((0, SHAPES[dtype]), device=torch.device("cuda", dev.device))) == 0
    finally:
        host.close(); dev.close()


# ---- 11. the memory-pool mirror on a real index
def test_the_mirror_on_a_real_index_follows_a_forced_recompute(fake_embedder):
    from comorag_amd import hooks
    from tests.update_rows_model import SecondEmbedder

    class Node:
        def __init__(self, probe, cue):
            self.probe, self.cue, self.embedding = probe, cue, None

    class Pool:                                  # utils/memory_utils.py:149-186 as far as the hook reads it
        def __init__(self, em):
            self.pool, self.embedding_model = [], em

        def compute_probe_note_embeddings(self, force_recompute=False):
            todo = [n for n in self.pool if n.embedding is None or force_recompute]
            if todo:
                for n, e in zip(todo, self.embedding_model.encode([f"{n.probe} {n.cue}" for n in todo]).numpy()):
                    n.embedding = e

    pool = hooks.install_memory_pool(Pool(fake_embedder))
    for cycle in range(2):
        for j in range(25):
            pool.pool.append(Node(f"probe {cycle}", f"cue {cycle}-{j}"))
        pool.retrieve_similar_nodes(f"probe {cycle}", top_percent=0.5)
    index = pool._hip_state["index"]
    assert len(index) == 50
    pcts = (0.5, 0.2, 1.0)
    before = [[pool.pool.index(x) for x in pool.retrieve_similar_nodes("probe 2", top_percent=p)] for p in pcts]
    second = SecondEmbedder(32)
    pool.embedding_model = second
    pool.compute_probe_note_embeddings(force_recompute=True)
    got = [[pool.pool.index(x) for x in pool.retrieve_similar_nodes("probe 2", top_percent=p)] for p in pcts]
    assert pool._hip_state["index"] is index and len(index) == 50       # the same index, nothing re-appended
    fresh = hooks.install_memory_pool(Pool(second))                    # a freshly installed pool over the same nodes
    fresh.pool = list(pool.pool)
    want = [[fresh.pool.index(x) for x in fresh.retrieve_similar_nodes("probe 2", top_percent=p)] for p in pcts]
    assert got == want and got != before
    want_rows = fresh._hip_state["index"].get_rows(np.arange(50))
    _same((index.get_rows(np.arange(50)),), (want_rows,), "the mirror's rows are the fresh mirror's")
    index.close(); fresh._hip_state["index"].close()
