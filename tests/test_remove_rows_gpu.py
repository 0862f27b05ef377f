"""Row removal by in-place compaction (cmr_index_remove_ids, cmr_mindex_remove_ids, EmbeddingStore.delete).  The
oracle is code that existed before the feature: after `remove_ids(R)` every call must return, bit for bit, what the TWIN — a fresh
`DenseIndex` built by appending the surviving rows in their old order — returns.  Every comparison is `np.array_equal` on ids and on
score bits, no tolerance.  Corpora as in tests/test_filtered_ids_gpu.py: seeded, row-normalised, half the queries planted; its shapes."""
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
        _cache[key] = (X, Q)
    return _cache[key]


def teardown_module(module):
    _cache.clear()


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


PATTERNS = {
    "row0": lambda n, rng: np.array([0]),
    "last": lambda n, rng: np.array([n - 1]),
    "tail": lambda n, rng: np.arange(n - 45, n),
    "panel1": lambda n, rng: np.arange(32, 64),
    "every_other": lambda n, rng: np.arange(0, n, 2),
    "random1pct": lambda n, rng: rng.choice(n, max(1, n // 100), replace=False),
    "block10pct": lambda n, rng: np.arange(n // 2 - n // 20, n // 2 + n // 20),
    "all_but_one": lambda n, rng: np.delete(np.arange(n), n // 3),
}
CASES = [(dt, N_SMALL, p) for dt in SHAPES for p in PATTERNS] + \
        [("bf16", n, p) for n in (N_ONE_LEVEL, N_TWO_LEVELS) for p in ("row0", "every_other", "random1pct")]


# ---- 1. removal patterns, each against the twin
@pytest.mark.parametrize("dtype,n,pattern", CASES)
def test_pattern_equals_the_twin(dtype, n, pattern):
    X, Q = _rows(dtype, n)
    gone = PATTERNS[pattern](n, np.random.default_rng(7))
    keep = np.ones(n, bool); keep[gone] = False
    idx, twin = _index(dtype, X), _index(dtype, X[keep])
    try:
        assert idx.remove_ids(gone) == len(gone)
        moved = idx.get_option("remove_chunks_last")
        assert (moved == 0) == (pattern in ("last", "tail")), "only a tail removal is a truncate"
        _check_search(idx, twin, Q, pattern)
        _check_rows(idx, twin, pattern)
        _same((idx.scores(Q[:2]),), (twin.scores(Q[:2]),), "scores")
    finally:
        idx.close(); twin.close()


@pytest.mark.parametrize("dtype", list(SHAPES))
def test_remove_everything_then_append(dtype):
    X, Q = _rows(dtype, N_SMALL)
    idx, fresh = _index(dtype, X), _index(dtype, X[100:400])
    try:
        assert idx.remove_ids(np.arange(N_SMALL)) == N_SMALL
        assert len(idx) == 0 and idx.remove_ids([0, 1]) == 0
        idx.append(X[100:400])
        _check_search(idx, fresh, Q, "after re-append")
        _check_rows(idx, fresh)
    finally:
        idx.close(); fresh.close()


# ---- 2. every route after a removal
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL, N_TWO_LEVELS])
def test_routes_after_removal(n):
    X, Q = _rows("bf16", n)
    rng = np.random.default_rng(n)
    gone = np.unique(np.concatenate([[0], rng.choice(n, n // 100, replace=False)]))
    keep = np.ones(n, bool); keep[gone] = False
    idx, twin = _index("bf16", X), _index("bf16", X[keep])
    try:
        assert idx.remove_ids(gone) == len(gone)
        _check_search(idx, twin, Q)
        _same(idx.search(Q[:3], 200), twin.search(Q[:3], 200), "k = 200")
        _same((idx.scores(Q[:3]),), (twin.scores(Q[:3]),), "scores")
        _same(idx.sorted_scores(Q[:2]), twin.sorted_scores(Q[:2]), "sorted_scores")
        _same(idx.search_min_score(Q[:8], 10, 0.3), twin.search_min_score(Q[:8], 10, 0.3), "min_score")
        top = twin.search(Q[:8], 5, with_minmax=False)[0]      # exclusion lists in the NEW numbering
        _same(idx.search_filtered_ids(Q[:8], 10, exclude=top), twin.search_filtered_ids(Q[:8], 10, exclude=top), "filtered ids, per query")
        _same(idx.search_filtered_ids(Q[:8], 10, exclude=top.reshape(-1)), twin.search_filtered_ids(Q[:8], 10, exclude=top.reshape(-1)), "filtered ids, shared")
        _check_rows(idx, twin)
    finally:
        idx.close(); twin.close()


@pytest.mark.parametrize("dtype,n", [("bf16", N_SMALL), ("f16", N_SMALL), ("bf16", N_ONE_LEVEL)])
def test_shadow_is_compacted_too(dtype, n):
    X, Q = _rows(dtype, n)
    gone = np.unique(np.concatenate([[0, 33], np.random.default_rng(5).choice(n, n // 10, replace=False)]))
    keep = np.ones(n, bool); keep[gone] = False
    idx, twin = _index(dtype, X, keep_f32=True), _index(dtype, X[keep], keep_f32=True)
    try:
        assert idx.remove_ids(gone) == len(gone)
        for nq in (1, 8):
            _same(idx.search_exact(Q[:nq], 10), twin.search_exact(Q[:nq], 10), "search_exact")
        cand = twin.search(Q[:8], 50, with_minmax=False)[0]
        _same(idx.rescore(Q[:8], cand, 10), twin.rescore(Q[:8], cand, 10), "rescore")
        _check_search(idx, twin, Q, nqs=(8,))
    finally:
        idx.close(); twin.close()


# ---- 3. chunking: tiny staging buffers force many chunks, same bits
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL])
@pytest.mark.parametrize("stage", [2, 3, 5])
def test_staging_size_never_changes_the_result(n, stage):
    X, Q = _rows("bf16", n)
    gone = np.unique(np.concatenate([[0], np.random.default_rng(stage).choice(n, n // 3, replace=False)]))
    keep = np.ones(n, bool); keep[gone] = False
    idx, dflt, twin = _index("bf16", X, keep_f32=True), _index("bf16", X, keep_f32=True), _index("bf16", X[keep], keep_f32=True)
    try:
        idx.set_option("remove_stage_panels", stage)
        assert idx.get_option("remove_stage_panels") == stage
        assert idx.remove_ids(gone) == len(gone) and dflt.remove_ids(gone) == len(gone)
        panels = (n + 31) // 32
        assert idx.get_option("remove_chunks_last") == -(-panels // (stage - 1)) > 1      # (row 0 goes: every panel is affected)
        assert dflt.get_option("remove_chunks_last") == 1
        for other in (dflt, twin):
            _same((idx.scores(Q[:8]),), (other.scores(Q[:8]),), "scores")
            _same((idx.get_rows(np.arange(len(twin))),), (other.get_rows(np.arange(len(twin))),), "rows")
            _same(idx.search_exact(Q[:8], 10), other.search_exact(Q[:8], 10), "search_exact")
            _check_search(idx, other, Q, nqs=(8,))
    finally:
        idx.close(); dflt.close(); twin.close()


# ---- 4. id rules
def test_id_rules_and_padded_results():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    idx = _index("bf16", X)
    try:
        before = idx.search(Q[:8], 10)
        assert idx.remove_ids([]) == 0 and idx.remove_ids([-1, -7, n, n + 5, 1 << 40]) == 0
        assert idx.get_option("remove_chunks_last") == 0
        _same(idx.search(Q[:8], 10), before, "a removal of nothing changes nothing")
        junk = np.array([-1, -1, -12, n, 1 << 40, 5, 5, 900, 5, 64, 900], dtype=np.int64)
        assert idx.remove_ids(junk) == 3 and len(idx) == n - 3
        keep = np.ones(n, bool); keep[[5, 64, 900]] = False
        # a padded 2-d result goes in as it is: k beyond what the filter leaves gives -1 columns
        res = idx.search_filtered_ids(Q[:4], 20, allow=[[1, 2, 3], [4], [], [7, 8]])[0]
        assert (res == -1).any() and res.ndim == 2
        held = np.unique(res[res >= 0])
        assert idx.remove_ids(res) == len(held)
        keep[np.flatnonzero(keep)[held]] = False
        twin = _index("bf16", X[keep])
        try:
            _check_search(idx, twin, Q)
        finally:
            twin.close()
    finally:
        idx.close()


def test_id_base_is_taken_and_kept():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    gone = np.array([0, 17, 500, n - 1])
    keep = np.ones(n, bool); keep[gone] = False
    idx, twin = _index("bf16", X), _index("bf16", X[keep])
    try:
        idx.set_id_base(BASE); twin.set_id_base(BASE)
        assert idx.remove_ids(gone) == 0                       # plain row numbers are below the base: not held
        assert idx.remove_ids(np.concatenate([gone + BASE, [BASE - 1, BASE + n]])) == len(gone)
        _check_search(idx, twin, Q)
        assert idx.search(Q[:1], 5)[0].min() >= BASE
    finally:
        idx.close(); twin.close()


def test_block_table_is_refused_and_left_alone():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    idx = _index("bf16", X)
    try:
        idx.set_id_blocks([0, n // 3, 2 * n // 3], [100, 100 + n // 3 + 50, 5_000_000])
        before = idx.search(Q[:8], 10)
        with pytest.raises(L.CmrError) as e:
            idx.remove_ids([100, 101])
        assert e.value.code == L.CMR_ERR_UNSUPPORTED
        assert len(idx) == n
        _same(idx.search(Q[:8], 10), before, "untouched")
    finally:
        idx.close()


# ---- 5. sequences
def test_remove_append_remove_append():
    X, Q = _rows("bf16", N_ONE_LEVEL)
    rng = np.random.default_rng(11)
    cur = X[:3000]
    idx = _index("bf16", cur)
    try:
        for step in range(2):
            gone = rng.choice(len(cur), len(cur) // 7, replace=False)
            assert idx.remove_ids(gone) == len(gone)
            keep = np.ones(len(cur), bool); keep[gone] = False
            cur = cur[keep]
            twin = _index("bf16", cur)
            _check_search(idx, twin, Q, f"remove {step}"); _check_rows(idx, twin); twin.close()
            more = X[3000 + 1500 * step: 3000 + 1500 * (step + 1)]
            idx.append(more)
            cur = np.concatenate([cur, more])
            twin = _index("bf16", cur)
            _check_search(idx, twin, Q, f"append {step}"); _check_rows(idx, twin); twin.close()
        before = idx.search(Q[:8], 10)
        assert idx.remove_ids([-1, len(cur)]) == 0
        _same(idx.search(Q[:8], 10), before)
    finally:
        idx.close()


# ---- 6. the int8 pre-filter catches up from the first removed row
@pytest.mark.parametrize("n", [PF_SMALL, PF_MID])
def test_prefiltered_pipelined_search_after_removal(n):
    from comorag_amd.index import DenseIndex
    d = 128
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    gone = np.unique(n // 3 + rng.choice(n - n // 3, max(1, n // 100), replace=False))      # starts in the first third or later ...
    gone[0] = n // 4                                                                       # ... make it the first third
    keep = np.ones(n, bool); keep[gone] = False

    def pipelined(idx):
        done, _, oi, os_ = _enqueue(idx, Q, 10)
        idx.sync(done)
        return oi.cpu().numpy(), os_.cpu().numpy()

    idx, twin = DenseIndex(d, "bf16", options={"prefilter": 1}), DenseIndex(d, "bf16", options={"prefilter": 1})
    try:
        idx.append(X); twin.append(X[keep])
        pipelined(idx)
        assert idx.get_option("prefilter_active") == 1 and idx.get_option("prefilter_rows") == n
        assert idx.remove_ids(gone) == len(gone)
        got, want = pipelined(idx), pipelined(twin)
        assert idx.get_option("prefilter_active") == 1 and twin.get_option("prefilter_active") == 1
        assert idx.get_option("prefilter_rows") == n - len(gone)
        _same(got, want, "pre-filtered")
    finally:
        idx.close(); twin.close()


# ---- 7. searches of another thread see the index before or after, never in between
def test_searches_race_one_removal():
    n = N_SMALL
    X, Q = _rows("bf16", n)
    gone = np.random.default_rng(3).choice(n, 100, replace=False)
    keep = np.ones(n, bool); keep[gone] = False
    idx, after = _index("bf16", X), _index("bf16", X[keep])
    try:
        want_before = [idx.search(Q[i:i + 1], 10) for i in range(NQ_MAX)]
        want_after = [after.search(Q[i:i + 1], 10) for i in range(NQ_MAX)]
        go, removed, errors = threading.Event(), [], []

        def remover():
            go.wait()
            try:
                removed.append(idx.remove_ids(gone))
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        t = threading.Thread(target=remover)
        t.start()
        results = []
        for i in range(200):
            if i == 40:
                go.set()
            results.append((i % NQ_MAX, idx.search(Q[i % NQ_MAX:i % NQ_MAX + 1], 10)))
        t.join()
        assert not errors and removed == [100]
        for qi, got in results:
            is_after = got[0].shape == want_after[qi][0].shape and all(np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a, b.view(np.uint32) if b.dtype.kind == "f" else b)
                                                                      for a, b in zip(got, want_after[qi]))
            if not is_after:
                _same(got, want_before[qi], "neither the index before nor the index after")
        _same(idx.search(Q[:8], 10), after.search(Q[:8], 10))
    finally:
        idx.close(); after.close()


# ---- 8. MultiDeviceIndex: global ids in, one DenseIndex twin
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("pattern", ["row0", "every_other", "block"])
def test_multi_device_index_equals_one_twin(S, pattern):
    from comorag_amd.multi_index import MultiDeviceIndex
    n = N_SMALL
    X, Q = _rows("bf16", n)
    multi = MultiDeviceIndex(SHAPES["bf16"], "bf16", devices=[0] * S, options={"append_block_rows": 64})
    twin = None
    try:
        for a in range(0, 800, 100):      # several calls: every shard ends up with several blocks
            multi.append(X[a:a + 100])
        gone = {"row0": np.array([0]), "every_other": np.arange(0, 800, 2), "block": np.arange(64, 128)}[pattern]
        keep = np.ones(800, bool); keep[gone] = False
        assert multi.remove_ids(np.concatenate([gone, [-1, 800, gone[0]]])) == len(gone)
        assert len(multi) == 800 - len(gone) == sum(multi.shard_rows())
        cur = X[:800][keep]
        for step in range(2):
            twin = _index("bf16", cur)
            for nq in (1, 65):
                _same(multi.search(Q[:nq], 10), twin.search(Q[:nq], 10), f"search nq={nq} step {step}")
            _same((multi.scores(Q[:3]),), (twin.scores(Q[:3]),), "scores")
            top = twin.search(Q[:8], 5, with_minmax=False)[0]
            _same(multi.search_filtered_ids(Q[:8], 10, exclude=top), twin.search_filtered_ids(Q[:8], 10, exclude=top), "filtered ids")
            _check_rows(multi, twin)
            twin.close(); twin = None
            if step == 0:                 # more rows to both: global ids stay dense in append order
                multi.append(X[800:900]); multi.append(X[900:1000])
                cur = np.concatenate([cur, X[800:1000]])
    finally:
        multi.close()
        if twin is not None:
            twin.close()


# ---- 9. the store's mirror follows a delete
def test_store_delete_keeps_the_mirror_in_step(tmp_path):
    from comorag_amd.embedding_store import EmbeddingStore
    from comorag_amd.index import DenseIndex
    from tests.conftest import FakeEmbedder
    enc = FakeEmbedder(32)
    st = EmbeddingStore(enc, str(tmp_path), 8, "chunk")
    texts = [f"passage {i}" for i in range(150)]
    st.insert_strings(texts)
    mirror = st.device_index(dtype="bf16")
    ids0 = list(st.hash_ids)
    dead = [ids0[i] for i in (0, 31, 32, 77, 149)]
    dead_texts = {st.hash_id_to_text[h] for h in dead}
    assert st.delete(dead + ["chunk-unknown"]) == 5
    assert len(mirror) == st._n == 145
    Q = enc.batch_encode([texts[0], texts[77], texts[5], "something else"])
    got = mirror.search(Q, 10)
    for row in got[0]:
        assert not ({st.texts[i] for i in row} & dead_texts)
    assert st.texts[got[0][2, 0]] == texts[5]
    twin = DenseIndex(32, "bf16")
    try:
        twin.append(st._mat[:st._n])
        _same(got, twin.search(Q, 10), "mirror")
        _same((mirror.get_rows(np.arange(145)),), (twin.get_rows(np.arange(145)),))
        st.insert_strings([texts[77]])                      # a deleted text comes back as the last row, in the mirror too
        assert st.hash_id_to_idx[ids0[77]] == 145 and len(mirror) == 146
        assert mirror.search(enc.batch_encode([texts[77]]), 1)[0][0, 0] == 145
    finally:
        twin.close()
