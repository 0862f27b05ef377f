"""In-place row update, the parts that need no device: the planner cmr_mindex_plan_update — the only parser of an
update's ids — against the model in tests/update_rows_model.py, the argument checks that come before any device call, the Python shape
errors, and the memory-pool mirror of hooks.install_memory_pool on the reference's own MemoryPool after a forced recompute."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle.ref_loader import reference_available
from tests import update_rows_model as M


def _p(a):
    return a.ctypes.data if len(a) else None


def _plan(shard_rows, n_blocks, ls, gs, ids):
    shard_rows, n_blocks = np.asarray(shard_rows, np.int64), np.asarray(n_blocks, np.int32)
    ls, gs, ids = np.asarray(ls, np.int64), np.asarray(gs, np.int64), np.asarray(ids, np.int64)
    S, n = len(shard_rows), len(ids)
    shard, local, src = np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.full(n, -7, np.int64)
    count, m = np.full(S, -7, np.int64), C.c_int64(-7)
    L.check(L.lib().cmr_mindex_plan_update(S, _p(shard_rows), _p(n_blocks), _p(ls), _p(gs), _p(ids), n, _p(shard), _p(local), _p(src),
                                           _p(count), C.byref(m)))
    m = m.value
    assert np.all(shard[m:] == -7) and np.all(local[m:] == -7) and np.all(src[m:] == -7)      # nothing written behind the valid entries
    return shard[:m], local[:m], src[:m], count, m


def _check(rows, nb, ls, gs, ids):
    want = M.plan(rows, nb, ls, gs, ids)
    shard, local, src, count, m = _plan(rows, nb, ls, gs, ids)
    assert m == len(want[0]) == int(count.sum())
    assert np.array_equal(shard, want[0]) and np.array_equal(local, want[1]) and np.array_equal(src, want[2]) and np.array_equal(count, want[3])
    # stated on their own, whatever the model says: grouped by shard, strictly ascending local rows inside a shard, rows the shard has
    assert np.all(np.diff(shard) >= 0)
    for s in range(len(rows)):
        l = local[shard == s]
        assert np.all(np.diff(l) > 0) and (len(l) == 0 or (l[0] >= 0 and l[-1] < rows[s]))
    ids = np.asarray(ids, np.int64)
    assert len(set(ids[src].tolist())) == m                       # an id counts once ...
    for j in range(m):
        assert not np.any(ids[src[j] + 1:] == ids[src[j]])        # ... and its LAST occurrence is the source
    return shard, local, src, count


def _random_layout(rng, S, n_blocks_total, dense):
    """blocks of 1..9 rows dealt to random shards in global order; dense: global ids 0, 1, 2, ..., else with gaps between the blocks"""
    owner = rng.integers(0, S, n_blocks_total)
    lens = rng.integers(1, 10, n_blocks_total)
    g, per = 0, [[] for _ in range(S)]
    for o, ln in zip(owner, lens):
        if not dense:
            g += int(rng.integers(0, 4))
        per[o].append((g, int(ln)))
        g += int(ln)
    rows, nb, ls, gs = [], [], [], []
    for s in range(S):
        at = 0
        for g0, ln in per[s]:
            ls.append(at); gs.append(g0); at += ln
        rows.append(at); nb.append(len(per[s]))
    return rows, nb, ls, gs, g


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("seed", range(4))
def test_plan_update_matches_the_model_on_random_tables(seed, S, dense):
    rng = np.random.default_rng(100 * seed + S)
    rows, nb, ls, gs, top = _random_layout(rng, S, int(rng.integers(S, 25)), dense)
    for frac in (0.0, 0.05, 0.5, 1.0):
        pick = np.flatnonzero(rng.random(top) < frac)       # (with gaps: some of these ids lie in a gap and are held by nobody)
        ids = np.concatenate([pick, [-1, -9, top, top + 100, 1 << 40], pick[:5], pick[:2]]).astype(np.int64)
        rng.shuffle(ids)
        _check(rows, nb, ls, gs, ids)
    _check(rows, nb, ls, gs, [])


def test_plan_update_named_cases():
    # shard 0: globals [0, 4) and [10, 13); shard 1: [4, 10); shard 2: [13, 15)
    rows, nb, ls, gs = [7, 6, 2], [2, 1, 1], [0, 4, 0, 0], [0, 10, 4, 13]
    sh, lo, sr, ct = _check(rows, nb, ls, gs, [])
    assert len(sh) == 0 and ct.tolist() == [0, 0, 0]
    sh, lo, sr, ct = _check(rows, nb, ls, gs, [-1, 99, 15, -5])
    assert len(sh) == 0
    sh, lo, sr, ct = _check(rows, nb, ls, gs, [14, 12, 4, 0, 12, -1, 9])
    assert sh.tolist() == [0, 0, 1, 1, 2] and lo.tolist() == [0, 6, 0, 5, 1] and sr.tolist() == [3, 4, 2, 6, 0] and ct.tolist() == [2, 2, 1]
    # one index with an id base is the one-shard case: base 1000, 5 rows
    sh, lo, sr, ct = _check([5], [1], [0], [1000], [3, 1004, 1000, 999, 1005, 1004])
    assert lo.tolist() == [0, 4] and sr.tolist() == [2, 5]
    # a three-block table with gaps on one shard
    sh, lo, sr, ct = _check([9], [3], [0, 3, 6], [100, 200, 5000], [102, 103, 199, 200, 5002, 5003, 100])
    assert lo.tolist() == [0, 2, 3, 8] and sr.tolist() == [6, 0, 3, 4]
    _check([0, 3], [0, 1], [0], [0], [1, 1, 2])          # a shard without blocks


def test_bad_arguments_come_back_invalid_without_a_device():
    lib = L.lib()
    ids = np.array([1, 2], np.int64)
    rows = np.zeros((2, 4), np.float32)
    n = C.c_int64(5)
    fake = C.c_void_p(8)      # never dereferenced: the argument checks come first
    for fn in (lib.cmr_index_update_rows, lib.cmr_mindex_update_rows):
        assert fn(None, ids.ctypes.data, rows.ctypes.data, 2, C.byref(n)) == L.CMR_ERR_INVALID and n.value == 0
        assert b"NULL" in lib.cmr_last_error()
        assert fn(None, None, None, 0, None) == L.CMR_ERR_INVALID
        assert fn(fake, None, rows.ctypes.data, 2, None) == L.CMR_ERR_INVALID
        assert fn(fake, ids.ctypes.data, None, 2, None) == L.CMR_ERR_INVALID
        assert fn(fake, ids.ctypes.data, rows.ctypes.data, -1, None) == L.CMR_ERR_INVALID
    f = lib.cmr_index_update_rows_dev
    assert f(None, ids.ctypes.data, fake, 2, None, C.byref(n)) == L.CMR_ERR_INVALID and n.value == 0
    assert f(fake, None, fake, 2, None, None) == L.CMR_ERR_INVALID
    assert f(fake, ids.ctypes.data, None, 2, None, None) == L.CMR_ERR_INVALID
    assert f(fake, ids.ctypes.data, fake, -3, None, None) == L.CMR_ERR_INVALID
    one, nb = np.array([1], np.int64), np.array([1], np.int32)
    out32, out = np.zeros(2, np.int32), np.zeros(2, np.int64)
    p = lib.cmr_mindex_plan_update
    assert p(0, one.ctypes.data, nb.ctypes.data, None, None, None, 0, None, None, None, None, None) == L.CMR_ERR_INVALID
    assert p(1, one.ctypes.data, nb.ctypes.data, one.ctypes.data, one.ctypes.data, None, 2, out32.ctypes.data, out.ctypes.data, out.ctypes.data, None, None) == L.CMR_ERR_INVALID
    assert p(1, one.ctypes.data, nb.ctypes.data, one.ctypes.data, one.ctypes.data, ids.ctypes.data, 2, None, out.ctypes.data, out.ctypes.data, None, None) == L.CMR_ERR_INVALID
    assert p(1, one.ctypes.data, nb.ctypes.data, one.ctypes.data, one.ctypes.data, ids.ctypes.data, -1, None, None, None, None, None) == L.CMR_ERR_INVALID
    assert p(1, one.ctypes.data, nb.ctypes.data, None, None, ids.ctypes.data, 2, out32.ctypes.data, out.ctypes.data, out.ctypes.data, None, None) == L.CMR_ERR_INVALID


def test_python_shape_errors_come_before_the_library():
    from comorag_amd.index import HostArrayIndex

    calls = []

    class Calls:
        @staticmethod
        def update_rows(h, ids, rows, n, out):
            calls.append(n)
            return 0

    class Ix(HostArrayIndex):
        dim = 4
        _h = None
        _c = Calls

    ix = Ix()
    good = np.zeros((3, 4), np.float32)
    for ids, rows in (([0, 1], good), ([[0, 1, 2]], good), ([0, 1, 2], np.zeros((3, 5), np.float32)), ([0, 1, 2], np.zeros((3, 4, 1), np.float32)),
                      ([0], np.zeros(4, np.float32)), (0, good), ([0.5, 1.0, 2.0], good), (1, np.zeros(5, np.float32))):
        with pytest.raises(ValueError):
            ix.update_rows(ids, rows)
    assert calls == []
    assert ix.update_rows([0, 1, 2], good) == 0 and ix.update_rows(7, np.zeros(4, np.float32)) == 0 and ix.update_rows(np.int64(7), [0.0, 1.0, 2.0, 3.0]) == 0
    assert ix.update_rows([], np.zeros((0, 4), np.float32)) == 0
    assert calls == [3, 1, 1, 0]


# ---- the memory-pool mirror after a forced recompute, on the reference's own MemoryPool
@pytest.mark.skipif(not reference_available(), reason="reference tree not present")
def test_mirror_follows_a_forced_recompute_on_a_real_pool(fake_embedder, numpy_index_cls):
    """compute_probe_note_embeddings(force_recompute=True) (utils/memory_utils.py:149-186) gives every node a new embedding: the mirror
    must replace its rows — one update_rows call over all of them, no append — and select what the reference selects."""
    from oracle.ref_loader import ref_modules
    mu = ref_modules()["memory_utils"]
    from comorag_amd import hooks

    ours, ref = (mu.MemoryPool(embedding_model=fake_embedder, agent=None) for _ in range(2))
    appended, updated = [], []

    class Ix(numpy_index_cls):
        def append(self, rows):
            appended.append(len(np.asarray(rows).reshape(-1, self.dim)))
            super().append(rows)

        def update_rows(self, ids, rows):
            ids, rows = np.asarray(ids, np.int64), np.asarray(rows, np.float32).reshape(-1, self.dim)
            assert ids.ndim == 1 and len(ids) == len(rows)
            updated.append(ids.tolist())
            self._x[ids] = rows
            return len(set(ids.tolist()))

    hooks.install_memory_pool(ours, index_factory=lambda dim, dtype, device: Ix(dim, dtype, device))
    cue = 0
    probes = ["where is the slipper?", "who is the stepmother?"]
    for probe in probes:
        for pool in (ours, ref):
            c = cue
            for kind in (mu.NodeType.VER, mu.NodeType.SEM, mu.NodeType.EPI):
                for j in range(3):
                    pool.add_to_temp_pool(mu.MemoryNode(probe=probe, node_type=kind, original_content=[f"text {c}"], cue=f"cue number {c}"))
                    c += 1
            pool.merge_temp_to_main()
        cue = c
        a, b = ours.retrieve_similar_nodes(probe, top_percent=0.5), ref.retrieve_similar_nodes(probe, top_percent=0.5)
        assert [ours.pool.index(n) for n in a] == [ref.pool.index(n) for n in b]
    n = len(ours.pool)
    assert appended == [9, 9] and updated == [] and n == 18
    probe, pcts = "what happened at midnight?", (0.5, 0.2, 1.0)
    before = [[ref.pool.index(x) for x in ref.retrieve_similar_nodes(probe, top_percent=p)] for p in pcts]
    assert [[ours.pool.index(x) for x in ours.retrieve_similar_nodes(probe, top_percent=p)] for p in pcts] == before
    assert appended == [9, 9] and updated == []                 # without changes there is no update_rows call

    second = M.SecondEmbedder(32)
    for pool in (ours, ref):
        pool.embedding_model = second
        pool.compute_probe_note_embeddings(force_recompute=True)
    after = [[ref.pool.index(x) for x in ref.retrieve_similar_nodes(probe, top_percent=p)] for p in pcts]
    got = [[ours.pool.index(x) for x in ours.retrieve_similar_nodes(probe, top_percent=p)] for p in pcts]
    assert any(x != y for x, y in zip(before, after)), "the second embedder must change the reference's own selection"
    assert got == after
    assert updated == [list(range(n))] and appended == [9, 9]    # ONE call over every indexed row, nothing re-appended
    # a single reassigned embedding is one more call of one row
    for pool in (ours, ref):
        pool.pool[4].embedding = second.batch_encode(["something else entirely"])[0]
    assert [ours.pool.index(x) for x in ours.retrieve_similar_nodes(probe, top_percent=0.5)] == \
           [ref.pool.index(x) for x in ref.retrieve_similar_nodes(probe, top_percent=0.5)]
    assert updated == [list(range(n)), [4]] and appended == [9, 9]
