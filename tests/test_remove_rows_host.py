"""Row removal, the parts that need no device: the block-table arithmetic of cmr_mindex_remove_ids
(cmr_mindex_plan_remove) against the numpy model in tests/remove_rows_model.py, `renumber_after_removal` against a loop, the argument
checks of the two entry points, and `EmbeddingStore.delete` in both persist modes with its crash windows."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.embedding_store import EmbeddingStore
from comorag_amd.index import renumber_after_removal
from tests import remove_rows_model as M
from tests.conftest import FakeEmbedder


def _p(a):
    return a.ctypes.data if len(a) else None


def _plan(shard_rows, n_blocks, ls, gs, ids, skip=None):
    shard_rows, n_blocks = np.asarray(shard_rows, np.int64), np.asarray(n_blocks, np.int32)
    ls, gs, ids = np.asarray(ls, np.int64), np.asarray(gs, np.int64), np.asarray(ids, np.int64)
    S = len(shard_rows)
    new_rows, new_nb = np.full(S, -7, np.int64), np.full(S, -7, np.int32)
    new_ls, new_gs = np.full(len(ls), -7, np.int64), np.full(len(ls), -7, np.int64)
    removed = C.c_int64(-7)
    skip_arr = None if skip is None else np.array([1 if s in skip else 0 for s in range(S)], np.int32)
    L.check(L.lib().cmr_mindex_plan_remove(S, _p(shard_rows), _p(n_blocks), _p(ls), _p(gs), _p(ids), len(ids),
                                           None if skip is None else skip_arr.ctypes.data, _p(new_rows), _p(new_nb),
                                           _p(new_ls), _p(new_gs), C.byref(removed)))
    nb = int(new_nb.sum())
    assert np.all(new_ls[nb:] == -7) and np.all(new_gs[nb:] == -7)      # nothing written behind the blocks that are left
    return new_rows, new_nb, new_ls[:nb], new_gs[:nb], removed.value


def _random_layout(rng, S, n_blocks_total, dense=True):
    """blocks of 1..9 rows dealt to random shards in global order; dense: global ids 0, 1, 2, ... (a multi-device index), else with gaps"""
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


def _check(rows, nb, ls, gs, ids, skip=None):
    tri = M.triples(rows, nb, ls, gs)
    want, want_removed = M.remove(tri, ids, skip or ())
    new_rows, new_nb, new_ls, new_gs, removed = _plan(rows, nb, ls, gs, ids, skip)
    for s in (skip or ()):
        assert new_rows[s] == rows[s]
    assert removed == want_removed
    got = M.triples(new_rows, new_nb, new_ls, new_gs)
    assert np.array_equal(got, want)
    at = 0
    for s in range(len(rows)):      # no empty blocks, local starts ascending from 0
        l = new_ls[at:at + new_nb[s]]
        assert (new_nb[s] == 0) == (new_rows[s] == 0)
        if new_nb[s]:
            assert l[0] == 0 and np.all(np.diff(l) > 0) and l[-1] < new_rows[s]
        at += new_nb[s]
    assert int(new_rows.sum()) == len(tri) - want_removed
    return new_rows, new_nb, new_ls, new_gs


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_plan_remove_matches_the_model_on_random_tables(seed, dense):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(1, 6))
    rows, nb, ls, gs, top = _random_layout(rng, S, int(rng.integers(1, 25)), dense)
    for frac in (0.0, 0.05, 0.5, 1.0):
        pick = rng.random(top) < frac
        ids = np.concatenate([np.flatnonzero(pick), [-1, -9, top, top + 100], np.flatnonzero(pick)[:3]]).astype(np.int64)
        rng.shuffle(ids)
        _check(rows, nb, ls, gs, ids)
        # the tables cmr_mindex_remove_ids installs when the compaction of some shards failed: their ids count as not listed
        _check(rows, nb, ls, gs, ids, skip=set(int(x) for x in rng.choice(S, int(rng.integers(0, S + 1)), replace=False)))


def test_plan_remove_named_cases():
    # shard 0: globals [0, 4) and [10, 13); shard 1: [4, 10); shard 2: [13, 15)
    rows, nb, ls, gs = [7, 6, 2], [2, 1, 1], [0, 4, 0, 0], [0, 10, 4, 13]
    n = _check(rows, nb, ls, gs, [])                                          # nothing
    assert n[0].tolist() == rows and n[1].tolist() == nb and n[2].tolist() == ls and n[3].tolist() == gs
    n = _check(rows, nb, ls, gs, [-1, 99, 15])                                # nothing held
    assert n[0].tolist() == rows and n[3].tolist() == gs
    n = _check(rows, nb, ls, gs, [10, 11, 12])                                # empties a block of shard 0
    assert n[0].tolist() == [4, 6, 2] and n[1].tolist() == [1, 1, 1] and n[3].tolist() == [0, 4, 10]
    n = _check(rows, nb, ls, gs, [13, 14, 14])                                # empties shard 2
    assert n[0].tolist() == [7, 6, 0] and n[1].tolist() == [2, 1, 0]
    n = _check(rows, nb, ls, gs, [0])                                         # row 0: every later block starts one lower
    assert n[3].tolist() == [0, 9, 3, 12] and n[2].tolist() == [0, 3, 0, 0]
    n = _check(rows, nb, ls, gs, np.arange(15))                               # everything
    assert n[0].tolist() == [0, 0, 0] and n[1].tolist() == [0, 0, 0]
    _check([0, 3], [0, 1], [0], [0], [1])                                     # a shard without blocks
    n = _check(rows, nb, ls, gs, [0, 5, 10, 13], skip={0})                    # shard 0 failed: its ids 0 and 10 stay, 5 and 13 go
    assert n[0].tolist() == [7, 5, 1] and n[3].tolist() == [0, 9, 4, 12]
    # ... and the same list again once shard 0 works removes exactly the rest: 0 and 10 are still ids 0 and 9
    n2 = _check(n[0], n[1], n[2], n[3], renumber_after_removal([0, 5, 10, 13], [5, 13]))
    assert n2[0].tolist() == [5, 5, 1]


def test_renumber_after_removal_matches_a_loop():
    rng = np.random.default_rng(3)
    for n, n_gone in ((1, 1), (50, 0), (50, 7), (1000, 400)):
        removed = rng.choice(n, n_gone, replace=False)
        ids = np.concatenate([rng.integers(-3, n, 200), [-1, 0, n - 1]]).astype(np.int64).reshape(-1, 7)[:29]
        gone = set(int(x) for x in removed)
        want = np.array([[-1 if (x < 0 or x in gone) else x - sum(1 for g in gone if g < x) for x in row] for row in ids.tolist()], dtype=np.int64)
        got = renumber_after_removal(ids, np.concatenate([removed, removed[:2], [-1]]))      # duplicates and padding in the removed list
        assert got.dtype == np.int64 and got.shape == ids.shape and np.array_equal(got, want)
    assert renumber_after_removal([], [1, 2]).shape == (0,)


def test_bad_arguments_come_back_invalid_without_a_device():
    lib = L.lib()
    ids = np.array([1, 2], np.int64)
    n = C.c_int64(5)
    fake = C.c_void_p(8)      # never dereferenced: the argument checks come first
    for fn in (lib.cmr_index_remove_ids, lib.cmr_mindex_remove_ids):
        assert fn(None, ids.ctypes.data, 2, C.byref(n)) == L.CMR_ERR_INVALID and n.value == 0
        assert b"NULL" in lib.cmr_last_error()
        assert fn(None, None, 0, None) == L.CMR_ERR_INVALID
        assert fn(fake, None, 2, None) == L.CMR_ERR_INVALID
        assert fn(fake, ids.ctypes.data, -1, None) == L.CMR_ERR_INVALID
    one = np.array([1], np.int64)
    assert lib.cmr_mindex_plan_remove(0, one.ctypes.data, None, None, None, None, 0, None, None, None, None, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_mindex_plan_remove(1, one.ctypes.data, np.array([1], np.int32).ctypes.data, one.ctypes.data, one.ctypes.data, None, 2, None, None, None,
                                      None, None, None) == L.CMR_ERR_INVALID


# ---- EmbeddingStore.delete
TEXTS = [f"text number {i}" for i in range(12)]


def _same_store(a, b):
    assert list(a.hash_ids) == list(b.hash_ids) and list(a.texts) == list(b.texts) and a._n == b._n == len(a.hash_ids)
    assert np.array_equal(a._mat[:a._n], b._mat[:b._n])
    for name in ("hash_id_to_idx", "hash_id_to_row", "hash_id_to_text", "text_to_hash_id"):
        assert getattr(a, name) == getattr(b, name)


@pytest.mark.parametrize("persist", ["parquet", "sidecar"])
def test_store_delete_persists_and_reloads(tmp_path, persist):
    enc = FakeEmbedder(16)
    st = EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist)
    st.insert_strings(TEXTS)
    ids0, mat0 = list(st.hash_ids), st._mat[:st._n].copy()
    assert st.delete(["chunk-unknown", "nothing"]) == 0 and st.delete([]) == 0
    _same_store(st, EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist))
    gone = [ids0[0], ids0[5], ids0[11], "chunk-unknown", ids0[5]]
    assert st.delete(gone) == 3
    keep = [i for i in range(12) if i not in (0, 5, 11)]
    assert list(st.hash_ids) == [ids0[i] for i in keep] and list(st.texts) == [TEXTS[i] for i in keep]
    assert np.array_equal(st._mat[:st._n], mat0[keep])
    assert st.hash_id_to_idx == {ids0[i]: j for j, i in enumerate(keep)}
    assert ids0[5] not in st.hash_id_to_row and TEXTS[5] not in st.text_to_hash_id
    _same_store(st, EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist))
    # a deleted text comes back as the last row
    st.insert_strings([TEXTS[5], TEXTS[1]])
    assert st.hash_id_to_idx[ids0[5]] == 9 and len(st.hash_ids) == 10 and np.array_equal(st._mat[9], mat0[5])
    _same_store(st, EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist))
    assert st.delete(ids0[1]) == 1                      # a single id
    assert st.delete(list(st.hash_ids)) == 9            # everything
    assert st._n == 0 and st.hash_id_to_idx == {}
    assert len(EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist).hash_ids) == 0
    st.insert_strings(TEXTS[:2])
    _same_store(st, EmbeddingStore(enc, str(tmp_path), 8, "chunk", persist=persist))


def test_store_delete_drops_a_mirror_that_failed(tmp_path):
    """the mirror's removal raises (it may have moved rows already): the host side stays as it was and the mirror is dropped, so the
    next device_index() rebuilds it and row ids keep equalling hash_id_to_idx"""
    class Mirror:
        closed = False

        def remove_ids(self, ids):
            raise RuntimeError("device lost")

        def close(self):
            self.closed = True

    enc = FakeEmbedder(16)
    st = EmbeddingStore(enc, str(tmp_path), 8, "chunk")
    st.insert_strings(TEXTS)
    ids0, mat0 = list(st.hash_ids), st._mat[:st._n].copy()
    st._index = mirror = Mirror()
    with pytest.raises(RuntimeError, match="device lost"):
        st.delete([ids0[3]])
    assert st._index is None and mirror.closed
    assert list(st.hash_ids) == ids0 and np.array_equal(st._mat[:st._n], mat0) and st.hash_id_to_idx[ids0[3]] == 3
    _same_store(st, EmbeddingStore(enc, str(tmp_path), 8, "chunk"))

    class Short(Mirror):
        def remove_ids(self, ids):
            return 0

    st._index = Short()
    with pytest.raises(RuntimeError, match="removed 0 rows of 1"):
        st.delete([ids0[3]])
    assert st._index is None and list(st.hash_ids) == ids0
    assert st.delete([ids0[3]]) == 1 and len(st.hash_ids) == 11


def test_sidecar_delete_crash_windows(tmp_path):
    """Every state a crash inside the sidecar rewrite can leave — the temporary files of each step left in place — loads as the old
    store (before the commit marker) or the new one (from the marker on), never a mix."""
    enc = FakeEmbedder(16)
    old_dir, new_dir = tmp_path / "old", tmp_path / "new"
    st = EmbeddingStore(enc, str(old_dir), 8, "c", persist="sidecar")
    st.insert_strings(TEXTS)
    shutil.copytree(old_dir, new_dir)
    new = EmbeddingStore(enc, str(new_dir), 8, "c", persist="sidecar")
    assert new.delete([new.hash_ids[0], new.hash_ids[7]]) == 2
    assert sorted(os.listdir(new_dir)) == sorted(os.listdir(old_dir))      # no temporary file survives a completed delete
    rows, mat = "vdb_c.rows.jsonl", "vdb_c.f32"
    marker = rows + ".del.commit"

    def state(name, base, extra):
        d = tmp_path / name
        shutil.copytree(base, d)
        for dst, (src_dir, src) in extra.items():
            if src_dir is None:
                (d / dst).write_text(src)
            else:
                shutil.copy(src_dir / src, d / dst)
        return EmbeddingStore(enc, str(d), 8, "c", persist="sidecar"), d

    torn = (new_dir / mat).read_bytes()[:37]
    (tmp_path / "torn.f32").write_bytes(torn)
    before = [  # step 1 under way or done, no marker: the old store
        {mat + ".del": (tmp_path, "torn.f32")},
        {mat + ".del": (new_dir, mat)},
        {mat + ".del": (new_dir, mat), rows + ".del": (new_dir, rows)},
        {mat + ".del": (new_dir, mat), rows + ".del": (new_dir, rows), marker + ".tmp": (None, '{"ro')},
    ]
    for i, extra in enumerate(before):
        got, d = state(f"b{i}", old_dir, extra)
        _same_store(got, st)
        assert sorted(os.listdir(d)) == sorted(os.listdir(old_dir))
    # marker written: the new store, whichever replaces had happened
    after = [
        (old_dir, {mat + ".del": (new_dir, mat), rows + ".del": (new_dir, rows), marker: (None, '{"rows": 10}')}),      # neither replace
        (old_dir, {mat: (new_dir, mat), rows + ".del": (new_dir, rows), marker: (None, '{"rows": 10}')}),              # the matrix replaced
        (new_dir, {marker: (None, '{"rows": 10}')}),                                                                   # both replaced, marker left
    ]
    for i, (base, extra) in enumerate(after):
        got, d = state(f"a{i}", base, extra)
        _same_store(got, new)
        assert sorted(os.listdir(d)) == sorted(os.listdir(old_dir))
        got.insert_strings(["one more"])                                                                              # and it goes on appending
        _same_store(got, EmbeddingStore(enc, str(d), 8, "c", persist="sidecar"))
