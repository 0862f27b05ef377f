"""Filtered search from row-id lists (cmr_index_row_masks_dev, cmr_index_search_ids*, cmr_mindex_search_ids).  Every
comparison is `np.array_equal` on ids and on score bits, no tolerance.  The oracle is code that existed before the feature:
`pack_row_mask(s)` for the words, `search_filtered(_each)` on packed masks for the results; for indexes with an id base or a block table
the local rows come from the numpy model in tests/filtered_ids_model.py (held against `pack_row_masks` in tests/test_filtered_ids_host.py).
Corpora and indexes are built once per module, with the shapes of tests/test_filtered_each_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_id_lists, pack_row_mask, pack_row_masks
from tests import filtered_ids_model as M

pytestmark = pytest.mark.gpu

CHAIN, MORE_PASSES, FILTERED, EACH, IDS = 3, 1 << 11, 1 << 12, 1 << 13, 1 << 14
N_SMALL = 1000                  # no sampling, partial last panel
N_ONE_LEVEL = 8192 + 5          # 257 panels: one sampling level
N_TWO_LEVELS = 131072 + 7       # 4097 panels: in-scan thresholds at nq <= 2, the single 128-panel level at nq <= 8, two levels above
SHAPES = {"bf16": 128, "f16": 96, "f32": 96}      # dim 96 is padded to 128
NQ_MAX = 65
BASE = 1_000_000

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


def _blocks(n):
    """a 3-block table with gaps for n rows: ids below 100, between the blocks and beyond the last one are held by nobody.  (n < 3: the
    later blocks start at or beyond the last row and hold nothing.)"""
    ls = [0, max(1, n // 3), max(2, 2 * n // 3)]
    return ls, [100, 100 + ls[1] + 50, 5_000_000]


def _index(dtype, n, kind="plain"):
    """kind: "plain" (ids = local rows), "based" (set_id_base(BASE)), "blocked" (set_id_blocks(*_blocks(n)))"""
    from comorag_amd.index import DenseIndex
    key = ("index", dtype, n, kind)
    if key not in _cache:
        idx = DenseIndex(SHAPES[dtype], dtype)
        idx.append(_rows(dtype, n)[0])
        if kind == "based":
            idx.set_id_base(BASE)
        elif kind == "blocked":
            idx.set_id_blocks(*_blocks(n))
        _cache[key] = idx
    return _cache[key]


def _domain(kind, n):
    """(keyword arguments of the model, local row -> id as the searches return it)"""
    if kind == "plain":
        return {}, lambda r: np.asarray(r, dtype=np.int64)
    if kind == "based":
        return {"base": BASE}, lambda r: np.asarray(r, dtype=np.int64) + BASE
    ls, gs = _blocks(n)

    def to_global(r):
        r = np.asarray(r, dtype=np.int64)
        b = np.searchsorted(np.asarray(ls), r, side="right") - 1
        return np.asarray(gs)[b] + r - np.asarray(ls)[b]
    return {"blocks": (ls, gs)}, to_global


def teardown_module(module):
    for key, v in list(_cache.items()):
        if key[0] == "index":
            v.close()
    _cache.clear()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """(ids, scores, min, max) against (ids, scores, min, max): ids whole, everything else by its bits"""
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), what
    for a, b in zip(got[1:], want[1:]):
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _device_words(idx, mode, offsets, ids, nq=1):
    import torch
    dev = torch.device("cuda", 0)
    ids_t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(dev)
    off_t = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(dev) if offsets is not None else None
    w = idx.row_masks_dev(ids_t, off_t, nq=nq, mode=mode)
    torch.cuda.synchronize(dev)
    return w.cpu().numpy().view(np.uint32)


# ---- 1. the builder writes the words of pack_row_masks, whole
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 8197])
@pytest.mark.parametrize("kind", ["plain", "based", "blocked"])
def test_builder_writes_the_words_of_pack_row_masks(n, kind):
    idx = _index("bf16", n, kind)
    kw, glob = _domain(kind, n)
    rng = np.random.default_rng(n)
    edge = sorted({0, min(31, n - 1), min(32, n - 1), n - 1})
    beyond = glob([n - 1])[0]
    junk = np.array([-1, -1, -5, -(1 << 40), beyond + 1, beyond + 12345, 1 << 40], dtype=np.int64)      # padding, other negatives, ids past the last row
    if kind == "based":
        junk = np.concatenate([junk, [0, BASE - 1]])                                                    # below the base: not held
    if kind == "blocked":
        ls, gs = _blocks(n)
        junk = np.concatenate([junk, [0, 99, gs[0] + ls[1], gs[1] - 1, gs[2] - 1]])                      # below the first block and in the gaps
    few = rng.choice(n, min(n, 5), replace=False)
    lists = {"empty": np.empty(0, np.int64), "every": glob(np.arange(n)), "edges": glob(edge), "dups": glob(np.concatenate([few, few, edge])),
             "junk": junk, "mixed": rng.permutation(np.concatenate([glob(few), junk, glob(edge)]))}
    assert len(idx) == n
    for mode in ("exclude", "allow"):
        for name, lst in lists.items():                 # one shared list -> the words of ONE pack_row_mask
            got = _device_words(idx, mode, None, lst)
            want = M.words_of(n, 1, mode, None, lst, **kw)
            assert got.shape == want.shape and np.array_equal(got, want), (kind, n, mode, name)
        names = list(lists)
        for nq in (1, 3):                               # per-query lists, every kind of list at every position
            for rot in range(len(names) if nq == 3 else 1):
                per = [lists[names[(rot + i) % len(names)]] for i in range(nq)] if nq == 3 else [lists["mixed"]]
                off, flat = pack_id_lists(**{mode: per})
                got = _device_words(idx, mode, off, flat)
                want = M.words_of(n, nq, mode, off, flat, **kw)
                assert got.shape == (nq, (n + 31) // 32) and np.array_equal(got, want), (kind, n, mode, nq, rot)
    if kind == "plain":                                 # the model itself, once more against the plain packer on this size
        held = [r for r in lists["mixed"].tolist() if 0 <= r < n]
        assert np.array_equal(M.words_of(n, 1, "exclude", None, lists["mixed"]), pack_row_mask(n, exclude=held))
        assert np.array_equal(_device_words(idx, "exclude", None, lists["empty"]), pack_row_mask(n))      # tail bits zero
    # a wrong word count is refused before anything is written
    import torch
    ids_t = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    w_t = torch.zeros(((n + 31) // 32) + 1, dtype=torch.int32, device="cuda:0")
    rc = L.lib().cmr_index_row_masks_dev(idx._h, 0, 1, None, C.c_void_p(ids_t.data_ptr()), 1, C.c_void_p(w_t.data_ptr()), w_t.shape[0], None)
    assert rc == L.CMR_ERR_INVALID and b"n_words" in L.lib().cmr_last_error()


# ---- 2. the search equals search_filtered_each on packed masks
def _mixed_lists(n, nq, seed):
    """a few rows, half of the rows, nothing, every row — dealt round robin, so every kind meets every lane position"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nq):
        j = i % 4
        out.append(rng.choice(n, 7, replace=False) if j == 0 else np.flatnonzero(rng.random(n) < 0.5) if j == 1 else np.empty(0, np.int64) if j == 2
                   else np.arange(n))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("n", [N_SMALL, N_ONE_LEVEL])
def test_search_equals_the_per_query_masked_call(dtype, n):
    idx = _index(dtype, n)
    k = 20
    for nq in (1, 8, 33, 65):
        Q = _rows(dtype, n)[1][:nq]
        lists = _mixed_lists(n, nq, seed=n + nq)
        for mode in ("exclude", "allow"):               # exclude a few / half / nothing / everything; allow a few / half / nothing / everything
            got = idx.search_filtered_ids(Q, k, **{mode: lists})
            r = idx.get_option("last_route")
            want = idx.search_filtered_each(Q, k, masks=pack_row_masks(n, **{mode: lists}))
            r_want = idx.get_option("last_route")
            _same(got, want, f"{dtype} n={n} nq={nq} {mode}")
            assert got[0].shape == (nq, k)
            assert r & 0xF == CHAIN and r & FILTERED and r & EACH and r & IDS, hex(r)          # bits 12, 13, 14
            assert r == r_want | IDS and not r_want & IDS, (hex(r), hex(r_want))               # the masked route's bits plus bit 14
            if nq > 64:
                assert r & MORE_PASSES, hex(r)
            none = [i for i in range(nq) if (i % 4 == 3 if mode == "exclude" else i % 4 == 2)]          # queries that allow nothing
            if none:
                assert (got[0][none] == -1).all() and np.isneginf(got[1][none]).all()
                assert np.isposinf(got[2][none]).all() and np.isneginf(got[3][none]).all()
    assert idx.search_filtered_ids(Q, k, exclude=lists, with_minmax=False)[2:] == (None, None)
    idx.search(Q, k)
    assert not idx.get_option("last_route") & (FILTERED | EACH | IDS)


# ---- 3. adversarial lists
@pytest.mark.parametrize("n", [N_ONE_LEVEL, N_TWO_LEVELS])
@pytest.mark.parametrize("nq", [1, 2, 8, 33])
def test_adversarial_lists(n, nq):
    """every query excludes exactly its OWN unfiltered top-k (ids as `search` returned them): a sampling threshold taken from unmasked
    rows loses allowed rows; then every query allows only 3k rows: its sample holds fewer than k"""
    dtype, k = "bf16", 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    top = idx.search(Q, k)[0]
    got = idx.search_filtered_ids(Q, k, exclude=top)                    # the 2-d result goes straight back in
    want = idx.search_filtered_each(Q, k, masks=pack_row_masks(n, exclude=list(top)))
    _same(got, want, f"own top-k n={n} nq={nq}")
    for i in range(nq):
        assert not np.isin(got[0][i], top[i]).any() and (got[0][i] >= 0).all()
    few = [np.random.default_rng(n + nq + i).choice(n, 3 * k, replace=False) for i in range(nq)]
    got = idx.search_filtered_ids(Q, k, allow=few)
    want = idx.search_filtered_each(Q, k, masks=pack_row_masks(n, allow=few))
    _same(got, want, f"3k rows n={n} nq={nq}")
    for i in range(nq):
        assert np.isin(got[0][i], few[i]).all()


# ---- 4. a shared list is the shared-mask call
@pytest.mark.parametrize("n,nq", [(N_SMALL, 33), (N_ONE_LEVEL, 65), (N_TWO_LEVELS, 8)])
def test_shared_list_equals_the_shared_mask_call(n, nq):
    dtype, k = "bf16", 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    rng = np.random.default_rng(n)
    pool = np.unique(idx.search(Q, k)[0])                               # what a pool dedup holds: rows earlier searches returned
    for mode, lst in (("exclude", pool), ("allow", rng.choice(n, n // 2, replace=False)), ("exclude", []), ("allow", [])):
        got = idx.search_filtered_ids(Q, k, **{mode: lst})
        r = idx.get_option("last_route")
        want = idx.search_filtered(Q, k, mask=pack_row_mask(n, **{mode: lst}))
        assert r == idx.get_option("last_route") | IDS, hex(r)
        kk = want[0].shape[1]                                           # search_filtered trims to the allowed rows, the id form always has k columns
        _same((got[0][:, :kk], got[1][:, :kk], got[2], got[3]), want, f"shared {mode} n={n}")
        assert (got[0][:, kk:] == -1).all() and np.isneginf(got[1][:, kk:]).all()
        assert r & 0xF == CHAIN and r & FILTERED and r & IDS and not r & EACH, hex(r)
    _same(idx.search_filtered_ids(Q, k, exclude=[])[:2], idx.search(Q, k)[:2], "exclude nothing is the plain search")


# ---- 5. ids in the returned domain
@pytest.mark.parametrize("kind", ["based", "blocked"])
def test_ids_are_in_the_domain_the_searches_return(kind):
    dtype, n, nq, k = "f16", N_SMALL, 8, 20
    idx = _index(dtype, n, kind)
    kw, glob = _domain(kind, n)
    Q = _rows(dtype, n)[1][:nq]
    top = idx.search(Q, k)[0]
    got = idx.search_filtered_ids(Q, k, exclude=top)
    for i in range(nq):
        assert not np.isin(got[0][i], top[i]).any() and (got[0][i] >= 0).all()
    off, flat = pack_id_lists(exclude=top)
    keeps = M.keeps_of(n, nq, "exclude", off, flat, **kw)
    assert all(int((~kp).sum()) == k for kp in keeps)                   # the model found every returned id on this index
    _same(got, idx.search_filtered_each(Q, k, masks=pack_row_masks(n, allow=keeps)), kind)
    shared = np.unique(top)
    got = idx.search_filtered_ids(Q, k, allow=shared)
    keep = M.keeps_of(n, 1, "allow", None, shared, **kw)[0]
    want = idx.search_filtered(Q, k, mask=pack_row_mask(n, allow=keep))
    _same(got, want, kind + " shared")
    assert np.isin(got[0], shared).all()
    # the same rows through the plain index: ids moved, score bits not
    plain = _index(dtype, n).search_filtered_each(Q, k, masks=pack_row_masks(n, allow=keeps))
    full = idx.search_filtered_ids(Q, k, exclude=top)
    assert np.array_equal(full[0], glob(plain[0])) and np.array_equal(_bits(full[1]), _bits(plain[1]))


def test_a_padded_result_passed_back_leaves_nothing():
    from comorag_amd.index import DenseIndex
    dtype, k = "bf16", 20
    X, Q = _rows(dtype, N_SMALL)
    idx = DenseIndex(SHAPES[dtype], dtype)
    try:
        idx.append(X[:10])
        ids = np.empty((2, k), np.int64); sc = np.empty((2, k), np.float32)
        L.check(L.lib().cmr_index_search(idx._h, Q[:2].ctypes.data, 2, k, ids.ctypes.data, sc.ctypes.data, None, None))
        assert (ids[:, :10] >= 0).all() and (ids[:, 10:] == -1).all()   # ten rows, then -1 padding
        got = idx.search_filtered_ids(Q[:2], k, exclude=ids)
        assert (got[0] == -1).all() and np.isneginf(got[1]).all() and np.isposinf(got[2]).all() and np.isneginf(got[3]).all()
        got = idx.search_filtered_ids(Q[:2], k, exclude=ids[0])        # the same as ONE shared list
        assert (got[0] == -1).all() and np.isposinf(got[2]).all()
        got = idx.search_filtered_ids(Q[:2], k, allow=ids)             # ... and allowed instead: the ten rows, padding behind
        assert np.array_equal(got[0], ids) and np.array_equal(_bits(got[1]), _bits(sc))
    finally:
        idx.close()


# ---- 6. the device forms equal the host form
@pytest.mark.parametrize("n,nq", [(N_SMALL, 8), (N_ONE_LEVEL, 65), (N_TWO_LEVELS, 2)])
def test_dev_forms_equal_the_host_form(n, nq):
    import torch
    dtype, k = "bf16", 20
    idx = _index(dtype, n)
    Q = _rows(dtype, n)[1][:nq]
    lists = _mixed_lists(n, nq, seed=3 * n + nq)
    dev = torch.device("cuda", 0)
    q_t = torch.from_numpy(Q).to(dev)
    for mode in ("exclude", "allow"):
        host = idx.search_filtered_ids(Q, k, **{mode: lists})
        off, flat = pack_id_lists(**{mode: lists})
        ids_t, off_t = torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)
        # build once, search many times
        words_t = idx.row_masks_dev(ids_t, off_t, mode=mode)
        assert tuple(words_t.shape) == (nq, (n + 31) // 32)
        for _ in range(2):
            mn_t = torch.empty(nq, dtype=torch.float32, device=dev); mx_t = torch.empty(nq, dtype=torch.float32, device=dev)
            oi_t, os_t = idx.search_filtered_each_dev(q_t, k, words_t, out_min=mn_t, out_max=mx_t)
            torch.cuda.synchronize(dev)
            _same((oi_t.cpu().numpy(), os_t.cpu().numpy(), mn_t.cpu().numpy(), mx_t.cpu().numpy()), host, f"builder + masked_each_dev {mode}")
        # the one-call device form
        mn_t = torch.empty(nq, dtype=torch.float32, device=dev); mx_t = torch.empty(nq, dtype=torch.float32, device=dev)
        oi_t, os_t = idx.search_filtered_ids_dev(q_t, k, ids_t, off_t, mode=mode, out_min=mn_t, out_max=mx_t)
        torch.cuda.synchronize(dev)
        r = idx.get_option("last_route")
        _same((oi_t.cpu().numpy(), os_t.cpu().numpy(), mn_t.cpu().numpy(), mx_t.cpu().numpy()), host, f"search_ids_dev {mode}")
        assert r & IDS and r & EACH and bool(r & MORE_PASSES) == (nq > 64), hex(r)
        # a shared list on the device
        sh_t = torch.from_numpy(np.ascontiguousarray(lists[0], dtype=np.int64)).to(dev)
        oi_t, os_t = idx.search_filtered_ids_dev(q_t, k, sh_t, None, mode=mode)
        torch.cuda.synchronize(dev)
        want = idx.search_filtered_ids(Q, k, **{mode: lists[0]})
        _same((oi_t.cpu().numpy(), os_t.cpu().numpy()), want[:2], f"shared search_ids_dev {mode}")
    assert not idx.query_status()
    with pytest.raises(ValueError):
        idx.search_filtered_ids_dev(q_t, k, ids_t, off_t[:-1])
    with pytest.raises(ValueError):
        idx.search_filtered_ids_dev(q_t, k, ids_t, off_t, mode="neither")


# ---- 7. the multi-device index, logical shards on one GPU
@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("block_rows", [256, 1024])
def test_multi_device_index_equals_one_index(S, block_rows):
    from comorag_amd.multi_index import MultiDeviceIndex
    dtype, n, k = "bf16", N_ONE_LEVEL, 20
    X, Qall = _rows(dtype, n)
    one = _index(dtype, n)
    multi = MultiDeviceIndex(SHAPES[dtype], dtype, devices=[0] * S, options={"append_block_rows": block_rows})
    try:
        empty = multi.search_filtered_ids(Qall[:3], k, exclude=[1, 2])
        assert (empty[0] == -1).all() and np.isneginf(empty[1]).all() and np.isposinf(empty[2]).all() and np.isneginf(empty[3]).all()
        for a, b in ((0, 700), (700, 3001), (3001, n)):                 # three uneven pieces: shards hold several blocks
            multi.append(X[a:b])
        assert len(multi) == n and (S == 1 or min(multi.shard_rows()) > 0)
        nq = 8
        Q = Qall[:nq]
        top = multi.search(Q, k)[0]
        assert np.array_equal(top, one.search(Q, k)[0])
        # each query excludes its own top-k
        _same(multi.search_filtered_ids(Q, k, exclude=top), one.search_filtered_each(Q, k, exclude=list(top)), f"S={S} own top-k")
        # query 0 allows only rows of ONE shard, query 1 nothing, the others a random 1 % / half
        sh = multi.shard(S - 1)
        on_one_shard = np.unique(sh.search(Q[:1], 128)[0][0])
        assert len(on_one_shard) == 128
        rng = np.random.default_rng(S * 10000 + block_rows)
        allow = [on_one_shard, np.empty(0, np.int64)] + [np.flatnonzero(rng.random(n) < (0.01 if i % 2 else 0.5)) for i in range(2, nq)]
        got = multi.search_filtered_ids(Q, k, allow=allow)
        _same(got, one.search_filtered_each(Q, k, allow=allow), f"S={S} one shard / nothing / random")
        assert np.isin(got[0][0], on_one_shard).all() and (got[0][1] == -1).all() and np.isposinf(got[2][1]) and np.isneginf(got[3][1])
        # a shared list
        pool = np.unique(top)
        got = multi.search_filtered_ids(Q, k, exclude=pool)
        want = one.search_filtered(Q, k, exclude=pool)
        _same(got, want, f"S={S} shared")
        assert not np.isin(got[0], pool).any()
        # nq = 65: more than one group of the builder
        lists = _mixed_lists(n, NQ_MAX, seed=S + block_rows)
        _same(multi.search_filtered_ids(Qall, k, exclude=lists), one.search_filtered_each(Qall, k, exclude=lists), f"S={S} nq=65")
        # an id lands on exactly one shard: the union of the shards' rows under "allow everything" is every row once
        every = multi.search_filtered_ids(Q[:1], 128, allow=np.arange(n))
        _same(every, one.search_filtered_each(Q[:1], 128, allow=[np.arange(n)]), f"S={S} everything")
        with pytest.raises(L.CmrError) as e:
            multi.search_filtered_ids(Q, 129, exclude=top)
        assert e.value.code == L.CMR_ERR_UNSUPPORTED
    finally:
        multi.close()


# ---- 8. errors on a live index; nothing else moves
def test_errors_and_other_calls_keep_their_bits():
    dtype, n, nq, k = "bf16", N_ONE_LEVEL, 8, 20
    idx = _index(dtype, n)
    Q = np.ascontiguousarray(_rows(dtype, n)[1][:nq])
    shared = np.random.default_rng(9).random(n) < 0.5
    keeps = [np.random.default_rng(5 + 7919 * i).random(n) < 0.5 for i in range(nq)]

    def others():
        return [*idx.search(Q, k), *idx.search_filtered(Q, k, allow=shared), *idx.search_filtered_each(Q, k, allow=keeps)]

    before, stats = others(), idx.combine_stats()
    top = idx.search(Q, k)[0]
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_ids(Q, 129, exclude=top)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_ids(Q, 0, exclude=top)
    assert e.value.code == L.CMR_ERR_INVALID
    with pytest.raises(ValueError):
        idx.search_filtered_ids(Q, k, exclude=list(top[:3]))           # three lists for eight queries
    with pytest.raises(ValueError):
        idx.search_filtered_ids(Q, k)
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    ids = np.zeros((nq, k), np.int64); sc = np.zeros((nq, k), np.float32)
    off, flat = pack_id_lists(exclude=top)
    call = L.lib().cmr_index_search_ids
    assert call(idx._h, p(Q), nq, k, 2, p(off), p(flat), len(flat), p(ids), p(sc), None, None) == L.CMR_ERR_INVALID      # mode 2 is refused
    bad = off.copy(); bad[3] = bad[2] - 1
    assert call(idx._h, p(Q), nq, k, 0, p(bad), p(flat), len(flat), p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), nq, k, 0, p(off), p(flat), len(flat) - 1, p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), nq, k, 0, p(off), None, len(flat), p(ids), p(sc), None, None) == L.CMR_ERR_INVALID
    assert call(idx._h, p(Q), nq, k, 0, p(off), p(flat), len(flat), p(ids), p(sc), None, None) == L.CMR_OK
    bad_q = Q.copy(); bad_q[1, 3] = np.nan
    with pytest.raises(L.CmrError) as e:
        idx.search_filtered_ids(bad_q, k, exclude=top)
    assert e.value.code == L.CMR_ERR_NONFINITE
    good = idx.search_filtered_ids(Q, k, exclude=top)                   # the flag is re-armed: the next call is served
    _same(good, idx.search_filtered_each(Q, k, exclude=list(top)))
    idx.set_option("combine", 4); idx.set_option("combine_filtered", 1)  # never combined, whether or not combine_filtered is set
    try:
        _same(idx.search_filtered_ids(Q, k, exclude=top), good)
        assert idx.combine_stats() == stats
    finally:
        idx.set_option("combine_filtered", 0); idx.set_option("combine", 0)
    after = others()
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert idx.combine_stats() == stats


# ---- 9. the retrieval sibling
def test_retrieval_sibling_on_both_index_classes():
    from comorag_amd.multi_index import MultiDeviceIndex
    from comorag_amd.retrieval import dense_passage_topk, dense_passage_topk_filtered_each, dense_passage_topk_filtered_ids
    dtype, n, k = "bf16", N_SMALL, 20
    idx = _index(dtype, n)
    X, Q = _rows(dtype, n)
    Q = Q[:4]
    top_ids, _ = dense_passage_topk(idx, Q, k)
    pools = [np.unique(top_ids[i, : 3 + 2 * i]) for i in range(4)]          # every question's pool holds some of ITS best rows
    ids, sc = dense_passage_topk_filtered_ids(idx, Q, k, exclude_ids=pools)
    want = dense_passage_topk_filtered_each(idx, Q, k, exclude_rows=pools)
    assert np.array_equal(ids, want[0]) and np.array_equal(_bits(sc), _bits(want[1]))
    for i in range(4):
        assert not np.isin(ids[i], pools[i]).any()
    allow = [np.flatnonzero(~np.isin(np.arange(n), pools[i])) for i in range(4)]
    ids2, sc2 = dense_passage_topk_filtered_ids(idx, Q, k, allow_ids=allow)
    assert np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc))
    multi = MultiDeviceIndex(SHAPES[dtype], dtype, devices=[0] * 3, options={"append_block_rows": 128})
    try:
        multi.append(X[:450]); multi.append(X[450:])
        ids3, sc3 = dense_passage_topk_filtered_ids(multi, Q, k, exclude_ids=pools)
        assert np.array_equal(ids3, ids) and np.array_equal(_bits(sc3), _bits(sc))
    finally:
        multi.close()
