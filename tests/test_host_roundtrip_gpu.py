"""The host round trip behind the synchronous top-k calls: `search`, `search_filtered`, `search_filtered_each` and
`search_filtered_ids` on ONE index from one thread, so every call takes the same pooled workspace — its packed device buffer with the
non-finite flag at its head, its pinned host buffer, its query / mask / list scratch.  What is pinned is the interplay: buffers that grow
in the middle of a sequence and are reused afterwards, a flag left by one form and met by another, the mapped unfiltered path and the
copied filtered paths taking turns on one pinned buffer.
The oracle of every call is the matching `_dev` form on device tensors (`search_dev`, `search_filtered_dev`, `search_filtered_each_dev`,
`search_filtered_ids_dev`), which writes straight into the caller's tensors and never touches the packed path; it runs on an index of
its own that holds the same rows, once per (form, nq, k).  Every comparison is `np.array_equal` on ids and on the bits of scores, min
and max."""
import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_id_lists, pack_row_mask, pack_row_masks

pytestmark = pytest.mark.gpu

N, DIM = 1000, 40                # 32 panels, the last one partial
# the third shape outgrows the 4096-byte first packed buffer and the pinned buffer (both are reallocated mid-sequence) and, beyond 64
# queries, takes two groups in the per-query id-list form; the fourth runs in the grown buffers
SHAPES = [(1, 1), (3, 20), (70, 128), (1, 1)]
NQ_MAX = 70
FORMS = ["search", "filtered", "each", "ids_shared", "ids_each"]
FILTERED_FORMS = FORMS[1:]
MORE_PASSES = 1 << 11

_cache = {}


def _data():
    if "data" not in _cache:
        rng = np.random.default_rng(40_1000)
        X = rng.standard_normal((N, DIM)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        Q = rng.standard_normal((NQ_MAX, DIM)).astype(np.float32)
        Q[::2] = X[rng.integers(0, N, len(Q[::2]))] + 0.05 * Q[::2]
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        keep = rng.random((NQ_MAX, N)) < 0.5
        keep[1] = False
        keep[1, [3, 31, 32, 500, N - 1]] = True          # fewer than k rows: padded
        keep[5] = False                                   # no row at all
        lists = [rng.choice(N, size=int(rng.integers(0, 400)), replace=False).astype(np.int64) for _ in range(NQ_MAX)]
        lists[2] = np.empty(0, dtype=np.int64)
        _cache["data"] = {"X": X, "Q": Q, "mask": pack_row_mask(N, allow=rng.random(N) < 0.5), "masks": pack_row_masks(N, allow=keep),
                          "shared": rng.choice(N, size=100, replace=False).astype(np.int64), "lists": lists}
    return _cache["data"]


def _index(zero_copy):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(DIM, "bf16", options={"zero_copy": zero_copy})
    idx.append(_data()["X"])
    return idx


def teardown_module(module):
    if "oracle_index" in _cache:
        _cache["oracle_index"].close()
    _cache.clear()


def _oracle(form, nq, k):
    """(ids [nq,k], scores [nq,k], min [nq], max [nq]) of the `_dev` form, -1 / -inf padded"""
    key = ("oracle", form, nq, k)
    if key in _cache:
        return _cache[key]
    import torch
    if "oracle_index" not in _cache:
        _cache["oracle_index"] = _index(1)
    idx, d, dev = _cache["oracle_index"], _data(), torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q_t = up(d["Q"][:nq])
    mn, mx = torch.empty(nq, dtype=torch.float32, device=dev), torch.empty(nq, dtype=torch.float32, device=dev)
    if form == "search":
        ids, sc = idx.search_dev(q_t, k, out_min=mn, out_max=mx)
    elif form == "filtered":
        ids, sc = idx.search_filtered_dev(q_t, k, up(d["mask"].view(np.int32)), out_min=mn, out_max=mx)
    elif form == "each":
        ids, sc = idx.search_filtered_each_dev(q_t, k, up(d["masks"][:nq].view(np.int32)), out_min=mn, out_max=mx)
    elif form == "ids_shared":
        ids, sc = idx.search_filtered_ids_dev(q_t, k, up(d["shared"]), None, mode="exclude", out_min=mn, out_max=mx)
    else:
        off, lst = pack_id_lists(exclude=d["lists"][:nq])
        ids, sc = idx.search_filtered_ids_dev(q_t, k, up(lst), up(off), mode="exclude", out_min=mn, out_max=mx)
    torch.cuda.synchronize(dev)
    _cache[key] = tuple(t.cpu().numpy() for t in (ids, sc, mn, mx))
    return _cache[key]


def _host(idx, form, q, k):
    d, nq = _data(), len(q)
    if form == "search":
        return idx.search(q, k)
    if form == "filtered":
        return idx.search_filtered(q, k, mask=d["mask"])
    if form == "each":
        return idx.search_filtered_each(q, k, masks=d["masks"][:nq])
    if form == "ids_shared":
        return idx.search_filtered_ids(q, k, exclude=d["shared"])
    return idx.search_filtered_ids(q, k, exclude=d["lists"][:nq])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(idx, form, nq, k, what):
    """the host form against its oracle; the host forms that know how many rows are allowed return only those columns"""
    ids, sc, mn, mx = _host(idx, form, _data()["Q"][:nq], k)
    w_ids, w_sc, w_mn, w_mx = _oracle(form, nq, k)
    what = f"{what}: {form} nq={nq} k={k}"
    cols = ids.shape[1]
    assert ids.shape == sc.shape == (nq, cols) and cols <= k, what
    assert np.array_equal(ids, w_ids[:, :cols]), what
    assert np.array_equal(_bits(sc), _bits(w_sc[:, :cols])), what
    assert np.all(w_ids[:, cols:] == -1), what
    assert np.array_equal(_bits(mn), _bits(w_mn)) and np.array_equal(_bits(mx), _bits(w_mx)), what


def _rotation(idx, what):
    for nq, k in SHAPES:
        for form in FORMS:
            _check(idx, form, nq, k, what)
            if form == "ids_each":
                assert bool(idx.get_option("last_route") & MORE_PASSES) == (nq > 64), f"{what}: groups of the id-list form at nq={nq}"


def _expect_nonfinite(idx, form, nq=3, k=20):
    q = _data()["Q"][:nq].copy()
    q[nq // 2, 7] = np.nan
    with pytest.raises(L.CmrError) as e:
        _host(idx, form, q, k)
    assert e.value.code == L.CMR_ERR_NONFINITE, form


def test_every_form_growing_shapes():
    idx = _index(0)
    try:
        _rotation(idx, "copied")
    finally:
        idx.close()


def test_flag_cleared_across_forms():
    """the flag lives in the shared packed buffer: whichever form left it, the next call — of another form — must not meet it"""
    idx = _index(0)
    try:
        for i, form in enumerate(FORMS):          # (the unfiltered copy path is the fifth user of the same flag)
            for step in (1, 2):
                _expect_nonfinite(idx, form)
                _check(idx, FORMS[(i + step) % len(FORMS)], 3, 20, f"after a NaN {form}")
    finally:
        idx.close()


def test_mapped_path_shares_the_workspace():
    """zero_copy = 1: the unfiltered calls map the pinned buffer, the filtered ones copy through it"""
    idx = _index(1)
    try:
        _rotation(idx, "mapped")
        for form in FILTERED_FORMS:
            _expect_nonfinite(idx, form)
            _check(idx, "search", 3, 20, f"mapped search after a NaN {form}")
            _check(idx, form, 3, 20, f"{form} after a mapped search")
    finally:
        idx.close()
