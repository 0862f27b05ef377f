"""Cases and the oracle of tests/test_range_search_gpu.py (range search: every row at or above a score bound, as CSR lists).  numpy
only; tests/test_range_inputs.py checks here, without a device, the properties the GPU tests rely on.  The inputs are the threshold
tests' own (tests/threshold_inputs.py, family C): they hold empty lists, lists above 128 (one selection list) and above 2048 (one tile of
the count / compaction kernels) hits."""
import numpy as np

from tests import threshold_inputs as ti

TILE = 2048          # CMR_RANGE_TILE
ROUTE_RANGE = 11     # CMR_ROUTE_RANGE
EXTRA_BOUNDS = [0.0, 0.3]

# tag -> (dtype, d, n, nq, seed): family C at the threshold routes' shapes and seeds, every dtype
CASES = {
    "c64-3-bf16": ("bf16", 64, 5003, 3, 51),
    "c64-40-f16": ("f16", 64, 5003, 40, 102),
    "c64-40-f32": ("f32", 64, 5003, 40, 102),
    "c768-bf16": ("bf16", 768, 8197, 70, 53),
    "c768-f16": ("f16", 768, 8197, 70, 54),
    "c200-f32": ("f32", 200, 8197, 70, 105),
}
# the issue's table: hits per query of the nq queries at bound 0.0 in fp64, (low, high)
ZERO_BOUND_HITS = {(64, 5003, 40, 102): (2383, 2626), (768, 8197, 70, 53): (3940, 4252), (200, 8197, 70, 105): (3918, 4251)}


def bounds(b_dup):
    return ti.bounds_around(b_dup) + EXTRA_BOUNDS


def make(tag):
    """-> (X, Q of the case's nq queries, index of the query with the tied rows, info)"""
    dtype, d, n, nq, seed = CASES[tag]
    X, Qall, info = ti.family_c(n, d, nq, seed)
    Q, q_dup = ti.pick_queries(Qall, nq)
    return X, Q, q_dup, info


def oracle(S, b, ids=None):
    """The lists a range search with bound b must return, from the scores S [nq, n] the library's own all-scores call gave: per query the
    rows with S >= float32(b), by descending score, then ascending row (-0.0 == +0.0 in both comparisons, as numpy compares); the score
    bits are S's.  ids: what row r is called (None: r).  -> (lims int64 [nq + 1], ids int64, scores fp32)"""
    S = np.asarray(S, np.float32)
    rows = np.arange(S.shape[1], dtype=np.int64)
    names = rows if ids is None else np.asarray(ids, np.int64)
    lims, out_ids, out_sc = [0], [], []
    for i in range(len(S)):
        keep = np.flatnonzero(S[i] >= np.float32(b))
        order = keep[np.lexsort((names[keep], -S[i][keep]))]
        out_ids.append(names[order]); out_sc.append(S[i][order])
        lims.append(lims[-1] + len(order))
    return (np.array(lims, np.int64), np.concatenate(out_ids).astype(np.int64) if out_ids else np.empty(0, np.int64),
            np.concatenate(out_sc).astype(np.float32) if out_sc else np.empty(0, np.float32))


def same(got, want, what=""):
    """bit for bit: lims, ids, and the scores as fp32 words"""
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float32, what
    assert np.array_equal(got[0], want[0]), (what, "lims")
    assert np.array_equal(got[1], want[1]), (what, "ids")
    assert np.array_equal(np.ascontiguousarray(got[2]).view(np.uint32), np.ascontiguousarray(want[2]).view(np.uint32)), (what, "score bits")


def lists(res):
    lims, ids, sc = res
    return [(ids[lims[i]:lims[i + 1]], sc[lims[i]:lims[i + 1]]) for i in range(len(lims) - 1)]


# ---- a -0.0 score next to +0.0 (no padding columns: d = 128 is the padded dim; bf16 / f32 hold 1e-30)
SIGNED_ZERO = dict(d=128, n=2100, neg_row=2077, zero_rows=[5, 2060])


def family_signed_zero(seed=0):
    """-> (X [n, 128], Q [3, 128]).  Query 0 is 1e-30 in every component: a unit row scores ~1e-31 (a normal fp32), the zero rows +0.0 —
    every product is +0.0 —, and row neg_row, -1e-30 in every component, a sum of products of -1e-60 each: below the smallest subnormal,
    so the fused multiply-adds of an fp32 index keep the sum at -0.0 (a 16-bit index rounds each product and adds -0.0 to +0.0: +0.0).
    Queries 1, 2: unit vectors."""
    z = SIGNED_ZERO
    rng = np.random.default_rng(9100 + seed)
    X = rng.standard_normal((z["n"], z["d"]), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X[z["zero_rows"]] = 0.0
    X[z["neg_row"]] = np.float32(-1e-30)
    Q = rng.standard_normal((3, z["d"]), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[0] = np.float32(1e-30)
    return X, Q
