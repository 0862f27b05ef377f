"""The numpy model of the diversified top-k (include/comorag_hip.h states the contract) and the inputs its tests share.

`select` is the selection exactly as the header defines it, in float32 numpy operations (numpy does not fuse a multiply into a subtract);
`gram` builds the pair scores from the calls that existed before the feature — `scores(get_rows(ids))[:, ids]` — with void positions at
-inf.  Inputs are clustered rows with near-duplicates: at lambda 0.5 every query's MMR list differs from its plain top-k (checked by the
tests that use them), at lambda 1 it equals it."""
import numpy as np

NEG_INF = np.float32(-np.inf)
# (n, d, nq, F, k): the shapes at which the recipe below was checked on bf16-rounded operands
SHAPES = [(200, 64, 5, 32, 8), (1000, 768, 3, 128, 20), (333, 40, 65, 33, 10), (70, 768, 2, 31, 31)]


def inputs(n, d, nq, seed=0):
    """8 unit centres; row i = normalise(centre[i % 8] + 0.25 N(0, I) / sqrt(d)); rows 17, n // 2 and n - 1 are bit-equal copies of row 3;
    a query is the normalised sum of 1.0 / 0.6 / 0.3 x three random centres.  -> X [n, d], Q [nq, d] float32"""
    rng = np.random.default_rng(9000 + seed)
    C = rng.standard_normal((8, d)).astype(np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    X = C[np.arange(n) % 8] + np.float32(0.25 / np.sqrt(d)) * rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    for r in (17, n // 2, n - 1):
        if 3 < n and r < n:
            X[r] = X[3]
    Q = np.empty((nq, d), np.float32)
    for i in range(nq):
        c = rng.choice(8, size=3, replace=False)
        v = 1.0 * C[c[0]] + 0.6 * C[c[1]] + 0.3 * C[c[2]]
        Q[i] = v / np.linalg.norm(v)
    return np.ascontiguousarray(X, np.float32), Q


def void_positions(ids, G=None):
    """bool [F]: negative id, an earlier position with the same id, or (G given) a position whose own pair score is -inf — how `gram` and
    `pair_scores` mark an id the index does not hold"""
    ids = np.asarray(ids, np.int64)
    v = ids < 0
    seen = set()
    for p, i in enumerate(ids.tolist()):
        if i in seen:
            v[p] = True
        seen.add(i)
    if G is not None:
        v |= np.isneginf(np.diag(np.asarray(G, np.float32)))
    return v


def select_one(rel, G, ids, k, lam):
    rel, G, ids = np.asarray(rel, np.float32), np.asarray(G, np.float32), np.asarray(ids, np.int64)
    F = len(ids)
    lam32 = np.float32(lam)
    oml = np.float32(1.0) - lam32
    open_ = ~void_positions(ids, G)
    pen = np.full(F, NEG_INF, np.float32)
    out_ids, out_sc = np.full(k, -1, np.int64), np.full(k, NEG_INF, np.float32)
    with np.errstate(invalid="ignore"):
        for n in range(k):
            cand = np.flatnonzero(open_)
            if len(cand) == 0:
                break
            val = rel if n == 0 else (lam32 * rel) - (oml * pen)          # two rounded products, one rounded difference
            assert val.dtype == np.float32
            best = cand[int(np.argmax(val[cand]))]                         # IEEE comparisons; the first of equal values
            out_ids[n], out_sc[n] = ids[best], rel[best]
            open_[best] = False
            pen = np.maximum(pen, G[best])
    return out_ids, out_sc


def select(rel, G, ids, k, lam):
    """rel [nq, F], G [nq, F, F], ids [nq, F] -> (ids [nq, k], scores [nq, k]) in pick order, -1 / -inf padded"""
    rel, G, ids = np.atleast_2d(rel), np.asarray(G), np.atleast_2d(ids)
    if G.ndim == 2:
        G = G[None]
    got = [select_one(rel[i], G[i], ids[i], k, lam) for i in range(len(ids))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def gram(idx, ids, base=0):
    """[nq, F, F] (or [F, F]) pair scores from the existing calls: G[s, c] = idx.scores(idx.get_rows([ids[s]]))[0, ids[c] - base]; rows and
    columns of void positions (negative, outside [base, base + len), repeated) are -inf"""
    ids = np.asarray(ids, np.int64)
    one = ids.ndim == 1
    ids2 = ids[None] if one else ids
    n = len(idx)
    held = (ids2 >= base) & (ids2 < base + n)
    uniq = np.unique(ids2[held])
    S = idx.scores(idx.get_rows(uniq)) if len(uniq) else np.empty((0, n), np.float32)      # [U, n]: one call for every query
    at = {int(u): j for j, u in enumerate(uniq.tolist())}
    out = np.full(ids2.shape + (ids2.shape[1],), NEG_INF, np.float32)
    for q in range(len(ids2)):
        ok = held[q] & ~void_positions(ids2[q])
        pos = np.flatnonzero(ok)
        if len(pos):
            rows = np.array([at[int(i)] for i in ids2[q][pos]])
            out[q][np.ix_(pos, pos)] = S[rows][:, ids2[q][pos] - base]
    return out[0] if one else out


def gram_f64(Xr, ids):
    """pair scores from fp64 products of the (rounded) rows Xr, cast to fp32; void positions -inf"""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(Xr)) & ~void_positions(ids)
    pos = np.flatnonzero(ok)
    out = np.full((len(ids), len(ids)), NEG_INF, np.float32)
    R = Xr[ids[pos]].astype(np.float64)
    out[np.ix_(pos, pos)] = (R @ R.T).astype(np.float32)
    return out


def topk(S, k):
    """the exported order (score descending, row ascending) of score rows S [nq, n] -> ids [nq, k], scores [nq, k]"""
    ids = np.stack([np.lexsort((np.arange(S.shape[1]), -r.astype(np.float64)))[:k] for r in S]).astype(np.int64)
    return ids, np.take_along_axis(S, ids, axis=1)
