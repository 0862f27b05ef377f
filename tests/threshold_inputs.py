"""Input families, the route table and the cut rule of tests/test_threshold_search_gpu.py (the threshold search — search_min_score —
on every route and through every entry point, compared bit for bit).  numpy only: tests/test_threshold_inputs.py checks here,
without a device, the properties the GPU tests rely on, so that none of them passes vacuously."""
import numpy as np

from oracle import retrieval_np as orc
from tests import value_domain_inputs as vd

FLT_MAX = float(np.finfo(np.float32).max)
KS = [1, 20, 33, 128]
P_K = 128                      # the plain search every cut is taken from: CMR_MAX_K, the longest list a threshold search returns
FIXED_BOUNDS = [0.95, 0.9, 0.8]      # with the attained bound: the bounds that leave empty, short and full lists of 20 side by side


# ---- the exact cut
def cut(P_ids, P_scores, b, k):
    """What the threshold search with bound b must return, bit for bit, from the plain search's lists P (score descending, row
    ascending, k <= their P_K columns; fewer columns and -1 / -inf entries where the index holds fewer rows):
    c_i = count(P_scores[i] >= b) compared in fp32 over the real entries; row i = P[i, :min(k, c_i)], then -1 / -inf.
    -> (ids int64 [nq, k], scores fp32 [nq, k], c int [nq])"""
    P_ids = np.asarray(P_ids, np.int64)
    P_scores = np.asarray(P_scores, np.float32)
    assert P_ids.shape == P_scores.shape and P_ids.ndim == 2 and 1 <= k <= P_K
    passes = (P_scores >= np.float32(b)) & (P_ids >= 0)
    c = passes.sum(axis=1)
    assert all(passes[i, :c[i]].all() for i in range(len(c))), "P is not sorted by descending score"
    ids = np.full((len(P_ids), k), -1, np.int64)
    sc = np.full((len(P_ids), k), -np.inf, np.float32)
    for i in range(len(P_ids)):
        m = min(k, int(c[i]))
        ids[i, :m] = P_ids[i, :m]
        sc[i, :m] = P_scores[i, :m]
    return ids, sc, c


def branch(c, k):
    return "empty" if c == 0 else "short" if c < k else "full"


def bounds_around(b_dup):
    """the bounds of every tagged route: the attained one and its two fp32 neighbours, the fixed ones, both infinities, +-FLT_MAX"""
    b = np.float32(b_dup)
    return [float(b), float(np.nextafter(b, np.float32(np.inf))), float(np.nextafter(b, np.float32(-np.inf)))] + FIXED_BOUNDS + \
           [-0.9, -np.inf, np.inf, FLT_MAX, -FLT_MAX]


# ---- family C: planted clusters
CENTRES = [7 + 13 * j for j in range(4)]      # queries 0..3 are these rows
MEMBERS = (0, 3, 40, 150)                     # rows planted around centre j
DUP_CLUSTER, DUP_MEMBER, Q_DUP, Q_NEG = 2, 20, 2, 4
PICK3 = [1, 2, 4]                             # a route of three queries takes these: a short list, the full one with the ties, the empty one


def dup_rows(n):
    """the three copies of member 20 of cluster 2: first panel, a middle panel, the last (partial) panel"""
    return [31, n // 2, n - 1]


def family_c(n, d, nq, seed=0):
    """-> (X [n, d], Q [max(nq, 5), d], info).  Rows: orc.synthetic_corpus; around centre j = row 7 + 13 j, MEMBERS[j] rows
    normalise(centre + s_i / sqrt(d) g), s_i = 0.05 + 0.55 i / m_j (scores from ~0.999 down to ~0.86), at seeded scattered positions
    inside [64, n - 64); member 20 of cluster 2 copied to dup_rows(n): four bit-equal rows, whose score for query 2 is the attained
    bound.  Queries: orc.synthetic_queries, 0..3 = the centres, 4 = -centre 1 (no row anywhere near).  info: members (positions per
    cluster), tied (the four bit-equal rows, ascending)."""
    assert n >= 1024 and n % 32
    X = orc.synthetic_corpus(n, d, seed=8000 + seed)
    Q = orc.synthetic_queries(max(nq, 5), d, seed=8100 + seed)
    rng = np.random.default_rng(8200 + seed)
    pos = rng.permutation(np.arange(64, n - 64))
    pos = pos[pos != n // 2][:sum(MEMBERS)]
    centres = X[CENTRES].copy()
    members, at = [], 0
    for j, m in enumerate(MEMBERS):
        rows = []
        for i in range(m):
            s = 0.05 + 0.55 * i / m
            v = centres[j] + np.float32(s / np.sqrt(d)) * rng.standard_normal(d, dtype=np.float32)
            X[pos[at]] = v / np.linalg.norm(v)
            rows.append(int(pos[at]))
            at += 1
        members.append(rows)
    src = members[DUP_CLUSTER][DUP_MEMBER]
    X[dup_rows(n)] = X[src]
    Q[:4] = centres
    Q[Q_NEG] = -centres[1]
    return X, Q, dict(members=members, tied=sorted([src] + dup_rows(n)))


def pick_queries(Q, nq):
    """-> (the route's nq queries, the index of the query with the tied rows among them)"""
    if nq < 5:
        assert nq == 3
        return np.ascontiguousarray(Q[PICK3]), PICK3.index(Q_DUP)
    return np.ascontiguousarray(Q[:nq]), Q_DUP


# ---- routes.  last_route of a threshold search: the path in the low byte with NO sampling level, bit 10 set
WIDE_PASS = {768: 256, 1024: 128}      # wide_pass_queries (csrc/search_plan.h) with wide_mode = 1 on a 16-bit index: queries of one wide pass
THRESHOLD = 1 << 10
BIG_OPTS = {"scan_no_small": 1, "scan_fin": 0, "sample_single": 0}      # vd's "chain2": the plain search of these few queries samples twice
ROUTES = {
    "narrow-1": dict(seed=51, dtype="bf16", d=64, n=5003, nq=3, opts={}, path=vd.CHAIN, nqt=1),
    "narrow-2": dict(seed=102, dtype="f16", d=64, n=5003, nq=40, opts={}, path=vd.CHAIN, nqt=2),
    "wide": dict(seed=53, dtype="bf16", d=768, n=8197, nq=70, opts={"wide_mode": 1}, path=vd.WIDE),
    "quad": dict(seed=54, dtype="f16", d=768, n=8197, nq=70, opts={"wide_mode": 2}, path=vd.QSPLIT),
    "quad-f32": dict(seed=105, dtype="f32", d=200, n=8197, nq=70, opts={}, path=vd.QSPLIT),
    "two-pass": dict(seed=106, dtype="bf16", d=768, n=8197, nq=WIDE_PASS[768] + 5, opts={"wide_mode": 1}, path=vd.WIDE, more=True),
    "big": dict(seed=57, dtype="bf16", d=64, n=vd.N_BIG, nq=3, opts=BIG_OPTS, path=vd.CHAIN, nqt=1, plain_levels=2),
}
# the (dtype, d, n, nq) at which family C's counts were designed, beside the table's own
C_SHAPES = sorted({(s["dtype"], s["d"], s["n"], s["nq"], s["seed"]) for s in ROUTES.values()} |
                  {(t, d, n, nq, 60 + i) for i, (d, n, nq) in enumerate([(768, 8197, 70), (64, 5003, 40), (200, 8197, 70)]) for t in ("bf16", "f16", "f32")})


def route_ok(r, spec):
    """None, or what is wrong with last_route r after a threshold search on the route spec"""
    if r & 0xFF != vd.route_code(spec["path"], 0):
        return f"last_route {r:#x}: low byte {r & 0xFF:#x}, expected {vd.route_code(spec['path'], 0):#x} (the path, no sampling level)"
    if (r >> 4) & 3:
        return f"last_route {r:#x}: a threshold search ran {(r >> 4) & 3} sampling level(s)"
    if not r & THRESHOLD:
        return f"last_route {r:#x}: bit 10 (threshold search) is not set"
    if "nqt" in spec and (r >> 8) & 3 != spec["nqt"]:
        return f"last_route {r:#x}: {(r >> 8) & 3} query tiles, expected {spec['nqt']}"
    if bool(r & vd.MORE_PASSES) != bool(spec.get("more")):
        return f"last_route {r:#x}: bit 11 (more passes) is {'not ' if spec.get('more') else ''}set"
    return None


# ---- deep lists: ascending scores (the family of test_search_gpu.test_wide_batch_ascending_scores_force_compaction)
SCAN_WAVES = 8      # CMR_SCAN_WAVES: the narrow kernel keeps one candidate list per wave, the wide kernel one per workgroup


def list_cap(k):
    """cmr_scan_geom's cap as make_geom (csrc/search_plan.h) sets it for a top-k pass"""
    return 256 if k > 32 else 128


def deep_n(k, n_cu):
    """rows at which each of n_cu candidate lists (per query) scans at least 2 * cap rows, plus 13: no multiple of 32.  The wide
    kernel runs min(panels, n_cu) workgroups with one list each; the query-split grid gets as many lists through deep_grid."""
    return 2 * list_cap(k) * n_cu + 13


def deep_grid(n_cu, groups):
    """option "scan_grid" for the query-split grid: `groups` twins per virtual workgroup and SCAN_WAVES lists in each, so
    groups * (n_cu / SCAN_WAVES) workgroups keep n_cu lists per query"""
    return groups * max(1, n_cu // SCAN_WAVES)


def deep_lists(n, n_cu, wide, groups=2):
    """candidate lists per query of the pass, and the rows the shortest-served one scans"""
    npanels = (n + 31) // 32
    if wide:
        W = min(npanels, n_cu)
    else:
        vg = deep_grid(n_cu, groups) // groups
        if vg >= 8:
            vg &= ~7
        W = max(vg, 1) * SCAN_WAVES
    return W, (npanels // W) * 32 - (32 - n % 32 if npanels % W == 0 else 0)


def family_asc(n, d, nq, seed=0):
    """every query's score grows with the row index: each panel beats the running threshold, so with a bound of -inf and no
    sampling every list overflows and compacts"""
    rng = np.random.default_rng(8300 + seed)
    u = rng.standard_normal(d).astype(np.float32); u /= np.linalg.norm(u)
    X = np.float32(0.25 / np.sqrt(d)) * rng.standard_normal((n, d), dtype=np.float32) + np.linspace(0.0, 1.0, n, dtype=np.float32)[:, None] * u
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = u[None, :] + np.float32(0.05 / np.sqrt(d)) * rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return X, Q.astype(np.float32)


# ---- few rows, id tables
FEW_ROWS = [1, 31, 32, 33, 37]
ID_BASE = 10 ** 6


def id_blocks(n):
    """a three-block table: local starts, global starts (gaps between the runs)"""
    return [0, n // 3, 2 * n // 3], [100, 100 + n // 3 + 50, 5_000_000]


def map_ids(ids, n, base=None):
    """local row ids -> what an index with the id base (or, base None, with id_blocks(n)) returns; -1 stays -1"""
    ids = np.asarray(ids, np.int64)
    if base is not None:
        return np.where(ids >= 0, ids + base, -1)
    ls, gs = (np.array(a, np.int64) for a in id_blocks(n))
    b = np.searchsorted(ls, np.maximum(ids, 0), side="right") - 1
    return np.where(ids >= 0, ids - ls[b] + gs[b], -1)


# ---- pipelines


def pipe_bounds(b_dup, n_blocks):
    b = np.float32(b_dup)
    cyc = [float(b), np.inf, 0.8, -np.inf, float(np.nextafter(b, np.float32(np.inf)))]
    return [cyc[i % len(cyc)] for i in range(n_blocks)]


def alternate(i, slots):
    """block i of a pipeline of `slots` slots (block i runs in slot (first + i) % slots): 0 | 1 such that every slot sees 0, 1, 0, ...
    in turn and neighbouring blocks differ within a round, whatever slot the first block takes"""
    return (i // slots + i % slots) % 2
