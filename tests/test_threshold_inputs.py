"""CPU tier: the cut rule, the input families and the route table of tests/test_threshold_search_gpu.py have the properties its
assertions rely on (numpy oracle only), at every dtype and shape that file uses — so that none of its tests passes vacuously."""
import numpy as np
import pytest

from oracle import retrieval_np as orc
from tests import threshold_inputs as ti
from tests import value_domain_inputs as vd

MARGIN = vd.ERR * 1.01 * 1.01      # the project's bound at the norms of rounded unit rows and queries (vd.row_tol)


# ---------------------------------------------------------------------------------------------- the cut rule
def _lists(rows):
    """hand-made plain-search lists: per query [(id, score), ...] already in the exported order"""
    w = max(len(r) for r in rows)
    ids = np.full((len(rows), w), -1, np.int64); sc = np.full((len(rows), w), -np.inf, np.float32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = [a for a, _ in r]; sc[i, :len(r)] = [b for _, b in r]
    return ids, sc


def test_cut_ties_at_the_bound():
    b = np.float32(0.75)
    up, down = np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))
    P = _lists([[(9, 0.9), (2, b), (5, b), (11, b), (40, b), (3, down), (1, 0.1)],
                [(4, up), (0, down)]])
    ids, sc, c = ti.cut(*P, b, 6)      # >= keeps every tied row, the fp32 neighbour below does not pass
    assert c.tolist() == [5, 1]
    assert ids.tolist() == [[9, 2, 5, 11, 40, -1], [4, -1, -1, -1, -1, -1]]
    assert np.array_equal(sc[0, :5], P[1][0, :5]) and np.all(np.isneginf(sc[0, 5:])) and np.all(np.isneginf(sc[1, 1:]))
    ids, sc, c = ti.cut(*P, up, 6)      # one step up: all four tied rows go
    assert c.tolist() == [1, 1] and ids[0].tolist() == [9, -1, -1, -1, -1, -1]
    ids, sc, c = ti.cut(*P, down, 6)      # one step down: the row that sits there comes in
    assert c.tolist() == [6, 2] and ids[0].tolist() == [9, 2, 5, 11, 40, 3] and ids[1].tolist() == [4, 0, -1, -1, -1, -1]
    ids, sc, c = ti.cut(*P, b, 3)      # k cuts inside the ties: the lowest rows, as the plain search orders them
    assert ids.tolist() == [[9, 2, 5], [4, -1, -1]] and c.tolist() == [5, 1]
    assert ids.dtype == np.int64 and sc.dtype == np.float32


def test_cut_all_rows_none_and_a_full_plain_list():
    rng = np.random.default_rng(1)
    s = np.sort(rng.uniform(-1, 1, (2, ti.P_K)).astype(np.float32), axis=1)[:, ::-1]
    P = (np.stack([rng.permutation(1000)[:ti.P_K] for _ in range(2)]).astype(np.int64), np.ascontiguousarray(s))
    for b in (-np.inf, -ti.FLT_MAX, -1.0):      # every row passes: c = 128, the first k columns of P, no padding
        for k in ti.KS:
            ids, sc, c = ti.cut(*P, b, k)
            assert c.tolist() == [ti.P_K] * 2 and np.array_equal(ids, P[0][:, :k]) and np.array_equal(sc.view(np.uint32), P[1][:, :k].view(np.uint32))
    for b in (np.inf, ti.FLT_MAX, 1.0):      # no row passes: all padding
        ids, sc, c = ti.cut(*P, b, 20)
        assert c.tolist() == [0, 0] and np.all(ids == -1) and np.all(np.isneginf(sc))
    # a short plain list (an index of 3 rows, k' = 3 columns; and one with padding inside P): -inf keeps the real rows only
    ids, sc, c = ti.cut(np.int64([[2, 0, 1]]), np.float32([[0.5, 0.0, -0.5]]), -np.inf, 5)
    assert c.tolist() == [3] and ids.tolist() == [[2, 0, 1, -1, -1]] and np.all(np.isneginf(sc[0, 3:]))
    ids, sc, c = ti.cut(*_lists([[(7, 0.5)], [(1, 0.4), (3, 0.2)]]), -np.inf, 2)
    assert c.tolist() == [1, 2] and ids.tolist() == [[7, -1], [1, 3]]
    # the two zeros are one bound; the smallest subnormal is above them
    Z = _lists([[(3, 0.0), (8, -0.0), (1, -1e-3)]])
    assert ti.cut(*Z, 0.0, 3)[2].tolist() == [2] and ti.cut(*Z, -0.0, 3)[2].tolist() == [2] and ti.cut(*Z, 1e-45, 3)[2].tolist() == [0]
    assert np.float32(1e-45) > 0 and ti.cut(*Z, -1e-45, 3)[2].tolist() == [2]
    assert [ti.branch(c, 20) for c in (0, 1, 19, 20, 128)] == ["empty", "short", "short", "full", "full"]


def test_bounds_list():
    b = np.float32(0.9473)
    bs = ti.bounds_around(b)
    assert len(bs) == 11 and bs[0] == float(b) and np.float32(bs[1]) > b > np.float32(bs[2])
    assert np.float32(bs[1]).view(np.uint32) - b.view(np.uint32) == 1 and b.view(np.uint32) - np.float32(bs[2]).view(np.uint32) == 1
    assert bs[3:] == [0.95, 0.9, 0.8, -0.9, -np.inf, np.inf, ti.FLT_MAX, -ti.FLT_MAX] and np.isfinite(np.float32(ti.FLT_MAX))
    assert not any(np.isnan(bs))
    cyc = ti.pipe_bounds(b, 9)
    assert cyc[:5] == [bs[0], np.inf, 0.8, -np.inf, bs[1]] and cyc[5:] == cyc[:4]


# ---------------------------------------------------------------------------------------------- family C
@pytest.mark.parametrize("dtype,d,n,nq,seed", ti.C_SHAPES)
def test_family_c_counts(dtype, d, n, nq, seed):
    X, Q, info = ti.family_c(n, d, nq, seed)
    rnd = vd.ROUND[dtype]
    Xr, Qr = rnd(X), rnd(Q)
    assert len(Q) == max(nq, 5) and np.array_equal(Q[:4], X[ti.CENTRES]) and np.array_equal(Q[ti.Q_NEG], -X[ti.CENTRES[1]])
    assert np.abs(np.linalg.norm(Xr.astype(np.float64), axis=1) - 1).max() < 0.01 and np.abs(np.linalg.norm(Qr.astype(np.float64), axis=1) - 1).max() < 0.01
    # the four tied rows: bit-equal, in the first panel, a middle panel and the last, partial one; on no centre and no other member
    tied = info["tied"]
    assert len(set(tied)) == 4 and tied == sorted(tied) and set(ti.dup_rows(n)) < set(tied) and all(np.array_equal(X[t], X[tied[0]]) for t in tied)
    assert 31 // 32 == 0 and 0 < (n // 2) // 32 < (n - 1) // 32 == (n + 31) // 32 - 1 and n % 32
    planted = [r for rows in info["members"] for r in rows]
    assert [len(rows) for rows in info["members"]] == list(ti.MEMBERS) and len(set(planted)) == len(planted)
    assert all(64 <= r < n - 64 for r in planted) and not set(planted) & set(ti.dup_rows(n)) and max(ti.CENTRES) < 64
    S = orc.exact_scores_f64(Xr, Qr)
    b_dup = S[ti.Q_DUP, tied[0]]
    assert 0.93 < b_dup < 0.96 and np.all(S[ti.Q_DUP, tied] == b_dup), b_dup
    # nothing else within rounding of the attained bound, and no pair within rounding of a fixed one: the counts below are the device's
    others = np.delete(S[ti.Q_DUP], tied)
    assert np.abs(others - b_dup).min() > MARGIN
    for b in ti.FIXED_BOUNDS + [-0.9]:
        assert np.abs(S - b).min() > MARGIN, (b, np.abs(S - b).min())
    counts = {b: (S[:5] >= b).sum(axis=1) for b in [b_dup] + ti.FIXED_BOUNDS}
    for b, c in counts.items():
        assert c[ti.Q_NEG] == 0 and c[0] == 1 and 3 <= c[1] <= 4 and 21 <= c[2] <= 44 and 73 <= c[3] <= 151, (b, c)
        # with k = 20: an empty list, short lists and at least two full ones — also among the three queries a small route takes
        assert {ti.branch(x, 20) for x in c} == {"empty", "short", "full"} and sum(ti.branch(x, 20) == "full" for x in c) >= 2
        assert [ti.branch(c[q], 20) for q in ti.PICK3] == ["short", "full", "empty"]
    assert counts[0.8][3] == 151 > ti.P_K      # more rows pass than the longest list holds: c = 128 in the plain search's list
    assert counts[b_dup][ti.Q_DUP] <= ti.P_K      # the tied rows end the list of their query at k = 128
    assert S[:4].min() > -0.9 + 0.1      # -0.9: every row of queries 0..3 passes
    assert (S[ti.Q_NEG] >= -0.9).sum() >= n - 1 - ti.MEMBERS[1] and S[ti.Q_NEG].max() < 0.8 - 0.1
    Qp, q_dup = ti.pick_queries(Q, nq)
    assert len(Qp) == nq and np.array_equal(Qp[q_dup], Q[ti.Q_DUP])


def test_family_p_negative_attained_bound():
    s = ti.ROUTES["narrow-1"]
    X, Q = vd.family_p(s["n"], s["d"], s["nq"], seed=s["seed"])
    S = orc.exact_scores_f64(vd.ROUND[s["dtype"]](X), vd.ROUND[s["dtype"]](-Q))
    top = np.sort(S[0])[::-1]
    assert S.max() < -0.3 and top[9] - top[10] > MARGIN and top[8] - top[9] > MARGIN      # the 10th best is attained once and is < 0
    X, Q = vd.family_z(s["n"], s["d"], s["nq"], seed=s["seed"])      # the zero rows: +0.0 exactly, every other score far below
    S = orc.exact_scores_f64(vd.ROUND[s["dtype"]](X), vd.ROUND[s["dtype"]](Q))
    assert np.all(S[:, vd.zero_rows(s["n"])] == 0) and np.delete(S, vd.zero_rows(s["n"]), axis=1).max() < -0.3


# ---------------------------------------------------------------------------------------------- routes, deep lists, ids, pipelines
def test_route_table():
    assert list(ti.ROUTES) == ["narrow-1", "narrow-2", "wide", "quad", "quad-f32", "two-pass", "big"]
    seeds = [s["seed"] for s in ti.ROUTES.values()]
    assert len(set(seeds)) == len(seeds) and all(s["n"] % 32 for s in ti.ROUTES.values())
    assert ti.ROUTES["two-pass"]["nq"] == 256 + 5 and ti.ROUTES["big"]["n"] == vd.N_BIG and ti.ROUTES["big"]["opts"] == vd.SEARCH_ROUTES["chain2"]["opts"]
    for tag in ("wide", "quad", "quad-f32"):      # the rows the value-domain table routes the plain search with
        assert all(ti.ROUTES[tag][f] == vd.SEARCH_ROUTES[tag][f] for f in ("dtype", "d", "n", "nq", "opts"))
    spec = ti.ROUTES["narrow-2"]
    good = vd.route_code(vd.CHAIN, 0) | 2 << 8 | ti.THRESHOLD
    assert ti.route_ok(good, spec) is None
    for bad in (good & ~ti.THRESHOLD, good | 1 << 4, good | 2 << 4, (good & ~0xF) | vd.WIDE, good ^ (3 << 8), good | vd.MORE_PASSES, good | 1 << 6, good | 1 << 7):
        assert ti.route_ok(bad, spec) is not None, hex(bad)
    two = vd.route_code(vd.WIDE, 0) | 1 << 8 | ti.THRESHOLD
    assert ti.route_ok(two | vd.MORE_PASSES, ti.ROUTES["two-pass"]) is None and ti.route_ok(two, ti.ROUTES["two-pass"]) is not None


@pytest.mark.parametrize("n_cu", [256, 304, 64])
@pytest.mark.parametrize("k", [20, 100])
def test_deep_lists_get_twice_their_capacity(k, n_cu):
    n = ti.deep_n(k, n_cu)
    cap = ti.list_cap(k)
    assert n % 32 == 13 and (ti.list_cap(32), ti.list_cap(33)) == (128, 256)
    for wide in (True, False):
        W, rows = ti.deep_lists(n, n_cu, wide)
        assert W <= n_cu and rows >= 2 * cap, (W, rows)
    assert ti.deep_grid(n_cu, 2) % 2 == 0 and ti.deep_grid(n_cu, 2) <= n_cu


def test_family_asc_scores_ascend():
    X, Q = ti.family_asc(4109, 768, 70)
    S = orc.exact_scores_f64(orc.bf16_round(X), orc.bf16_round(Q))
    best = np.argsort(-S, axis=1)[:, :100]
    assert best.min() > 4109 - 1500      # the best rows are the last ones: every panel on the way beats the running threshold
    assert np.all(S[:, 3000:].mean(axis=1) - S[:, :1000].mean(axis=1) > 0.5)


def test_id_maps_and_pipeline_order():
    n = 5003
    ls, gs = ti.id_blocks(n)
    ids = np.int64([[0, ls[1] - 1, ls[1], -1], [ls[2], n - 1, -1, -1]])
    assert ti.map_ids(ids, n).tolist() == [[100, 100 + ls[1] - 1, gs[1], -1], [5_000_000, 5_000_000 + n - 1 - ls[2], -1, -1]]
    assert ti.map_ids(ids, n, ti.ID_BASE).tolist() == [[10 ** 6, 10 ** 6 + ls[1] - 1, 10 ** 6 + ls[1], -1], [10 ** 6 + ls[2], 10 ** 6 + n - 1, -1, -1]]
    assert gs[0] + ls[1] <= gs[1] and gs[1] + (ls[2] - ls[1]) <= gs[2]      # the runs do not overlap
    for slots in (2, 3, 4):
        nb = 2 * slots + 1
        for first in range(slots):      # whatever slot the first block takes: every slot alternates, and sees both kinds
            per_slot = {}
            for i in range(nb):
                per_slot.setdefault((first + i) % slots, []).append(ti.alternate(i, slots))
            assert all(a != b for seq in per_slot.values() for a, b in zip(seq, seq[1:]))
            assert max(len(seq) for seq in per_slot.values()) == 3 and {0, 1} == {x for seq in per_slot.values() for x in seq}
