"""CPU tier: the cases and the oracle of tests/test_range_search_gpu.py have the properties its assertions rely on (numpy only, fp64 scores
of the rounded operands), so that none of the GPU tests passes vacuously."""
import numpy as np
import pytest

from oracle import retrieval_np as orc
from tests import range_inputs as ri
from tests import threshold_inputs as ti
from tests import value_domain_inputs as vd

MARGIN = vd.ERR * 1.01 * 1.01


def _scores(tag):
    dtype, d, n, nq, seed = ri.CASES[tag]
    X, Q, q_dup, info = ri.make(tag)
    rnd = vd.ROUND[dtype]
    return orc.exact_scores_f64(rnd(X), rnd(Q)), q_dup, info


@pytest.mark.parametrize("tag", list(ri.CASES))
def test_family_c_has_empty_long_and_tile_crossing_lists(tag):
    dtype, d, n, nq, seed = ri.CASES[tag]
    S, q_dup, info = _scores(tag)
    assert S.shape == (nq, n) and n % ri.TILE and n > 2 * ri.TILE      # more than two tiles, the last one partial
    c08 = (S >= 0.8).sum(axis=1)
    c0 = (S >= 0.0).sum(axis=1)
    cneg = (S >= -0.9).sum(axis=1)
    assert np.abs(S - 0.8).min() > MARGIN and np.abs(S + 0.9).min() > MARGIN      # nothing within rounding of these bounds: the device counts the same
    if nq >= 5:
        # 0.8: empty lists (the unclustered queries and -centre), short ones, and the 151 of cluster 3: above one selection list (128)
        assert (c08 == 0).sum() == nq - 4 and c08[ti.Q_NEG] == 0 and c08[3] == 1 + ti.MEMBERS[3] == 151 > ti.P_K and c08[0] == 1
        assert sorted(c08[c08 > 0].tolist())[:3][0] == 1 and (c08 > 0).sum() == 4
    else:      # the three picked queries: short, the tied one, empty
        assert c08[2] == 0 and 3 <= c08[0] <= 4 and 21 <= c08[1] <= 44
    # 0.0: about half of the rows — every list crosses a tile (2048 hits) and most tiles of it hold hits
    assert c0.min() > ri.TILE and c0.max() < n - ri.TILE
    key = (d, n, nq, seed)
    if key in ri.ZERO_BOUND_HITS:
        lo, hi = ri.ZERO_BOUND_HITS[key]
        X, Q, _, _ = ri.make(tag)
        cx = (orc.exact_scores_f64(X, Q) >= 0.0).sum(axis=1)      # the table is of the operands as generated; rounding them moves a row or two across 0.0
        assert (cx.min(), cx.max()) == (lo, hi) and np.abs(c0 - cx).max() <= 8, (cx.min(), cx.max(), np.abs(c0 - cx).max())
    if (d, n, nq, seed) == (64, 5003, 40, 102):
        assert (c08 == 0).sum() == 36
    # -0.9: every row, or all but a few
    assert cneg.max() == n and cneg.min() >= n - 1 - ti.MEMBERS[1]
    # 0.3 lies between: lists that are neither empty nor half the corpus
    c03 = (S >= 0.3).sum(axis=1)
    assert c03.max() < c0.min() and c03.max() >= c08.max()


@pytest.mark.parametrize("tag", list(ri.CASES))
def test_tied_rows_sit_in_several_tiles_and_move_the_count_by_four(tag):
    dtype, d, n, nq, seed = ri.CASES[tag]
    S, q_dup, info = _scores(tag)
    tied = info["tied"]
    src = [t for t in tied if t not in ti.dup_rows(n)]
    assert len(src) == 1 and len(set(tied)) == 4
    # the three copies lie in three different tiles (first, a middle one, the last, partial one); the source in one of the tiles between
    tiles = [r // ri.TILE for r in ti.dup_rows(n)]
    assert tiles[0] == 0 and tiles[2] == (n - 1) // ri.TILE and len(set(tiles)) == 3
    assert 0 <= src[0] // ri.TILE <= tiles[2]
    if n > 4 * ri.TILE:
        assert len({r // ri.TILE for r in tied}) >= 3
    b = S[q_dup, tied[0]]
    assert np.all(S[q_dup, tied] == b)
    others = np.delete(S[q_dup], tied)
    assert np.abs(others - b).min() > MARGIN      # so in fp32 the attained bound and its two neighbours differ by exactly the four rows
    b32 = np.float32(b)
    up, down = np.nextafter(b32, np.float32(np.inf)), np.nextafter(b32, np.float32(-np.inf))
    S32 = S[q_dup].astype(np.float32)      # the tied rows round to one fp32 value; nothing else lands on it or its neighbours
    at, above, below = (S32 >= b32).sum(), (S32 >= up).sum(), (S32 >= down).sum()
    assert at - above == 4 and below == at
    assert set(np.flatnonzero((S32 >= b32) & ~(S32 >= up)).tolist()) == set(tied)


def test_oracle_order_bits_and_names():
    nz, pz = np.float32(-0.0), np.float32(0.0)
    S = np.array([[0.5, nz, pz, 0.5, -1.0, 0.25], [-1.0, -2.0, -3.0, -1.0, -5.0, -6.0]], np.float32)
    lims, ids, sc = ri.oracle(S, 0.0)
    assert lims.tolist() == [0, 5, 5] and ids.tolist() == [0, 3, 5, 1, 2]      # ties by ascending row; the two zeros are one value
    assert sc.view(np.uint32).tolist() == [np.float32(x).view(np.uint32) for x in (0.5, 0.5, 0.25, nz, pz)]      # ... and keep their bits
    ri.same(ri.oracle(S, -0.0), (lims, ids, sc))
    assert ri.oracle(S, 1e-45)[0].tolist() == [0, 3, 3]
    lims, ids, sc = ri.oracle(S, -1.0)
    assert lims.tolist() == [0, 6, 8] and ids[6:].tolist() == [0, 3]
    assert ri.oracle(S, np.inf)[0].tolist() == [0, 0, 0] and ri.oracle(S, -np.inf)[0].tolist() == [0, 6, 12]
    assert ri.oracle(S, -ti.FLT_MAX)[0].tolist() == [0, 6, 12]
    # names: the tie rule is on the ids the index returns (monotone in the row for an id base or a block table)
    names = ti.map_ids(np.arange(6), 6)
    assert ri.oracle(S, 0.0, names)[1].tolist() == names[[0, 3, 5, 1, 2]].tolist()
    got = ri.lists(ri.oracle(S, -1.0))
    assert len(got) == 2 and got[1][0].tolist() == [0, 3] and got[1][1].tolist() == [-1.0, -1.0]
    with pytest.raises(AssertionError):
        ri.same((lims, ids, sc), (lims, ids, np.where(sc == 0, pz, sc)))      # +0.0 in place of -0.0 is another bit pattern


def test_signed_zero_family():
    z = ri.SIGNED_ZERO
    for rnd in (vd.ROUND["bf16"], vd.ROUND["f32"]):
        X, Q = ri.family_signed_zero()
        Xr, Qr = rnd(X), rnd(Q)
        assert z["d"] % 128 == 0 and z["n"] > ri.TILE and z["n"] % 32
        assert np.all(Xr[z["neg_row"]] < 0) and np.all(Qr[0] > 0) and np.all(Xr[z["zero_rows"]] == 0)
        # every product of the negative row underflows past the smallest subnormal (1.4e-45): no partial sum is anything but -0.0
        assert np.all(np.abs(Xr[z["neg_row"]].astype(np.float64) * Qr[0].astype(np.float64)) * z["d"] < 1e-50)
        # every other row of query 0: a normal fp32 score or a zero, never a subnormal one
        S = orc.exact_scores_f64(Xr, Qr)
        rest = np.delete(S[0], z["zero_rows"] + [z["neg_row"]])
        assert np.abs(rest).min() > 1e-36 and (rest > 0).sum() > 900 and (rest < 0).sum() > 900
        assert z["neg_row"] // ri.TILE == 1 and z["zero_rows"][0] // ri.TILE == 0 and z["zero_rows"][0] < z["neg_row"] < z["n"]
