"""The numpy side of the filtered score-bound searches' tests (range_search_filtered*, range_count_filtered*, search_min_score_filtered*;
DESIGN.md §4.19): the mask family, and the two helpers that turn the result of an EXISTING call into what the filtered call must
return — `drop` (an unfiltered range search without the entries of disallowed rows) and `pad_below` (a filtered top-k with the entries
below the bound turned into padding).  numpy only; tests/test_filtered_range_host.py checks the helpers against hand-made lists."""
import numpy as np

ROUTE_CHAIN, ROUTE_RANGE = 3, 11                                            # CMR_ROUTE_CHAIN, CMR_ROUTE_RANGE
THRESHOLD, FILTERED, FILTERED_EACH, FILTERED_IDS = 1 << 10, 1 << 12, 1 << 13, 1 << 14
N_FAMILY = 8


def n_words(n):
    return (n + 31) // 32


def rows_of(words, n):
    """the local rows (ascending, int64) a bitmap allows among the first n: bits at or beyond n do not count"""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n]
    return np.flatnonzero(bits).astype(np.int64)


def words_of(n, rows):
    bits = np.zeros(n_words(n) * 32, np.uint8)
    bits[np.asarray(rows, np.int64)] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def family(n, tied, seed=0):
    """The eight masks of an index of n >= 4100 rows, uint32 [8, ceil(n / 32)].  0: all ones WITH the garbage bits beyond n set; 1: all
    zeros; 2: 0xAAAAAAAA (the odd rows; garbage beyond n too); 3: one row, a tied one; 4: rows [2040, 2060) and [4090, 4100), across the
    boundaries of the 2048-row tiles; 5: a random half; 6: a random 1 %; 7: everything but one of the tied rows."""
    assert n >= 4100 and n % 32, "the last word must be partial: the garbage bits of masks 0 and 2 live there"
    rng = np.random.default_rng(4190 + seed)
    nw = n_words(n)
    M = np.zeros((N_FAMILY, nw), np.uint32)
    M[0] = 0xFFFFFFFF
    M[2] = 0xAAAAAAAA
    M[3] = words_of(n, [tied[1]])
    M[4] = words_of(n, list(range(2040, 2060)) + list(range(4090, 4100)))
    M[5] = words_of(n, np.flatnonzero(rng.random(n) < 0.5))
    M[6] = words_of(n, np.flatnonzero(rng.random(n) < 0.01))
    M[7] = words_of(n, np.setdiff1d(np.arange(n), [tied[2]]))
    return M


def small_family(n, seed=0):
    """an index of a few rows (0 included): all ones with garbage, zeros, the odd rows, the last row alone, a random half"""
    rng = np.random.default_rng(4290 + seed)
    nw = n_words(n)
    M = np.zeros((5, nw), np.uint32)
    if nw:
        M[0] = 0xFFFFFFFF
        M[2] = 0xAAAAAAAA
        M[3] = words_of(n, [n - 1])
        M[4] = words_of(n, np.flatnonzero(rng.random(n) < 0.5))
    return M


def per_query(M, nq, mod=7):
    """query i takes mask i mod 7 of the family"""
    return np.ascontiguousarray(M[[i % min(mod, len(M)) for i in range(nq)]])


def drop(res, allowed_ids):
    """res = (lims, ids, scores) of an unfiltered range search; allowed_ids: ONE array of allowed row ids (every query), or a list with
    one array per query — in the id domain of `res`.  -> the lists without the entries of disallowed rows, order and score bits kept"""
    lims, ids, sc = res
    nq = len(lims) - 1
    shared = isinstance(allowed_ids, np.ndarray)
    assert shared or len(allowed_ids) == nq
    out_l, out_i, out_s = [0], [], []
    for i in range(nq):
        seg = slice(int(lims[i]), int(lims[i + 1]))
        keep = np.isin(ids[seg], allowed_ids if shared else allowed_ids[i])
        out_i.append(ids[seg][keep]); out_s.append(sc[seg][keep])
        out_l.append(out_l[-1] + int(keep.sum()))
    return (np.array(out_l, np.int64), np.concatenate(out_i).astype(np.int64) if out_i else np.empty(0, np.int64),
            np.concatenate(out_s).astype(np.float32) if out_s else np.empty(0, np.float32))


def pad_below(ids, sc, b, k):
    """ids / scores [nq, k'] of a filtered top-k search with this k (k' <= k columns, -1 / -inf padded where fewer rows are allowed) ->
    [nq, k] with every entry whose score is below float32(b) — and everything that was padding — as -1 / -inf"""
    ids = np.asarray(ids, np.int64)
    sc = np.asarray(sc, np.float32)
    assert ids.shape == sc.shape and ids.ndim == 2 and ids.shape[1] <= k
    out_i = np.full((len(ids), k), -1, np.int64)
    out_s = np.full((len(ids), k), -np.inf, np.float32)
    keep = (ids >= 0) & (sc >= np.float32(b))
    kk = ids.shape[1]
    out_i[:, :kk][keep] = ids[keep]
    out_s[:, :kk][keep] = sc[keep]
    return out_i, out_s


def same_rows(got, want, what=""):
    """bit for bit: ids and the scores as fp32 words"""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, want[0].shape)
    assert np.array_equal(got[0], want[0]), (what, "ids")
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32)), (what, "score bits")
