"""numpy model of what the device does with the row-id lists of `search_filtered_ids` (cmr_index_search_ids): translate
ids in the domain the searches return (id base, or a block table) into local rows, drop what the index does not hold, and lay the result
out as `pack_row_masks` words.  The oracle of the GPU tests for based and blocked indexes; itself held against `pack_row_masks` on
hand-written local rows in tests/test_filtered_ids_host.py."""
import numpy as np

from comorag_amd.index import pack_row_mask, pack_row_masks


def local_rows(ids, n, base=0, blocks=None):
    """ids (any integers) -> the local rows in [0, n) they name, in list order; negative ids and ids the index does not hold are dropped.
    blocks = (local_starts, global_starts): block b holds local rows [local_starts[b], local_starts[b + 1]) (the last one up to n) as the
    global ids global_starts[b] + 0, 1, ..."""
    out = []
    for g in np.asarray(ids, dtype=np.int64).reshape(-1).tolist():
        if g < 0:
            continue
        if blocks is None:
            r = g - base
            if 0 <= r < n:
                out.append(r)
            continue
        ls, gs = blocks
        for b in range(len(ls)):
            end = ls[b + 1] if b + 1 < len(ls) else n
            if gs[b] <= g < gs[b] + (end - ls[b]) and ls[b] + (g - gs[b]) < n:
                out.append(ls[b] + (g - gs[b]))
                break
    return np.asarray(out, dtype=np.int64)


def keeps_of(n, nq, mode, offsets, ids, base=0, blocks=None):
    """bool [n] per query (ONE entry when offsets is None: the shared list)"""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    lists = [ids] if offsets is None else [ids[offsets[i]:offsets[i + 1]] for i in range(nq)]
    keeps = []
    for lst in lists:
        keep = np.zeros(n, bool) if mode == "allow" else np.ones(n, bool)
        keep[local_rows(lst, n, base, blocks)] = mode == "allow"
        keeps.append(keep)
    return keeps


def words_of(n, nq, mode, offsets, ids, base=0, blocks=None):
    """uint32 [nq, ceil(n / 32)] with offsets, [ceil(n / 32)] without: the words cmr_index_row_masks_dev must write"""
    keeps = keeps_of(n, nq, mode, offsets, ids, base, blocks)
    return pack_row_mask(n, allow=keeps[0]) if offsets is None else pack_row_masks(n, allow=keeps)
