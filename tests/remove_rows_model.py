"""numpy model of row removal over the shards of a multi-device index (cmr_mindex_plan_remove), written from the
semantics and not from the C code: a layout is the list of its rows as (shard, local row, global id) triples; removing ids drops
their triples, the survivors keep their order and are renumbered densely — globally in the old global order, locally per shard."""
import numpy as np


def triples(shard_rows, n_blocks, local_start, global_start):
    """block tables (the layout cmr_mindex_plan_remove takes and returns: per-shard block counts, starts concatenated in shard
    order) -> int64 [rows, 3] of (shard, local row, global id), in shard order then local order"""
    out, at = [], 0
    for s, (rows, nb) in enumerate(zip(shard_rows, n_blocks)):
        for b in range(nb):
            l0 = int(local_start[at + b])
            l1 = int(local_start[at + b + 1]) if b + 1 < nb else int(rows)
            for r in range(l0, l1):
                out.append((s, r, int(global_start[at + b]) + r - l0))
        at += nb
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def remove(tri, ids, skip_shards=()):
    """the triples after `ids` (global; negative ids, ids nobody holds, ids held by a shard of `skip_shards` and duplicates are ignored)
    are gone -> (triples, rows removed)"""
    gone = np.isin(tri[:, 2], np.asarray(ids, dtype=np.int64)) & ~np.isin(tri[:, 0], np.asarray(list(skip_shards), dtype=np.int64))
    left = tri[~gone].copy()
    removed = np.sort(tri[gone, 2])
    left[:, 2] -= np.searchsorted(removed, left[:, 2])      # every survivor moves down by the removed ids below it: dense ids stay dense
    for s in np.unique(left[:, 0]):
        m = left[:, 0] == s
        left[m, 1] = np.arange(int(m.sum()))
    return left, int(gone.sum())
