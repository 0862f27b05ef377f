"""numpy / loop model of cmr_mindex_plan_update: from the shards' block tables and an id list to the per-shard work
lists of a row update.  Written from the contract in include/comorag_hip.h, independent of the C++: one dictionary pass.  Also the
second embedder the mirror tests switch to."""
import hashlib

import numpy as np


def holders(shard_rows, n_blocks, local_start, global_start):
    """{global id: (shard, local row)} of the flat tables (n_blocks[s] blocks per shard, concatenated in shard order)"""
    where, at = {}, 0
    for s, (rows, nb) in enumerate(zip(shard_rows, n_blocks)):
        for b in range(nb):
            l0, g0 = int(local_start[at + b]), int(global_start[at + b])
            end = int(local_start[at + b + 1]) if b + 1 < nb else int(rows)
            for j in range(end - l0):
                where[g0 + j] = (s, l0 + j)
        at += nb
    return where


def plan(shard_rows, n_blocks, local_start, global_start, ids):
    """→ (shard [m], local [m], src [m], count [S]): ignored ids dropped, the last occurrence of an id kept, entries ordered by
    (shard, local row); src = index of the winning entry of `ids`"""
    where = holders(shard_rows, n_blocks, local_start, global_start)
    last = {}
    for i, g in enumerate(np.asarray(ids, np.int64).tolist()):
        if g >= 0 and g in where:
            last[where[g]] = i
    entries = sorted((s, l, i) for (s, l), i in last.items())
    shard = np.array([e[0] for e in entries], np.int32)
    local = np.array([e[1] for e in entries], np.int64)
    src = np.array([e[2] for e in entries], np.int64)
    return shard, local, src, np.bincount(shard, minlength=len(shard_rows)).astype(np.int64)


class SecondEmbedder:
    """conftest.FakeEmbedder's construction with another seed per text: what a model or instruction change does to every vector"""

    def __init__(self, dim=32):
        self.embedding_dim = dim

    def batch_encode(self, texts, **kw):
        if isinstance(texts, str):
            texts = [texts]
        out = []
        for t in texts:
            seed = int.from_bytes(hashlib.md5(("second model: " + t).encode()).digest()[:8], "little")
            v = np.random.default_rng(seed).standard_normal(self.embedding_dim).astype(np.float32)
            out.append(v / np.linalg.norm(v))
        return np.stack(out).astype(np.float32)

    def encode(self, texts, **kw):
        import torch
        return torch.from_numpy(self.batch_encode(texts))
