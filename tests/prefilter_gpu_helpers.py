"""What the device tests of the certified int8 pre-filter share (tests/test_prefilter_gpu.py, tests/test_prefilter_tighten_gpu.py): the
corpus sizes and batches, cached inputs, an index over them, one pipelined call and the bit-for-bit comparison of two results."""
import functools

import numpy as np

from tests import prefilter_model as pm

MAX_K = 128      # CMR_MAX_K
# n: no sampling level / one level, partial last panel / two levels
N_SMALL, N_MID, N_BIG = 70, 8197, 140_003
BATCHES = [(1, 1), (33, 20), (64, MAX_K)]


@functools.lru_cache(maxsize=None)
def _data(family, n, d, seed=0):
    X, Q = pm.family(family, n, d, 64, seed)
    X.setflags(write=False); Q.setflags(write=False)
    return X, Q


def _index(X, d, dtype, id_base=0, capacity_hint=0):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(d, dtype, capacity_hint=capacity_hint)
    idx.append(X)
    if id_base:
        idx.set_id_base(id_base)
    return idx


def _enqueue(idx, Q, k, minmax=False):
    """one pipelined call, not waited for: (done event, queries, ids, scores) — the tensors live as long as the caller keeps them"""
    import torch
    dev = torch.device("cuda", idx.device)
    qt = torch.from_numpy(np.array(Q, np.float32)).to(dev)
    oi = torch.empty((len(Q), k), dtype=torch.int64, device=dev)
    os_ = torch.empty((len(Q), k), dtype=torch.float32, device=dev)
    mn = torch.empty(len(Q), dtype=torch.float32, device=dev) if minmax else None
    mx = torch.empty(len(Q), dtype=torch.float32, device=dev) if minmax else None
    return idx.search_pipelined(qt, k, oi, os_, mn, mx), qt, oi, os_


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
