"""Certified int8 pre-filter of the pipelined search on the device: with the option "prefilter" = 1 (filter + re-score)
and 2 (the re-score alone: the filter keeps every row) a pipelined call returns, bit for bit, the ids and scores of the same index
with "prefilter" = 0 and of the synchronous search."""
import numpy as np
import pytest

from tests import prefilter_model as pm
from tests.prefilter_gpu_helpers import BATCHES, N_BIG, N_MID, N_SMALL, _data, _enqueue, _index, _same_bits

pytestmark = pytest.mark.gpu


def _pipelined(idx, Q, k, mode, minmax=False):
    idx.set_option("prefilter", mode)
    done, _, oi, os_ = _enqueue(idx, Q, k, minmax)
    idx.sync(done)
    assert idx.query_status() is False
    return oi.cpu().numpy(), os_.cpu().numpy()


def _check_all_modes(idx, Q, k, want_active=True):
    """modes 1 and 2 against mode 0 and against the synchronous search; returns the candidates mode 1 kept and the mode-0 result"""
    n = len(idx)
    ref = _pipelined(idx, Q, k, 0)
    assert idx.get_option("prefilter_active") == 0
    sync = idx.search(Q, k, with_minmax=False)[:2]
    kk = min(k, n)
    assert _same_bits((ref[0][:, :kk], ref[1][:, :kk]), sync)
    kept = None
    for mode in (2, 1):
        got = _pipelined(idx, Q, k, mode)
        assert idx.get_option("prefilter_active") == (1 if want_active else 0)
        assert _same_bits(got, ref), f"prefilter={mode} differs from prefilter=0"
        if not want_active:
            continue
        assert idx.get_option("prefilter_rows") == n
        kept = idx.get_option("prefilter_candidates")
        distinct = len(np.unique(ref[0][ref[0] >= 0]))
        assert distinct <= kept <= n
        if mode == 2:
            assert kept == n
    return kept, ref


# ---- every shape: dims 128 / 768, bf16 / f16, the three corpus sizes, the three batches
SHAPES = [(128, "bf16", N_SMALL), (128, "f16", N_SMALL), (768, "bf16", N_SMALL), (768, "f16", N_SMALL),
          (128, "bf16", N_MID), (128, "f16", N_MID), (768, "bf16", N_MID), (768, "f16", N_MID),
          (128, "f16", N_BIG), (768, "bf16", N_BIG)]


@pytest.mark.parametrize("d,dtype,n", SHAPES)
def test_same_bits_as_unfiltered_and_synchronous(d, dtype, n):
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, dtype, id_base=1000 if d == 128 else 0)
    try:
        for nq, k in BATCHES:
            kept, ref = _check_all_modes(idx, Q[:nq], k)
            if n == N_BIG:
                assert kept < n      # Gaussian rows, two sampling levels: the filter filters
            if d == 128:
                assert ref[0][ref[0] >= 0].min() >= 1000
        assert idx.get_option("prefilter_bytes") >= n * (((d + 127) // 128) * 128 + 8)
    finally:
        idx.close()


# ---- every input family, at the size with one sampling level and a partial last panel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["one-signed", "equal", "zeros", "norms", "spike"])
def test_input_families(family, dtype):
    d, n = 128, N_MID
    X, Q = _data(family, n, d)
    idx = _index(X, d, dtype)
    try:
        for nq, k in BATCHES[1:]:
            kept, _ = _check_all_modes(idx, Q[:nq], k)
            if family == "equal":
                assert kept == n      # every row ties with the threshold: nothing may be dropped
    finally:
        idx.close()


def test_two_level_families_at_768():
    d, n = 768, N_BIG
    X, Q = _data("norms", n, d)
    idx = _index(X, d, "bf16", id_base=7)
    try:
        _check_all_modes(idx, Q[:33], 20)
    finally:
        idx.close()


# ---- appends: into the last panel and across its boundary (no capacity growth), then beyond the capacity
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_appends_keep_the_companion_current(dtype):
    d = 128
    X, Q = _data("gauss", 40_000, d, seed=3)
    idx = _index(X[:8170], d, dtype, capacity_hint=20_000)
    try:
        _check_all_modes(idx, Q[:33], 20)
        bytes0 = idx.get_option("prefilter_bytes")
        idx.append(X[8170:8197])           # 8170 -> 8197 rows: fills panel 255 and starts panel 256
        _check_all_modes(idx, Q[:33], 20)
        assert idx.get_option("prefilter_bytes") == bytes0
        idx.append(X[8197:40_000])         # beyond the 20 000 rows allocated: the corpus buffer — and the companion — are replaced
        _check_all_modes(idx, Q[:64], 20)
        assert idx.get_option("prefilter_bytes") > bytes0
        st = idx.prefilter_stats()
        a_r, m, b_r, nx = pm.quantise_rows(idx.get_rows(np.arange(len(idx))))
        for got, want in zip(st, (nx.astype(np.float64).max(), b_r.astype(np.float64).max())):
            assert want <= got <= want * (1 + 1e-4)
    finally:
        idx.close()


# ---- the companion's statistics against a numpy recomputation from the stored rows
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["gauss", "norms", "spike", "zeros"])
def test_companion_stats(family, dtype):
    d, n = 128, N_MID
    X, Q = _data(family, n, d)
    idx = _index(X, d, dtype)
    try:
        assert idx.prefilter_stats() == (0.0, 0.0)      # no companion before the first call that uses one
        _pipelined(idx, Q[:3], 5, 1)
        got_nx, got_b = idx.prefilter_stats()
        Xs = idx.get_rows(np.arange(n))
        e64 = Xs.astype(np.float64)
        a_r, m, b_r, nx = pm.quantise_rows(Xs)
        want_nx = np.sqrt((e64 * e64).sum(axis=1)).max()
        e = e64 - a_r.astype(np.float64)[:, None] * m
        want_b = np.sqrt((e * e).sum(axis=1)).max()
        assert want_nx <= got_nx <= want_nx * (1 + 1e-4)
        assert want_b <= got_b <= want_b * (1 + 1e-4)
    finally:
        idx.close()


# ---- not eligible: min / max outputs, an fp32 index, a batch of more than one narrow pass
def test_min_max_buffers_turn_the_route_off():
    d, n = 128, N_MID
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "bf16")
    try:
        _pipelined(idx, Q[:5], 20, 1)
        assert idx.get_option("prefilter_active") == 1
        _pipelined(idx, Q[:5], 20, 1, minmax=True)
        assert idx.get_option("prefilter_active") == 0
        _pipelined(idx, Q[:5], 20, -1)                  # auto: a scan this short stays on the 16-bit kernel
        assert idx.get_option("prefilter_active") == 0
        with pytest.raises(Exception):
            idx.set_option("prefilter", 3)
    finally:
        idx.close()


def test_fp32_index_is_not_eligible():
    d, n = 128, N_MID
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "f32")
    try:
        _check_all_modes(idx, Q[:5], 20, want_active=False)
        assert idx.get_option("prefilter_bytes") == 0
    finally:
        idx.close()
