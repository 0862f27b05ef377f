"""Exact fp32 top-k from a 16-bit index (cmr_index_search_exact): the ids of the reference's fp32 np.dot + argsort
(ComoRAG.py:958-966) with a certificate that is never 1 without proof."""
import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import retrieval_np as orc

pytestmark = pytest.mark.gpu

ROUND = {"bf16": orc.bf16_round, "f16": orc.f16_round}


def _unit(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _planted(rng, q, scores):
    """unit rows whose fp32 inner product with the unit query q is scores[j] (up to fp32 rounding)"""
    q64 = q.astype(np.float64)
    u = rng.standard_normal((len(scores), len(q)))
    u -= np.outer(u @ q64, q64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s = np.asarray(scores, np.float64)[:, None]
    return (s * q64[None] + np.sqrt(1.0 - s * s) * u).astype(np.float32)


def _exact64(X, Q, blk=50_000):
    out = np.empty((len(Q), len(X)))
    Q64 = Q.astype(np.float64)
    for r0 in range(0, len(X), blk):
        out[:, r0:r0 + blk] = Q64 @ X[r0:r0 + blk].astype(np.float64).T
    return out


def _e_q(q, dim, mx, mdx, dtype):
    """the certificate's bound restated: ||dq|| M_x + ||q|| M_dx + 2 gamma ||q~|| M_x, gamma = dim 2^-23"""
    q64 = q.astype(np.float64)
    qt = ROUND[dtype](q[None])[0].astype(np.float64)
    g = dim * 2.0 ** -23
    return np.linalg.norm(qt - q64) * mx + np.linalg.norm(q64) * mdx + 2 * g * np.linalg.norm(qt) * mx


def _check_certified(ids, sc, ex, X, Q, k, E64=None):
    """every query whose flag is 1 has the fp32 host ranking's ids (tie rule 4e-6) and fp64 scores within 2e-6"""
    E64 = _exact64(X, Q) if E64 is None else E64
    ref_ids, _ = orc.topk_rule(Q @ X.T, k)          # the reference's fp32 arithmetic (ComoRAG.py:958-966)
    for i in np.flatnonzero(ex):
        orc.assert_topk_equivalent(ids[i], ref_ids[i], E64[i], 4e-6)
        np.testing.assert_allclose(sc[i], E64[i][ids[i]], atol=2e-6)
    return ref_ids, E64


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [768, 1024, 200])
def test_adversarial_near_ties(dtype, d):
    from comorag_amd.index import DenseIndex
    n, b, k = 200_000, 4, 20
    rng = np.random.default_rng(d + (0 if dtype == "bf16" else 1))
    X = _unit(rng, n, d)
    Q = _unit(rng, b, d)
    at = rng.choice(n, size=(b, 30), replace=False)
    gap = 1e-4 if dtype == "bf16" else 5e-6       # (f16 keeps 3 more bits: its rounding moves a score at 0.9 by ~1e-5)
    for i in range(b):     # 30 rows per query `gap` apart around 0.9: the 16-bit rounding reorders them
        X[at[i]] = _planted(rng, Q[i], 0.9 + gap * (np.arange(30) - 15))
    idx = DenseIndex(d, dtype, keep_f32=True)
    idx.append(X)
    ids, sc, ex = idx.search_exact(Q, k)
    assert ex.all(), ex
    ref_ids, E64 = _check_certified(ids, sc, ex, X, Q, k)
    plain, _, _, _ = idx.search(Q, k)
    assert any(not np.array_equal(plain[i], ref_ids[i]) for i in range(b)), "the planted near-ties do not bite"
    for i in range(b):
        orc.assert_topk_equivalent(ids[i], ref_ids[i], E64[i], 4e-6)
    np.testing.assert_allclose(sc, np.take_along_axis(E64, ids, 1), atol=2e-6)
    idx.close()


def test_scope_f32_and_missing_shadow():
    from comorag_amd.index import DenseIndex
    rng = np.random.default_rng(3)
    X, Q = _unit(rng, 5000, 128), _unit(rng, 3, 128)
    f = DenseIndex(128, "f32")
    f.append(X)
    ids, sc, ex = f.search_exact(Q, 10)
    pi, ps, _, _ = f.search(Q, 10)
    assert ex.all() and np.array_equal(ids, pi) and np.array_equal(sc, ps)
    f.close()
    h = DenseIndex(128, "bf16")
    h.append(X)
    with pytest.raises(L.CmrError) as e:
        h.search_exact(Q, 10)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED
    h.close()
    s = DenseIndex(128, "bf16", keep_f32=True)
    s.append(X)
    with pytest.raises(L.CmrError) as e:
        s.search_exact(Q, 65)
    assert e.value.code == L.CMR_ERR_UNSUPPORTED
    s.close()


def test_certificate_honesty():
    """q0: 30 planted near-ties (certified by stage 1); q1: ~300 rows inside its window (stage 1 cannot certify it, stage 2 can);
    q2: ~5 000 rows inside its window (nobody can); q3: no planted rows."""
    import torch
    from comorag_amd.index import DenseIndex
    n, d, k = 200_000, 768, 20
    rng = np.random.default_rng(11)
    X = _unit(rng, n, d)
    Q = _unit(rng, 4, d)
    rows = rng.choice(n, size=30 + 300 + 5000, replace=False)
    X[rows[:30]] = _planted(rng, Q[0], 0.9 + 1e-4 * (np.arange(30) - 15))
    X[rows[30:330]] = _planted(rng, Q[1], 0.9 - 3e-3 * np.arange(300) / 300)
    X[rows[330:]] = _planted(rng, Q[2], 0.9 - 3e-3 * np.arange(5000) / 5000)
    idx = DenseIndex(d, "bf16", keep_f32=True)
    idx.append(X)
    mx, mdx = idx.round_stats()
    assert 2 * _e_q(Q[1], d, mx, mdx, "bf16") > 3e-3          # the planted rows are inside the window
    qt = torch.from_numpy(Q).cuda()
    oi = torch.empty((4, k), dtype=torch.int64, device="cuda")
    osc = torch.empty((4, k), dtype=torch.float32, device="cuda")
    oex = torch.empty(4, dtype=torch.int32, device="cuda")
    DenseIndex.sync(idx.search_exact_pipelined(qt, k, oi, osc, oex))
    pex = oex.cpu().numpy()
    assert pex.tolist() == [1, 0, 0, 1], pex
    E64 = _check_certified(oi.cpu().numpy(), osc.cpu().numpy(), pex, X, Q, k)[1]
    ids, sc, ex = idx.search_exact(Q, k)
    assert ex.tolist() == [True, True, False, True], ex
    _check_certified(ids, sc, ex, X, Q, k, E64)
    for i in (0, 3):
        assert np.array_equal(ids[i], oi.cpu().numpy()[i]) and np.array_equal(sc[i], osc.cpu().numpy()[i])
    idx.close()


def test_bound_soundness_and_round_stats():
    import torch
    from comorag_amd.index import DenseIndex
    d = 768
    rng = np.random.default_rng(21)

    def want(rows, dtype):
        r = ROUND[dtype](rows).astype(np.float64)
        return np.linalg.norm(r, axis=1).max(), np.linalg.norm(r - rows.astype(np.float64), axis=1).max()

    for dtype in ("bf16", "f16"):
        idx = DenseIndex(d, dtype, capacity_hint=4096, keep_f32=True)
        assert idx.round_stats() == (0.0, 0.0)
        A = _unit(rng, 3000, d) * rng.uniform(0.5, 2.0, (3000, 1)).astype(np.float32)
        idx.append(A)
        np.testing.assert_allclose(idx.round_stats(), want(A, dtype), rtol=1e-6)
        B = (_unit(rng, 1000, d) * 2.5).astype(np.float32)
        idx.append_dev(torch.from_numpy(B).cuda())
        np.testing.assert_allclose(idx.round_stats(), want(np.concatenate([A, B]), dtype), rtol=1e-6)
        C_ = (_unit(rng, 20_000, d) * 3.0).astype(np.float32)        # capacity doubling (4096 -> more)
        idx.append(C_)
        X = np.concatenate([A, B, C_])
        st = idx.round_stats()
        np.testing.assert_allclose(st, want(X, dtype), rtol=1e-6)
        bad = _unit(rng, 10, d) * 9.0
        bad[3, 5] = np.nan
        with pytest.raises(L.CmrError):
            idx.append(bad)                       # rejected: the maxima stay
        with pytest.raises(L.CmrError):
            idx.append_dev(torch.from_numpy(bad.astype(np.float32)).cuda())
        assert idx.round_stats() == st and len(idx) == len(X)
        # max_r |scan - fp32| <= E_q on every row of every query
        Q = _unit(rng, 8, d)
        S = idx.scores(Q).astype(np.float64)
        E64 = _exact64(X, Q)
        for i in range(len(Q)):
            assert np.abs(S[i] - E64[i]).max() <= _e_q(Q[i], d, *st, dtype)
        idx.close()


def test_route_equality_pipelined_and_shards():
    import torch
    from comorag_amd.index import DenseIndex
    from comorag_amd.multi_index import MultiDeviceIndex
    n, d, k = 150_000, 768, 20
    rng = np.random.default_rng(31)
    X = _unit(rng, n, d)
    Qs = [_unit(rng, 16, d) for _ in range(2)]
    for Q in Qs:
        at = rng.choice(n, size=(len(Q), 20), replace=False)
        for i in range(len(Q)):
            X[at[i]] = _planted(rng, Q[i], 0.8 + 2e-4 * np.arange(20))
    idx = DenseIndex(d, "bf16", keep_f32=True)
    idx.append(X)
    want = [idx.search_exact(Q, k) for Q in Qs]
    for w, Q in zip(want, Qs):
        assert w[2].all()
        _check_certified(*w, X, Q, k)
    # pipelined: both batches in turn, every slot of the pipeline and its steady state
    outs = [(torch.empty((16, k), dtype=torch.int64, device="cuda"), torch.empty((16, k), dtype=torch.float32, device="cuda"),
             torch.empty(16, dtype=torch.int32, device="cuda")) for _ in range(2)]
    qts = [torch.from_numpy(Q).cuda() for Q in Qs]
    for step in range(8):
        j = step % 2
        DenseIndex.sync(idx.search_exact_pipelined(qts[j], k, *outs[j]))
        pi, ps, pe = (t.cpu().numpy() for t in outs[j])
        assert pe.all(), (step, pe)
        assert np.array_equal(pi, want[j][0]) and np.array_equal(ps, want[j][1]), step
    # logical shards, a block table from small appends on some of them
    Q = Qs[0]
    for S in (1, 2, 4):
        m = MultiDeviceIndex(d, "bf16", devices=[0] * S, keep_f32=True, options={"append_block_rows": 8192})
        for r0 in range(0, n, 30_000):
            m.append(X[r0:r0 + 30_000])
        mi, ms, me = m.search_exact(Q, k)
        both = me & want[0][2]
        assert both.sum() >= len(Q) // 2, me
        assert np.array_equal(mi[both], want[0][0][both]) and np.array_equal(ms[both], want[0][1][both]), S
        m.close()
    idx.close()


@pytest.mark.timeout(1200)
def test_headline_ten_million_pipelined_exact():
    """10 M x 768 bf16 keep_f32, B = 64, k = 20, pipelined exact, against the fp32 ranking over the fp32 rows: candidates per
    250 K-row block from an fp64 product on the device, ranked on the host in fp32 (the reference's arithmetic) with a running
    top-k, tie-arbitrated in fp64 on the rows in question."""
    import torch
    from comorag_amd.index import DenseIndex
    n, d, b, k, blk = 10_000_000, 768, 64, 20, 250_000
    dev = torch.device("cuda", 0)
    idx = DenseIndex(d, "bf16", capacity_hint=n, keep_f32=True)
    rng = np.random.default_rng(5)
    Q = _unit(rng, b, d)
    Qd = torch.from_numpy(Q.astype(np.float64)).to(dev)
    best_s = np.full((b, 0), -np.inf, np.float32); best_i = np.zeros((b, 0), np.int64)
    rows = {}
    for bi in range(n // blk):
        g = torch.Generator(device=dev); g.manual_seed(515_000 + bi)
        x = torch.randn((blk, d), generator=g, device=dev, dtype=torch.float32)
        x = (x / x.norm(dim=1, keepdim=True)).contiguous()
        if bi % 3 == 0:                          # planted near-neighbours: scores around 0.9 for a few queries
            for j in range(4):
                qi = (bi // 3 * 4 + j) % b
                x[777 + j] = torch.from_numpy(Q[qi]).to(dev) + 0.45 * x[777 + j]
                x[777 + j] /= x[777 + j].norm()
        idx.append_dev(x)
        cand = torch.topk(Qd @ x.double().T, 3 * k, dim=1).indices            # [b, 3k] per block
        u = torch.unique(cand).cpu().numpy()
        xh = x[torch.from_numpy(u).to(dev)].cpu().numpy()
        s = Q @ xh.T                                                          # fp32 host arithmetic
        cs = np.concatenate([best_s, s], 1); ci = np.concatenate([best_i, np.broadcast_to(u + bi * blk, s.shape)], 1)
        order = np.lexsort((ci, -cs), axis=1)[:, :3 * k]
        best_s, best_i = np.take_along_axis(cs, order, 1), np.take_along_axis(ci, order, 1)
        for j, r in enumerate(u):
            rows[int(r + bi * blk)] = xh[j]
        keep = set(np.unique(best_i).tolist())
        rows = {r: v for r, v in rows.items() if r in keep}
    qt = torch.from_numpy(Q).to(dev)
    oi = torch.empty((b, k), dtype=torch.int64, device=dev)
    osc = torch.empty((b, k), dtype=torch.float32, device=dev)
    oex = torch.empty(b, dtype=torch.int32, device=dev)
    for _ in range(3):                           # steady state of the pipeline
        done = idx.search_exact_pipelined(qt, k, oi, osc, oex)
    DenseIndex.sync(done)
    ids, sc, ex = oi.cpu().numpy(), osc.cpu().numpy(), oex.cpu().numpy()
    assert ex.all(), np.flatnonzero(ex == 0)
    swaps = 0
    for i in range(b):
        ref = best_i[i, :k]
        assert all(int(c) in rows for c in ids[i]), "a row the host ranking never had among its best"
        ex64 = {int(c): float(rows[int(c)].astype(np.float64) @ Q[i].astype(np.float64)) for c in np.union1d(ids[i], best_i[i])}
        np.testing.assert_allclose(sc[i], [ex64[int(c)] for c in ids[i]], atol=2e-6)
        if not np.array_equal(ids[i], ref):
            swaps += 1
            exv = np.full(n, -np.inf); exv[list(ex64)] = list(ex64.values())
            orc.assert_topk_equivalent(ids[i], ref, exv, 4e-6)
    assert swaps <= 2, swaps
    idx.close()
