"""The length-driven encoder kernels of comorag_amd/csrc/encoder_kernels.hip at EVERY length 1 .. L of a padded mini-batch, with answers that
cannot hide behind a tolerance.

Attention (attn_fwd_kernel<*, 4, 64>, <*, 8, 64>, <*, 4, 32>, attn_fwd_f32_kernel<64>, <32>): b = L sequences, lens[s] = s + 1.
  * the exact-weight probes of tests/encoder_probes.py (softmax weights 1 / len, 1 or 1 / 2 by construction; tests/test_encoder_probes.py
    proves the closed forms on the host): a 16-bit kernel must return the closed form to ONE unit in the last place of its output type — its
    fp32 result is within a few 1e-6 (relative) of the exact value, the single rounding into 16 bits can move it by one unit and only at a tie,
    a wrong, dropped, doubled or unmasked key moves it by order 1; an fp32 kernel to 2^-20 of the row's largest expected magnitude.
    (Before units are counted, the 16-bit comparison takes off what fp32 arithmetic itself may differ by — ep.leak_slack, ~2e-6 absolute:
    where the two targets of a two-hot query cancel the closed form is exactly 0 and the bf16 HD = 32 kernel was measured at -2^-24.)
    Measured on an MI355X: uniform 0.50, one-hot 0, two-hot 0.50 units at most for every 16-bit kernel; fp32 kernels <= 0.11 * 2^-20.
  * Gaussian inputs under the project's protocol e_got <= 4 e_ref + 4 ulp(max|want|): `want` the formula in fp64 on the rounded inputs; for
    the 16-bit kernels `ref` is a torch fp32 evaluation with the kernel's two rounding points (the weights exp(s - max) rounded to the 16-bit
    type in front of the PV product and normalised by their UNROUNDED fp32 sum, the result rounded to the 16-bit type) and ulp that of the
    16-bit type; for the fp32 kernels the protocol of tests/test_encoder_fp32_gpu.py as it is.
The folded LayerNorm + pool (add_ln16_pool_kernel, both feeds) at b = l = 64, lens = 1 .. 64: every position inside and across the 16-token
blocks, blocks of padding only included; references and tolerances of the existing tests of these entry points."""
import ctypes as C

import numpy as np
import pytest

from tests import encoder_probes as ep

pytestmark = pytest.mark.gpu

HEADS = ep.HEADS
# (head width, dtype, L = b, query rows per workgroup): the five kernels, the 16-bit ones in both types
KERNELS = [
    pytest.param(64, "bfloat16", 160, 128, id="attn_fwd<bf16,4,64>-L160"),
    pytest.param(64, "float16", 160, 128, id="attn_fwd<f16,4,64>-L160"),
    pytest.param(64, "bfloat16", 288, 256, id="attn_fwd<bf16,8,64>-L288"),
    pytest.param(64, "float16", 288, 256, id="attn_fwd<f16,8,64>-L288"),
    pytest.param(32, "bfloat16", 160, 128, id="attn_fwd<bf16,4,32>-L160"),
    pytest.param(32, "float16", 160, 128, id="attn_fwd<f16,4,32>-L160"),
    pytest.param(64, "float32", 160, 128, id="attn_fwd_f32<64>-L160"),
    pytest.param(32, "float32", 160, 128, id="attn_fwd_f32<32>-L160"),
]


def _stages(hidden, heads, tdt, eps=1e-12):
    from tests.test_encoder_head32_gpu import _Stages
    return _Stages(hidden, heads, tdt, eps)


def _ulp16_t(x, dtype):
    """ep.ulp16 on a float64 CUDA tensor"""
    import torch
    bits, emin = (7, -126) if dtype == "bfloat16" else (10, -14)
    a = x.abs()
    e = torch.frexp(a)[1] - 1
    e = torch.where(a == 0, torch.full_like(e, emin), e.clamp(min=emin))
    return torch.ldexp(torch.ones_like(a), e - bits)


# ---------------------------------------------------------------------------------------------------------------- 1. the probes
@pytest.mark.parametrize("HD,dtype,L,qblock", KERNELS)
def test_attention_exact_weight_probes_at_every_length(HD, dtype, L, qblock):
    import torch
    tdt = getattr(torch, dtype)
    fz = _stages(HEADS * HD, HEADS, tdt)
    lens = ep.lengths(L)
    lens_dev = torch.from_numpy(lens).cuda()
    pos = torch.arange(L, device="cuda")[None, :]
    live = pos < lens_dev[:, None]                                                                  # [b, L]: the rows that are compared
    beyond = pos >= ((lens_dev[:, None] + qblock - 1) // qblock) * qblock                           # rows of a query block wholly behind the length
    assert bool(beyond.any()) and int(lens.min()) == 1 and int(lens.max()) == L
    x = torch.tensor([0.0, 1.0, 3e-6, 1.5, -300.0], dtype=torch.float64, device="cuda")
    for name in ("bfloat16", "float16"):
        assert np.array_equal(_ulp16_t(x, name).cpu().numpy(), ep.ulp16(x.cpu().numpy(), name))
    failures = []
    for kind in ep.PROBES:
        qkv_np, _, want_np = ep.build(kind, HD, L, vdtype="bf16" if dtype == "bfloat16" else "f16")
        qkv = torch.from_numpy(qkv_np).cuda().to(tdt)
        assert torch.equal(qkv.float().cpu(), torch.from_numpy(qkv_np))                            # the inputs went in unrounded
        want = torch.from_numpy(want_np).cuda()                                                     # fp64 [b, L, heads, HD]
        out = fz.attention(qkv, lens_dev, L, L)
        torch.cuda.synchronize()
        assert out.dtype == tdt and torch.isfinite(out.float()).all(), kind                        # padding rows included
        got = out.double().view(L, L, HEADS, HD)
        assert not bool(got[beyond].any()), f"{kind}: rows of a padding-only query block must be zeros"
        err = (got - want).abs()
        if dtype == "float32":
            unit = 2.0 ** -20 * want.abs().amax(dim=-1, keepdim=True).expand_as(want)             # of the (sequence, query, head) row
        else:
            # one unit in the last place at the closed form, after what the kernel's fp32 arithmetic itself may differ by (ep.leak_slack: ~2e-6
            # absolute, i.e. a unit of the 16-bit type below |expected| ~ 1e-3 only; it is what is left where a two-hot query's targets cancel to 0)
            vmax = qkv.double().view(L, L, 3, HEADS, HD)[:, :, 2].abs().amax(dim=(1, 3))            # [sequence, head]
            slack = torch.from_numpy(ep.leak_slack(kind, vmax.cpu().numpy())).cuda()
            err = (err - slack[:, None, :, None]).clamp(min=0.0)
            unit = _ulp16_t(want, dtype)
        dev = torch.where(live[:, :, None, None], err / unit, torch.zeros_like(err))
        worst = float(dev.max())
        at = tuple(int(i) for i in np.unravel_index(int(dev.argmax()), tuple(dev.shape)))
        what = "2^-20 of the row's max" if dtype == "float32" else f"units in the last place of {dtype}"
        print(f"probe {kind} HD={HD} {dtype} L={L}: largest deviation {worst:.3f} {what} "
              f"(length {at[0] + 1}, query {at[1]}, head {at[2]}, d {at[3]}: got {float(got[at]):.9g}, expected {float(want[at]):.9g})")
        if worst > 1.0:
            bad = (dev > 1.0).sum(dim=(1, 2, 3)).nonzero().flatten()
            failures.append(f"{kind}: {worst:.3f} at length {at[0] + 1} query {at[1]} head {at[2]} d {at[3]}; {len(bad)} lengths off, first {(bad[:8] + 1).tolist()}")
    assert not failures, failures


@pytest.mark.parametrize("HD", [64, 32])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
def test_attention_an_empty_sequence_is_finite_and_leaves_its_neighbours_alone(dtype, HD):
    """b = 3, L = 100, lens = [100, 0, 37]: finite everywhere, and sequences 0 and 2 carry the bits of a call without the empty one."""
    import torch
    tdt, b, L = getattr(torch, dtype), 3, 100
    g = torch.Generator(device="cuda").manual_seed(100 + HD)
    qkv = (torch.randn((b * L, 3 * HEADS * HD), generator=g, device="cuda") * 1.5).to(tdt)
    fz = _stages(HEADS * HD, HEADS, tdt)
    got = fz.attention(qkv, torch.tensor([100, 0, 37], dtype=torch.int32, device="cuda"), b, L).view(b, L, -1)
    two = fz.attention(torch.cat([qkv[:L], qkv[2 * L:]]).contiguous(), torch.tensor([100, 37], dtype=torch.int32, device="cuda"), 2, L).view(2, L, -1)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got[0], two[0]) and torch.equal(got[2], two[1])


# ---------------------------------------------------------------------------------------------------------------- 2. Gaussian inputs, every length
def _formula(qkv, lens_dev, b, l, HD, p_dtype=None):
    """softmax(Q K^T / sqrt(HD), keys >= lens masked) V in qkv's own precision: [b, l, heads, HD].  p_dtype: the 16-bit kernels' rounding point
    inside — the weights exp(s - max) go through p_dtype in front of the PV product and are normalised by their unrounded sum."""
    import torch
    x = qkv.view(b, l, 3, HEADS, HD)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    scores = q @ k.transpose(-1, -2) / (HD ** 0.5)
    keymask = torch.arange(l, device=qkv.device)[None, :] >= lens_dev[:, None]
    scores = scores.masked_fill(keymask[:, None, None, :], float("-inf"))
    if p_dtype is None:
        return (torch.softmax(scores, dim=-1) @ v).permute(0, 2, 1, 3)
    p = torch.exp(scores - scores.amax(dim=-1, keepdim=True))
    return ((p.to(p_dtype).to(qkv.dtype) @ v) / p.sum(dim=-1, keepdim=True)).permute(0, 2, 1, 3)


@pytest.mark.parametrize("HD,dtype,L,qblock", KERNELS)
def test_attention_gaussian_inputs_at_every_length(HD, dtype, L, qblock):
    import torch
    from tests.test_encoder_fp32_gpu import _within_protocol as within32
    from tests.test_encoder_small_m_gpu import _within_protocol as within16
    tdt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(L * 1000 + HD)
    qkv = (torch.randn((L * L, 3 * HEADS * HD), generator=g, device="cuda") * 1.5).to(tdt)        # peaked, non-symmetric scores
    lens_dev = torch.from_numpy(ep.lengths(L)).cuda()
    out = _stages(HEADS * HD, HEADS, tdt).attention(qkv, lens_dev, L, L)
    torch.cuda.synchronize()
    assert out.dtype == tdt and torch.isfinite(out.float()).all()                                  # padding rows included
    live = torch.arange(L, device="cuda")[None, :] < lens_dev[:, None]
    want = _formula(qkv.double(), lens_dev, L, L, HD)[live].contiguous()
    got = out.view(L, L, HEADS, HD)[live]
    what = f"attention HD={HD} {dtype} lens 1..{L}"
    if dtype == "float32":
        within32(got.contiguous(), _formula(qkv, lens_dev, L, L, HD)[live].contiguous(), want, what)
    else:
        ref_all = _formula(qkv.float(), lens_dev, L, L, HD, p_dtype=tdt).to(tdt)                  # the second rounding point: the output
        within16(got, ref_all[live], want, dtype, what)
        # the same protocol length by length: the largest values (and errors) belong to the shortest sequences, a long one is held to its own
        keep = live[:, :, None, None]
        want_all = _formula(qkv.double(), lens_dev, L, L, HD)
        amax = lambda t: torch.where(keep, t, torch.zeros_like(t)).amax(dim=(1, 2, 3))
        e_got, e_ref = amax((out.view(L, L, HEADS, HD).double() - want_all).abs()), amax((ref_all.double() - want_all).abs())
        bound = 4.0 * e_ref + 4.0 * _ulp16_t(amax(want_all.abs()), dtype)
        ratio = e_got / e_ref.clamp(min=1e-30)
        at = int(torch.where(e_ref > 0, ratio, torch.zeros_like(ratio)).argmax())
        print(f"{what}, per length: largest e_got / e_ref {float(ratio[at]):.2f} at length {at + 1} (e_got {float(e_got[at]):.3e}); "
              f"largest e_got / bound {float((e_got / bound).max()):.3f}")
        assert bool((e_got <= bound).all()), (what, (e_got > bound).nonzero().flatten().add(1).tolist())


# ---------------------------------------------------------------------------------------------------------------- 3. folded LayerNorm + pool
def _ln_inputs(b, l, d, dt):
    import torch
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l + d)
    y = torch.randn((b * l, d), generator=g, device="cuda").to(dt)
    res = torch.randn((b * l, d), generator=g, device="cuda").to(dt)
    bias, gamma, beta = (torch.randn(d, generator=g, device="cuda").to(dt) for _ in range(3))
    return y, res, bias, gamma, beta


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("d", [256, 384])
@pytest.mark.parametrize("normalize", [True, False])
def test_folded_layernorm_pool_at_every_length(dtype, d, normalize):
    """test_last_layer_layernorm_with_the_encoder_tail_folded_in (tests/test_encoder_fused_gpu.py) — its two references, its tolerances — at
    b = l = 64, lens = 1 .. 64."""
    import torch
    from comorag_amd.embedding_model.bge import pool_l2norm
    b = l = 64
    dt = getattr(torch, dtype)
    y, res, bias, gamma, beta = _ln_inputs(b, l, d, dt)
    lens = torch.arange(1, l + 1, dtype=torch.int32)
    mask = (torch.arange(l)[None, :] < lens[:, None]).to(torch.int64)
    fz = _stages(d, 1, dt)
    hidden = fz.add_layernorm(y, bias, res, gamma, beta).view(b, l, d)
    two = pool_l2norm(hidden, mask.cuda(), normalize=normalize)
    one = fz.add_layernorm_pool(y, bias, res, gamma, beta, lens.cuda(), b, l, normalize)
    torch.cuda.synchronize()
    assert one.dtype == torch.float32 and one.shape == (b, d) and torch.isfinite(one).all()
    want = (hidden.float() * mask.cuda()[..., None]).sum(1) / lens.cuda()[:, None].float()
    if normalize:
        want = torch.nn.functional.normalize(want, p=2, dim=1)
    tol = 3e-6 if normalize else 3e-5                          # b * l = 4096 > 256 rows: add_layernorm runs the sixteen-lanes-per-row kernel, the folded kernel's order
    print(f"folded LN + pool {dtype} d={d} normalize={normalize}: max abs diff vs the formula {float((one - want).abs().max()):.3e}, vs the two-step path {float((one - two).abs().max()):.3e}")
    np.testing.assert_allclose(one.cpu().numpy(), want.cpu().numpy(), atol=tol, rtol=1e-5)
    np.testing.assert_allclose(one.cpu().numpy(), two.cpu().numpy(), atol=tol, rtol=1e-5)


@pytest.mark.parametrize("d", [256, 384])
@pytest.mark.parametrize("normalize", [True, False])
def test_folded_layernorm_pool_fp32_at_every_length(d, normalize):
    """test_add_layernorm_pool_fp32_vs_fp64 (tests/test_encoder_fp32_gpu.py), its protocol, at b = l = 64, lens = 1 .. 64; and the two-step path."""
    import torch
    import torch.nn.functional as F
    from comorag_amd.embedding_model.bge import pool_l2norm
    from oracle import encode_torch as enc
    from tests.test_encoder_fp32_gpu import _within_protocol
    b = l = 64
    y, res, bias, gamma, beta = _ln_inputs(b, l, d, torch.float32)
    lens = torch.arange(1, l + 1, dtype=torch.int32)
    mask = (torch.arange(l)[None, :] < lens[:, None]).to(torch.int64).cuda()
    fz = _stages(d, 1, torch.float32)
    got = fz.add_layernorm_pool(y, bias, res, gamma, beta, lens.cuda(), b, l, normalize)
    two = pool_l2norm(fz.add_layernorm(y, bias, res, gamma, beta).view(b, l, d), mask, normalize=normalize)

    def formula(dt):
        h = F.layer_norm(y.to(dt) + bias.to(dt) + res.to(dt), (d,), gamma.to(dt), beta.to(dt), 1e-12).view(b, l, d)
        e = enc.mean_pooling(h, mask)
        return F.normalize(e, p=2, dim=1) if normalize else e

    want = formula(torch.float64)
    _within_protocol(got, formula(torch.float32), want, f"add_layernorm_pool {(b, l, d)} lens 1..{l} normalize={normalize}")
    _within_protocol(two, formula(torch.float32), want, f"add_layernorm, then pool_l2norm {(b, l, d)} lens 1..{l} normalize={normalize}")
    if normalize:
        np.testing.assert_allclose((got.double() ** 2).sum(1).cpu().numpy(), 1.0, atol=1e-6, rtol=0)


@pytest.mark.parametrize("normalize", [True, False])
def test_folded_layernorm_pool_fed_by_slabs_at_every_length(normalize):
    """cmr_encoder_add_layernorm_partials_pool, bf16, d = 256, b = l = 64, lens = 1 .. 64.  The slabs are random fp32 numbers on a grid coarse
    enough that their sum in slab order is exact and IS the y of the other form, so both feeds of the kernel see the same rows: the
    tolerance of test_last_layer_partials_with_the_encoder_tail_folded_in (tests/test_encoder_small_m_gpu.py) against the formula on the 16-bit
    LayerNorm output, and equal bits between the two feeds."""
    import torch
    import torch.nn.functional as F
    from comorag_amd import _lib as L
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    b = l = 64
    d, k, dt = 256, 1024, torch.bfloat16
    ns, nbytes = C.c_int32(0), C.c_int64(0)
    L.check(L.lib().cmr_encoder_linear_small_split(1, d, k, L.CMR_BF16, C.byref(ns), C.byref(nbytes)))      # the split of a (d x k) weight; bytes of ONE token row's slabs
    n_split = int(ns.value)
    assert n_split >= 2 and int(nbytes.value) == n_split * d * 4
    y, res, bias, gamma, beta = _ln_inputs(b, l, d, dt)
    y = torch.where(y.abs() < 2.0 ** -8, torch.zeros_like(y), y)                                    # last bit of every y >= 2^-15 (exactness below)
    g = torch.Generator(device="cuda").manual_seed(n_split)
    part = torch.empty((n_split, b * l, d), dtype=torch.float32, device="cuda")
    assert part.numel() * 4 == int(nbytes.value) * b * l
    # multiples of 2^-10 in [-2, 2]: a running sum stays below 2^4 on that grid (14 bits); y - sum then spans 2^4 .. 2^-15 — exact in fp32
    part[:-1] = (torch.randn((n_split - 1, b * l, d), generator=g, device="cuda") * 1024.0).round().clamp_(-2048.0, 2048.0) / 1024.0
    run = torch.zeros((b * l, d), dtype=torch.float32, device="cuda")
    for sp in range(n_split - 1):
        run += part[sp]
    part[-1] = y.float() - run
    assert torch.equal(run + part[-1], y.float())                                                   # the slab-order fp32 sum is y, to the bit
    lens = torch.arange(1, l + 1, dtype=torch.int32, device="cuda")
    fz = _stages(d, 1, dt)
    got = FusedBertLayers.add_layernorm_partials_pool(fz, part, bias, res, gamma, beta, lens, b, l, normalize)
    other = fz.add_layernorm_pool(y, bias, res, gamma, beta, lens, b, l, normalize)
    hidden = fz.add_layernorm(y, bias, res, gamma, beta).view(b, l, d)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (b, d) and torch.isfinite(got).all()
    mask = torch.arange(l, device="cuda")[None, :] < lens[:, None]
    want = (hidden.float() * mask[..., None]).sum(1) / lens[:, None].float()
    if normalize:
        want = F.normalize(want, p=2, dim=1)
    ulp = 2.0 ** -8
    tol = max(3e-6 if normalize else 3e-5, 1.5 * ulp * float(want.abs().max()))
    print(f"slab-fed LN + pool normalize={normalize}: split {n_split}, max abs diff {float((got - want).abs().max()):.3e} (tol {tol:.3e}), "
          f"vs the y-fed form {float((got - other).abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=tol, rtol=1e-5)
    assert torch.equal(got, other)                                                                  # same rows, same order of every sum
