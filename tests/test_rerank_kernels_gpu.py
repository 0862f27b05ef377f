"""The two kernels of the cross-encoder tail (comorag_amd/csrc/encoder_kernels.hip): cmr_encoder_attention_cls — the attention of token 0 of
every sequence alone — against the softmax formula on the same rounded inputs, and cmr_encoder_cls_head — the one-logit classification head —
against its formula in fp64.  16-bit tolerances: TOL of tests/test_encoder_fused_gpu.py; fp32 and the head's fp32 output: the
e_got <= 4 e_ref + 4 ulp32(max|want|) protocol of tests/test_encoder_fp32_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests.test_encoder_fp32_gpu import _within_protocol
from tests.test_encoder_fused_gpu import TOL

pytestmark = pytest.mark.gpu

DTYPES = ["bfloat16", "float16", "float32"]
SHAPES = [(3, 100, 2, 64), (5, 37, 4, 64), (2, 129, 1, 64), (1, 64, 3, 64), (2, 300, 2, 64), (2, 65, 2, 64), (1, 63, 1, 64), (3, 100, 3, 32), (2, 129, 2, 32)]


class _Stages:
    """FusedBertLayers' kernel wrappers without a model around them."""
    def __init__(self, hidden, heads, dtype):
        import torch
        from comorag_amd import _lib as L
        from comorag_amd.embedding_model.fused_bert import FusedBertLayers
        self.hidden, self.n_heads = hidden, heads
        self.cmr_dtype = {torch.bfloat16: L.CMR_BF16, torch.float16: L.CMR_F16, torch.float32: L.CMR_F32}[dtype]
        self.attention = FusedBertLayers.attention.__get__(self)
        self.attention_cls = FusedBertLayers.attention_cls.__get__(self)
        self.cls_head = FusedBertLayers.cls_head.__get__(self)


def _cls_formula(qkv, lens_dev, b, l, heads, hd):
    """softmax(q K^T / sqrt(hd), keys >= lens masked) V for the query row of token 0, in qkv's own precision: [b, heads * hd]."""
    import torch
    x = qkv.view(b, l, 3, heads, hd)
    q, k, v = x[:, 0, 0], x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)            # [b, heads, hd], [b, heads, l, hd] x 2
    scores = (k @ q[..., None])[..., 0] / float(np.sqrt(hd))                                         # [b, heads, l]
    keymask = torch.arange(l, device=qkv.device)[None, :] >= lens_dev[:, None]
    scores = scores.masked_fill(keymask[:, None, :], float("-inf"))
    return (torch.softmax(scores, dim=-1)[:, :, None, :] @ v)[:, :, 0].reshape(b, heads * hd)


def _case(b, l, heads, hd, tdt):
    import torch
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l + hd)
    qkv = (torch.randn((b * l, 3 * heads * hd), generator=g, device="cuda") * 1.5).to(tdt)           # peaked, non-symmetric scores
    lens = np.random.default_rng(l).integers(1, l + 1, size=b).astype(np.int32)
    lens[0] = l
    if b > 1:
        lens[1] = 1 if l < 200 else l - 130
    return qkv, lens


def _check(got, qkv, lens_dev, b, l, heads, hd, dtype, what):
    import torch
    assert torch.isfinite(got.float()).all()
    if dtype == "float32":
        _within_protocol(got, _cls_formula(qkv, lens_dev, b, l, heads, hd), _cls_formula(qkv.double(), lens_dev, b, l, heads, hd), what)
    else:
        want = _cls_formula(qkv.float(), lens_dev, b, l, heads, hd)
        print(f"{what}: max|got - want| {float((got.float() - want).abs().max()):.3e}")
        np.testing.assert_allclose(got.float().cpu().numpy(), want.cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attention_cls_vs_softmax_formula(dtype, shape):
    import torch
    b, l, heads, hd = shape
    tdt = getattr(torch, dtype)
    qkv, lens = _case(b, l, heads, hd, tdt)
    lens_dev = torch.from_numpy(lens).cuda()
    fz = _Stages(heads * hd, heads, tdt)
    got = fz.attention_cls(qkv, lens_dev, b, l)
    again = fz.attention_cls(qkv, lens_dev, b, l)
    assert got.dtype == tdt and got.shape == (b, heads * hd)
    assert torch.equal(got, again)                                                                   # two runs, identical bits
    _check(got, qkv, lens_dev, b, l, heads, hd, dtype, f"attention_cls {dtype} {shape}")
    for s in range(b):                                                                               # a sequence alone: the bits it has in the batch
        alone = fz.attention_cls(qkv[s * l:(s + 1) * l].contiguous(), torch.from_numpy(lens[s:s + 1].copy()).cuda(), 1, l)
        assert torch.equal(alone[0], got[s]), s
    v0 = qkv.view(b, l, 3, heads * hd)[:, 0, 2]
    for s in np.nonzero(lens == 1)[0]:                                                               # one key: its weight is exactly 1
        assert torch.equal(got[s], v0[s]), s
    poisoned = qkv.clone().view(b, l, -1)
    for s in range(b):
        poisoned[s, lens[s]:] = float("nan")                                                         # rows >= lens[s] are never read
    assert torch.equal(fz.attention_cls(poisoned.view(b * l, -1), lens_dev, b, l), got)
    full = fz.attention(qkv, lens_dev, b, l).view(b, l, heads * hd)[:, 0]                             # row 0 of the all-rows kernel
    tol = TOL.get(dtype, 1e-5)
    np.testing.assert_allclose(got.float().cpu().numpy(), full.float().cpu().numpy(), atol=tol, rtol=tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [64, 32])
def test_attention_cls_every_length(dtype, hd):
    import torch
    b = l = 80
    heads, tdt = 2, getattr(torch, dtype)
    qkv, _ = _case(b, l, heads, hd, tdt)
    lens = np.arange(1, 81, dtype=np.int32)
    lens_dev = torch.from_numpy(lens).cuda()
    got = _Stages(heads * hd, heads, tdt).attention_cls(qkv, lens_dev, b, l)
    _check(got, qkv, lens_dev, b, l, heads, hd, dtype, f"attention_cls {dtype} every length hd {hd}")
    assert torch.equal(got[0], qkv.view(b, l, 3, heads * hd)[0, 0, 2])


def test_attention_cls_argument_checks():
    import torch
    from comorag_amd import _lib as L
    x = torch.zeros((16, 192), device="cuda", dtype=torch.bfloat16)
    lens = torch.ones((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((2, 64), device="cuda", dtype=torch.bfloat16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = L.lib().cmr_encoder_attention_cls
    xp, lp, op = C.c_void_p(x.data_ptr()), C.c_void_p(lens.data_ptr()), C.c_void_p(out.data_ptr())
    assert f(0, xp, L.CMR_BF16, lp, 1, 16, 1, 64, op, st) == L.CMR_OK
    assert f(0, None, L.CMR_BF16, lp, 1, 16, 1, 64, op, st) == L.CMR_ERR_INVALID
    assert f(0, xp, L.CMR_BF16, lp, 0, 16, 1, 64, op, st) == L.CMR_ERR_INVALID
    assert f(0, xp, L.CMR_BF16, lp, 1, 16, 1, 48, op, st) == L.CMR_ERR_INVALID
    assert f(0, xp, 7, lp, 1, 16, 1, 64, op, st) == L.CMR_ERR_INVALID
    assert f(0, xp, L.CMR_BF16, lp, 1, 16, 1, 64, C.c_void_p(out.data_ptr() + 8), st) == L.CMR_ERR_INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- classification head
def _head_case(d, b, stride_mul, tdt, biases):
    """x rows stride_mul * d apart; w1's rows scaled so that a third of the pre-activations saturate (|.| > 10), a third sit near 0."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(d * 7 + stride_mul)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    xs = rnd(33, stride_mul * d).to(tdt)
    scale = torch.tensor([30.0, 1.0, 0.01], device="cuda").repeat(d)[:d]
    w1 = (rnd(d, d) / float(np.sqrt(d)) * scale[:, None]).to(tdt)
    w2 = (rnd(d) * 0.25).to(tdt)
    b1 = (rnd(d) * 0.1).to(tdt) if biases else None
    b2 = rnd(1).to(tdt) if biases else None
    return xs[:b], (w1, b1, w2, b2)


def _head_formula(x, head, d, prec):
    import torch
    w1, b1, w2, b2 = (t.to(prec) if t is not None else None for t in head)
    pre = x[:, :d].to(prec) @ w1.t() + (b1 if b1 is not None else 0)
    return torch.tanh(pre) @ w2 + (b2[0] if b2 is not None else 0), pre


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [256, 384, 768, 1024, 2048])
@pytest.mark.parametrize("layout", ["contiguous", "strided", "no-bias"])
def test_cls_head_vs_fp64_formula(dtype, d, layout):
    """b = 1, 3 and 33 rows of one input set: the protocol's maxima run over the 37 outputs of the three calls (a single output's fp32
    reference error can be zero by chance), and a row's bits do not depend on b — row s of every call is row s of the 33-row call."""
    import torch
    tdt = getattr(torch, dtype)
    stride_mul, biases = (5 if layout == "strided" else 1), layout != "no-bias"
    fz = _Stages(d, 1, tdt)
    got, ref, want = [], [], []
    for b in (33, 3, 1):
        x, head = _head_case(d, b, stride_mul, tdt, biases)
        out = fz.cls_head(x, stride_mul * d, head, b)
        assert out.dtype == torch.float32 and out.shape == (b,)
        assert torch.equal(out, fz.cls_head(x, stride_mul * d, head, b))                              # two runs, identical bits
        w, pre = _head_formula(x, head, d, torch.float64)
        if b == 33:
            assert float((pre.abs() > 10).float().mean()) > 0.1 and float((pre.abs() < 0.1).float().mean()) > 0.1
        else:
            assert torch.equal(out, got[0][:b])                                                       # a row alone / among three: its bits in the batch
        got.append(out); ref.append(_head_formula(x, head, d, torch.float32)[0]); want.append(w)
    _within_protocol(torch.cat(got), torch.cat(ref), torch.cat(want), f"cls_head {dtype} d {d} {layout}")


def test_cls_head_argument_checks():
    import torch
    from comorag_amd import _lib as L
    f = L.lib().cmr_encoder_cls_head
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = torch.zeros((2056 * 2056,), device="cuda", dtype=torch.bfloat16)
    out = torch.zeros((4,), device="cuda")
    p, o = C.c_void_p(w.data_ptr()), C.c_void_p(out.data_ptr())
    assert f(0, p, 256, p, p, p, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_OK
    for d in (2050, 260):
        assert f(0, p, d, p, p, p, p, 2, d, L.CMR_BF16, o, st) == L.CMR_ERR_UNSUPPORTED
    assert f(0, p, 264, p, p, p, p, 2, 264, L.CMR_BF16, o, st) == L.CMR_OK                            # a multiple of 8 that is none of 16
    assert f(0, p, 260, p, p, p, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_ERR_UNSUPPORTED               # rows that are not 16-byte aligned
    assert f(0, p, 256, p, p, p, p, 2, 256, 7, o, st) == L.CMR_ERR_INVALID
    assert f(0, None, 256, p, p, p, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_ERR_INVALID
    assert f(0, p, 256, None, p, p, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_ERR_INVALID
    assert f(0, p, 256, p, p, None, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_ERR_INVALID
    assert f(0, p, 256, p, p, p, p, 2, 256, L.CMR_BF16, None, st) == L.CMR_ERR_INVALID
    assert f(0, p, 128, p, p, p, p, 2, 256, L.CMR_BF16, o, st) == L.CMR_ERR_INVALID                   # x_stride < d
    torch.cuda.synchronize()
