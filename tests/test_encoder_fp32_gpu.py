"""The fp32 path of the fused encoder stack (comorag_amd/csrc/encoder_kernels.hip with dtype = CMR_F32, fused_bert.FusedBertLayers(fp32=True),
config `embedding_fused_fp32`): every HIP stage against the same function in fp64, measured next to torch's own fp32 evaluation, and the whole
encoder against the CPU oracle and the transformers fp32 forward.

Tolerance protocol of the kernel tests: `want` is the function in fp64 (torch on the GPU) on the same fp32 inputs, `ref` the same formula in
torch fp32 ops on the GPU (what the transformers forward computes), `got` the kernel.  With e_ref = max|ref - want| and e_got = max|got - want|
over every compared element, e_got <= 4 e_ref + 4 ulp32(max|want|): both are fp32 evaluations that differ in summation order, the chunked
online softmax adds one rescale rounding per 64-key chunk; a wrong lane map, a missed mask or a dropped chunk gives 1e-2 and more."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _Stages:
    """FusedBertLayers' kernel wrappers without a model around them, fp32."""
    def __init__(self, hidden, heads, eps=1e-12):
        from comorag_amd import _lib as L
        from comorag_amd.embedding_model.fused_bert import FusedBertLayers
        self.hidden, self.n_heads, self.eps = hidden, heads, eps
        self.cmr_dtype = L.CMR_F32
        self.attention = FusedBertLayers.attention.__get__(self)
        self.add_layernorm = FusedBertLayers.add_layernorm.__get__(self)
        self.add_layernorm_pool = FusedBertLayers.add_layernorm_pool.__get__(self)


def _within_protocol(got, ref, want, what):
    """e_got <= 4 e_ref + 4 ulp32(max|want|); prints the figures first (pytest -s shows them)."""
    import torch
    assert got.dtype == torch.float32 and ref.dtype == torch.float32 and want.dtype == torch.float64
    assert torch.isfinite(got).all()
    e_got = float((got.double() - want).abs().max())
    e_ref = float((ref.double() - want).abs().max())
    ulp = float(np.spacing(np.float32(float(want.abs().max()))))
    print(f"{what}: e_got {e_got:.3e}  e_ref {e_ref:.3e}  ratio {e_got / max(e_ref, 1e-30):.2f}  ulp32(max|want|) {ulp:.3e}")
    assert e_got <= 4.0 * e_ref + 4.0 * ulp, (what, e_got, e_ref, ulp)


# ---------------------------------------------------------------------------------------------------------------- attention
def _attention_formula(qkv, lens_dev, b, l, heads):
    """softmax(Q K^T / 8, keys >= lens masked) V in qkv's own precision: [b, l, heads, 64]."""
    import torch
    x = qkv.view(b, l, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    scores = q @ k.transpose(-1, -2) / 8.0
    keymask = torch.arange(l, device=qkv.device)[None, :] >= lens_dev[:, None]
    scores = scores.masked_fill(keymask[:, None, None, :], float("-inf"))
    return (torch.softmax(scores, dim=-1) @ v).permute(0, 2, 1, 3)


def _attention_case(b, l, heads):
    import torch
    hidden = heads * 64
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l)
    qkv = torch.randn((b * l, 3 * hidden), generator=g, device="cuda") * 1.5                      # peaked, non-symmetric scores
    lens = np.random.default_rng(l).integers(1, l + 1, size=b).astype(np.int32)
    lens[0] = l
    if b > 1:
        lens[1] = 1 if l < 200 else l - 130                                                       # a one-token row / a block of padding only
    return qkv, lens


# the issue's five shapes, then one on each side of the kernel's two switches: the 64-key chunk count (64 | 65, 128 | 129 keys) and the
# 128-row query block count (128 | 129 rows); one workgroup shape (4 waves) serves every l
@pytest.mark.parametrize("shape", [(3, 100, 2), (5, 37, 4), (2, 129, 1), (1, 64, 3), (2, 300, 2), (2, 65, 2), (2, 128, 2), (1, 63, 1)])
def test_attention_fp32_vs_fp64(shape):
    import torch
    b, l, heads = shape
    qkv, lens = _attention_case(b, l, heads)
    lens_dev = torch.from_numpy(lens).cuda()
    fz = _Stages(heads * 64, heads)
    got = fz.attention(qkv, lens_dev, b, l)
    again = fz.attention(qkv, lens_dev, b, l)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.isfinite(got).all()                                # padding rows included
    assert torch.equal(got, again)                                                                 # two runs, identical bits
    got = got.view(b, l, heads, 64)
    ref = _attention_formula(qkv, lens_dev, b, l, heads)
    want = _attention_formula(qkv.double(), lens_dev, b, l, heads)
    live = (torch.arange(l, device="cuda")[None, :] < lens_dev[:, None])                           # every row < lens[s], nothing left out
    _within_protocol(got[live], ref[live].contiguous(), want[live].contiguous(), f"attention {shape}")


def test_attention_fp32_a_sequence_alone_gives_the_same_bits():
    import torch
    b, l, heads = 3, 100, 2
    qkv, lens = _attention_case(b, l, heads)
    fz = _Stages(heads * 64, heads)
    whole = fz.attention(qkv, torch.from_numpy(lens).cuda(), b, l).view(b, l, -1)
    for s in range(b):
        alone = fz.attention(qkv[s * l:(s + 1) * l].contiguous(), torch.from_numpy(lens[s:s + 1].copy()).cuda(), 1, l).view(l, -1)
        assert torch.equal(alone, whole[s])


def test_fp32_entry_points_still_refuse_other_dtypes_and_misaligned_buffers():
    import ctypes as C
    import torch
    from comorag_amd import _lib as L
    x = torch.zeros((16, 192), device="cuda")
    lens = torch.ones((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((17, 64), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().cmr_encoder_attention(0, C.c_void_p(x.data_ptr()), 7, C.c_void_p(lens.data_ptr()), 1, 16, 1, 64, C.c_void_p(out.data_ptr()), st)
    assert rc == L.CMR_ERR_INVALID and "or f32" in L.lib().cmr_last_error().decode()
    g = torch.ones((64,), device="cuda")
    rc = L.lib().cmr_encoder_add_layernorm(0, C.c_void_p(out.data_ptr() + 8), None, None, C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr()), 1e-12, 4, 64,
                                           L.CMR_F32, C.c_void_p(out.data_ptr() + 2048), st)
    assert rc == L.CMR_ERR_INVALID                                                                 # fp32 rows are read as 16-byte vectors


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("d,rows", [(256, 7), (40, 130), (2048, 33), (768, 256), (768, 257), (1024, 64)])      # 768: either side of ENC_LN_FEW_ROWS
@pytest.mark.parametrize("parts", ["bias+residual", "residual", "plain"])
def test_add_layernorm_fp32_vs_fp64(d, rows, parts):
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(d + rows)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    y, res = rnd(rows, d) * 2 + 0.3, rnd(rows, d)
    bias, gamma, beta = rnd(d), 1 + 0.2 * rnd(d), 0.1 * rnd(d)
    use_b, use_r = parts == "bias+residual", parts != "plain"
    got = _Stages(d, 1).add_layernorm(y, bias if use_b else None, res if use_r else None, gamma, beta)
    z = y + (bias if use_b else 0) + (res if use_r else 0)
    ref = F.layer_norm(z, (d,), gamma, beta, 1e-12)
    z64 = y.double() + (bias.double() if use_b else 0) + (res.double() if use_r else 0)
    want = F.layer_norm(z64, (d,), gamma.double(), beta.double(), 1e-12)
    _within_protocol(got, ref, want, f"add_layernorm d={d} rows={rows} {parts}")


# Every vectors-per-lane bucket of both LayerNorm forms, every element type.  rows = 300: sixteen lanes per row, (d / 8 + 15) / 16 = 3, 4, 5, 7, 10,
# 14 -> buckets 4, 4, 6, 8, 12, 16.  rows = 7 (<= ENC_LN_FEW_ROWS): a wave per row, (d / 4 + 63) / 64 = 2, 2, 3, 4, 5, 7 -> buckets 2, 2, 3, 4, 6, 8.
# 16-bit: test_add_layernorm_kernel's fp32 reference and tolerances (tests/test_encoder_fused_gpu.py); fp32: the protocol above.
@pytest.mark.parametrize("dtype", ["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("rows", [7, 300])
@pytest.mark.parametrize("d", [384, 512, 640, 896, 1280, 1792])
def test_add_layernorm_every_vectors_per_lane_bucket(d, rows, dtype):
    import torch
    import torch.nn.functional as F
    from comorag_amd import _lib as L
    from tests.test_encoder_fused_gpu import TOL
    tdt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(d + rows)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    y, res = (rnd(rows, d) * 2 + 0.3).to(tdt), rnd(rows, d).to(tdt)
    bias, gamma, beta = rnd(d).to(tdt), (1 + 0.2 * rnd(d)).to(tdt), (0.1 * rnd(d)).to(tdt)
    fz = _Stages(d, 1)
    fz.cmr_dtype = {"bfloat16": L.CMR_BF16, "float16": L.CMR_F16, "float32": L.CMR_F32}[dtype]
    got = fz.add_layernorm(y, bias, res, gamma, beta)
    assert got.dtype == tdt and got.shape == (rows, d)
    ref = F.layer_norm(y.float() + bias.float() + res.float(), (d,), gamma.float(), beta.float(), 1e-12)
    if dtype == "float32":
        want = F.layer_norm(y.double() + bias.double() + res.double(), (d,), gamma.double(), beta.double(), 1e-12)
        _within_protocol(got, ref, want, f"add_layernorm d={d} rows={rows}")
    else:
        np.testing.assert_allclose(got.float().cpu().numpy(), ref.cpu().numpy(), atol=TOL[dtype], rtol=TOL[dtype])


@pytest.mark.parametrize("b,l,d", [(2, 16, 256), (5, 64, 768), (1, 32, 72), (4, 48, 2048)])
@pytest.mark.parametrize("normalize", [True, False])
def test_add_layernorm_pool_fp32_vs_fp64(b, l, d, normalize):
    """The last layer's LayerNorm with mean_pooling + F.normalize folded in, fp32: the LayerNorm output joins the partial row unrounded."""
    import torch
    import torch.nn.functional as F
    from oracle import encode_torch as enc
    g = torch.Generator(device="cuda").manual_seed(b * 1000 + l + d)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda")
    y, res = rnd(b * l, d), rnd(b * l, d)
    bias, gamma, beta = rnd(d), rnd(d), rnd(d)
    lens = torch.tensor(([1, l, max(1, l - 5), max(1, l // 2 + 3), 17] * 8)[:b], dtype=torch.int32).clamp_(max=l)      # a one-token row, a full one
    if b == 1:
        lens[0] = l - 5
    mask = (torch.arange(l)[None, :] < lens[:, None]).to(torch.int64).cuda()
    got = _Stages(d, 1).add_layernorm_pool(y, bias, res, gamma, beta, lens.cuda(), b, l, normalize)

    def formula(dt):
        h = F.layer_norm(y.to(dt) + bias.to(dt) + res.to(dt), (d,), gamma.to(dt), beta.to(dt), 1e-12).view(b, l, d)
        e = enc.mean_pooling(h, mask)
        return F.normalize(e, p=2, dim=1) if normalize else e

    _within_protocol(got, formula(torch.float32), formula(torch.float64), f"add_layernorm_pool {(b, l, d)} normalize={normalize}")
    if normalize:
        np.testing.assert_allclose((got.double() ** 2).sum(1).cpu().numpy(), 1.0, atol=1e-6, rtol=0)


# ---------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("kind", ["bert", "xlmr"])                                               # position offset 0 and 2
def test_embedding_kernels_fp32_vs_transformers_module(kind):
    import torch
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers, position_offset
    from oracle import encode_torch as enc
    model, tok = (enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=96) if kind == "bert"
                  else enc.tiny_xlmr(hidden=256, layers=1, heads=4, inter=512, max_pos=98))
    with torch.no_grad():
        for p in model.embeddings.parameters():
            p.mul_(30.0).add_(0.05)                   # init std 0.02: make the sum and its LayerNorm non-trivial
    model = model.to("cuda").eval()
    assert position_offset(model) == (0 if kind == "bert" else 2)
    fz = FusedBertLayers(model, fp32=True)
    b, l = 5, 96
    g = torch.Generator(device="cuda").manual_seed(7)
    ids = torch.randint(5, model.config.vocab_size, (b, l), generator=g, device="cuda")            # (no pad id: XLM-R derives positions from it)
    tt = torch.randint(0, 2, (b, l), generator=g, device="cuda") if kind == "bert" else None
    model64 = copy.deepcopy(model).double()
    for types in ((None, tt) if kind == "bert" else (None,)):
        got = fz.embed(ids, types).view(b, l, 256)
        with torch.no_grad():
            ref = model.embeddings(input_ids=ids, token_type_ids=types)
            want = model64.embeddings(input_ids=ids, token_type_ids=types)
        _within_protocol(got, ref, want, f"embed {kind} token types {'given' if types is not None else 'none'}")
    # the ragged kernel: the padded one's rows, bit for bit, on the real tokens
    lens = np.array([1, l, 33, 16, 95], np.int32)
    head = np.concatenate([lens, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)])
    packed = torch.from_numpy(np.concatenate([head, *[ids[r, :n].cpu().numpy().astype(np.int32) for r, n in enumerate(lens)]]).astype(np.int32)).cuda()
    a = fz.embed(ids, None).view(b, l, -1)
    r = fz.embed_ragged(packed[2 * b + 1:], packed[b:2 * b + 1], b, l).view(b, l, -1)
    assert torch.isfinite(r).all()
    for i, n in enumerate(lens):
        assert torch.equal(a[i, :n], r[i, :n])
    wide = fz.embed(torch.full((1, 3), 10 ** 9, device="cuda", dtype=torch.int64))                # out-of-table ids are clamped, not a fault
    assert torch.isfinite(wide).all()


# ---------------------------------------------------------------------------------------------------------------- the whole stack
_TEXTS = [f"the prince and the golden slipper number {i} " + "and the bird in the tree " * (i % 5) for i in range(11)]
_TEXTS += ["she was good and pious " * 40, "midnight"]


def _model_class():
    from comorag_amd.embedding_model import _get_embedding_model_class
    return _get_embedding_model_class("bge-tiny-random")


def _make(model, tok, **kw):
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=4, embedding_max_seq_len=2048, **kw)
    return _model_class()(global_config=cfg, embedding_model_name=cfg.embedding_model_name, model=copy.deepcopy(model), tokenizer=tok)


@pytest.mark.parametrize("kind", ["bert", "xlmr"])
def test_fp32_stack_vs_oracle_and_the_flag_changes_nothing_when_absent(kind):
    import torch
    from oracle import encode_torch as enc
    if kind == "bert":
        (model, tok), ml = enc.tiny_bert(hidden=128, layers=2, heads=2, inter=256, max_pos=128), 128
    else:
        (model, tok), ml = enc.tiny_xlmr(hidden=128, layers=1, heads=2, inter=128, max_pos=66), 64
    assert next(model.parameters()).dtype == torch.float32
    want = enc.batch_encode(model, tok, _TEXTS, batch_size=4, max_length=ml)                       # the CPU oracle
    want_one = enc.batch_encode(model, tok, "midnight", batch_size=4, max_length=ml)
    plain, fused = _make(model, tok), _make(model, tok, embedding_fused_fp32=True)
    # flag absent: the path of today, with today's reason
    assert plain.encoder_path.startswith("transformers (") and "16-bit" in plain.encoder_path and plain._fused is None
    assert fused.encoder_path == "hip-fused-layers" and fused._fused.dtype == torch.float32 and fused._fused.gelu_path == "exact-erf-kernel"
    err = {}
    for name, em in (("transformers", plain), ("fused", fused)):
        got, one = em.batch_encode(_TEXTS), em.batch_encode("midnight")
        assert got.shape == want.shape == (13, 128) and got.dtype == np.float32 and np.isfinite(got).all()
        err[name] = max(float(np.abs(got - want).max()), float(np.abs(one - want_one).max()))
    print(f"{kind}: max abs error vs the CPU oracle: fused {err['fused']:.3e}, transformers forward {err['transformers']:.3e}")
    assert err["fused"] <= 2.0 * err["transformers"] + 1e-6
    assert err["fused"] <= 2e-5
    plain.close(); fused.close()


def _peaked_fp32_bert():
    import torch
    from oracle import encode_torch as enc
    model, tok = enc.tiny_bert(hidden=256, layers=3, heads=4, inter=512, max_pos=128)
    with torch.no_grad():                              # random-init scores are ~0 (uniform attention): make the softmax matter
        for lyr in model.encoder.layer:
            lyr.attention.self.query.weight.mul_(12.0)
            lyr.attention.self.key.weight.mul_(12.0)
    return model, tok


def test_fp32_captured_graphs_equal_eager_forwards_also_from_many_threads():
    from concurrent.futures import ThreadPoolExecutor
    from comorag_amd.utils.config_utils import BaseConfig
    model, tok = _peaked_fp32_bert()
    mk = lambda **kw: _model_class()(global_config=BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=8, embedding_max_seq_len=128,
                                                              embedding_fused_fp32=True, embedding_query_cache=0, **kw),
                                     embedding_model_name="bge-tiny-random", model=copy.deepcopy(model), tokenizer=tok)
    em, eager = mk(), mk(embedding_hip_graphs=0)
    assert em.encoder_path == eager.encoder_path == "hip-fused-layers"
    queries = ["midnight", "what did the mother wish " * 3, "the prince and the golden slipper " * 6, "she was good and pious " * 12,
               "who how when", "the bird in the tree and the king and his son went to the dance " * 2]
    want = [eager.batch_encode(q) for q in queries]
    assert not eager._fused._graphs
    for rep in range(4):                                   # rep 0 eager, rep 1 captures, reps 2-3 replay
        for q, w in zip(queries, want):
            np.testing.assert_allclose(em.batch_encode(q), w, atol=2e-6)
    shapes = set(em._fused._graphs)
    assert 1 <= len(shapes) <= len(queries) and all(key[1] % 16 == 0 for key in shapes)
    with ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda i: em.batch_encode(queries[i % len(queries)]), range(96)))
    for i, g in enumerate(got):
        np.testing.assert_allclose(g, want[i % len(queries)], atol=2e-6)
    em.close(); eager.close()


def test_fp32_two_replicas_give_the_single_replica_rows():
    import torch
    from comorag_amd.utils.config_utils import BaseConfig
    model, tok = _peaked_fp32_bert()
    texts = [f"the prince and the golden slipper number {i} " + "and the bird in the tree " * (i % 4) + "midnight " * (i % 3) for i in range(40)]
    def make(**kw):
        cfg = BaseConfig(embedding_model_name="bge-tiny-random", embedding_batch_size=8, embedding_max_seq_len=128, embedding_fused_fp32=True, **kw)
        return _model_class()(global_config=cfg, embedding_model_name=cfg.embedding_model_name, model=copy.deepcopy(model), tokenizer=tok)
    one, many = make(), make(embedding_encode_replicas=2)
    assert len(one._replicas) == 0 and len(many._replicas) == 2 and many._replicas[1].fused.dtype == torch.float32
    want = one.batch_encode(texts)
    for rep in range(2):
        got = many.batch_encode(texts)
        assert got.shape == want.shape and np.array_equal(got, want), (rep, float(np.abs(got - want).max()))
    assert all(len(r.fused._seen) + len(r.fused._graphs) > 0 for r in many._replicas)
    one.close(); many.close()
