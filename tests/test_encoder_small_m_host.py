"""Host logic of the short-row route of the fused encoder stack (`FusedBertLayers(small_m=True)`, config `embedding_fused_small_m` /
`embedding_small_m_rows`): off by default, ignored by fp32 models, bound in the ctypes table, and argument checks that need no device."""
import ctypes as C
import inspect


def test_config_defaults_are_off_and_the_row_limit_is_the_kernels():
    from comorag_amd.embedding_model import fused_bert
    from comorag_amd.utils.config_utils import BaseConfig
    cfg = BaseConfig()
    assert cfg.embedding_fused_small_m is False
    assert 1 <= cfg.embedding_small_m_rows <= fused_bert.SMALL_M_MAX_ROWS == 128
    assert cfg.embedding_small_m_rows == fused_bert.SMALL_M_ROWS
    assert BaseConfig(embedding_fused_small_m=True, embedding_small_m_rows=48).embedding_small_m_rows == 48
    sig = inspect.signature(fused_bert.FusedBertLayers.__init__)
    assert sig.parameters["small_m"].default is False and sig.parameters["small_m_rows"].default is None


def test_fp32_models_ignore_the_flag_and_16_bit_ones_arm_it():
    import torch
    from comorag_amd.embedding_model import fused_bert
    from oracle import encode_torch as enc
    model, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    assert next(model.parameters()).dtype == torch.float32
    assert fused_bert.FusedBertLayers(model, fp32=True, small_m=True).small_m_rows == 0           # fp32: the flag is ignored
    m16 = model.to(torch.bfloat16)
    assert fused_bert.FusedBertLayers(m16).small_m_rows == 0                                      # not asked for
    assert fused_bert.FusedBertLayers(m16, small_m=True).small_m_rows == fused_bert.SMALL_M_ROWS
    assert fused_bert.FusedBertLayers(m16, small_m=True, small_m_rows=48).small_m_rows == 48
    assert fused_bert.FusedBertLayers(m16, small_m=True, small_m_rows=4096).small_m_rows == 128   # the kernels' limit
    assert fused_bert.FusedBertLayers(m16, small_m=True, small_m_rows=0).small_m_rows == 0


def test_why_not_is_unchanged():
    import torch
    from comorag_amd.embedding_model import fused_bert
    from oracle import encode_torch as enc
    assert list(inspect.signature(fused_bert.why_not).parameters) == ["model", "fp32", "head32"]
    m32, _ = enc.tiny_bert(hidden=128, layers=1, heads=4, inter=256, max_pos=32)
    m64, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    assert "16-bit" in fused_bert.why_not(m64) and fused_bert.why_not(m64, fp32=True) is None
    assert fused_bert.why_not(m32.to(torch.bfloat16)) == "head width is not 64"
    assert fused_bert.why_not(m32, head32=True) is None


def test_ctypes_table_carries_the_new_symbols_and_checks_come_before_any_device_call():
    from comorag_amd import _lib as L
    new = ["cmr_encoder_linear_small", "cmr_encoder_linear_small_partials", "cmr_encoder_linear_small_split", "cmr_encoder_add_layernorm_partials",
           "cmr_encoder_add_layernorm_partials_pool"]
    lib = L.lib()
    for name in new:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.cmr_abi_version() == L.ABI_VERSION == 2                                            # functions added only
    s, nbytes = C.c_int32(0), C.c_int64(0)
    # the split is a function of (n, k): the same for every m, bf16 and f16; the slab bytes follow m
    for n, k in [(768, 768), (768, 3072), (1024, 4096), (1024, 1024), (384, 1536), (384, 384), (96, 64)]:
        got = set()
        for m in (1, 17, 80, 128):
            for dt in (L.CMR_BF16, L.CMR_F16):
                assert lib.cmr_encoder_linear_small_split(m, n, k, dt, C.byref(s), C.byref(nbytes)) == L.CMR_OK
                assert nbytes.value == s.value * m * n * 4
                got.add(s.value)
        assert len(got) == 1 and (k // 32) % s.value == 0 and k // s.value >= min(k, 128), (n, k, got)
    assert lib.cmr_encoder_linear_small_split(80, 768, 3072, L.CMR_BF16, C.byref(s), C.byref(nbytes)) == L.CMR_OK and (768 // 16) * s.value >= 192
    # refusals that need no device: this runs on a host without one
    buf = (C.c_char * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert lib.cmr_encoder_linear_small(0, None, p, p, 16, 64, 64, L.CMR_BF16, 0, p, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_linear_small(0, p, p, p, 0, 64, 64, L.CMR_BF16, 0, p, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_linear_small(0, p, p, p, 129, 64, 64, L.CMR_BF16, 0, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_linear_small(0, p, p, p, 16, 64, 48, L.CMR_BF16, 0, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_linear_small(0, p, p, p, 16, 40, 64, L.CMR_F16, 0, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_linear_small(0, p, p, p, 16, 64, 64, L.CMR_F32, 0, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_linear_small(0, C.c_void_p(p.value + 8), p, p, 16, 64, 64, L.CMR_BF16, 0, p, None) == L.CMR_ERR_UNSUPPORTED
    assert b"aligned" in lib.cmr_last_error()
    assert lib.cmr_encoder_linear_small_partials(0, p, p, 16, 64, 64, L.CMR_BF16, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_linear_small_partials(0, p, p, 129, 64, 64, L.CMR_BF16, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_add_layernorm_partials(0, None, 1, None, None, p, p, 1e-12, 4, 64, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_add_layernorm_partials(0, p, 0, None, None, p, p, 1e-12, 4, 64, L.CMR_BF16, p, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_add_layernorm_partials(0, p, 1, None, None, p, p, 1e-12, 4, 64, L.CMR_F32, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_add_layernorm_partials_pool(0, p, 1, None, None, p, p, 1e-12, 1, 16, 64, L.CMR_BF16, None, 1, p, p, None) == L.CMR_ERR_INVALID
    assert lib.cmr_encoder_add_layernorm_partials_pool(0, p, 1, None, None, p, p, 1e-12, 1, 20, 64, L.CMR_BF16, p, 1, p, p, None) == L.CMR_ERR_UNSUPPORTED
    assert lib.cmr_encoder_add_layernorm_partials_pool(0, p, 1, None, None, p, p, 1e-12, 1, 16, 64, L.CMR_F32, p, 1, p, p, None) == L.CMR_ERR_UNSUPPORTED


def test_the_route_is_not_armed_where_the_tanh_epilogue_runs(monkeypatch):
    """The route's GELU is the erf form: with gelu = "epilogue" in effect a model would compute two functions depending on the batch size."""
    import torch
    from comorag_amd.embedding_model import fused_bert
    from oracle import encode_torch as enc
    model, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    m16 = model.to(torch.bfloat16)
    monkeypatch.setattr(fused_bert, "gelu_epilogue_available", lambda device, dtype: True)
    fz = fused_bert.FusedBertLayers(m16, gelu="epilogue", small_m=True)
    assert fz.gelu_path == "hipblaslt-epilogue-tanh" and fz.small_m_rows == 0
    monkeypatch.setattr(fused_bert, "gelu_epilogue_available", lambda device, dtype: False)
    fz = fused_bert.FusedBertLayers(m16, gelu="epilogue", small_m=True)      # the build does not fuse it: exact path, route armed
    assert fz.gelu_path == "exact-erf-kernel" and fz.small_m_rows == fused_bert.SMALL_M_ROWS


def test_strided_views_are_refused_before_any_call():
    import types
    import pytest
    import torch
    from comorag_amd import _lib as L
    from comorag_amd.embedding_model.fused_bert import FusedBertLayers
    fz = types.SimpleNamespace(cmr_dtype=L.CMR_BF16)
    x, w = torch.zeros((16, 128), dtype=torch.bfloat16), torch.zeros((64, 128), dtype=torch.bfloat16)
    for call in (FusedBertLayers.linear_small, FusedBertLayers.linear_small_partials):
        with pytest.raises(AssertionError):
            call(fz, x[:, ::2], w[:, :64].contiguous())
        with pytest.raises(AssertionError):
            call(fz, x, w.t().contiguous().t())                        # [64, 128], column-major
        with pytest.raises(AssertionError):
            call(fz, x, w[:, :64].contiguous())                              # k mismatch
