"""Host logic of the 32-wide-head opt-in of the fused encoder stack (embedding_model/fused_bert.py, config `embedding_fused_head32`): which
models `why_not(model, head32=True)` accepts, how the flag combines with `fp32=True`, and that nothing changes for a caller who passes neither."""


def test_head32_gate_is_opt_in_and_combines_with_the_fp32_gate():
    import torch
    from comorag_amd.embedding_model import fused_bert
    from comorag_amd.utils.config_utils import BaseConfig
    from oracle import encode_torch as enc
    m32, _ = enc.tiny_bert(hidden=128, layers=1, heads=4, inter=256, max_pos=32)      # 32-wide heads
    assert next(m32.parameters()).dtype == torch.float32
    # the fp32 model: refused with head32 alone, for the 16-bit reason; accepted with both flags
    assert "16-bit" in fused_bert.why_not(m32, head32=True)
    assert "head width" in fused_bert.why_not(m32, fp32=True)
    assert fused_bert.why_not(m32, fp32=True, head32=True) is None
    # the same model in bf16: the default and the fp32 flag keep today's refusal, head32 admits it
    m32 = m32.to(torch.bfloat16)
    assert "head width" in fused_bert.why_not(m32) and "head width" in fused_bert.why_not(m32, fp32=True)
    assert fused_bert.why_not(m32, head32=False) == "head width is not 64"
    assert fused_bert.why_not(m32, head32=True) is None
    assert fused_bert.why_not(m32.to(torch.float16), head32=True) is None
    # 16-wide heads stay refused, with the reason every other width keeps
    m16, _ = enc.tiny_bert(hidden=64, layers=1, heads=4, inter=128, max_pos=32)
    assert fused_bert.why_not(m16.to(torch.bfloat16), head32=True) == "head width is not 64"
    # a 64-wide model is accepted with and without the flag
    m64, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    m64 = m64.to(torch.bfloat16)
    assert fused_bert.why_not(m64) is None and fused_bert.why_not(m64, head32=True) is None
    # every other reason applies unchanged
    m32.config.hidden_act = "relu"
    assert "activation" in fused_bert.why_not(m32, head32=True)
    assert BaseConfig().embedding_fused_head32 is False
    assert BaseConfig(embedding_fused_head32=True, embedding_fused_fp32=True).embedding_fused_head32 is True
