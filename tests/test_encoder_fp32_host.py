"""Host logic of the fp32 opt-in of the fused encoder stack (embedding_model/fused_bert.py, config `embedding_fused_fp32`): which models
`why_not(model, fp32=True)` accepts, and that nothing changes for a caller who does not pass the flag."""


def test_fp32_gate_is_opt_in_and_every_other_reason_still_applies():
    import torch
    from comorag_amd.embedding_model import fused_bert
    from comorag_amd.utils.config_utils import BaseConfig
    from oracle import encode_torch as enc
    m32, _ = enc.tiny_bert(hidden=128, layers=1, heads=4, inter=256, max_pos=32)      # 32-wide heads
    m64, _ = enc.tiny_bert(hidden=256, layers=1, heads=4, inter=512, max_pos=32)
    assert next(m64.parameters()).dtype == torch.float32
    assert "16-bit" in fused_bert.why_not(m64) and "16-bit" in fused_bert.why_not(m64, fp32=False)
    assert fused_bert.why_not(m64, fp32=True) is None
    assert "head width" in fused_bert.why_not(m32, fp32=True)
    assert fused_bert.why_not(m64.to(torch.bfloat16), fp32=True) is None                # the 16-bit models are accepted either way
    mx, _ = enc.tiny_xlmr(hidden=128, layers=1, heads=2, inter=128, max_pos=66)
    assert fused_bert.why_not(mx, fp32=True) is None and "16-bit" in fused_bert.why_not(mx)
    assert "16-bit" in fused_bert.why_not(mx.double(), fp32=True)                       # fp64 is no dtype of the kernels
    m64.float().config.hidden_act = "relu"
    assert "activation" in fused_bert.why_not(m64, fp32=True)
    assert fused_bert.why_not(object(), fp32=True) == "not a BERT / RoBERTa / XLM-R encoder"
    assert BaseConfig().embedding_fused_fp32 is False
    assert BaseConfig(embedding_fused_fp32=True).embedding_fused_fp32 is True
