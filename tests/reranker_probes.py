"""Models, tokenizers and pairs of the cross-encoder reranker tests (tests/test_rerank_host.py, tests/test_rerank_gpu.py) — TEST
INFRASTRUCTURE.  No bge-reranker weights exist offline: the sequence classifiers are seed-initialised at the shapes of
oracle.encode_torch.tiny_bert / tiny_xlmr, with the base model's own state dict, and scaled so that the logits vary
(query / key weights x 12 as tests/test_encoder_fused_gpu._peaked_tiny_bert, both head weights x 8: 25 pairs give logits of std ~0.16)."""
import copy

import numpy as np

WORDS = ("the a an and of to in she he it her his was were had be good pious mother grave snow spring prince slipper golden ball "
         "pumpkin coach midnight stepmother sisters bird tree wish dress dance king son generate representation for this sentence "
         "retrieve relevant articles what who how did when").split()


class XlmrPairTokenizer:
    """tiny_xlmr's tokenizer has no pair template: `<s> A </s></s> B </s>` assembled here (XLM-R's own pair format), truncated as
    transformers' `truncation=True` does (tokens leave the longer segment one at a time)."""
    padding_side = "right"

    def __init__(self, fast):
        self.fast, self.pad_token_id = fast, fast.pad_token_id

    def __call__(self, queries, passages, truncation=True, max_length=512, **kw):
        rows = []
        for q, p in zip(queries, passages):
            a = list(self.fast(q, add_special_tokens=False)["input_ids"])
            b = list(self.fast(p, add_special_tokens=False)["input_ids"])
            while truncation and len(a) + len(b) > max_length - 4:
                (a if len(a) > len(b) else b).pop()
            rows.append([0] + a + [2, 2] + b + [2])
        return {"input_ids": rows}


def make_cross_encoder(kind: str, dtype=None, num_labels: int = 1, layers: int = 3, **config_overrides):
    """(model, tokenizer): `kind` = "bert" (BertForSequenceClassification, pairs carry token type 1) or "xlmr"
    (XLMRobertaForSequenceClassification, one token type).  The weights are rounded to `dtype` and returned as fp32: the oracle's fp32
    arithmetic runs on the SAME 16-bit-representable weights the 16-bit model holds."""
    import torch
    from transformers import BertForSequenceClassification, XLMRobertaForSequenceClassification
    from oracle import encode_torch as enc
    if kind == "bert":
        base, tok = enc.tiny_bert(hidden=256, layers=layers, heads=4, inter=512, max_pos=128)
    else:
        base, fast = enc.tiny_xlmr(hidden=256, layers=layers, heads=4, inter=512, max_pos=514)
        tok = XlmrPairTokenizer(fast)
    cfg = copy.deepcopy(base.config)
    cfg.num_labels = num_labels
    for k, v in config_overrides.items():
        setattr(cfg, k, v)
    torch.manual_seed(11)
    model = (BertForSequenceClassification if kind == "bert" else XLMRobertaForSequenceClassification)(cfg).eval()
    inner = model.bert if kind == "bert" else model.roberta
    inner.load_state_dict(base.state_dict(), strict=False)
    with torch.no_grad():
        for lyr in inner.encoder.layer:
            lyr.attention.self.query.weight.mul_(12.0)
            lyr.attention.self.key.weight.mul_(12.0)
        if kind == "bert":
            inner.pooler.dense.weight.mul_(8.0)
            model.classifier.weight.mul_(8.0)
        else:
            model.classifier.dense.weight.mul_(8.0)
            model.classifier.out_proj.weight.mul_(8.0)
        if dtype is not None:
            model.to(dtype).float()
    return model, tok


def make_pairs(n: int = 25, seed: int = 3):
    """n (query, passage) pairs of vocabulary words (digits would be [UNK]): a one-word passage, one long enough to be truncated at
    128 tokens, the others 2 .. 90 words."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        q = " ".join(rng.choice(WORDS, size=int(rng.integers(3, 9))))
        plen = 1 if i == 0 else (200 if i == 1 else int(rng.integers(2, 90)))
        out.append((q, " ".join(rng.choice(WORDS, size=plen))))
    return out


def tokenize(tok, pairs, max_length: int):
    """(ids, token types or None) per pair, as CrossEncoderReranker.tokenize_pairs calls the tokenizer."""
    enc = tok([q for q, _ in pairs], [p for _, p in pairs], truncation=True, max_length=max_length, return_token_type_ids=True)
    ids = [list(r) for r in enc["input_ids"]]
    try:
        types = [list(r) for r in enc["token_type_ids"]]
    except (KeyError, TypeError):
        types = None
    return ids, types


def reference_logits(model, ids, types, pad_id: int, batch: int = 8) -> np.ndarray:
    """The transformers forward of `model` (its own dtype and device) over the pairs in arrival-order mini-batches padded to their longest
    row: logits[:, 0] as float64."""
    import torch
    dev = next(model.parameters()).device
    out = []
    with torch.no_grad():
        for i in range(0, len(ids), batch):
            rows = ids[i:i + batch]
            l = max(len(r) for r in rows)
            arr = np.full((len(rows), l), pad_id, np.int64)
            mask = np.zeros((len(rows), l), np.int64)
            tt = np.zeros((len(rows), l), np.int64)
            for j, r in enumerate(rows):
                arr[j, :len(r)], mask[j, :len(r)] = r, 1
                if types is not None:
                    tt[j, :len(r)] = types[i + j]
            kw = {"token_type_ids": torch.from_numpy(tt).to(dev)} if types is not None else {}
            logits = model(input_ids=torch.from_numpy(arr).to(dev), attention_mask=torch.from_numpy(mask).to(dev), **kw).logits
            out.append(logits[:, 0].double().cpu().numpy())
    return np.concatenate(out)
