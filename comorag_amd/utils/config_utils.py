"""The configuration fields the embedding / retrieval path reads.

The reference keeps one big dataclass (src/comorag/utils/config_utils.py:17-298); only the fields
below are read on this path.  Any object with these attributes works — in
particular the reference's own `BaseConfig` instance — because every consumer here uses getattr
with the reference default.
"""
from dataclasses import dataclass, field
from typing import Optional


@dataclass
class BaseConfig:
    # reference fields (same names, same defaults: utils/config_utils.py:128-176 of the reference)
    embedding_model_name: str = field(default="nvidia/NV-Embed-v2", metadata={"ref": "config_utils.py:128-129"})   # the reference's default (its factory
                                                  # has no class for it and returns None, embedding_model/__init__.py:10-17: set a "bge-" model)
    embedding_batch_size: int = 32                # :132
    embedding_return_as_normalized: bool = True   # :136
    embedding_max_seq_len: int = 2048             # :140
    embedding_model_dtype: str = "auto"           # :144  (never read by the reference; honoured here)
    linking_top_k: int = 5                        # :176
    synonymy_edge_topk: int = 2047                # :152
    synonymy_edge_query_batch_size: int = 1000    # :156
    synonymy_edge_key_batch_size: int = 10000     # :160
    synonymy_edge_sim_threshold: float = 0.8      # :164
    need_cluster: bool = True
    # new, opt-in (reference behaviour by default)
    index_dtype: str = "f32"                      # "f32" | "bf16" | "f16": storage dtype of the HBM index
    device: int = 0
    num_shards: int = 1                           # > 1: the HBM indexes are row-sharded over that many shards in THIS process (MultiDeviceIndex)
    devices: Optional[list] = None                # GPU of every shard (a device may repeat: logical shards); None = round the visible devices
    index_options: Optional[dict] = None          # route selectors for the HBM indexes (cmr_index_set_option names; "append_block_rows" for sharded ones)
    store_format: str = "parquet"                 # "parquet" (reference behaviour) | "sidecar" (append-only files)
    embedding_cache_enabled: bool = False         # probed with hasattr by the reference (BGEEmbedding.py:57-61)
    embedding_cache_path: Optional[str] = None
    embedding_length_bucketing: bool = True       # group a batch_encode call's prompts into mini-batches of similar token count
    embedding_tokenizer_threads: int = 2          # host threads tokenising ahead of the forward
    embedding_bucket_window: int = 4              # length bucketing sorts within windows of this many batches (the next windows are tokenised meanwhile)
    embedding_tokenizer_processes: int = 0        # 0: threads only; -1: worker PROCESSES started by the first corpus-sized batch_encode (>= 2 windows); N: N processes (the Rust tokenizer holds the GIL)
    embedding_forward_batches: int = 1            # length-bucketed path: a forward mini-batch holds up to this many reference batches' worth of tokens
    embedding_hip_graphs: int = 24                # fused encoder: mini-batch shapes kept as captured hipGraphs (0 = launch every forward eagerly)
    embedding_fused_encoder: bool = True          # 16-bit BERT encoders: HIP attention + bias/residual/LayerNorm stages, one QKV GEMM (embedding_model/fused_bert.py)
    embedding_fused_fp32: bool = False            # opt-in: fp32 BERT encoders (embedding_model_dtype "auto" / fp32 checkpoints) run the fused stack too, fp32 end to end (f32-input MFMA attention, fp32 LayerNorm kernels)
    embedding_fused_head32: bool = False          # opt-in: 32-wide heads (384 hidden / 12 heads: bge-small, e5-small, MiniLM) run the fused stack too (HD = 32 attention kernels); combinable with embedding_fused_fp32.  Off ONLY because three existing tests pin the default refusal "head width is not 64" (tests/test_encoder_fused_gpu.py, test_store_host.py, test_encoder_fp32_host.py): flip the default together with those tests
    embedding_fused_small_m: bool = False         # opt-in: a mini-batch of at most embedding_small_m_rows token rows (one short query) runs its linear layers on the library's weight-streaming small-M kernels instead of hipBLASLt (16-bit models; fp32 ones ignore it; not armed with embedding_gelu = "epilogue" in effect: the route's GELU is the exact erf form)
    embedding_small_m_rows: int = 96              # token rows b*l up to which that route is taken (at most 128): the measured crossover, profiles/encoder_small_m.json
    embedding_combine: int = 0                    # opt-in: W in 2..16 lets concurrent one-prompt encodes (ComoRAG's question threads) share ONE forward of up to W prompts of equal padded width, each caller with the bits of its solo call; needs embedding_fused_small_m (otherwise not armed); 0 = off (`combine_stats()`)
    embedding_combine_wait_us: int = 0            # that queue's gather window: the first caller waits until W prompts have joined or the window has passed; 0 = batches form only from calls that arrive while an earlier forward runs
    embedding_devices: Optional[list] = None     # GPUs of the corpus-encode replicas (BGEEmbedding.py:77 `device_map="auto"`): one copy of the layer stack each, bucketing windows dealt round them; None = `device` only
    embedding_encode_replicas: int = 0            # > the device count: logical replicas going round `embedding_devices` (rehearsal on a one-GPU box); 0 = one per device
    embedding_query_cache: int = 256              # single-string batch_encode results kept (by prompt, max_length, normalisation): a question is encoded three times per tri_retrieve — the same prompt each time; 0 = off
    # cross-encoder reranker (rerank.CrossEncoderReranker); inert unless one is constructed.  It also reads embedding_fused_fp32, embedding_fused_head32,
    # embedding_fused_small_m, embedding_small_m_rows, embedding_gelu and embedding_length_bucketing with the meaning they have above
    rerank_model_name: Optional[str] = None       # a one-logit sequence classifier (bge-reranker-base / -large / -v2-m3): AutoModelForSequenceClassification.from_pretrained
    rerank_model_dtype: str = "bf16"              # "bf16" | "f16"; anything else keeps the checkpoint's dtype (fp32 runs fused with embedding_fused_fp32)
    rerank_batch_size: int = 32                   # pairs per forward mini-batch
    rerank_max_seq_len: int = 512                 # pair truncation, clamped to the model's positions
    rerank_cls_tail: bool = False                 # True: the last layer runs for the CLS rows alone (cmr_encoder_attention_cls); off by measurement: 0.95 - 0.97 x the whole stack at 512 tokens, a tie by the rule at large bf16 (profiles/rerank.json)
    embedding_gelu: str = "exact"                 # fused encoder: "exact" = erf-form GELU kernel (the reference's function); "epilogue" = opt-in: FFN-up bias + GELU inside the hipBLASLt GEMM (TANH form, <= 4.8e-4 per activation away, ~7 % faster forward)


def cfg_get(cfg, name, default):
    return getattr(cfg, name, default) if cfg is not None else default
