"""Model hyper-parameters read from GGUF metadata (llama / mixtral / granite families)."""
from __future__ import annotations

from dataclasses import dataclass

SUPPORTED_ARCHS = ("llama", "granite", "mistral", "mixtral", "qwen2", "qwen3", "qwen3moe")
NEOX_ARCHS = ("qwen2", "qwen3", "qwen3moe")   # llama.cpp LLAMA_ROPE_TYPE_NEOX families
QK_NORM_ARCHS = ("qwen3", "qwen3moe")  # per-head RMSNorm on Q and K before the RoPE (attn_q_norm / attn_k_norm)
MOE_ONLY_ARCHS = ("qwen3moe",)    # every FFN is routed experts: the file must carry expert_count


@dataclass
class ModelConfig:
    arch: str
    n_layer: int
    d_model: int
    n_head: int
    n_kv_head: int
    head_dim: int
    d_ff: int
    vocab: int
    ctx: int
    rope_base: float
    eps: float
    n_expert: int = 0
    n_expert_used: int = 0
    d_ff_expert: int = 0             # FFN width of one routed expert; 0: d_ff (Mixtral). See expert_ff
    tied_embeddings: bool = False
    embedding_scale: float = 1.0
    residual_scale: float = 1.0
    attention_scale: float = 0.0
    logit_scale: float = 1.0
    rope_neox: bool = False
    rope_pos_scale: float = 1.0      # 1 / rope.scaling.factor for linear scaling
    qk_norm: bool = False            # per-head Q/K RMSNorm over head_dim, before the RoPE (Qwen3)

    @property
    def attn_softmax_scale(self) -> float:
        return self.attention_scale if self.attention_scale > 0 else self.head_dim ** -0.5

    @property
    def expert_ff(self) -> int:
        """FFN width of a routed expert ({arch}.expert_feed_forward_length, else feed_forward_length)."""
        return self.d_ff_expert or self.d_ff

    @property
    def q_dim(self) -> int:
        return self.n_head * self.head_dim

    @property
    def kv_dim(self) -> int:
        return self.n_kv_head * self.head_dim

    @classmethod
    def from_gguf(cls, md: dict, tensor_names=()) -> "ModelConfig":
        a = str(md["general.architecture"])
        if a not in SUPPORTED_ARCHS:
            raise NotImplementedError(f"architecture {a!r} not supported (supported: {SUPPORTED_ARCHS})")

        def g(k, d=None):
            return md.get(f"{a}.{k}", d)

        if a in MOE_ONLY_ARCHS and not int(g("expert_count", 0) or 0):
            raise NotImplementedError(f"architecture {a!r} without {a}.expert_count is not supported "
                                      "(its FFNs are routed experts)")
        d = int(g("embedding_length"))
        nh = int(g("attention.head_count"))
        nkv = int(g("attention.head_count_kv", nh))
        hd = int(g("attention.key_length", d // nh))
        vl = g("attention.value_length")
        if vl is not None and int(vl) != hd:
            raise NotImplementedError(f"attention.key_length {hd} != attention.value_length {int(vl)}: "
                                      "K and V heads of different sizes are not supported")
        vocab = g("vocab_size")
        if vocab is None:
            vocab = len(md.get("tokenizer.ggml.tokens", []))
        return cls(
            arch=a, n_layer=int(g("block_count")), d_model=d, n_head=nh, n_kv_head=nkv, head_dim=hd,
            d_ff=int(g("feed_forward_length")), vocab=int(vocab), ctx=int(g("context_length", 4096)),
            rope_base=float(g("rope.freq_base", 10000.0)), eps=float(g("attention.layer_norm_rms_epsilon", 1e-5)),
            n_expert=int(g("expert_count", 0) or 0), n_expert_used=int(g("expert_used_count", 0) or 0),
            d_ff_expert=int(g("expert_feed_forward_length", 0) or 0),
            tied_embeddings="output.weight" not in set(tensor_names) if tensor_names else False,
            embedding_scale=float(g("embedding_scale", 1.0)), residual_scale=float(g("residual_scale", 1.0)),
            attention_scale=float(g("attention.scale", 0.0)), logit_scale=float(g("logit_scale", 1.0)),
            rope_neox=a in NEOX_ARCHS, qk_norm=a in QK_NORM_ARCHS,
            rope_pos_scale=(1.0 / float(g("rope.scaling.factor", 1.0) or 1.0)
                            if str(g("rope.scaling.type", "none")) == "linear" else 1.0),
        )
