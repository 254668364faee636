"""The prompt encoders on the HIP path: the T5-XXL encoder (``text_encoder_2``) and the CLIP-L text tower (``text_encoder``) that
``FluxPriorReduxPipeline.encode_prompt`` runs on a prompt-cache miss (reached from pipe_prior_redux(...), batch_generate_flux_kshot.py:459-465,
outpainting_updown_sampling_redux.py:1237-1243; the reference loads both in bf16, batch_…:120-137).

Both classes follow upstream's bf16 graphs op for op (transformers modeling_t5.py with eager attention, modeling_clip.py with SDPA):
every Linear is ``drag_gemm_bf16`` (bias and residual adds in its epilogue, each rounded where torch rounds), the rest is
csrc/textenc.hip (attention, T5's RMSNorm and gated NewGELU, CLIP's QuickGELU, the embedding gather) and the affine LayerNorm of
``drag_layernorm_modulate_bf16``.  Tokenizers stay the reference's host tokenizers.  They keep the call surface ``encode_prompt_with``
uses — ``parameters()``, ``__call__(input_ids, output_hidden_states=False)`` with ``.pooler_output`` / ``[0]`` — so ``TextCache`` and
``FluxPriorReduxPipeline.from_pretrained(text_encoder=..., text_encoder_2=...)`` take them in place of the ``transformers`` modules.

Row i of a batch has the bits of prompt i alone (every launch is row-independent and the GEMM tile policy computes the same bits for
every tile choice); work buffers are cached per input shape (LRU of 3) and outputs are fresh tensors.
"""
from __future__ import annotations

import json
import math
import os
import re
from collections import OrderedDict
from dataclasses import dataclass, fields

import torch

from . import ops
from .flux_params import load_safetensors_dir

MAX_TOKENS = 512            # the attention kernel's limit: T5's max_sequence_length in the reference


@dataclass
class T5EncoderConfig:
    """the T5Config fields the encoder reads (names as in ``config.json``)"""
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"
    is_decoder: bool = False

    @classmethod
    def from_dict(cls, d: dict) -> "T5EncoderConfig":
        cfg = cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})
        cfg.validate()
        return cfg

    @classmethod
    def from_json(cls, path: str) -> "T5EncoderConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def validate(self) -> None:
        act = self.feed_forward_proj.split("-")
        if self.is_decoder:
            raise NotImplementedError("T5EncoderHIP: a T5 decoder is not supported (the text encoder is an encoder stack)")
        if self.d_kv != 64:
            raise NotImplementedError(f"T5EncoderHIP: head_dim (d_kv) {self.d_kv} is not supported (the attention kernel is head_dim 64)")
        if len(act) != 2 or act[0] != "gated" or act[1] not in ("gelu", "gelu_new"):
            raise NotImplementedError(f"T5EncoderHIP: feed_forward_proj {self.feed_forward_proj!r} is not supported (only 'gated-gelu', "
                                      "i.e. gated NewGELU as in FLUX.1's T5-XXL)")
        if self.d_model % 64 or self.d_ff % 64 or self.d_model > 4096:
            raise NotImplementedError(f"T5EncoderHIP: d_model {self.d_model} / d_ff {self.d_ff} must be multiples of 64, d_model <= 4096")


@dataclass
class ClipTextConfig:
    """the CLIPTextConfig fields the text tower reads (names as in ``config.json``)"""
    vocab_size: int = 49408
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    max_position_embeddings: int = 77
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"
    eos_token_id: int = 2

    @classmethod
    def from_dict(cls, d: dict) -> "ClipTextConfig":
        d = d.get("text_config", d)
        cfg = cls(**{f.name: d[f.name] for f in fields(cls) if f.name in d})
        cfg.validate()
        return cfg

    @classmethod
    def from_json(cls, path: str) -> "ClipTextConfig":
        with open(path) as f:
            return cls.from_dict(json.load(f))

    def validate(self) -> None:
        if self.hidden_size % self.num_attention_heads or self.hidden_size // self.num_attention_heads != 64:
            raise NotImplementedError(f"ClipTextHIP: head_dim {self.hidden_size / self.num_attention_heads:g} is not supported (the attention "
                                      "kernel is head_dim 64)")
        if self.hidden_act != "quick_gelu":
            raise NotImplementedError(f"ClipTextHIP: hidden_act {self.hidden_act!r} is not supported (CLIP-L's is 'quick_gelu')")
        if self.hidden_size % 64 or self.intermediate_size % 64 or self.hidden_size > 4096:
            raise NotImplementedError("ClipTextHIP: hidden / intermediate sizes must be multiples of 64, hidden <= 4096")
        if self.max_position_embeddings > MAX_TOKENS:
            raise NotImplementedError(f"ClipTextHIP: max_position_embeddings {self.max_position_embeddings} > {MAX_TOKENS}")


def t5_relative_buckets(S: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """bucket ids of the relative positions k - q = -(S-1) ... S-1 of a bidirectional (encoder) T5 attention, int64 [2S-1]: the arithmetic of
    ``T5Attention._relative_position_bucket`` (float32 log on the host), once per offset instead of once per (q, k) pair"""
    rel = torch.arange(-(S - 1), S, dtype=torch.long)
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    rel = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return out + torch.where(rel < max_exact, rel, large)


def clip_pool_index(ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """the row CLIPTextTransformer pools per prompt: argmax(ids) when ``eos_token_id == 2`` (configs older than transformers PR #24773,
    FLUX.1's among them), else the first position of ``eos_token_id`` (0 when absent, as argmax of all-false)"""
    ids = ids.to(torch.int64)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


class EncoderOutput:
    """``last_hidden_state`` [B, S, D] bf16 (also ``out[0]``) and, for CLIP, ``pooler_output`` [B, D] bf16"""

    def __init__(self, last_hidden_state: torch.Tensor, pooler_output: torch.Tensor | None = None):
        self.last_hidden_state, self.pooler_output = last_hidden_state, pooler_output

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]


def _strip(sd: dict, prefix: str) -> dict:
    return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}


class _Mapping:
    """consumes a ``transformers`` state dict key by key: a missing key is named, and so is any key left unread at the end"""

    def __init__(self, sd: dict, who: str):
        self.sd, self.who, self.used = sd, who, set()

    def __call__(self, *names: str) -> torch.Tensor:
        for n in names:
            if n in self.sd:
                self.used.add(n)
                return self.sd[n]
        raise KeyError(f"{self.who}: state dict has no {' / '.join(names)}")

    def finish(self, ignore: str = r"$^") -> None:
        left = sorted(k for k in self.sd if k not in self.used and not re.fullmatch(ignore, k))
        if left:
            raise KeyError(f"{self.who}: unexpected state-dict keys {left[:8]}{' ...' if len(left) > 8 else ''}")


def _dev(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.bfloat16).contiguous()


class _EncoderBase:
    def __init__(self, device):
        self.device = torch.device(device)
        self._bufs: OrderedDict = OrderedDict()

    def parameters(self):
        return iter(self._params)

    def eval(self):
        return self

    def _buffers(self, key, make):
        """work buffers of one input shape (LRU of 3: the encoders see B x 512 / B x 77 tokens, B the prompt count)"""
        if key in self._bufs:
            self._bufs.move_to_end(key)
        else:
            self._bufs[key] = make()
            while len(self._bufs) > 3:
                self._bufs.popitem(last=False)
        return self._bufs[key]

    def _ids(self, input_ids, vocab: int, max_len: int) -> tuple[torch.Tensor, torch.Tensor]:
        """(host int64 ids, device int64 ids), checked on the host before any launch"""
        ids = torch.as_tensor(input_ids).detach().to("cpu", torch.int64)
        if ids.dim() == 1:
            ids = ids[None]
        if ids.dim() != 2 or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= max_len:
            raise ValueError(f"{type(self).__name__}: expected input_ids [B, S] with 1 <= S <= {max_len}, got {tuple(ids.shape)}")
        if int(ids.min()) < 0 or int(ids.max()) >= vocab:
            raise ValueError(f"{type(self).__name__}: token id outside [0, {vocab})")
        return ids, ids.to(self.device)


class T5EncoderHIP(_EncoderBase):
    """``T5EncoderModel`` (FLUX.1's ``text_encoder_2``, T5-XXL v1.1: gated NewGELU, no attention scaling, bucketed relative-position
    bias from layer 0 shared by every layer), all-bf16 as the reference loads it."""

    def __init__(self, cfg: T5EncoderConfig, state_dict: dict, device="cuda"):
        super().__init__(device)
        cfg.validate()
        self.cfg = cfg
        m = _Mapping(state_dict, "T5EncoderHIP")
        dev = self.device
        self.embed = _dev(m("shared.weight", "encoder.embed_tokens.weight"), dev)
        for alias in ("shared.weight", "encoder.embed_tokens.weight"):     # tied: either or both may be present
            if alias in state_dict:
                m.used.add(alias)
        self.layers = []
        for i in range(cfg.num_layers):
            a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
            self.layers.append(dict(
                ln1=_dev(m(a + "layer_norm.weight"), dev),
                wqkv=_dev(torch.cat([m(a + f"SelfAttention.{n}.weight") for n in "qkv"]), dev),
                wo=_dev(m(a + "SelfAttention.o.weight"), dev),
                ln2=_dev(m(f + "layer_norm.weight"), dev),
                wi=_dev(torch.cat([m(f + "DenseReluDense.wi_0.weight"), m(f + "DenseReluDense.wi_1.weight")]), dev),
                wff=_dev(m(f + "DenseReluDense.wo.weight"), dev)))
        # [num_buckets, H] stays on the host: the [H, 2S-1] Toeplitz rows are gathered from it once per S
        self.rel_bias = m("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight").detach().to("cpu", torch.bfloat16)
        self.final_ln = _dev(m("encoder.final_layer_norm.weight"), dev)
        m.finish()
        inner = cfg.num_heads * cfg.d_kv
        if self.layers and tuple(self.layers[0]["wqkv"].shape) != (3 * inner, cfg.d_model):
            raise ValueError(f"T5EncoderHIP: q/k/v weights {tuple(self.layers[0]['wqkv'].shape)} do not match the config")
        self._params = [self.embed, self.final_ln] + [t for L in self.layers for t in L.values()]
        self._rel: OrderedDict = OrderedDict()

    @classmethod
    def from_pretrained(cls, path: str, device="cuda") -> "T5EncoderHIP":
        """a ``text_encoder_2`` directory: config.json + *.safetensors"""
        return cls(T5EncoderConfig.from_json(os.path.join(path, "config.json")), load_safetensors_dir(path), device)

    @classmethod
    def from_module(cls, module, device=None) -> "T5EncoderHIP":
        """the weights of a live ``transformers`` T5EncoderModel"""
        dev = device if device is not None else next(module.parameters()).device
        return cls(T5EncoderConfig.from_dict(module.config.to_dict()), module.state_dict(), dev)

    @classmethod
    def synthetic(cls, cfg: T5EncoderConfig, seed: int = 0, device="cuda") -> "T5EncoderHIP":
        """seeded random parameters of the architecture (no checkpoint offline)"""
        return cls(cfg, synthetic_t5_state_dict(cfg, seed), device)

    def _rel_table(self, S: int) -> torch.Tensor:
        if S not in self._rel:
            b = t5_relative_buckets(S, self.cfg.relative_attention_num_buckets, self.cfg.relative_attention_max_distance)
            self._rel[S] = self.rel_bias[b].t().contiguous().to(self.device)
            while len(self._rel) > 3:
                self._rel.popitem(last=False)
        return self._rel[S]

    def __call__(self, input_ids, output_hidden_states: bool = False, **_) -> EncoderOutput:
        if output_hidden_states:
            raise NotImplementedError("T5EncoderHIP: output_hidden_states is not supported (encode_prompt does not use it)")
        cfg = self.cfg
        _, ids = self._ids(input_ids, cfg.vocab_size, MAX_TOKENS)
        B, S = ids.shape
        M, D, H, F = B * S, cfg.d_model, cfg.num_heads, cfg.d_ff
        inner = H * cfg.d_kv
        bf = dict(dtype=torch.bfloat16, device=self.device)
        w = self._buffers((B, S), lambda: dict(x0=torch.empty((M, D), **bf), x1=torch.empty((M, D), **bf), n=torch.empty((M, D), **bf),
                                               qkv=torch.empty((M, 3 * inner), **bf), att=torch.empty((M, inner), **bf),
                                               h=torch.empty((M, 2 * F), **bf), g=torch.empty((M, F), **bf)))
        rel = self._rel_table(S)
        x, y, n, qkv = w["x0"], w["x1"], w["n"], w["qkv"]
        ops.embed_gather(ids, self.embed, x)
        eps = cfg.layer_norm_epsilon
        for L in self.layers:
            ops.t5_rmsnorm(x, L["ln1"], n, eps)
            ops.gemm(n, L["wqkv"], qkv)
            ops.textenc_attention(qkv, qkv[:, inner:], qkv[:, 2 * inner:], w["att"], B, S, H, ld=3 * inner, batch_stride=S * 3 * inner,
                                  scale=1.0, rel_bias=rel, eager=True)
            ops.gemm(w["att"], L["wo"], y, resid=x)
            x, y = y, x
            ops.t5_rmsnorm(x, L["ln2"], n, eps)
            ops.gemm(n, L["wi"], w["h"])
            ops.gated_new_gelu(w["h"], w["g"])
            ops.gemm(w["g"], L["wff"], y, resid=x)
            x, y = y, x
        out = torch.empty((B, S, D), **bf)
        ops.t5_rmsnorm(x, self.final_ln, out, eps)
        return EncoderOutput(out)


class ClipTextHIP(_EncoderBase):
    """``CLIPTextModel`` (FLUX.1's ``text_encoder``, CLIP ViT-L/14 text tower: causal, scale 1/8, QuickGELU, pre-LN), all-bf16;
    ``pooler_output`` is the final LayerNorm's row at ``clip_pool_index``."""

    def __init__(self, cfg: ClipTextConfig, state_dict: dict, device="cuda"):
        super().__init__(device)
        cfg.validate()
        self.cfg = cfg
        m = _Mapping(_strip(state_dict, "text_model."), "ClipTextHIP")
        dev = self.device
        self.tok = _dev(m("embeddings.token_embedding.weight"), dev)
        self.pos = _dev(m("embeddings.position_embedding.weight"), dev)
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            self.layers.append(dict(
                ln1_g=_dev(m(p + "layer_norm1.weight"), dev), ln1_b=_dev(m(p + "layer_norm1.bias"), dev),
                wqkv=_dev(torch.cat([m(a + f"{n}_proj.weight") for n in "qkv"]), dev),
                bqkv=_dev(torch.cat([m(a + f"{n}_proj.bias") for n in "qkv"]), dev),
                wo=_dev(m(a + "out_proj.weight"), dev), bo=_dev(m(a + "out_proj.bias"), dev),
                ln2_g=_dev(m(p + "layer_norm2.weight"), dev), ln2_b=_dev(m(p + "layer_norm2.bias"), dev),
                w1=_dev(m(p + "mlp.fc1.weight"), dev), b1=_dev(m(p + "mlp.fc1.bias"), dev),
                w2=_dev(m(p + "mlp.fc2.weight"), dev), b2=_dev(m(p + "mlp.fc2.bias"), dev)))
        self.lnf_g, self.lnf_b = _dev(m("final_layer_norm.weight"), dev), _dev(m("final_layer_norm.bias"), dev)
        m.finish(ignore=r"embeddings\.position_ids")        # a buffer older checkpoints carry
        self._params = [self.tok, self.pos, self.lnf_g, self.lnf_b] + [t for L in self.layers for t in L.values()]

    @classmethod
    def from_pretrained(cls, path: str, device="cuda") -> "ClipTextHIP":
        """a ``text_encoder`` directory: config.json + *.safetensors"""
        return cls(ClipTextConfig.from_json(os.path.join(path, "config.json")), load_safetensors_dir(path), device)

    @classmethod
    def from_module(cls, module, device=None) -> "ClipTextHIP":
        """the weights of a live ``transformers`` CLIPTextModel"""
        dev = device if device is not None else next(module.parameters()).device
        return cls(ClipTextConfig.from_dict(module.config.to_dict()), module.state_dict(), dev)

    @classmethod
    def synthetic(cls, cfg: ClipTextConfig, seed: int = 0, device="cuda") -> "ClipTextHIP":
        return cls(cfg, synthetic_clip_state_dict(cfg, seed), device)

    def __call__(self, input_ids, output_hidden_states: bool = False, **_) -> EncoderOutput:
        if output_hidden_states:
            raise NotImplementedError("ClipTextHIP: output_hidden_states is not supported (encode_prompt does not use it)")
        cfg = self.cfg
        host_ids, ids = self._ids(input_ids, cfg.vocab_size, cfg.max_position_embeddings)
        B, S = ids.shape
        M, D, H, F = B * S, cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
        bf = dict(dtype=torch.bfloat16, device=self.device)
        w = self._buffers((B, S), lambda: dict(x0=torch.empty((M, D), **bf), x1=torch.empty((M, D), **bf), n=torch.empty((M, D), **bf),
                                               qkv=torch.empty((M, 3 * D), **bf), att=torch.empty((M, D), **bf),
                                               h=torch.empty((M, F), **bf)))
        x, y, n, qkv = w["x0"], w["x1"], w["n"], w["qkv"]
        ops.embed_gather(ids, self.tok, x, pos=self.pos)
        eps = cfg.layer_norm_eps
        for L in self.layers:
            ops.layernorm(x, n, M, D, gamma=L["ln1_g"], beta=L["ln1_b"], eps=eps)
            ops.gemm(n, L["wqkv"], qkv, bias=L["bqkv"])
            ops.textenc_attention(qkv, qkv[:, D:], qkv[:, 2 * D:], w["att"], B, S, H, ld=3 * D, batch_stride=S * 3 * D,
                                  scale=(D // H) ** -0.5, causal=True, eager=False)
            ops.gemm(w["att"], L["wo"], y, bias=L["bo"], resid=x)
            x, y = y, x
            ops.layernorm(x, n, M, D, gamma=L["ln2_g"], beta=L["ln2_b"], eps=eps)
            ops.gemm(n, L["w1"], w["h"], bias=L["b1"])
            ops.quick_gelu(w["h"], w["h"])
            ops.gemm(w["h"], L["w2"], y, bias=L["b2"], resid=x)
            x, y = y, x
        out = torch.empty((B, S, D), **bf)
        ops.layernorm(x, out, M, D, gamma=self.lnf_g, beta=self.lnf_b, eps=eps)
        pooled = torch.empty((B, D), **bf)
        for b, i in enumerate(clip_pool_index(host_ids, cfg.eos_token_id).tolist()):
            pooled[b].copy_(out[b, i])
        return EncoderOutput(out, pooled)


def _randn(g: torch.Generator, *shape, std: float = 0.02) -> torch.Tensor:
    return (torch.randn(*shape, generator=g) * std).to(torch.bfloat16)


def synthetic_t5_state_dict(cfg: T5EncoderConfig, seed: int) -> dict:
    """seeded parameters under the ``transformers`` names (unit-scale norms, 1/sqrt(fan-in) projections)"""
    g = torch.Generator().manual_seed(int(seed))
    D, inner, F = cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff
    sd = {"shared.weight": _randn(g, cfg.vocab_size, D, std=1.0),
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": _randn(g, cfg.relative_attention_num_buckets, cfg.num_heads, std=1.0),
          "encoder.final_layer_norm.weight": torch.ones(D, dtype=torch.bfloat16)}
    for i in range(cfg.num_layers):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        for n in "qkv":
            sd[a + f"SelfAttention.{n}.weight"] = _randn(g, inner, D, std=D ** -0.5)
        sd[a + "SelfAttention.o.weight"] = _randn(g, D, inner, std=inner ** -0.5)
        sd[a + "layer_norm.weight"] = torch.ones(D, dtype=torch.bfloat16)
        sd[f + "DenseReluDense.wi_0.weight"] = _randn(g, F, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wi_1.weight"] = _randn(g, F, D, std=D ** -0.5)
        sd[f + "DenseReluDense.wo.weight"] = _randn(g, D, F, std=F ** -0.5)
        sd[f + "layer_norm.weight"] = torch.ones(D, dtype=torch.bfloat16)
    return sd


def synthetic_clip_state_dict(cfg: ClipTextConfig, seed: int) -> dict:
    g = torch.Generator().manual_seed(int(seed))
    D, F = cfg.hidden_size, cfg.intermediate_size
    sd = {"text_model.embeddings.token_embedding.weight": _randn(g, cfg.vocab_size, D),
          "text_model.embeddings.position_embedding.weight": _randn(g, cfg.max_position_embeddings, D, std=0.01),
          "text_model.final_layer_norm.weight": torch.ones(D, dtype=torch.bfloat16),
          "text_model.final_layer_norm.bias": torch.zeros(D, dtype=torch.bfloat16)}
    for i in range(cfg.num_hidden_layers):
        p = f"text_model.encoder.layers.{i}."
        for n in ("q", "k", "v", "out"):
            sd[p + f"self_attn.{n}_proj.weight"] = _randn(g, D, D, std=D ** -0.5)
            sd[p + f"self_attn.{n}_proj.bias"] = _randn(g, D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = _randn(g, F, D, std=D ** -0.5), _randn(g, F)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = _randn(g, D, F, std=F ** -0.5), _randn(g, D)
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + f"{n}.weight"], sd[p + f"{n}.bias"] = torch.ones(D, dtype=torch.bfloat16), torch.zeros(D, dtype=torch.bfloat16)
    return sd


class StandInTokenizer:
    """the tokenizer of ``--synthetic-weights`` runs, which have no tokenizer files: a prompt's UTF-8 bytes as ids ``3 + byte % (vocab_size - 5)`` (below
    ``vocab_size``), then ``eos_id``, padded with ``pad_id`` / truncated to ``max_length`` — deterministic, not a real vocabulary.  Same
    call surface as the ``transformers`` tokenizers where ``encode_prompt_with`` uses them."""

    def __init__(self, vocab_size: int, model_max_length: int, eos_id: int, pad_id: int, bos_id: int | None = None):
        self.vocab_size, self.model_max_length, self.eos_id, self.pad_id, self.bos_id = vocab_size, model_max_length, eos_id, pad_id, bos_id

    def __call__(self, texts, padding="max_length", max_length=None, truncation=True, return_tensors="pt", **_):
        L = max_length or self.model_max_length
        rows = []
        for t in ([texts] if isinstance(texts, str) else texts):
            ids = ([self.bos_id] if self.bos_id is not None else []) + [3 + (c % (self.vocab_size - 5)) for c in t.encode()]
            ids = ids[:L - 1] + [self.eos_id]
            rows.append(ids + [self.pad_id] * (L - len(ids)))

        class _Out:
            input_ids = torch.tensor(rows, dtype=torch.long)
        return _Out()
