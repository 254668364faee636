"""FluxTransformerHIP — host driver of the Flux DiT forward on MI355X.

Mirrors ``FluxTransformer2DModel.forward`` (diffusers 0.33.1; the call the reference reaches on
every denoise step from batch_generate_flux_kshot.py:467-474 and
outpainting_updown_sampling_redux.py:1246-1257).  All arithmetic is in libdomainrag_hip.so; torch
only owns the device buffers.  MI355X-first layout decisions:

* text and image streams live in ONE joint activation buffer ``x[B, S_txt+S_img, D]`` for the
  whole forward (the GEMM / LayerNorm kernels address "batched rows"), so there are no concat /
  split copies between double-stream and single-stream blocks;
* q/k/v projections are fused into one [3D, D] weight; single-stream blocks write attention and
  MLP outputs side by side into one [M, 5D] buffer that feeds proj_out directly;
* every block's AdaLN modulation is computed by ONE GEMM per forward (all modulation weights are
  stacked), instead of 76 tiny launches;
* workspaces are allocated once per (B, S) and reused: 288 GB of HBM keeps weights (23.7 GB bf16)
  plus B=8 activations resident.
"""
from __future__ import annotations

import math
import os

import torch

from . import ops
from .flux_params import FluxConfig
from .step_cache import (STEP_CACHE_DEFAULT, STEP_CACHE_MAX_RUN_DEFAULT, STEP_CACHE_ORDER_DEFAULT, STEP_CACHE_SCOPE_DEFAULT,      # noqa: F401
                         STEP_CACHE_SCOPES, STEP_CACHE_WARMUP_DEFAULT, StepCache, StepDecision, compact_pairs, forecast_coefficient,
                         parse_step_cache, parse_step_cache_count, parse_step_cache_order, parse_step_cache_scope, pipeline_step_cache)

_SEPARATE_QPREP = os.environ.get("DRAG_QPREP_SEPARATE", "") not in ("", "0")     # measurement switches, read once
# single blocks: to_q|k|v + proj_mlp as ONE two-destination launch.  At the headline's 42 696 rows it saves a partial tile round
# (54.8 instead of 24 + 32) and measured nothing (same-box A/B, two rounds: fused 0.4440 / 0.4435 vs separate 0.4468 / 0.4454 images/s);
# at BASELINE configs[1]'s 1536 rows the fused launch is two exact rounds of 256x256 tiles (1400 TFLOP/s) where the separate ones are
# one round + 4.5 rounds of small tiles (1132 / 800-1000).  So the choice follows the library's own cost model per launch shape
# (ops.gemm_cost: fused when it is >= 10 % cheaper); DRAG_QKV_MLP_FUSED=1 / =0 force it on / off.
_FUSED_QKV_MLP = {"": None, "0": False}.get(os.environ.get("DRAG_QKV_MLP_FUSED", ""), True)
# the precision of the blocks' Linears: "bf16" (default) or "mxfp8" (opt-in: OCP MXFP8 operands on the block-scaled matrix instruction,
# ops.quantize_mxfp8 + ops.gemm_mxfp8); $DRAG_LINEAR_PRECISION sets the process default, read once
LINEAR_PRECISIONS = ("bf16", "mxfp8")
_LINEAR_PRECISION = os.environ.get("DRAG_LINEAR_PRECISION", "") or "bf16"
if _LINEAR_PRECISION not in LINEAR_PRECISIONS:
    raise ValueError(f"DRAG_LINEAR_PRECISION must be one of {LINEAR_PRECISIONS}, not {_LINEAR_PRECISION!r}")
# the precision of the blocks' attention: "bf16" (default) or "mxfp8" (opt-in: ops.qkv_prep_mxfp8 + ops.attention_mxfp8, e4m3 operands for
# both products; the format and its cost in accuracy: mx.py).  Independent of the Linears' mode.  $DRAG_ATTENTION_PRECISION sets the process
# default, read once
ATTENTION_PRECISIONS = ("bf16", "mxfp8")
_ATTENTION_PRECISION = os.environ.get("DRAG_ATTENTION_PRECISION", "") or "bf16"
if _ATTENTION_PRECISION not in ATTENTION_PRECISIONS:
    raise ValueError(f"DRAG_ATTENTION_PRECISION must be one of {ATTENTION_PRECISIONS}, not {_ATTENTION_PRECISION!r}")
# Linear shapes (N, K) that stay on bf16 INSIDE "mxfp8" mode: those whose MX route, the quantise pass of the activations included, was
# not faster than drag_gemm_bf16 in the interleaved same-process A/B of scripts/bench_gemm_mxfp8.py at the headline's 42 696 rows
# (profiles/mxfp8_gemm_ab.log).  A shape that was not measured moves.  With the 128x128 MX kernel (800-890 TFLOP/s against 1348-1434 of
# the bf16 GEMM) every headline shape measured (MX + quantise) / bf16 between 1.62 and 1.84, so all six stay; the single blocks' 21 504-row
# weight runs as its 9216- and 12 288-row ranges on the MX route, both listed.
_MX_STAYS_BF16: frozenset = frozenset({(9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288), (21504, 3072), (3072, 15360)})


def rope_tables(ids: torch.Tensor, axes_dims=(16, 56, 56), theta: float = 10000.0):
    """FluxPosEmbed on the host in float64 (as diffusers does off-MPS) -> fp32 [S, 64] cos / sin."""
    cos, sin = [], []
    pos = ids.detach().to("cpu", torch.float64)
    for i, d in enumerate(axes_dims):
        freqs = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
        ang = torch.outer(pos[:, i], freqs)
        cos.append(ang.cos().float())
        sin.append(ang.sin().float())
    return torch.cat(cos, dim=1).contiguous(), torch.cat(sin, dim=1).contiguous()


def latent_image_ids(h: int, w: int) -> torch.Tensor:
    ids = torch.zeros(h, w, 3)
    ids[..., 1] = torch.arange(h)[:, None]
    ids[..., 2] = torch.arange(w)[None, :]
    return ids.reshape(h * w, 3)


def linear_locations(cfg: FluxConfig) -> dict:
    """Where :class:`FluxTransformerHIP` keeps each Linear weight: every 2-D name of ``flux_params.param_shapes(cfg)`` ->
    ``(holder, row0, rows)``.  A holder names one resident tensor: ``("w", name)`` = ``model.w[name]``, ``("double", i, key)`` /
    ``("single", i, key)`` = ``model.double[i][key]`` / ``model.single[i][key]`` (the stacked ``wqkv`` / ``cwqkv`` / ``wqkvm`` hold
    several names as row ranges), ``("mod_w",)`` = the stacked modulation matrix, whose row offsets are ``model.mod_off``'s.  A pure
    function of the config (the constructor's layout, restated); LoRA adapters find their targets with it."""
    D, F = cfg.dim, cfg.mlp_ratio * cfg.dim
    loc: dict = {}
    names = ["x_embedder", "context_embedder", "proj_out", "time_text_embed.timestep_embedder.linear_1",
             "time_text_embed.timestep_embedder.linear_2", "time_text_embed.text_embedder.linear_1", "time_text_embed.text_embedder.linear_2"]
    if cfg.guidance_embeds:
        names += ["time_text_embed.guidance_embedder.linear_1", "time_text_embed.guidance_embedder.linear_2"]
    rows_of = {"x_embedder": D, "context_embedder": D, "proj_out": cfg.out_channels}
    for n in names:
        loc[n + ".weight"] = (("w", n + ".weight"), 0, rows_of.get(n, D))
    off = 0
    for i in range(cfg.num_layers):
        p = f"transformer_blocks.{i}."
        for nm in ("norm1", "norm1_context"):
            loc[p + nm + ".linear.weight"] = (("mod_w",), off, 6 * D)
            off += 6 * D
        for key, parts in (("wqkv", ("attn.to_q", "attn.to_k", "attn.to_v")), ("cwqkv", ("attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"))):
            for j, n in enumerate(parts):
                loc[p + n + ".weight"] = (("double", i, key), j * D, D)
        for key, n, rows in (("wo", "attn.to_out.0", D), ("cwo", "attn.to_add_out", D), ("w1", "ff.net.0.proj", F), ("w2", "ff.net.2", D),
                             ("cw1", "ff_context.net.0.proj", F), ("cw2", "ff_context.net.2", D)):
            loc[p + n + ".weight"] = (("double", i, key), 0, rows)
    for i in range(cfg.num_single_layers):
        p = f"single_transformer_blocks.{i}."
        loc[p + "norm.linear.weight"] = (("mod_w",), off, 3 * D)
        off += 3 * D
        for j, n in enumerate(("attn.to_q", "attn.to_k", "attn.to_v")):
            loc[p + n + ".weight"] = (("single", i, "wqkvm"), j * D, D)
        loc[p + "proj_mlp.weight"] = (("single", i, "wqkvm"), 3 * D, F)
        loc[p + "proj_out.weight"] = (("single", i, "wo"), 0, D)
    loc["norm_out.linear.weight"] = (("mod_w",), off, 2 * D)
    return loc


class FluxTransformerHIP:
    def __init__(self, cfg: FluxConfig, params: dict, device="cuda", linear_precision: str | None = None,
                 attention_precision: str | None = None):
        """``linear_precision``: "bf16" | "mxfp8" (None: $DRAG_LINEAR_PRECISION, else "bf16") — also a settable attribute; the bf16
        weights are kept in either mode, so one process can A/B.  ``attention_precision``: the same for the blocks' attention (None:
        $DRAG_ATTENTION_PRECISION, else "bf16"), also settable; the two modes are independent"""
        if cfg.attention_head_dim != 128:
            raise ValueError("the HIP attention kernel is specialised for head_dim 128 (all FLUX.1 models)")
        self.cfg = cfg
        self.device = torch.device(device)
        D = cfg.dim
        dev = self.device

        def g(name):
            return params[name].to(dev, torch.bfloat16).contiguous()

        def cat(names):
            return torch.cat([params[n].to(dev, torch.bfloat16) for n in names], dim=0).contiguous()

        self.w = {}
        for n in ("x_embedder", "context_embedder", "proj_out",
                  "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2",
                  "time_text_embed.text_embedder.linear_1", "time_text_embed.text_embedder.linear_2"):
            self.w[n + ".weight"], self.w[n + ".bias"] = g(n + ".weight"), g(n + ".bias")
        if cfg.guidance_embeds:
            for n in ("time_text_embed.guidance_embedder.linear_1", "time_text_embed.guidance_embedder.linear_2"):
                self.w[n + ".weight"], self.w[n + ".bias"] = g(n + ".weight"), g(n + ".bias")

        # ---- stacked modulation weights: [double i: norm1 (6D) | norm1_context (6D)]*L, [single: 3D]*Ls, norm_out 2D
        mod_w, mod_b = [], []
        self.mod_off = {}
        off = 0
        for i in range(cfg.num_layers):
            for nm in ("norm1", "norm1_context"):
                key = f"transformer_blocks.{i}.{nm}.linear"
                mod_w.append(key + ".weight"); mod_b.append(key + ".bias")
                self.mod_off[(i, nm)] = off
                off += 6 * D
        for i in range(cfg.num_single_layers):
            key = f"single_transformer_blocks.{i}.norm.linear"
            mod_w.append(key + ".weight"); mod_b.append(key + ".bias")
            self.mod_off[("s", i)] = off
            off += 3 * D
        mod_w.append("norm_out.linear.weight"); mod_b.append("norm_out.linear.bias")
        self.mod_off["out"] = off
        off += 2 * D
        self.mod_total = off
        self.mod_w, self.mod_b = cat(mod_w), cat(mod_b)

        self.double = []
        for i in range(cfg.num_layers):
            p = f"transformer_blocks.{i}."
            self.double.append(dict(
                wqkv=cat([p + "attn.to_q.weight", p + "attn.to_k.weight", p + "attn.to_v.weight"]),
                bqkv=cat([p + "attn.to_q.bias", p + "attn.to_k.bias", p + "attn.to_v.bias"]),
                cwqkv=cat([p + "attn.add_q_proj.weight", p + "attn.add_k_proj.weight", p + "attn.add_v_proj.weight"]),
                cbqkv=cat([p + "attn.add_q_proj.bias", p + "attn.add_k_proj.bias", p + "attn.add_v_proj.bias"]),
                nq=g(p + "attn.norm_q.weight"), nk=g(p + "attn.norm_k.weight"),
                cnq=g(p + "attn.norm_added_q.weight"), cnk=g(p + "attn.norm_added_k.weight"),
                wo=g(p + "attn.to_out.0.weight"), bo=g(p + "attn.to_out.0.bias"),
                cwo=g(p + "attn.to_add_out.weight"), cbo=g(p + "attn.to_add_out.bias"),
                w1=g(p + "ff.net.0.proj.weight"), b1=g(p + "ff.net.0.proj.bias"),
                w2=g(p + "ff.net.2.weight"), b2=g(p + "ff.net.2.bias"),
                cw1=g(p + "ff_context.net.0.proj.weight"), cb1=g(p + "ff_context.net.0.proj.bias"),
                cw2=g(p + "ff_context.net.2.weight"), cb2=g(p + "ff_context.net.2.bias")))
        self.single = []
        for i in range(cfg.num_single_layers):
            p = f"single_transformer_blocks.{i}."
            # to_q | to_k | to_v | proj_mlp stacked in one weight: either two GEMMs over its row ranges (default) or ONE two-destination
            # launch ($DRAG_QKV_MLP_FUSED=1: q/k/v into the qkv buffer, the GELU'd MLP hidden into the [attn | mlp] buffer)
            self.single.append(dict(
                wqkvm=cat([p + "attn.to_q.weight", p + "attn.to_k.weight", p + "attn.to_v.weight", p + "proj_mlp.weight"]),
                bqkvm=cat([p + "attn.to_q.bias", p + "attn.to_k.bias", p + "attn.to_v.bias", p + "proj_mlp.bias"]),
                nq=g(p + "attn.norm_q.weight"), nk=g(p + "attn.norm_k.weight"),
                wo=g(p + "proj_out.weight"), bo=g(p + "proj_out.bias")))
        self._ws_key = None
        self._rope_key = None
        self._mx_ready = False
        self._loras: dict = {}           # name -> {"adapter", "scale"}: the active LoRA adapters, in load order
        self._pristine: dict = {}        # holder -> a copy of the resident tensor as built, while an adapter touches it
        self.linear_precision = linear_precision or _LINEAR_PRECISION
        self.attention_precision = attention_precision or _ATTENTION_PRECISION

    # ------------------------------------------------------------------ MXFP8 mode
    # What moves (blocks only): both streams' to_q|k|v, the attention out-projections, ff up (+GELU) and ff down, the single blocks'
    # q|k|v + proj_mlp and proj_out.  Embedders, the stacked modulation GEMV, the final proj_out and everything outside the DiT stay bf16.
    _MX_DOUBLE = ("wqkv", "cwqkv", "wo", "cwo", "w1", "cw1", "w2", "cw2")
    _MX_SINGLE = ("wqkvm", "wo")

    @property
    def linear_precision(self) -> str:
        return self._linear_precision

    @linear_precision.setter
    def linear_precision(self, value: str) -> None:
        if value not in LINEAR_PRECISIONS:
            raise ValueError(f"linear_precision must be one of {LINEAR_PRECISIONS}, not {value!r}")
        if value == "mxfp8" and not self._mx_ready:
            # the weights' MX copies, by the kernel that quantises the activations (rows are quantised one by one: stacking changes nothing)
            # (a weight none of whose launch shapes moves gets no copy)
            D, F = self.cfg.dim, self.cfg.mlp_ratio * self.cfg.dim
            self._linear_precision = value
            for blocks, keys in ((self.double, self._MX_DOUBLE), (self.single, self._MX_SINGLE)):
                for blk in blocks:
                    for k in keys:
                        N, K = blk[k].shape
                        if self._mx_moves(N, K) if k != "wqkvm" else (self._mx_moves(3 * D, D) or self._mx_moves(F, D)):
                            blk[k + "@mx"] = ops.quantize_mxfp8(blk[k])
            self._mx_ready = True
        self._linear_precision = value

    @property
    def attention_precision(self) -> str:
        return self._attention_precision

    @attention_precision.setter
    def attention_precision(self, value: str) -> None:
        if value not in ATTENTION_PRECISIONS:
            raise ValueError(f"attention_precision must be one of {ATTENTION_PRECISIONS}, not {value!r}")
        self._attention_precision = value

    @property
    def _precision_key(self) -> tuple:
        """what the launch sequence of a forward depends on besides the shapes: the graph key and the step cache hold it"""
        return (self._linear_precision, self._attention_precision)

    def _attention(self, ws, nb, S, St, wq_txt, wk_txt, wq_img, wk_img, cos, sin, out, ld_o, scale):
        """one block's attention over ws["qkv"] into ``out`` (rows of ``ld_o``).  "mxfp8": the MX prep pass (qkv stays as projected) and the
        MX kernel on the workspace's images (_SEPARATE_QPREP is a switch of the bf16 route and is ignored); a shape that kernel refuses
        by contract takes the bf16 launches, and the launch record shows them.  "bf16": k prepared in place + V^T, q on the kernel's load."""
        cfg = self.cfg
        D, H = cfg.dim, cfg.num_attention_heads
        qkv, vt = ws["qkv"], ws["vt"]
        if self._attention_precision == "mxfp8" and ops.attention_mxfp8_supported(nb, S, H):
            ops.qkv_prep_mxfp8(qkv, ws["mxa"], wq_txt, wk_txt, wq_img, wk_img, cos, sin, nb, S, H, 3 * D, St)
            ops.attention_mxfp8(ws["mxa"], out, nb, S, H, ld_o, S * ld_o, scale)
        elif _SEPARATE_QPREP:     # A/B switch: the round-1 route (q prepared by the pass, plain attention)
            ops.qk_norm_rope_vt(qkv, vt, wq_txt, wk_txt, wq_img, wk_img, cos, sin, nb, S, H, 3 * D, St)
            ops.attention(qkv, qkv.view(-1)[D:], vt, out, nb, S, H, 3 * D, S * 3 * D, ld_o, S * ld_o, scale)
        else:
            # k: RMSNorm + RoPE in place, V -> V^T; q: norm_q / norm_added_q + RoPE inside the attention kernel's Q load
            ops.k_norm_rope_vt(qkv, vt, wk_txt, wk_img, cos, sin, nb, S, H, 3 * D, St)
            ops.attention_qprep(qkv, qkv.view(-1)[D:], vt, out, nb, S, H, 3 * D, S * 3 * D, ld_o, S * ld_o, scale, wq_txt, wq_img, cos, sin, St)

    def _mx_moves(self, N: int, K: int) -> bool:
        return self._linear_precision == "mxfp8" and (N, K) not in _MX_STAYS_BF16 and K % 128 == 0 and N % 8 == 0

    @staticmethod
    def _mx_quant(ws, a, M, K, lda, rows_per_batch=0, batch_stride=0, row0=0):
        """quantise one Linear input (rows addressed as ``ops.gemm``'s ``a``) into the workspace's scratch, from dense row ``row0`` on"""
        out = (ws["mxq"][row0 * K:], ws["mxs"][row0 * (K // 32):])
        return ops.quantize_mxfp8(a, M=M, K=K, lda=lda, rows_per_batch=rows_per_batch, batch_stride=batch_stride, out=out)

    def _mx_gemm(self, ws, d, wmx, row0=0, qa=None):
        """one Linear given as ``ops.gemm`` keywords (``a``, ``out`` included) on the MX route: quantise its input unless ``qa`` has it"""
        M, K = d["M"], wmx[0].shape[1]
        if qa is None:
            qa = self._mx_quant(ws, d["a"], M, K, d.get("lda", K), d.get("a_rows_per_batch", 0), d.get("a_batch_stride", 0), row0)
        ops.gemm_mxfp8(qa[0], qa[1], wmx[0], wmx[1], d["out"], bias=d.get("bias"), act=d.get("act", ops.ACT_NONE), act_n0=d.get("act_n0", 0),
                       gate=d.get("gate"), resid=d.get("resid"), M=M, c_rows_per_batch=d.get("c_rows_per_batch", 0),
                       c_batch_stride=d.get("c_batch_stride", 0), ldc=d["ldc"], ldg=d.get("ldg", 0))

    def _pair(self, ws, blk, key1, d1, key2, d2):
        """a double block's image / text Linear pair: ``ops.gemm_pair`` in bf16, two quantise + GEMM launches each on the MX route (there
        is no MX pair form); the text rows' scratch follows the image rows'"""
        if not self._mx_moves(*blk[key1].shape):
            d1 = dict(d1, w=blk[key1]); d2 = dict(d2, w=blk[key2])
            ops.gemm_pair(d1, d2)
            return
        self._mx_gemm(ws, d1, blk[key1 + "@mx"])
        self._mx_gemm(ws, d2, blk[key2 + "@mx"], row0=d1["M"])

    # ------------------------------------------------------------------ LoRA adapters
    # Adapters are MERGED into the resident bf16 weights, in place (ops.lora_merge; the rule: lora.py): a forward with an adapter launches
    # what it launches without one, and a captured graph, which holds the weights' addresses, replays the new values.  Every change
    # re-merges each touched Linear from a pristine copy of its tensor, one launch over the concatenated ranks of all active adapters on
    # it, so the resident bits depend on the active set only, never on what was loaded before, and an unload is exact.  Adapters do not
    # change inside a denoise loop: the pipelines reset their step cache per call, so a cache never spans two adapter states.
    def _holder(self, holder):
        if holder[0] == "w":
            return self.w[holder[1]]
        if holder[0] == "mod_w":
            return self.mod_w
        return (self.double if holder[0] == "double" else self.single)[holder[1]][holder[2]]

    @property
    def loras(self) -> list:
        """the active adapters, in load order: name, scale, the ranks the file holds, the number of Linears it targets"""
        return [dict(name=n, scale=e["scale"], ranks=e["adapter"].ranks, targets=len(e["adapter"].entries)) for n, e in self._loras.items()]

    def load_lora(self, adapter_or_path, scale: float = 1.0, name: str | None = None) -> str:
        """Merge a LoRA adapter (a :class:`.lora.Adapter`, or the path of a ``.safetensors`` file in the diffusers / PEFT or the kohya
        spelling) into the resident weights at ``scale``; returns its name (``name``; None: the file's base name, else ``lora``, with ``_1``,
        ``_2``, ... appended while that name is taken).  Loading under a ``name`` that is loaded already replaces that adapter.  Not while a
        stream is capturing."""
        from . import lora
        ad = adapter_or_path if isinstance(adapter_or_path, lora.Adapter) else lora.read_adapter(os.fspath(adapter_or_path), self.cfg)
        loc = linear_locations(self.cfg)
        bad = [n for n, (down, up, _) in ad.entries.items() if n not in loc or (up.shape[0], down.shape[1]) != (loc[n][2], self._holder(loc[n][0]).shape[1])]
        if bad:
            raise ValueError(f"LoRA adapter: entries that fit no Linear of this DiT: {', '.join(sorted(bad)[:8])}")
        if name is None:
            base = os.path.splitext(os.path.basename(ad.path))[0] if ad.path else "lora"
            name, k = base, 0
            while name in self._loras:
                k += 1
                name = f"{base}_{k}"
        touched = set(ad.entries) | (set(self._loras[name]["adapter"].entries) if name in self._loras else set())
        self._lora_guard()
        self._loras.pop(name, None)
        self._loras[name] = dict(adapter=ad, scale=float(scale))
        self._lora_remerge(touched)
        return name

    def unload_lora(self, name: str | None = None) -> None:
        """take adapter ``name`` (None: every adapter) out of the weights: what it touched is merged again from the pristine copy with the
        adapters that remain, or copied back from it when none does — bit for bit the weights of a model that never saw it"""
        names = list(self._loras) if name is None else [name]
        if name is not None and name not in self._loras:
            raise KeyError(f"no LoRA adapter named {name!r} (loaded: {list(self._loras)})")
        self._lora_guard()
        touched = set()
        for n in names:
            touched |= set(self._loras.pop(n)["adapter"].entries)
        self._lora_remerge(touched)

    def set_lora_scale(self, name: str, scale: float) -> None:
        """change the scale of a loaded adapter: the same bits as loading it at ``scale`` in the first place"""
        if name not in self._loras:
            raise KeyError(f"no LoRA adapter named {name!r} (loaded: {list(self._loras)})")
        self._lora_guard()
        self._loras[name]["scale"] = float(scale)
        self._lora_remerge(set(self._loras[name]["adapter"].entries))

    @staticmethod
    def _lora_guard():
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("LoRA adapters cannot change while a stream is capturing (a graph replays weights, it does not merge them)")

    def _lora_remerge(self, linears) -> None:
        """bring the resident rows of every Linear in ``linears`` to the active set of adapters"""
        loc = linear_locations(self.cfg)
        dev = self.device
        active_holders = {loc[n][0] for e in self._loras.values() for n in e["adapter"].entries}
        changed = set()
        for n in sorted(linears):
            holder, row0, rows = loc[n]
            w = self._holder(holder)
            parts = [(e["adapter"].entries[n], e["scale"]) for e in self._loras.values() if n in e["adapter"].entries]
            if holder not in self._pristine:
                if not parts:
                    continue                                # (never touched, or restored already)
                self._pristine[holder] = w.clone()          # first touch: the tensor is still as built
            w0 = self._pristine[holder]
            changed.add(holder)
            if not parts:
                w[row0: row0 + rows].copy_(w0[row0: row0 + rows])
                continue
            R = sum(d.shape[0] for (d, _, _), _ in parts)
            up = torch.zeros((rows, (R + 7) // 8 * 8), dtype=torch.bfloat16, device=dev)[:, :R]
            down = torch.empty((R, w.shape[1]), dtype=torch.bfloat16, device=dev)
            scale = torch.empty(R, dtype=torch.float32)
            r0 = 0
            for (d, u, factor), s in parts:
                r = d.shape[0]
                up[:, r0: r0 + r].copy_(u); down[r0: r0 + r].copy_(d)
                scale[r0: r0 + r] = s * factor
                r0 += r
            ops.lora_merge(w0[row0: row0 + rows], w[row0: row0 + rows], up, down, scale.to(dev))
        for holder in changed:
            if holder[0] in ("double", "single"):
                blk = (self.double if holder[0] == "double" else self.single)[holder[1]]
                if holder[2] + "@mx" in blk:                # the MX copy follows, into the buffers it has
                    ops.quantize_mxfp8(blk[holder[2]], out=blk[holder[2] + "@mx"])
            if holder not in active_holders:
                del self._pristine[holder]                  # (rows of it that an adapter touched were copied back above)

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, B, St, Si):
        key = (B, St, Si)
        if self._ws_key == key:
            return self._ws
        cfg, dev = self.cfg, self.device
        D, S, H = cfg.dim, St + Si, cfg.num_attention_heads
        F = cfg.mlp_ratio * D
        bf = dict(dtype=torch.bfloat16, device=dev)
        s_pad = (S + 63) // 64 * 64
        ws = dict(
            x=torch.empty((B, S, D), **bf),
            nrm=torch.empty((B * S, D), **bf),
            qkv=torch.empty((B, S, 3 * D), **bf),
            vt=torch.empty((B, H, 128, s_pad), **bf),
            attn=torch.empty((B, S, D), **bf),
            cat=torch.empty((B * S, D + F), **bf),      # single: [attn | mlp]; double: MLP hidden (prefix)
            mod=torch.empty((B, self.mod_total), **bf),
            out=torch.empty((B * Si, cfg.out_channels), **bf),
        )
        self._ws_key, self._ws = key, ws
        return ws

    @staticmethod
    def _ids_key(txt_ids, img_ids):
        """identity of the position ids (order-sensitive: 4 x 6 and 6 x 4 latents have the same token count and sums)"""
        return (tuple(txt_ids.shape), tuple(img_ids.shape), hash(txt_ids.cpu().float().contiguous().numpy().tobytes()),
                hash(img_ids.cpu().float().contiguous().numpy().tobytes()))

    def _rope(self, txt_ids, img_ids):
        key = self._ids_key(txt_ids, img_ids)
        if self._rope_key != key:
            cos, sin = rope_tables(torch.cat([txt_ids.cpu().float(), img_ids.cpu().float()], dim=0), self.cfg.axes_dims_rope)
            self._rope_cs = (cos.to(self.device), sin.to(self.device))
            self._rope_key = key
        return self._rope_cs

    # ------------------------------------------------------------------ pieces
    def _set_times(self, timestep, guidance):
        """host fp32 [B] sigma / guidance scale -> persistent device buffers holding bf16(bf16(x) * 1000) as fp32
        (diffusers: ``timestep.to(hidden_states.dtype) * 1000``)."""
        B = timestep.numel()
        if getattr(self, "_t1000", None) is None or self._t1000.numel() != B:
            self._t1000 = torch.empty(B, dtype=torch.float32, device=self.device)
            self._g1000 = torch.empty(B, dtype=torch.float32, device=self.device)
        self._t1000.copy_((timestep.to(torch.bfloat16) * 1000).float())
        if guidance is not None:
            self._g1000.copy_((guidance.to(torch.bfloat16) * 1000).float())

    def _temb(self, pooled, use_guidance: bool):
        """CombinedTimestep(Guidance)TextProjEmbeddings on the times held in the device buffers (see _set_times)."""
        w = self.w
        tp = ops.timestep_embedding(self._t1000, 256)
        pre = "time_text_embed."
        h = ops.gemm(tp, w[pre + "timestep_embedder.linear_1.weight"], bias=w[pre + "timestep_embedder.linear_1.bias"], act=ops.ACT_SILU)
        emb = ops.gemm(h, w[pre + "timestep_embedder.linear_2.weight"], bias=w[pre + "timestep_embedder.linear_2.bias"])
        if use_guidance:
            gp = ops.timestep_embedding(self._g1000, 256)
            h = ops.gemm(gp, w[pre + "guidance_embedder.linear_1.weight"], bias=w[pre + "guidance_embedder.linear_1.bias"], act=ops.ACT_SILU)
            emb = ops.gemm(h, w[pre + "guidance_embedder.linear_2.weight"], bias=w[pre + "guidance_embedder.linear_2.bias"], resid=emb)
        h = ops.gemm(pooled, w[pre + "text_embedder.linear_1.weight"], bias=w[pre + "text_embedder.linear_1.bias"], act=ops.ACT_SILU)
        return ops.gemm(h, w[pre + "text_embedder.linear_2.weight"], bias=w[pre + "text_embedder.linear_2.bias"], resid=emb)

    # ------------------------------------------------------------------ blocks
    # Every workspace buffer is batch-leading or flat scratch, so its first ``nb`` slots are the workspace of a batch-``nb`` forward: the
    # blocks take the batch size they run at (B, or under a step cache of scope "image" the number of computing images).
    def _double_block(self, ws, i, nb, St, Si, cos, sin, taps):
        cfg = self.cfg
        D, H, S, LM = cfg.dim, cfg.num_attention_heads, St + Si, self.mod_total
        F = cfg.mlp_ratio * D
        Mi, Mt = nb * Si, nb * St
        x, nrm, qkv, vt, attn, modv = ws["x"], ws["nrm"], ws["qkv"], ws["vt"], ws["attn"], ws["mod"].view(-1)
        x_img = x.view(-1)[St * D:]          # joint buffer, image rows of batch 0 onwards
        nrm_img = nrm.view(-1)[: Mi * D]
        nrm_txt = nrm.view(-1)[Mi * D: (Mi + Mt) * D]
        qkv_img = qkv.view(-1)[St * 3 * D:]
        attn_img = attn.view(-1)[St * D:]
        hid = ws["cat"].view(-1)              # MLP hidden scratch for double blocks: image rows, then text rows
        hid_txt = hid[Mi * F:]
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        blk = self.double[i]
        mo, cmo = self.mod_off[(i, "norm1")], self.mod_off[(i, "norm1_context")]
        # chunk order: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        ops.layernorm(x_img, nrm_img, Mi, D, scale=modv[mo + D:], shift=modv[mo:], ldx=D, rows_per_batch=Si,
                      x_batch_stride=S * D, ld_mod=LM)
        ops.layernorm(x, nrm_txt, Mt, D, scale=modv[cmo + D:], shift=modv[cmo:], ldx=D, rows_per_batch=St,
                      x_batch_stride=S * D, ld_mod=LM)
        # the image-stream and text-stream Linears of a pair share N and K: one launch when they are small alone (ops.gemm_pair)
        self._pair(ws, blk, "wqkv", dict(a=nrm_img, out=qkv_img, bias=blk["bqkv"], M=Mi, lda=D, c_rows_per_batch=Si,
                                         c_batch_stride=S * 3 * D, ldc=3 * D),
                   "cwqkv", dict(a=nrm_txt, out=qkv, bias=blk["cbqkv"], M=Mt, lda=D, c_rows_per_batch=St,
                                 c_batch_stride=S * 3 * D, ldc=3 * D))
        self._attention(ws, nb, S, St, blk["cnq"], blk["cnk"], blk["nq"], blk["nk"], cos, sin, attn, D, scale)
        self._pair(ws, blk, "wo", dict(a=attn_img, out=x_img, bias=blk["bo"], M=Mi, a_rows_per_batch=Si, a_batch_stride=S * D,
                                       lda=D, c_rows_per_batch=Si, c_batch_stride=S * D, ldc=D, gate=modv[mo + 2 * D:], resid=x_img, ldg=LM),
                   "cwo", dict(a=attn, out=x, bias=blk["cbo"], M=Mt, a_rows_per_batch=St, a_batch_stride=S * D,
                               lda=D, c_rows_per_batch=St, c_batch_stride=S * D, ldc=D, gate=modv[cmo + 2 * D:], resid=x, ldg=LM))
        # MLPs (the two streams are independent: both LayerNorms, both up-projections, both down-projections)
        ops.layernorm(x_img, nrm_img, Mi, D, scale=modv[mo + 4 * D:], shift=modv[mo + 3 * D:], ldx=D,
                      rows_per_batch=Si, x_batch_stride=S * D, ld_mod=LM)
        ops.layernorm(x, nrm_txt, Mt, D, scale=modv[cmo + 4 * D:], shift=modv[cmo + 3 * D:], ldx=D,
                      rows_per_batch=St, x_batch_stride=S * D, ld_mod=LM)
        self._pair(ws, blk, "w1", dict(a=nrm_img, out=hid, bias=blk["b1"], act=ops.ACT_GELU_TANH, M=Mi, lda=D, ldc=F),
                   "cw1", dict(a=nrm_txt, out=hid_txt, bias=blk["cb1"], act=ops.ACT_GELU_TANH, M=Mt, lda=D, ldc=F))
        self._pair(ws, blk, "w2", dict(a=hid, out=x_img, bias=blk["b2"], M=Mi, lda=F, c_rows_per_batch=Si,
                                       c_batch_stride=S * D, ldc=D, gate=modv[mo + 5 * D:], resid=x_img, ldg=LM),
                   "cw2", dict(a=hid_txt, out=x, bias=blk["cb2"], M=Mt, lda=F, c_rows_per_batch=St,
                               c_batch_stride=S * D, ldc=D, gate=modv[cmo + 5 * D:], resid=x, ldg=LM))
        if taps is not None:
            taps[f"double.{i}"] = x[:nb].clone()

    def _blocks_after_first(self, ws, nb, St, Si, cos, sin, taps):
        """double blocks 1... and the single blocks on the first ``nb`` slots of the workspace"""
        cfg = self.cfg
        D, H, S, LM = cfg.dim, cfg.num_attention_heads, St + Si, self.mod_total
        F = cfg.mlp_ratio * D
        M = nb * S
        x, nrm, qkv, vt, catb, modv = ws["x"], ws["nrm"], ws["qkv"], ws["vt"], ws["cat"], ws["mod"].view(-1)
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        for i in range(1, len(self.double)):
            self._double_block(ws, i, nb, St, Si, cos, sin, taps)

        cat_mlp = catb.view(-1)[D:]
        fused_qkv_mlp = (3 * D) % 256 == 0 and (_FUSED_QKV_MLP if _FUSED_QKV_MLP is not None else
                                                ops.gemm_cost(M, 3 * D + F, D) * 10 <= (ops.gemm_cost(M, 3 * D, D) + ops.gemm_cost(M, F, D)) * 9)
        mx_qkv, mx_mlp, mx_out = self._mx_moves(3 * D, D), self._mx_moves(F, D), self._mx_moves(D, D + F)
        for i, blk in enumerate(self.single):
            mo = self.mod_off[("s", i)]      # shift, scale, gate
            ops.layernorm(x, nrm, M, D, scale=modv[mo + D:], shift=modv[mo:], ldx=D, ld_mod=LM, rows_per_batch=S,
                          x_batch_stride=S * D)
            if mx_qkv or mx_mlp:
                # one quantisation of the modulated LayerNorm output serves q|k|v and proj_mlp: two launches over the stacked weight's row
                # ranges (a range whose shape stays on bf16 takes the bf16 GEMM)
                qa = self._mx_quant(ws, nrm, M, D, D)
                wq, wsc = blk["wqkvm@mx"]
                for moves, lo, hi, dst, ldd, act_ in ((mx_qkv, 0, 3 * D, qkv, 3 * D, ops.ACT_NONE), (mx_mlp, 3 * D, 3 * D + F, cat_mlp, D + F, ops.ACT_GELU_TANH)):
                    if moves:
                        ops.gemm_mxfp8(qa[0], qa[1], wq[lo:hi], wsc[lo:hi], dst, bias=blk["bqkvm"][lo:hi], act=act_, M=M, ldc=ldd)
                    else:
                        ops.gemm(nrm, blk["wqkvm"][lo:hi], out=dst, bias=blk["bqkvm"][lo:hi], act=act_, M=M, lda=D, ldc=ldd)
            elif fused_qkv_mlp:
                ops.gemm(nrm, blk["wqkvm"], out=qkv, bias=blk["bqkvm"], act=ops.ACT_GELU_TANH, act_n0=3 * D, M=M, lda=D, ldc=3 * D,
                         out2=cat_mlp, ldc2=D + F, n_split=3 * D)
            else:       # (test-sized widths whose q|k|v block does not end on a tile boundary)
                ops.gemm(nrm, blk["wqkvm"][: 3 * D], out=qkv, bias=blk["bqkvm"][: 3 * D], M=M, lda=D, ldc=3 * D)
                ops.gemm(nrm, blk["wqkvm"][3 * D:], out=cat_mlp, bias=blk["bqkvm"][3 * D:], act=ops.ACT_GELU_TANH, M=M, lda=D, ldc=D + F)
            self._attention(ws, nb, S, 0, blk["nq"], blk["nk"], blk["nq"], blk["nk"], cos, sin, catb, D + F, scale)
            proj = dict(a=catb, out=x, bias=blk["bo"], M=M, lda=D + F, c_rows_per_batch=S, c_batch_stride=S * D,
                        ldc=D, gate=modv[mo + 2 * D:], resid=x, ldg=LM)
            if mx_out:
                self._mx_gemm(ws, proj, blk["wo@mx"])
            else:
                ops.gemm(proj.pop("a"), blk["wo"], **proj)
            if taps is not None:
                taps[f"single.{i}"] = x[:nb].clone()

    def forward(self, hidden, enc, pooled, timestep, img_ids, txt_ids, guidance=None, taps: dict | None = None,
                cache: StepCache | None = None):
        """hidden bf16 [B, S_img, in]; enc bf16 [B, S_txt, J]; pooled bf16 [B, P]; timestep / guidance
        fp32 [B] host or device; returns bf16 [B, S_img, out] (a view of an internal workspace).
        ``cache``: a :class:`StepCache` (opt-in; None is the plain forward, the same launches in the same order): after the first double block the
        step (scope "image": each image) reuses the cached residual of the remaining blocks (order 1: its first-order forecast along ``timestep``),
        or computes them and refreshes the cache."""
        cfg = self.cfg
        if cache is not None and (cfg.num_layers < 1 or cfg.num_layers + cfg.num_single_layers < 2):
            raise ValueError("a step cache needs a double block and at least one further block")
        D = cfg.dim
        F = cfg.mlp_ratio * D
        B, Si, _ = hidden.shape
        St = enc.shape[1]
        S = St + Si
        ws = self._workspace(B, St, Si)
        x, nrm, mod = ws["x"], ws["nrm"], ws["mod"]
        if "mxq" not in ws and any(self._mx_moves(n, k) for n, k in ((3 * D, D), (D, D), (F, D), (D, F), (D, D + F))):
            # the widest Linear input (the single blocks' [attn | mlp], D + F columns) as e4m3 bytes + its e8m0 scales
            ws["mxq"] = torch.empty(B * S * (D + F), dtype=torch.uint8, device=self.device)
            ws["mxs"] = torch.empty(B * S * (D + F) // 32, dtype=torch.uint8, device=self.device)
        if "mxa" not in ws and self._attention_precision == "mxfp8":
            ws["mxa"] = ops.attention_mxfp8_images(B, S, cfg.num_attention_heads, self.device)      # the six MXFP8 attention images
        cos, sin = self._rope(txt_ids, img_ids)
        hidden = hidden.contiguous(); enc = enc.contiguous(); pooled = pooled.contiguous()
        Mi, Mt = B * Si, B * St
        x_img = x.view(-1)[St * D:]          # joint buffer, image rows of batch 0 onwards

        # embedders write straight into the joint buffer
        ops.gemm(hidden.view(Mi, -1), self.w["x_embedder.weight"], out=x_img, bias=self.w["x_embedder.bias"], M=Mi,
                 c_rows_per_batch=Si, c_batch_stride=S * D, ldc=D)
        ops.gemm(enc.view(Mt, -1), self.w["context_embedder.weight"], out=x, bias=self.w["context_embedder.bias"], M=Mt,
                 c_rows_per_batch=St, c_batch_stride=S * D, ldc=D)
        if cfg.guidance_embeds and guidance is None:
            raise ValueError("this model has a guidance embedding: pass guidance")
        times = None                  # the host timesteps, for a step cache of order 1
        if timestep is not None:      # eager call: refresh the device-side times (a replayed graph gets them from forward_graphed)
            t_host = torch.as_tensor(timestep, dtype=torch.float32).cpu().reshape(-1)
            self._set_times(t_host, None if guidance is None else torch.as_tensor(guidance, dtype=torch.float32).cpu().reshape(-1))
            if cache is not None:
                times = t_host.tolist()
        temb = self._temb(pooled, cfg.guidance_embeds)
        st = ops.act(temb, ops.ACT_SILU)
        ops.gemm(st, self.mod_w, out=mod, bias=self.mod_b)          # every block's modulation in one GEMM
        modv = mod.view(-1)
        LM = self.mod_total
        if taps is not None:
            taps["temb"] = temb.clone()
            taps["x_embed"] = x[:, St:].clone(); taps["ctx_embed"] = x[:, :St].clone()

        nrm_img = nrm.view(-1)[: Mi * D]
        nb = B      # the batch size blocks 1... run at: under a step cache 0 on a reused step, the number of computing images on a mixed one
        if self.double:
            if cache is not None:
                cache.before_first_block(x, B, St, Si, D, self._precision_key, self.device)
            self._double_block(ws, 0, B, St, Si, cos, sin, taps)
            if cache is not None:
                nb = cache.after_first_block(x, mod, B, St, Si, D, taps, times=times)
        if nb:
            self._blocks_after_first(ws, nb, St, Si, cos, sin, taps)
        if cache is not None:
            cache.after_last_block(x, mod, B, St, Si, D)
        mo = self.mod_off["out"]             # AdaLayerNormContinuous: scale, shift
        ops.layernorm(x_img, nrm_img, Mi, D, scale=modv[mo:], shift=modv[mo + D:], ldx=D, rows_per_batch=Si,
                      x_batch_stride=S * D, ld_mod=LM)
        ops.gemm(nrm_img, self.w["proj_out.weight"], out=ws["out"], bias=self.w["proj_out.bias"], M=Mi, lda=D,
                 ldc=cfg.out_channels)
        return ws["out"].view(B, Si, cfg.out_channels)

    # ------------------------------------------------------------------ hipGraph replay
    MAX_GRAPHS = 3          # captured forwards kept alive (each owns a workspace: ~1 GB per image at 1024^2)

    def forward_graphed(self, hidden, enc, pooled, timestep, img_ids, txt_ids, guidance=None, cache: StepCache | None = None):
        """Same result as ``forward`` (bit-identical: same kernels, same order), but the ~800 launches of one forward
        are captured ONCE into a hipGraph and replayed; only the timestep / guidance values change between replays and
        travel through device buffers updated before the launch.  The GPU was never launch-bound (host enqueue 4.8 ms
        vs 83.7 ms of GPU time at B = 1): the replay (0.2 ms) frees the host thread for image I/O.
        A captured graph bakes in the addresses of everything the forward touched, so a cache entry OWNS its workspace,
        RoPE tables and time buffers (they must not be freed or reused while the graph lives), is keyed on the input
        addresses, the shapes AND the RoPE table identity (the same token count can be a different h x w), and the
        cache is a small LRU (image sizes vary from sample to sample in stage 3).  The Linear and the attention precision are part of the key: each
        combination is a different launch sequence.  A step cache cannot be replayed: its decision needs the host between two pieces of the forward."""
        if cache is not None:
            raise ValueError("forward_graphed takes no step cache (the decision needs the host): call forward(..., cache=...)")
        t = torch.as_tensor(timestep, dtype=torch.float32).cpu().reshape(-1)
        g = None if guidance is None else torch.as_tensor(guidance, dtype=torch.float32).cpu().reshape(-1)
        rope_key = self._ids_key(txt_ids, img_ids)
        key = (hidden.data_ptr(), enc.data_ptr(), pooled.data_ptr(), tuple(hidden.shape), tuple(enc.shape), tuple(pooled.shape),
               guidance is None, rope_key) + self._precision_key
        graphs = self.__dict__.setdefault("_graphs", {})
        ent = graphs.pop(key, None)
        if ent is None:
            while len(graphs) >= self.MAX_GRAPHS:
                graphs.pop(next(iter(graphs)))                 # least recently used: drops its graph, workspace and tables
            # private buffers for this capture: nothing the eager path (or another graph) will ever reallocate
            self._ws_key = self._rope_key = None
            self._t1000 = self._g1000 = None
            self._set_times(t, g)
            rope = self._rope(txt_ids, img_ids)              # host-side table build + upload happen outside capture
            ws = self._workspace(hidden.shape[0], enc.shape[1], hidden.shape[1])
            self.forward(hidden, enc, pooled, None, img_ids, txt_ids, g)   # warm-up: allocates every temporary
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self.forward(hidden, enc, pooled, None, img_ids, txt_ids, g)
            ent = dict(graph=graph, out=out, ws=ws, rope=rope, times=(self._t1000, self._g1000))
            # hand the buffers over: the next eager forward / capture allocates its own
            self._ws_key = self._rope_key = None
            self._t1000 = self._g1000 = None
        graphs[key] = ent                                     # (re)insert as most recently used
        t1000, g1000 = ent["times"]
        t1000.copy_((t.to(torch.bfloat16) * 1000).float())
        if g is not None:
            g1000.copy_((g.to(torch.bfloat16) * 1000).float())
        ent["graph"].replay()
        return ent["out"]

    __call__ = forward
