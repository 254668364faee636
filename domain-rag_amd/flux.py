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

from . import flux_layout, ops
from .flux_layout import linear_locations      # noqa: F401
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


class _Buffers:
    """what a forward's launches address besides weights and inputs: the workspace and the RoPE tables with the keys they were made for,
    and the two time buffers.  The model has one for the eager path; a captured graph, which bakes the addresses in, owns its own."""
    def __init__(self):
        self.ws_key = self.ws = self.rope_key = self.rope = self.t1000 = self.g1000 = None

    def set_times(self, timestep, guidance, device) -> None:
        """host fp32 [B] sigma / guidance scale -> persistent device buffers holding bf16(bf16(x) * 1000) as fp32
        (diffusers: ``timestep.to(hidden_states.dtype) * 1000``)."""
        B = timestep.numel()
        if self.t1000 is None or self.t1000.numel() != B:
            self.t1000 = torch.empty(B, dtype=torch.float32, device=device)
            self.g1000 = torch.empty(B, dtype=torch.float32, device=device)
        self.t1000.copy_((timestep.to(torch.bfloat16) * 1000).float())
        if guidance is not None:
            self.g1000.copy_((guidance.to(torch.bfloat16) * 1000).float())


class _Rows:
    """one row set of the joint buffers: ``per`` rows of every image from row ``first`` of its S on.  ``M`` rows in all; ``x`` / ``qkv`` /
    ``attn``: the workspace buffers from the set's first row on; the set's row map in the spellings ``ops.layernorm`` (``ln``: reading x)
    and ``ops.gemm`` take (``a_attn``: reading attn; ``c_x`` / ``c_qkv``: writing x / qkv)"""
    def __init__(self, ws, nb, first, per, S, D):
        self.M = nb * per
        self.x, self.qkv, self.attn = (ws[k].view(-1)[first * ld:] if first else ws[k] for k, ld in (("x", D), ("qkv", 3 * D), ("attn", D)))
        self.ln = dict(ldx=D, rows_per_batch=per, x_batch_stride=S * D)
        self.a_attn = dict(a_rows_per_batch=per, a_batch_stride=S * D, lda=D)
        self.c_x = dict(c_rows_per_batch=per, c_batch_stride=S * D, ldc=D)
        self.c_qkv = dict(c_rows_per_batch=per, c_batch_stride=S * 3 * D, ldc=3 * D)


class _Joint:
    """the joint [nb, St + Si, .] activation buffers of a forward at batch ``nb`` (text rows first): the three row sets the launches address
    (``img``, ``txt``, ``all``) and the dense scratch of the double blocks, image rows then text rows: the LayerNorm outputs ``nrm_img`` /
    ``nrm_txt`` and the MLP hidden ``hid`` / ``hid_txt``.  Every row-map keyword of the forward comes from here."""
    def __init__(self, ws, nb, St, Si, D, F):
        self.nb, self.St, self.S = nb, St, St + Si
        self.img, self.txt, self.all = _Rows(ws, nb, St, Si, self.S, D), _Rows(ws, nb, 0, St, self.S, D), _Rows(ws, nb, 0, self.S, self.S, D)
        Mi, Mt = self.img.M, self.txt.M
        nrm, self.hid = ws["nrm"].view(-1), ws["cat"].view(-1)
        self.nrm_img, self.nrm_txt, self.hid_txt = nrm[: Mi * D], nrm[Mi * D: (Mi + Mt) * D], self.hid[Mi * F:]


class FluxTransformerHIP:
    def __init__(self, cfg: FluxConfig, params: dict, device="cuda", linear_precision: str | None = None,
                 attention_precision: str | None = None):
        """``linear_precision``: "bf16" | "mxfp8" (None: $DRAG_LINEAR_PRECISION, else "bf16") — also a settable attribute; the bf16
        weights are kept in either mode, so one process can A/B.  ``attention_precision``: the same for the blocks' attention (None:
        $DRAG_ATTENTION_PRECISION, else "bf16"), also settable; the two modes are independent"""
        if cfg.attention_head_dim != 128:
            raise ValueError("the HIP attention kernel is specialised for head_dim 128 (all FLUX.1 models)")
        self.cfg = cfg
        self.device = dev = torch.device(device)

        def g(name):
            return params[name].to(dev, torch.bfloat16).contiguous()

        def stack(names, suffix):      # (one member: the parameter itself when it is on the device in bf16 already, no copy)
            return g(names[0] + suffix) if len(names) == 1 else torch.cat([params[n + suffix].to(dev, torch.bfloat16) for n in names], dim=0).contiguous()

        # ---- the resident tensors, by flux_layout's tables
        self.w = {n + sfx: g(n + sfx) for n in flux_layout.top_linears(cfg) for sfx in (".weight", ".bias")}
        mod = flux_layout.modulation(cfg)
        self.mod_w, self.mod_b = stack([n for _, n in mod], ".weight"), stack([n for _, n in mod], ".bias")
        self.mod_off, self.mod_total = {}, 0
        for key, n in mod:
            self.mod_off[key] = self.mod_total
            self.mod_total += params[n + ".weight"].shape[0]
        for kind, prefix, count, linears, norms in flux_layout.BLOCKS:
            blocks = []
            for i in range(getattr(cfg, count)):
                p = f"{prefix}.{i}."
                blk = {key: g(p + n + ".weight") for key, n in norms.items()}
                for key, (bias_key, members) in linears.items():
                    blk[key], blk[bias_key] = stack([p + m for m in members], ".weight"), stack([p + m for m in members], ".bias")
                blocks.append(blk)
            setattr(self, kind, blocks)                      # self.double, self.single
        # the two launch ranges of a single block's wqkvm, q|k|v and proj_mlp: it splits where proj_mlp begins
        _, lo, rows = linear_locations(cfg).get("single_transformer_blocks.0.proj_mlp.weight", (None, 0, 0))
        self._qkvm_rows = ((0, lo), (lo, lo + rows))
        self._buf = _Buffers()           # the eager path's; a captured graph owns its own (forward_graphed)
        self._graphs: dict = {}
        self._mx_ready = False
        self._loras: dict = {}           # name -> {"adapter", "scale"}: the active LoRA adapters, in load order
        self._pristine: dict = {}        # holder -> a copy of the resident tensor as built, while an adapter touches it
        self.linear_precision = linear_precision or _LINEAR_PRECISION
        self.attention_precision = attention_precision or _ATTENTION_PRECISION

    # ------------------------------------------------------------------ MXFP8 mode
    # What moves (blocks only): both streams' to_q|k|v, the attention out-projections, ff up (+GELU) and ff down, the single blocks'
    # q|k|v + proj_mlp and proj_out.  Embedders, the stacked modulation GEMV, the final proj_out and everything outside the DiT stay bf16.
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
            self._linear_precision = value
            for kind, _, _, linears, _ in flux_layout.BLOCKS:
                for blk in getattr(self, kind):
                    for k in linears:
                        N, K = blk[k].shape
                        if any(self._mx_moves(hi - lo, K) for lo, hi in (self._qkvm_rows if k == "wqkvm" else ((0, N),))):
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
        D, H = self.cfg.dim, self.cfg.num_attention_heads
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

    def _has_mx(self, blk, key) -> bool:
        """does a launch shape of this weight run on the MX route (decided at set-up: it has a copy)?"""
        return self._linear_precision == "mxfp8" and key + "@mx" in blk

    def _linear(self, ws, blk, key, kw, rows=None, qa=None, row0=0):
        """THE route of a block Linear: ``kw`` are its ``ops.gemm`` keywords (``a``, ``out`` included; ``bias`` the whole bias of ``blk[key]``),
        ``rows`` a row range (lo, hi) of a stacked weight.  bf16: that GEMM.  A shape that moves in "mxfp8" mode: quantise ``a`` into the
        workspace's scratch from dense row ``row0`` on (unless ``qa`` holds it already) + the MX GEMM with the same epilogue keywords."""
        kw, w = dict(kw), blk[key]
        lo, hi = rows or (0, w.shape[0])
        a, K = kw.pop("a"), w.shape[1]
        if rows:
            kw["bias"] = kw["bias"][lo:hi]
        if not self._mx_moves(hi - lo, K):
            return ops.gemm(a, w[lo:hi] if rows else w, **kw)
        lda, per, stride = kw.pop("lda", K), kw.pop("a_rows_per_batch", 0), kw.pop("a_batch_stride", 0)
        qa = qa or self._mx_quant(ws, a, kw["M"], K, lda, per, stride, row0)
        wq, wscale = blk[key + "@mx"]
        return ops.gemm_mxfp8(qa[0], qa[1], wq[lo:hi] if rows else wq, wscale[lo:hi] if rows else wscale, kw.pop("out"), **kw)

    def _pair(self, ws, blk, key1, d1, key2, d2):
        """a double block's image / text Linear pair (same N and K): ``ops.gemm_pair`` in bf16, two calls of the route where the shape moves
        (there is no MX pair form); the text rows' scratch follows the image rows'"""
        if self._has_mx(blk, key1):
            self._linear(ws, blk, key1, d1)
            self._linear(ws, blk, key2, d2, row0=d1["M"])
        else:
            ops.gemm_pair(dict(d1, w=blk[key1]), dict(d2, w=blk[key2]))

    # ------------------------------------------------------------------ LoRA adapters
    # Adapters are MERGED into the resident bf16 weights, in place (ops.lora_merge; the rule: lora.py): a forward with an adapter launches
    # what it launches without one, and a captured graph, which holds the weights' addresses, replays the new values.  Every change
    # re-merges each touched Linear from a pristine copy of its tensor, one launch over the concatenated ranks of all active adapters on
    # it, so the resident bits depend on the active set only, never on what was loaded before, and an unload is exact.  Adapters do not
    # change inside a denoise loop: the pipelines reset their step cache per call, so a cache never spans two adapter states.
    def _holder(self, holder):
        if holder[0] == "w":
            return self.w[holder[1]]
        return self.mod_w if holder[0] == "mod_w" else getattr(self, holder[0])[holder[1]][holder[2]]

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
                blk = getattr(self, holder[0])[holder[1]]
                if holder[2] + "@mx" in blk:                # the MX copy follows, into the buffers it has
                    ops.quantize_mxfp8(blk[holder[2]], out=blk[holder[2] + "@mx"])
            if holder not in active_holders:
                del self._pristine[holder]                  # (rows of it that an adapter touched were copied back above)

    # ------------------------------------------------------------------ workspaces
    def _workspace(self, B, St, Si):
        key = (B, St, Si)
        if self._buf.ws_key == key:
            return self._buf.ws
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
        self._buf.ws_key, self._buf.ws = key, ws
        return ws

    @staticmethod
    def _ids_key(txt_ids, img_ids):
        """identity of the position ids (order-sensitive: 4 x 6 and 6 x 4 latents have the same token count and sums)"""
        return (tuple(txt_ids.shape), tuple(img_ids.shape), hash(txt_ids.cpu().float().contiguous().numpy().tobytes()),
                hash(img_ids.cpu().float().contiguous().numpy().tobytes()))

    def _rope(self, txt_ids, img_ids):
        key, buf = self._ids_key(txt_ids, img_ids), self._buf
        if buf.rope_key != key:
            cos, sin = rope_tables(torch.cat([txt_ids.cpu().float(), img_ids.cpu().float()], dim=0), self.cfg.axes_dims_rope)
            buf.rope_key, buf.rope = key, (cos.to(self.device), sin.to(self.device))
        return buf.rope

    # ------------------------------------------------------------------ pieces
    def _temb(self, pooled, use_guidance: bool):
        """CombinedTimestep(Guidance)TextProjEmbeddings on the times held in the device buffers (_Buffers.set_times)."""
        w = self.w
        tp = ops.timestep_embedding(self._buf.t1000, 256)
        pre = "time_text_embed."
        h = ops.gemm(tp, w[pre + "timestep_embedder.linear_1.weight"], bias=w[pre + "timestep_embedder.linear_1.bias"], act=ops.ACT_SILU)
        emb = ops.gemm(h, w[pre + "timestep_embedder.linear_2.weight"], bias=w[pre + "timestep_embedder.linear_2.bias"])
        if use_guidance:
            gp = ops.timestep_embedding(self._buf.g1000, 256)
            h = ops.gemm(gp, w[pre + "guidance_embedder.linear_1.weight"], bias=w[pre + "guidance_embedder.linear_1.bias"], act=ops.ACT_SILU)
            emb = ops.gemm(h, w[pre + "guidance_embedder.linear_2.weight"], bias=w[pre + "guidance_embedder.linear_2.bias"], resid=emb)
        h = ops.gemm(pooled, w[pre + "text_embedder.linear_1.weight"], bias=w[pre + "text_embedder.linear_1.bias"], act=ops.ACT_SILU)
        return ops.gemm(h, w[pre + "text_embedder.linear_2.weight"], bias=w[pre + "text_embedder.linear_2.bias"], resid=emb)

    # ------------------------------------------------------------------ blocks
    # Every workspace buffer is batch-leading or flat scratch, so its first ``nb`` slots are the workspace of a batch-``nb`` forward: the
    # blocks take the batch size they run at (B, or under a step cache of scope "image" the number of computing images).
    def _double_block(self, ws, i, j, cos, sin, taps):
        cfg = self.cfg
        D, LM = cfg.dim, self.mod_total
        F = cfg.mlp_ratio * D
        img, txt, modv = j.img, j.txt, ws["mod"].view(-1)
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        blk = self.double[i]
        mo, cmo = self.mod_off[(i, "norm1")], self.mod_off[(i, "norm1_context")]
        # chunk order: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
        ops.layernorm(img.x, j.nrm_img, img.M, D, scale=modv[mo + D:], shift=modv[mo:], ld_mod=LM, **img.ln)
        ops.layernorm(txt.x, j.nrm_txt, txt.M, D, scale=modv[cmo + D:], shift=modv[cmo:], ld_mod=LM, **txt.ln)
        # the image-stream and text-stream Linears of a pair share N and K: one launch when they are small alone (ops.gemm_pair)
        self._pair(ws, blk, "wqkv", dict(a=j.nrm_img, out=img.qkv, bias=blk["bqkv"], M=img.M, lda=D, **img.c_qkv),
                   "cwqkv", dict(a=j.nrm_txt, out=txt.qkv, bias=blk["cbqkv"], M=txt.M, lda=D, **txt.c_qkv))
        self._attention(ws, j.nb, j.S, j.St, blk["cnq"], blk["cnk"], blk["nq"], blk["nk"], cos, sin, ws["attn"], D, scale)
        self._pair(ws, blk, "wo", dict(a=img.attn, out=img.x, bias=blk["bo"], M=img.M, gate=modv[mo + 2 * D:], resid=img.x, ldg=LM, **img.a_attn, **img.c_x),
                   "cwo", dict(a=txt.attn, out=txt.x, bias=blk["cbo"], M=txt.M, gate=modv[cmo + 2 * D:], resid=txt.x, ldg=LM, **txt.a_attn, **txt.c_x))
        # MLPs (the two streams are independent: both LayerNorms, both up-projections, both down-projections)
        ops.layernorm(img.x, j.nrm_img, img.M, D, scale=modv[mo + 4 * D:], shift=modv[mo + 3 * D:], ld_mod=LM, **img.ln)
        ops.layernorm(txt.x, j.nrm_txt, txt.M, D, scale=modv[cmo + 4 * D:], shift=modv[cmo + 3 * D:], ld_mod=LM, **txt.ln)
        self._pair(ws, blk, "w1", dict(a=j.nrm_img, out=j.hid, bias=blk["b1"], act=ops.ACT_GELU_TANH, M=img.M, lda=D, ldc=F),
                   "cw1", dict(a=j.nrm_txt, out=j.hid_txt, bias=blk["cb1"], act=ops.ACT_GELU_TANH, M=txt.M, lda=D, ldc=F))
        self._pair(ws, blk, "w2", dict(a=j.hid, out=img.x, bias=blk["b2"], M=img.M, lda=F, gate=modv[mo + 5 * D:], resid=img.x, ldg=LM, **img.c_x),
                   "cw2", dict(a=j.hid_txt, out=txt.x, bias=blk["cb2"], M=txt.M, lda=F, gate=modv[cmo + 5 * D:], resid=txt.x, ldg=LM, **txt.c_x))
        if taps is not None:
            taps[f"double.{i}"] = ws["x"][:j.nb].clone()

    def _blocks_after_first(self, ws, j, cos, sin, taps):
        """double blocks 1... and the single blocks on the first ``j.nb`` slots of the workspace"""
        cfg = self.cfg
        D, LM, M = cfg.dim, self.mod_total, j.all.M
        F = cfg.mlp_ratio * D
        x, nrm, qkv, catb, modv = ws["x"], ws["nrm"], ws["qkv"], ws["cat"], ws["mod"].view(-1)
        scale = 1.0 / math.sqrt(cfg.attention_head_dim)
        for i in range(1, len(self.double)):
            self._double_block(ws, i, j, cos, sin, taps)

        cat_mlp = catb.view(-1)[D:]
        fused_qkv_mlp = (3 * D) % 256 == 0 and (_FUSED_QKV_MLP if _FUSED_QKV_MLP is not None else
                                                ops.gemm_cost(M, 3 * D + F, D) * 10 <= (ops.gemm_cost(M, 3 * D, D) + ops.gemm_cost(M, F, D)) * 9)
        for i, blk in enumerate(self.single):
            mo = self.mod_off[("s", i)]      # shift, scale, gate
            ops.layernorm(x, nrm, M, D, scale=modv[mo + D:], shift=modv[mo:], ld_mod=LM, **j.all.ln)
            lin = dict(a=nrm, bias=blk["bqkvm"], M=M, lda=D)
            mx = self._has_mx(blk, "wqkvm")
            if fused_qkv_mlp and not mx:
                ops.gemm(w=blk["wqkvm"], out=qkv, ldc=3 * D, act=ops.ACT_GELU_TANH, act_n0=3 * D, out2=cat_mlp, ldc2=D + F, n_split=3 * D, **lin)
            else:
                # two launches over the stacked weight's row ranges (test-sized widths whose q|k|v block does not end on a tile boundary; "mxfp8":
                # ONE quantisation of the modulated LayerNorm output serves both, and a range whose shape stays on bf16 takes the bf16 GEMM)
                qa = self._mx_quant(ws, nrm, M, D, D) if mx else None
                self._linear(ws, blk, "wqkvm", dict(lin, out=qkv, ldc=3 * D), self._qkvm_rows[0], qa)
                self._linear(ws, blk, "wqkvm", dict(lin, out=cat_mlp, act=ops.ACT_GELU_TANH, ldc=D + F), self._qkvm_rows[1], qa)
            self._attention(ws, j.nb, j.S, 0, blk["nq"], blk["nk"], blk["nq"], blk["nk"], cos, sin, catb, D + F, scale)
            self._linear(ws, blk, "wo", dict(a=catb, out=x, bias=blk["bo"], M=M, lda=D + F, gate=modv[mo + 2 * D:], resid=x, ldg=LM, **j.all.c_x))
            if taps is not None:
                taps[f"single.{i}"] = x[:j.nb].clone()

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
        x, mod = ws["x"], ws["mod"]
        if "mxq" not in ws and self._linear_precision == "mxfp8" and any(k.endswith("@mx") for blk in self.double + self.single for k in blk):
            # the widest Linear input (the single blocks' [attn | mlp], D + F columns) as e4m3 bytes + its e8m0 scales
            ws["mxq"] = torch.empty(B * S * (D + F), dtype=torch.uint8, device=self.device)
            ws["mxs"] = torch.empty(B * S * (D + F) // 32, dtype=torch.uint8, device=self.device)
        if "mxa" not in ws and self._attention_precision == "mxfp8":
            ws["mxa"] = ops.attention_mxfp8_images(B, S, cfg.num_attention_heads, self.device)      # the six MXFP8 attention images
        cos, sin = self._rope(txt_ids, img_ids)
        hidden = hidden.contiguous(); enc = enc.contiguous(); pooled = pooled.contiguous()
        j = _Joint(ws, B, St, Si, D, F)
        img, txt = j.img, j.txt

        # embedders write straight into the joint buffer
        ops.gemm(hidden.view(img.M, -1), self.w["x_embedder.weight"], out=img.x, bias=self.w["x_embedder.bias"], M=img.M, **img.c_x)
        ops.gemm(enc.view(txt.M, -1), self.w["context_embedder.weight"], out=txt.x, bias=self.w["context_embedder.bias"], M=txt.M, **txt.c_x)
        if cfg.guidance_embeds and guidance is None:
            raise ValueError("this model has a guidance embedding: pass guidance")
        times = None                  # the host timesteps, for a step cache of order 1
        if timestep is not None:      # eager call: refresh the device-side times (a replayed graph gets them from forward_graphed)
            t_host = torch.as_tensor(timestep, dtype=torch.float32).cpu().reshape(-1)
            self._buf.set_times(t_host, None if guidance is None else torch.as_tensor(guidance, dtype=torch.float32).cpu().reshape(-1), self.device)
            if cache is not None:
                times = t_host.tolist()
        temb = self._temb(pooled, cfg.guidance_embeds)
        st = ops.act(temb, ops.ACT_SILU)
        ops.gemm(st, self.mod_w, out=mod, bias=self.mod_b)          # every block's modulation in one GEMM
        modv = mod.view(-1)
        if taps is not None:
            taps["temb"] = temb.clone()
            taps["x_embed"] = x[:, St:].clone(); taps["ctx_embed"] = x[:, :St].clone()

        nb = B      # the batch size blocks 1... run at: under a step cache 0 on a reused step, the number of computing images on a mixed one
        if self.double:
            if cache is not None:
                cache.before_first_block(x, B, St, Si, D, self._precision_key, self.device)
            self._double_block(ws, 0, j, cos, sin, taps)
            if cache is not None:
                nb = cache.after_first_block(x, mod, B, St, Si, D, taps, times=times)
        if nb:
            self._blocks_after_first(ws, j if nb == B else _Joint(ws, nb, St, Si, D, F), cos, sin, taps)
        if cache is not None:
            cache.after_last_block(x, mod, B, St, Si, D)
        mo = self.mod_off["out"]             # AdaLayerNormContinuous: scale, shift
        ops.layernorm(img.x, j.nrm_img, img.M, D, scale=modv[mo:], shift=modv[mo + D:], ld_mod=self.mod_total, **img.ln)
        ops.gemm(j.nrm_img, self.w["proj_out.weight"], out=ws["out"], bias=self.w["proj_out.bias"], M=img.M, lda=D, ldc=cfg.out_channels)
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
        graphs = self._graphs
        ent = graphs.pop(key, None)
        if ent is None:
            while len(graphs) >= self.MAX_GRAPHS:
                graphs.pop(next(iter(graphs)))                 # least recently used: drops its graph, workspace and tables
            # private buffers for this capture: nothing the eager path (or another graph) will ever reallocate
            self._buf = buf = _Buffers()
            buf.set_times(t, g, self.device)
            self._rope(txt_ids, img_ids)                     # host-side table build + upload happen outside capture
            self.forward(hidden, enc, pooled, None, img_ids, txt_ids, g)   # warm-up: allocates the workspace and every temporary
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self.forward(hidden, enc, pooled, None, img_ids, txt_ids, g)
            ent = dict(graph=graph, out=out, buf=buf)
            self._buf = _Buffers()                           # hand the buffers over: the next eager forward / capture allocates its own
        graphs[key] = ent                                     # (re)insert as most recently used
        ent["buf"].set_times(t, g, self.device)               # the entry's own time buffers (same B: the key holds the shapes)
        ent["graph"].replay()
        return ent["out"]

    __call__ = forward
