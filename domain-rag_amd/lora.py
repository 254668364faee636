"""LoRA adapters for the Flux DiT: reading an adapter file, and the merge rule written down (plain torch, CPU; host code only).

The rule (``drag_lora_merge_bf16``, include/domainrag_hip.h; ``FluxTransformerHIP.load_lora`` applies it to the resident weights):

    w[n, k] = bf16( f32(w0[n, k]) + sum_r scale[r] * up[n, r] * down[r, k] )

with ``down`` the file's ``lora_A`` / ``lora_down`` ``[r, K]``, ``up`` its ``lora_B`` / ``lora_up`` ``[N, r]``, ``scale[r]`` = the adapter's
scale times ``alpha / r`` of the entry the rank column comes from, the sum in float32 (any order) and one rounding to bf16 per element.
``merge_ref`` is that in float64; the tests hold the kernel and the model to it, no product path calls it.

An :class:`Adapter` is keyed by **diffusers Linear names** — the 2-D ``.weight`` names of ``flux_params.param_shapes`` — whichever
spelling the file uses:

* diffusers / PEFT: ``[transformer.]<module>.lora_A.weight``, ``.lora_B.weight`` and an optional scalar ``<module>.alpha`` (absent: the
  factor ``alpha / r`` is 1);
* kohya / BFL: ``lora_unet_<name>.lora_down.weight``, ``.lora_up.weight`` and an optional ``.alpha``, ``<name>`` one of ``KOHYA_NAMES``
  below.  A fused entry (``*_attn_qkv``, ``linear1``) is split by rows of ``up`` into one entry per diffusers name, all sharing ``down``.

The kohya table is written from the published converters' behaviour (diffusers' ``_convert_kohya_flux_lora_to_diffusers`` and the BFL
block layout); no real adapter file was available to confirm it.  Anything else in a file — an unknown module, a wrong shape, ``up`` and
``down`` of different rank, bias deltas, DoRA magnitudes, text-encoder adapters, kohya names outside the table — is refused by name.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import torch

from .flux_params import FluxConfig, param_shapes

# kohya / BFL block-local name -> diffusers block-local Linear names (a list of several: fused, split by rows of ``up`` in this order)
KOHYA_DOUBLE = {
    "img_attn_qkv": ["attn.to_q", "attn.to_k", "attn.to_v"],
    "img_attn_proj": ["attn.to_out.0"],
    "img_mlp_0": ["ff.net.0.proj"],
    "img_mlp_2": ["ff.net.2"],
    "img_mod_lin": ["norm1.linear"],
    "txt_attn_qkv": ["attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj"],
    "txt_attn_proj": ["attn.to_add_out"],
    "txt_mlp_0": ["ff_context.net.0.proj"],
    "txt_mlp_2": ["ff_context.net.2"],
    "txt_mod_lin": ["norm1_context.linear"],
}
KOHYA_SINGLE = {
    "linear1": ["attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp"],
    "linear2": ["proj_out"],
    "modulation_lin": ["norm.linear"],
}
KOHYA_NAMES = tuple(f"double_blocks_{{i}}_{k}" for k in KOHYA_DOUBLE) + tuple(f"single_blocks_{{i}}_{k}" for k in KOHYA_SINGLE)

_TEXT_ENCODER = re.compile(r"^(text_encoder(_2)?\.|lora_te)")
_DORA = ("dora_scale", "lora_magnitude_vector")
_BIAS = re.compile(r"(\.lora_B\.bias$|\.lora_up\.bias$|\.diff_b$|\.diff$)")


@dataclass
class Adapter:
    """``entries``: diffusers Linear name (``<module>.weight``) -> (down [r, K] bf16, up [N, r] bf16, alpha / r as a float), on the CPU"""
    entries: dict = field(default_factory=dict)
    path: str | None = None

    @property
    def ranks(self) -> list[int]:
        return sorted({d.shape[0] for d, _, _ in self.entries.values()})


def _linear_names(cfg: FluxConfig) -> dict[str, tuple]:
    return {n: s for n, s in param_shapes(cfg).items() if len(s) == 2}


def _refuse(what: str, keys) -> None:
    keys = sorted(keys)
    more = f" (+{len(keys) - 8} more)" if len(keys) > 8 else ""
    raise ValueError(f"LoRA file: {what}: {', '.join(keys[:8])}{more}")


def _triples(sd: dict, down_tag: str, up_tag: str) -> dict:
    """module -> {"down": key, "up": key, "alpha": key}; keys that fit none of the three forms are refused"""
    mods: dict = {}
    stray = []
    for k in sd:
        for tag, slot in ((f".{down_tag}.weight", "down"), (f".{up_tag}.weight", "up"), (".alpha", "alpha")):
            if k.endswith(tag):
                mods.setdefault(k[: -len(tag)], {})[slot] = k
                break
        else:
            stray.append(k)
    if stray:
        _refuse("keys that are neither a down / up weight nor an alpha", stray)
    half = [m[s] for m in mods.values() for s in m if not ("down" in m and "up" in m)]
    if half:
        _refuse("entries without both a down and an up weight", half)
    return mods


def read_adapter(path: str, cfg: FluxConfig | None = None) -> Adapter:
    """Read a LoRA ``.safetensors`` file in either spelling (module docstring) into an :class:`Adapter` for the DiT ``cfg`` describes
    (default: FLUX.1-dev).  Raises ``ValueError`` naming the offending keys for anything this library does not merge."""
    from safetensors.torch import load_file
    cfg = cfg or FluxConfig()
    sd = load_file(path, device="cpu")
    if not sd:
        raise ValueError(f"LoRA file {path}: no tensors")
    te = [k for k in sd if _TEXT_ENCODER.match(k)]
    if te:
        _refuse("text-encoder adapters are not supported (the text encoders take no adapters here)", te)
    dora = [k for k in sd if any(t in k for t in _DORA)]
    if dora:
        _refuse("DoRA magnitudes are not supported", dora)
    bias = [k for k in sd if _BIAS.search(k)]
    if bias:
        _refuse("bias / full-weight deltas are not supported", bias)
    shapes = _linear_names(cfg)
    kohya = any(k.startswith("lora_unet_") for k in sd)
    # module -> (targets [(diffusers weight name, rows)], key triple)
    plan: dict = {}
    if kohya:
        other = [k for k in sd if not k.startswith("lora_unet_")]
        if other:
            _refuse("keys of another spelling inside a kohya file", other)
        unknown = []
        for mod, t in _triples(sd, "lora_down", "lora_up").items():
            m = re.match(r"^lora_unet_(double|single)_blocks_(\d+)_(.+)$", mod)
            table = None if m is None else (KOHYA_DOUBLE if m.group(1) == "double" else KOHYA_SINGLE)
            if table is None or m.group(3) not in table:
                unknown.extend(t.values())
                continue
            pre = ("transformer_blocks." if m.group(1) == "double" else "single_transformer_blocks.") + m.group(2) + "."
            plan[mod] = ([pre + n + ".weight" for n in table[m.group(3)]], t)
        if unknown:
            _refuse("kohya names outside the supported table (lora.KOHYA_NAMES)", unknown)
    else:
        for mod, t in _triples(sd, "lora_A", "lora_B").items():
            name = mod[len("transformer."):] if mod.startswith("transformer.") else mod
            plan[mod] = ([name + ".weight"], t)
    unknown = [k for targets, t in plan.values() if any(n not in shapes for n in targets) for k in t.values()]
    if unknown:
        _refuse("modules that are no Linear of this DiT", unknown)
    entries: dict = {}
    for mod, (targets, t) in plan.items():
        down, up = sd[t["down"]], sd[t["up"]]
        if down.dim() != 2 or up.dim() != 2:
            _refuse("down / up weights must be 2-D", [t["down"], t["up"]])
        r = down.shape[0]
        if up.shape[1] != r or r < 1:
            _refuse(f"up {tuple(up.shape)} and down {tuple(down.shape)} differ in rank", [t["down"], t["up"]])
        rows = [shapes[n][0] for n in targets]
        K = shapes[targets[0]][1]
        if any(shapes[n][1] != K for n in targets) or down.shape[1] != K or up.shape[0] != sum(rows):
            _refuse(f"shapes down {tuple(down.shape)} / up {tuple(up.shape)} do not fit the weight [{sum(rows)}, {K}]", [t["down"], t["up"]])
        factor = 1.0
        if "alpha" in t:
            if sd[t["alpha"]].numel() != 1:
                _refuse("alpha must be a scalar", [t["alpha"]])
            factor = float(sd[t["alpha"]].double().item()) / r
        down = down.to(torch.bfloat16).contiguous()
        up = up.to(torch.bfloat16)
        row0 = 0
        for n, nr in zip(targets, rows):
            if n in entries:
                _refuse("two entries for one Linear", [t["down"], t["up"]])
            entries[n] = (down, up[row0: row0 + nr].contiguous(), factor)
            row0 += nr
    return Adapter(entries=entries, path=path)


def merge_ref(w0: torch.Tensor, entries) -> torch.Tensor:
    """the rule in float64: ``w0 + sum over entries (down, up, factor) of factor * up @ down``; ``factor`` a number, or one per rank column.
    The result is NOT rounded: ``.to(torch.bfloat16)`` is the one rounding of the rule."""
    out = w0.detach().cpu().double().clone()
    for down, up, factor in entries:
        f = torch.as_tensor(factor, dtype=torch.float64).reshape(-1).cpu()
        out += (up.detach().cpu().double() * f[None, :]) @ down.detach().cpu().double()
    return out


def parse_lora_arg(arg: str) -> tuple[str, float]:
    """``"PATH[:SCALE]"`` -> (path, scale): the tail after the last ``:`` is the scale only if it parses as a float (default 1.0)"""
    head, sep, tail = arg.rpartition(":")
    if sep and head:
        try:
            return head, float(tail)
        except ValueError:
            pass
    return arg, 1.0


def lora_spec(item) -> tuple[str, float]:
    """one element of ``Engine(lora=[...])``: a ``"PATH[:SCALE]"`` string or a (path, scale) pair"""
    if isinstance(item, str):
        return parse_lora_arg(item)
    path, scale = item
    return os.fspath(path), float(scale)
