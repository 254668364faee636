"""Which diffusers ``FluxTransformer2DModel`` parameters each resident tensor of :class:`.flux.FluxTransformerHIP` holds, stated once: the
constructor stacks by these tables, and ``linear_locations`` (LoRA's map), the modulation offsets and the set of weights with an MXFP8 copy
are read off them.  Row counts come from ``flux_params.param_shapes``; no offset is written down anywhere."""
from __future__ import annotations

from .flux_params import FluxConfig, param_shapes

_QKV = ("attn.to_q", "attn.to_k", "attn.to_v")
# per block: resident key -> (bias key, the Linears stacked in it by rows), and resident key -> RMSNorm vector.  The stacked Linears are the
# weights that have an MX copy in "mxfp8" mode (where a launch shape of theirs moves)
DOUBLE_LINEARS = {"wqkv": ("bqkv", _QKV), "cwqkv": ("cbqkv", ("attn.add_q_proj", "attn.add_k_proj", "attn.add_v_proj")),
                  "wo": ("bo", ("attn.to_out.0",)), "cwo": ("cbo", ("attn.to_add_out",)),
                  "w1": ("b1", ("ff.net.0.proj",)), "w2": ("b2", ("ff.net.2",)),
                  "cw1": ("cb1", ("ff_context.net.0.proj",)), "cw2": ("cb2", ("ff_context.net.2",))}
DOUBLE_NORMS = {"nq": "attn.norm_q", "nk": "attn.norm_k", "cnq": "attn.norm_added_q", "cnk": "attn.norm_added_k"}
# to_q | to_k | to_v | proj_mlp in one weight: two GEMMs over its row ranges, or ONE two-destination launch (flux._FUSED_QKV_MLP)
SINGLE_LINEARS = {"wqkvm": ("bqkvm", _QKV + ("proj_mlp",)), "wo": ("bo", ("proj_out",))}
SINGLE_NORMS = {"nq": "attn.norm_q", "nk": "attn.norm_k"}
# (model attribute, diffusers prefix, config field of the count, Linears, norms)
BLOCKS = (("double", "transformer_blocks", "num_layers", DOUBLE_LINEARS, DOUBLE_NORMS),
          ("single", "single_transformer_blocks", "num_single_layers", SINGLE_LINEARS, SINGLE_NORMS))


def top_linears(cfg: FluxConfig) -> list:
    """the Linears kept one by one in ``model.w``"""
    emb = ["timestep_embedder", "text_embedder"] + (["guidance_embedder"] if cfg.guidance_embeds else [])
    return ["x_embedder", "context_embedder", "proj_out"] + [f"time_text_embed.{e}.linear_{j}" for e in emb for j in (1, 2)]


def modulation(cfg: FluxConfig) -> list:
    """the stacked modulation matrix in row order: (``model.mod_off`` key, Linear) — [double i: norm1 (6D) | norm1_context (6D)], [single
    i: 3D], norm_out (2D); every block's AdaLN modulation is ONE GEMM per forward"""
    mod = [((i, nm), f"transformer_blocks.{i}.{nm}.linear") for i in range(cfg.num_layers) for nm in ("norm1", "norm1_context")]
    mod += [(("s", i), f"single_transformer_blocks.{i}.norm.linear") for i in range(cfg.num_single_layers)]
    return mod + [("out", "norm_out.linear")]


def linear_locations(cfg: FluxConfig) -> dict:
    """Where :class:`FluxTransformerHIP` keeps each Linear weight: every 2-D name of ``flux_params.param_shapes(cfg)`` ->
    ``(holder, row0, rows)``.  A holder names one resident tensor: ``("w", name)`` = ``model.w[name]``, ``("double", i, key)`` /
    ``("single", i, key)`` = ``model.double[i][key]`` / ``model.single[i][key]`` (the stacked ``wqkv`` / ``cwqkv`` / ``wqkvm`` hold
    several names as row ranges), ``("mod_w",)`` = the stacked modulation matrix, whose row offsets are ``model.mod_off``'s.  A pure
    function of the config; LoRA adapters find their targets with it."""
    stacks = {("w", n + ".weight"): (n,) for n in top_linears(cfg)}
    stacks[("mod_w",)] = [n for _, n in modulation(cfg)]
    for kind, prefix, count, linears, _ in BLOCKS:
        for i in range(getattr(cfg, count)):
            stacks.update({(kind, i, key): [f"{prefix}.{i}.{m}" for m in members] for key, (_, members) in linears.items()})
    shapes, loc = param_shapes(cfg), {}
    for holder, members in stacks.items():
        row0 = 0
        for n in members:
            loc[n + ".weight"] = (holder, row0, shapes[n + ".weight"][0])
            row0 += shapes[n + ".weight"][0]
    return loc
