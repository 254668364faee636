"""The flags stages 2 and 3 share, declared once, and the :class:`..engine.Engine` they describe (``--model_root`` stays with a stage's directory flags)."""
from __future__ import annotations

import os

from ..engine import Engine
from ..step_cache import parse_step_cache, parse_step_cache_count, parse_step_cache_order


def add_engine_arguments(p, batch_flag: str, steps: int, tiny: str, png_files: str, png_note: str = "", own=()) -> None:
    """``--synthetic-weights`` ... ``--png``.  ``batch_flag``: the stage's batch-size flag, which ``--step_cache``'s help names; ``tiny``, ``png_files``,
    ``png_note``: the stage's words in those two helps; ``own``: (flag, add_argument keywords) of the stage's flags listed before ``--io_workers``"""
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--tiny", action="store_true", help=f"test hook: tiny architectures, {tiny}")
    p.add_argument("--linear_precision", choices=["bf16", "mxfp8"], default=None,
                   help="the DiT blocks' Linears: bf16, or OCP MXFP8 operands on the block-scaled matrix instruction (opt-in, lower "
                        "precision); default: $DRAG_LINEAR_PRECISION, else bf16")
    p.add_argument("--attention_precision", choices=["bf16", "mxfp8"], default=None,
                   help="the DiT blocks' attention: bf16, or OCP MXFP8 operands for both products (opt-in, lower precision: about 5 %% rms "
                        "per attention against 0.2 %%); default: $DRAG_ATTENTION_PRECISION, else bf16")
    p.add_argument("--step_cache", type=parse_step_cache, default=None, metavar="THRESHOLD",
                   help="first-block step cache of the denoise loop (opt-in, lower fidelity): a step whose first-block residual moved by less "
                        "than THRESHOLD (relative L1, every image of the batch) since the last computed step reuses that step's remaining "
                        f"blocks; batch neighbours then influence a result (--step_cache_scope image or {batch_flag} 1 restores independence); "
                        "default: $DRAG_STEP_CACHE, else off")
    p.add_argument("--step_cache_scope", choices=["batch", "image"], default=None,
                   help="who decides a reuse when --step_cache is on: batch = every image of the batch must be under the threshold; image = "
                        "every image decides for itself and the remaining blocks run on the others only, so a result does not depend on its "
                        "batch neighbours; default: $DRAG_STEP_CACHE_SCOPE, else batch")
    p.add_argument("--step_cache_order", type=parse_step_cache_order, default=None, metavar="0|1",
                   help="what a reused step adds when --step_cache is on: 0 = the cached residual of the last computed step as it is; 1 = its "
                        "first-order forecast along the timestep, from the last two computed steps; default: $DRAG_STEP_CACHE_ORDER, else 0")
    p.add_argument("--step_cache_max_run", type=lambda v: parse_step_cache_count(v, "max_run"), default=None, metavar="N",
                   help="when --step_cache is on: after N reused steps in a row the next one computes (per image under --step_cache_scope "
                        "image); 0 = no limit; default: $DRAG_STEP_CACHE_MAX_RUN, else 0")
    p.add_argument("--step_cache_warmup", type=lambda v: parse_step_cache_count(v, "warmup"), default=None, metavar="N",
                   help="when --step_cache is on: the first N steps of a denoise loop compute; default: $DRAG_STEP_CACHE_WARMUP, else 0")
    p.add_argument("--lora", action="append", default=None, metavar="PATH[:SCALE]",
                   help="merge a LoRA adapter (.safetensors, diffusers / PEFT or kohya spelling) into the DiT's weights at SCALE (default 1.0); "
                        "repeatable, merged in the order given; default: none")
    p.add_argument("--text_encoder", choices=["transformers", "hip"], default="transformers",
                   help="what encodes a prompt without a prompt_cache file: the transformers T5 / CLIP modules (eager torch) or the HIP "
                        "encoders (domain_rag_amd.textenc); tokenizers are host Python either way")
    p.add_argument("--num_inference_steps", type=int, default=steps)
    for flag, kw in own:
        p.add_argument(flag, **kw)
    p.add_argument("--io_workers", type=int, default=4, help="background PNG encoder processes (0 = write inline like the reference)")
    p.add_argument("--png", choices=["gpu", "host"], default="gpu",
                   help=f"{png_files}: 'gpu' = encoded on the device (domain_rag_amd.png: same pixels, not Pillow's bytes), "
                        f"'host' = Pillow (zlib level 6) in the --io_workers processes{png_note}")


def pipe_step_cache_switches(pipe) -> tuple:
    """(threshold, scope, order, max_run, warmup) of a pipeline, for the stages' two parameter writers"""
    return (getattr(pipe, "step_cache", None), getattr(pipe, "step_cache_scope", "batch"), getattr(pipe, "step_cache_order", 0),
            getattr(pipe, "step_cache_max_run", 0), getattr(pipe, "step_cache_warmup", 0))


def pipe_attention_precision(pipe) -> str:
    """the attention precision of a pipeline's DiT, for the stages' two parameter writers"""
    return getattr(getattr(pipe, "tr", None), "attention_precision", "bf16")


def pipe_loras(pipe) -> list:
    """[{"file": base name, "scale": s}, ...] of the LoRA adapters merged into a pipeline's DiT (empty without one), for the stages' two
    parameter writers"""
    tr = getattr(pipe, "tr", None)
    return [{"file": os.path.basename(e["adapter"].path or n), "scale": e["scale"]} for n, e in getattr(tr, "_loras", {}).items()]


def engine_from_args(kind: str, args, device) -> Engine:
    return Engine(kind, args.model_root, synthetic=args.synthetic_weights, tiny=args.tiny, device=device, text_encoder=args.text_encoder,
                  linear_precision=args.linear_precision, attention_precision=args.attention_precision, step_cache=args.step_cache, step_cache_scope=args.step_cache_scope,
                  step_cache_order=args.step_cache_order, step_cache_max_run=args.step_cache_max_run, step_cache_warmup=args.step_cache_warmup, lora=getattr(args, "lora", None))
