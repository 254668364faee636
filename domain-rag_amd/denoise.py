"""What ``FluxTxt2ImgHIP`` (engine.py) and ``FluxFillHIP`` (fill_pipeline.py) share: the flow-Euler denoise loop and the switches that choose how a step's
DiT forward runs (hipGraph replay, eagerly under a sampling recorder, eagerly with the step cache); a pipeline adds its buffers, encodes and decode."""
from __future__ import annotations

import torch

from . import ops, step_cache as sc
from .scheduler import model_timestep


class DenoisePipeline:
    def __init__(self, transformer, vae, use_graph: bool = True, step_cache: float | None = None, step_cache_scope: str | None = None,
                 step_cache_order: int | None = None, step_cache_max_run: int | None = None, step_cache_warmup: int | None = None):
        self.tr, self.vae, self.dev, self.use_graph = transformer, vae, transformer.device, use_graph      # use_graph: replay the forward as a hipGraph
        # first-block step cache (step_cache.StepCache; opt-in): threshold (None = $DRAG_STEP_CACHE, else off; 0 = off; on = eager forwards with
        # one cache, reset at the start of each call; use_graph is ignored) and scope "batch" / "image" (None = $DRAG_STEP_CACHE_SCOPE, else "batch")
        self.step_cache = sc.STEP_CACHE_DEFAULT if step_cache is None else step_cache
        self.step_cache_scope = sc.STEP_CACHE_SCOPE_DEFAULT if step_cache_scope is None else sc.parse_step_cache_scope(step_cache_scope)
        # what a reused step adds (0: the cached residual; 1: its first-order forecast) and the reuse limits of a threshold decision (0: none);
        # None = $DRAG_STEP_CACHE_ORDER / _MAX_RUN / _WARMUP, else 0.  All three do nothing while the cache is off
        self.step_cache_order = sc.STEP_CACHE_ORDER_DEFAULT if step_cache_order is None else sc.parse_step_cache_order(step_cache_order)
        self.step_cache_max_run = sc.STEP_CACHE_MAX_RUN_DEFAULT if step_cache_max_run is None else sc.parse_step_cache_count(step_cache_max_run, "max_run")
        self.step_cache_warmup = sc.STEP_CACHE_WARMUP_DEFAULT if step_cache_warmup is None else sc.parse_step_cache_count(step_cache_warmup, "warmup")
        self.step_cache_forced = self.step_cache_forced_images = None      # measurement only (scripts/bench_step_cache.py): StepCache's patterns
        self.last_step_decisions = self.last_step_reused_images = self.last_step_forecasts = None      # of the last call
        self._cache = self._key = None      # (the one StepCache; the buffers' key)

    def denoise(self, tokens, ld, prompt_embeds, pooled, img_ids, txt_ids, guidance, sigmas, timesteps, first, last, recorder=None, on_step=None):
        """steps ``first`` ... ``last - 1`` in place on columns [0, 64) of ``tokens`` bf16 [B, n_tok, ld], the DiT's input rows.  ``recorder``: an
        ``ops.GemmRecorder`` that brackets every ``recorder.every``-th step, which then runs eagerly.  ``on_step(i, latents)``: called after every
        Euler update with a bf16 [B, n_tok, 64] COPY of the packed latents (what diffusers hands ``callback_on_step_end``)."""
        B, n_tok = tokens.shape[:2]
        cache = self._cache = sc.pipeline_step_cache(self._cache, self.step_cache, self.step_cache_forced, self.step_cache_scope, self.step_cache_forced_images,
                                                     self.step_cache_order, self.step_cache_max_run, self.step_cache_warmup)
        for i in range(first, last):
            t = torch.full((B,), model_timestep(timesteps[i]))
            timed = recorder is not None and (i - first) % recorder.every == 0
            if recorder is not None:
                ops.set_recorder(recorder if timed else None)
            if cache is None and self.use_graph and not timed:
                v = self.tr.forward_graphed(tokens, prompt_embeds, pooled, t, img_ids, txt_ids, guidance)
            else:
                v = self.tr.forward(tokens, prompt_embeds, pooled, t, img_ids, txt_ids, guidance, cache=cache)
            ops.flow_euler_rows(tokens, v, B * n_tok, 64, ld, 64, float(sigmas[i + 1] - sigmas[i]))
            if on_step is not None:
                on_step(i, tokens[:, :, :64].clone())
        self.last_step_decisions, self.last_step_reused_images = (None, None) if cache is None else (list(cache.decisions), list(cache.reused_images))
        self.last_step_forecasts = None if cache is None else list(cache.forecasts)
