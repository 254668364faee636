"""First-block step cache of the Flux DiT's denoise loop, host side: the switch's parsing and process defaults, and the :class:`StepCache`
whose three calls ``FluxTransformerHIP.forward(..., cache=...)`` makes around its blocks (arithmetic: csrc/stepcache.hip, ``ops.stepcache_*``)."""
from __future__ import annotations

import math
import os
from typing import NamedTuple, Sequence

import torch

from . import ops


def parse_step_cache(text: str | None) -> float | None:
    """a step-cache threshold as the environment / a command line gives it: None, "" and 0 mean off (None); a negative, NaN or unparsable
    value raises ValueError; ``inf`` is a threshold (every step whose ratio is finite reuses)"""
    if text is None or str(text).strip() == "":
        return None
    try:
        v = float(text)
    except (TypeError, ValueError):
        raise ValueError(f"step cache threshold must be a number >= 0, not {text!r}") from None
    if math.isnan(v) or v < 0:
        raise ValueError(f"step cache threshold must be a number >= 0, not {text!r}")
    return v if v > 0 else None


# the first-block step cache (StepCache below; opt-in, no default threshold): $DRAG_STEP_CACHE=<threshold> sets the process default of the
# pipelines' ``step_cache``, read once; unset, empty or 0 = off
STEP_CACHE_DEFAULT = parse_step_cache(os.environ.get("DRAG_STEP_CACHE", ""))

STEP_CACHE_SCOPES = ("batch", "image")


def parse_step_cache_scope(text: str | None) -> str:
    """a step-cache scope as the environment / a command line gives it: None and "" mean "batch"; anything but "batch" / "image" raises"""
    if text is None or str(text).strip() == "":
        return "batch"
    scope = str(text).strip()
    if scope not in STEP_CACHE_SCOPES:
        raise ValueError(f"step cache scope must be one of {STEP_CACHE_SCOPES}, not {text!r}")
    return scope


# who decides a reuse: "batch" (the batch as a whole: every image under the threshold) or "image" (every image for itself; the remaining
# blocks run on the computing images only); $DRAG_STEP_CACHE_SCOPE sets the process default of the pipelines' ``step_cache_scope``, read once
STEP_CACHE_SCOPE_DEFAULT = parse_step_cache_scope(os.environ.get("DRAG_STEP_CACHE_SCOPE", ""))


class StepDecision(NamedTuple):
    """one forward's entry of ``StepCache.decisions``: the per-image first-block residual ratios against the last computed step (None when
    there was none to compare with) and whether the step reused that step's cached residual (scope "image": whether EVERY image did;
    ``StepCache.reused_images`` has the per-image answer)"""
    ratios: tuple | None
    reused: bool


def compact_pairs(reused: Sequence[bool]) -> tuple:
    """``(k, pairs)`` that bring the computing images of a batch to its front: ``k`` is the number of computing (not reused) images, and
    ``pairs`` exchange each reusing image that sits in a slot < k with a computing image that sits in a slot >= k, both taken in increasing
    order (there are equally many of each).  After the swaps slots 0 ... k-1 hold exactly the computing images; the same swaps again
    restore the order; a batch that is already compact gives no pairs."""
    reused = [bool(r) for r in reused]
    k = reused.count(False)
    front = [i for i in range(k) if reused[i]]
    back = [i for i in range(k, len(reused)) if not reused[i]]
    return k, list(zip(front, back))


class StepCache:
    """First-block cache of the DiT forward (``FluxTransformerHIP.forward(..., cache=...)``): after double block 0 the change of that block's
    residual since the last COMPUTED step, sum |new - old| / sum |old| per image, is compared with ``threshold``.  The comparison is always
    against the last computed step, so the drift is bounded by the threshold and not by the number of reuses.  A NaN or infinite ratio
    never reuses.

    ``scope``: "batch" (default) — when every image of the batch is under the threshold, the cached residual of the remaining blocks is
    added instead of running them; one image over it makes all compute.  "image" — every image decides for itself: the remaining blocks run
    at batch k on the k computing images, compacted to the front of the workspace, and each reusing image adds its own cached residual, so
    an image's result does not depend on its batch neighbours.  "last computed step" is then per image.

    ``forced``: for measurement and tests — ``forced[i]`` is the value ``reused`` takes in forward number ``i`` since ``reset()`` whatever
    the ratios say (a forward with nothing valid to reuse still computes); forwards beyond its length follow the threshold.
    ``forced_images`` (scope "image" only): the same per image — ``forced_images[i]`` is a sequence of B bools for forward ``i``.

    ``decisions`` holds one :class:`StepDecision` per forward, ``reused_images`` the per-image tuple of bools next to it (under "batch"
    all equal).

    State: three dense bf16 [B, Si, D] buffers — E (scratch: the current first-block residual), F (the first-block residual of the last
    computed step), R (the residual of that step's remaining blocks, image rows only: the final projection reads nothing else) — the float64
    ratios and the reduction workspace.  Validity is per image (``valid_images``; ``valid``: all of them): every image is invalid after
    ``reset()``, after a change of (B, Si, D) and after a change of the model's ``linear_precision``.  Reading the ratios back is the one
    host synchronisation per step."""

    def __init__(self, threshold: float, forced: Sequence[bool] | None = None, scope: str = "batch",
                 forced_images: Sequence[Sequence[bool]] | None = None):
        self._key = self._precision = None
        self.configure(threshold, forced, scope, forced_images)
        self.E = self.F = self.R = self.ratios = self.workspace = None
        self.reset()

    def configure(self, threshold: float, forced: Sequence[bool] | None = None, scope: str = "batch",
                  forced_images: Sequence[Sequence[bool]] | None = None) -> None:
        threshold = float(threshold)
        if math.isnan(threshold) or threshold < 0:
            raise ValueError(f"StepCache threshold must be >= 0, not {threshold!r}")
        if scope not in STEP_CACHE_SCOPES:
            raise ValueError(f"StepCache scope must be one of {STEP_CACHE_SCOPES}, not {scope!r}")
        if forced_images is not None and scope != "image":
            raise ValueError('StepCache forced_images needs scope="image" (forced is the whole-batch form)')
        self.threshold = threshold
        self.scope = scope
        self.forced = None if forced is None else [bool(v) for v in forced]
        self.forced_images = None if forced_images is None else [tuple(bool(v) for v in m) for m in forced_images]

    @property
    def valid(self) -> bool:
        return bool(self.valid_images) and all(self.valid_images)

    @valid.setter
    def valid(self, value: bool) -> None:
        self.valid_images = [bool(value)] * (self._key[0] if self._key else 0)

    def reset(self) -> None:
        self.valid = False
        self._step = (0, None, ())      # after_first_block's (batch size of blocks 1..., computing images, compaction) for after_last_block
        self.decisions: list[StepDecision] = []
        self.reused_images: list[tuple] = []

    def _prepare(self, B: int, Si: int, D: int, precision: str, device) -> None:
        key = (B, Si, D, str(device))
        if self._key != key:
            bf = dict(dtype=torch.bfloat16, device=device)
            self.E, self.F, self.R = (torch.empty((B, Si, D), **bf) for _ in range(3))
            self.ratios = torch.empty(B, dtype=torch.float64, device=device)
            self.workspace = torch.empty(ops.stepcache_workspace_bytes(B, Si, D), dtype=torch.uint8, device=device)
            self._key, self.valid = key, False
        if self._precision != precision:
            self._precision, self.valid = precision, False
        if len(self.valid_images) != B:          # reset() before the first forward did not know B
            self.valid = False

    def _decide(self) -> tuple:
        """after ``stepcache_delta``: read the ratios back, record the decision, return the per-image ``reused``"""
        valid = self.valid_images
        B, n = len(valid), len(self.decisions)
        ratios = None
        if any(valid):
            ratios = tuple(r if v else None for r, v in zip(self.ratios.cpu().tolist(), valid))
        if self.scope == "image":
            if self.forced_images is not None and n < len(self.forced_images):
                want = self.forced_images[n]
                if len(want) != B:
                    raise ValueError(f"StepCache forced_images[{n}] has {len(want)} entries for a batch of {B}")
            elif self.forced is not None and n < len(self.forced):
                want = (self.forced[n],) * B
            else:
                want = tuple(v and ratios[b] < self.threshold for b, v in enumerate(valid))      # NaN and +inf compare False
            mask = tuple(bool(v and w) for v, w in zip(valid, want))
        else:
            if self.forced is not None and n < len(self.forced):
                want = self.forced[n]
            else:
                want = self.valid and all(r < self.threshold for r in ratios)      # NaN and +inf compare False
            mask = (bool(self.valid and want),) * B
        self.decisions.append(StepDecision(ratios, all(mask)))
        self.reused_images.append(mask)
        return mask

    # ---- the three calls of FluxTransformerHIP.forward on its workspace: ``x`` bf16 [B, St + Si, D] (text rows first), ``mod`` bf16 [B, mod_total].
    # An image is invalid exactly while its R holds the image rows after block 0 instead of a residual: between the last two calls.
    def before_first_block(self, x, B, St, Si, D, precision, device) -> None:
        """E <- the image rows as double block 0 receives them"""
        self._prepare(B, Si, D, precision, device)
        self.E.copy_(x[:, St:])

    def after_first_block(self, x, mod, B, St, Si, D, taps: dict | None = None) -> int:
        """E <- block 0's residual of the image rows, its ratio against the last computed step's (F), the decision.  Returns the batch size blocks
        1... run at: 0 (all reuse), B, or on a mixed step the number of computing images, which sit in the first slots until after_last_block."""
        S, LM, x_img = St + Si, mod.shape[1], x.view(-1)[St * D:]          # joint buffer, image rows of batch 0 onwards
        ops.stepcache_delta(x_img, self.E, self.F if any(self.valid_images) else None, self.ratios, self.workspace, B, Si, D, S * D)
        if taps is not None:
            taps["cache.delta"] = self.E.clone()
        mask = self._decide()
        if all(mask):      # add that step's residual of the remaining blocks and go to the final LayerNorm; F and R stay
            ops.stepcache_apply(x_img, self.R, B, Si, D, S * D, +1)
            if taps is not None:
                taps["cache.x_img"] = x[:, St:].clone()
        elif not any(mask):
            # computed step: this residual becomes F; R <- the image rows now, turned into the residual after the last block
            self.E, self.F = self.F, self.E
            self.valid = False
            self.R.copy_(x[:, St:])
            self._step = (B, None, ())
        else:
            # scope "image", some reuse: the same per image, then the computing images go to the front (whole joint rows, modulation rows)
            computing = [b for b in range(B) if not mask[b]]
            ops.stepcache_copy_images(self.F, self.E, Si * D, B, Si, D, computing)
            ops.stepcache_copy_images(self.R, x_img, S * D, B, Si, D, computing)
            ops.stepcache_apply_images(x_img, self.R, B, Si, D, S * D, +1, [b for b in range(B) if mask[b]])
            for b in computing:
                self.valid_images[b] = False
            nb, pairs = compact_pairs(mask)
            self._step = (nb, computing, pairs)
            ops.stepcache_swap(x, B, S, D, S * D, pairs)
            ops.stepcache_swap(mod, B, 1, LM, LM, pairs)
            if taps is not None:
                swapped = dict(pairs + [(b, a) for a, b in pairs])
                taps["cache.slots"] = tuple(swapped.get(i, i) for i in range(B))      # the image each slot holds while blocks 1... run
        return self._step[0]

    def after_last_block(self, x, mod, B, St, Si, D) -> None:
        """capture: R <- image rows - (image rows after block 0) for the images that computed, which are valid again"""
        S, LM, x_img = St + Si, mod.shape[1], x.view(-1)[St * D:]
        (nb, computing, pairs), self._step = self._step, (0, None, ())
        if computing is not None:
            # the tail runs at batch B in the batch's own order: it reads the image rows and norm_out's modulation, not the text rows
            ops.stepcache_swap(x_img, B, Si, D, S * D, pairs)
            ops.stepcache_swap(mod, B, 1, LM, LM, pairs)
            ops.stepcache_apply_images(x_img, self.R, B, Si, D, S * D, -1, computing)
            for b in computing:
                self.valid_images[b] = True
        elif nb:
            ops.stepcache_apply(x_img, self.R, B, Si, D, S * D, -1)
            self.valid = True


def pipeline_step_cache(cache: StepCache | None, threshold: float | None, forced: Sequence[bool] | None = None, scope: str = "batch",
                        forced_images: Sequence[Sequence[bool]] | None = None) -> StepCache | None:
    """the cache one pipeline call runs with: None when the mode is off (``threshold`` None or 0); else the pipeline's one StepCache (its
    buffers are kept from call to call), brought to ``threshold`` / ``forced`` / ``scope`` / ``forced_images`` and RESET, so that no state
    leaks between samples"""
    if threshold is None or float(threshold) == 0:
        return None
    if cache is None:
        return StepCache(threshold, forced, scope, forced_images)
    cache.configure(threshold, forced, scope, forced_images)
    cache.reset()
    return cache
