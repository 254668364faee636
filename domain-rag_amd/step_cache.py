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


STEP_CACHE_ORDERS = (0, 1)


def parse_step_cache_order(text) -> int:
    """a step-cache forecast order as the environment / a command line gives it: None and "" mean 0; anything but 0 / 1 raises"""
    if text is None or str(text).strip() == "":
        return 0
    try:
        order = int(str(text).strip())
    except ValueError:
        order = None
    if order not in STEP_CACHE_ORDERS:
        raise ValueError(f"step cache order must be one of {STEP_CACHE_ORDERS}, not {text!r}")
    return order


def parse_step_cache_count(text, what: str = "limit") -> int:
    """a step-cache reuse limit (``max_run``, ``warmup``) as the environment / a command line gives it: None and "" mean 0 (no limit); a
    negative or unparsable value raises"""
    if text is None or str(text).strip() == "":
        return 0
    try:
        count = int(str(text).strip())
    except ValueError:
        count = -1
    if count < 0:
        raise ValueError(f"step cache {what} must be an integer >= 0, not {text!r}")
    return count


# what a reused step adds: order 0 (default) the cached residual R of the last computed step as it is; order 1 its first-order forecast
# R + c (R - P) from the computed step before (StepCache).  The reuse limits of a threshold decision: after ``max_run`` reused forwards in
# a row the next one computes; the first ``warmup`` forwards compute (0 = no limit).  $DRAG_STEP_CACHE_ORDER / _MAX_RUN / _WARMUP set the
# process defaults of the pipelines' ``step_cache_order`` / ``step_cache_max_run`` / ``step_cache_warmup``, read once
STEP_CACHE_ORDER_DEFAULT = parse_step_cache_order(os.environ.get("DRAG_STEP_CACHE_ORDER", ""))
STEP_CACHE_MAX_RUN_DEFAULT = parse_step_cache_count(os.environ.get("DRAG_STEP_CACHE_MAX_RUN", ""), "max_run")
STEP_CACHE_WARMUP_DEFAULT = parse_step_cache_count(os.environ.get("DRAG_STEP_CACHE_WARMUP", ""), "warmup")

_F32_MAX = 3.4028234663852886e38


def forecast_coefficient(t_now: float, t_last: float, t_prev: float) -> float | None:
    """``c`` of the first-order forecast ``R + c (R - P)``: R the residual of the computed step at ``t_last``, P that of the computed step
    before it at ``t_prev``, the reused step at ``t_now`` — ``(t_now - t_last) / (t_last - t_prev)`` in Python floats.  None when the two
    computed steps share a time (nothing to extrapolate along) or when the quotient is no finite float32: the step then reuses at order 0."""
    t_now, t_last, t_prev = float(t_now), float(t_last), float(t_prev)
    if t_last == t_prev:
        return None
    c = (t_now - t_last) / (t_last - t_prev)
    return c if abs(c) <= _F32_MAX else None      # NaN compares False


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

    ``order``: what a reused step adds.  0 (default) — R, the remaining-blocks residual of the last computed step, unchanged.  1 — its
    first-order forecast ``R + c (R - P)``: P is the residual of the computed step before the last one and
    ``c = (t_now - t_last) / (t_last - t_prev)`` per image, from the model timesteps the forward passes as ``times``
    (:func:`forecast_coefficient`; ``ops.stepcache_forecast_images``).  An image with fewer than two computed steps behind it, or whose two
    computed steps share a time, reuses at order 0, bit for bit.  ``forecasts`` holds per forward the per-image coefficient used (None
    where the image computed or fell back to order 0).

    ``max_run`` / ``warmup``: limits of a THRESHOLD decision (0, the default: none; ``forced`` / ``forced_images`` entries are obeyed as they
    are).  An image that has reused ``max_run`` forwards in a row computes the next one (the count is per image and a computed step resets
    it; under scope "batch" all images share one count); a forward whose index since ``reset()`` is below ``warmup`` computes.

    State: three dense bf16 [B, Si, D] buffers — E (scratch: the current first-block residual), F (the first-block residual of the last
    computed step), R (the residual of that step's remaining blocks, image rows only: the final projection reads nothing else) — with order
    1 a fourth, P, and per image ``t_last``, ``t_prev`` (host floats) and ``has_prev``; the float64 ratios and the reduction workspace.
    Validity is per image (``valid_images``; ``valid``: all of them): every image is invalid, and has no P, after ``reset()``, after a
    change of (B, Si, D) and after a change of the model's ``linear_precision`` or ``attention_precision``.  Reading the ratios back is the one host synchronisation
    per step."""

    def __init__(self, threshold: float, forced: Sequence[bool] | None = None, scope: str = "batch",
                 forced_images: Sequence[Sequence[bool]] | None = None, order: int = 0, max_run: int = 0, warmup: int = 0):
        self._key = self._precision = None
        self.E = self.F = self.R = self.P = self.ratios = self.workspace = None
        self.configure(threshold, forced, scope, forced_images, order, max_run, warmup)
        self.reset()

    def configure(self, threshold: float, forced: Sequence[bool] | None = None, scope: str = "batch",
                  forced_images: Sequence[Sequence[bool]] | None = None, order: int = 0, max_run: int = 0, warmup: int = 0) -> None:
        threshold = float(threshold)
        if math.isnan(threshold) or threshold < 0:
            raise ValueError(f"StepCache threshold must be >= 0, not {threshold!r}")
        if scope not in STEP_CACHE_SCOPES:
            raise ValueError(f"StepCache scope must be one of {STEP_CACHE_SCOPES}, not {scope!r}")
        if forced_images is not None and scope != "image":
            raise ValueError('StepCache forced_images needs scope="image" (forced is the whole-batch form)')
        if isinstance(order, bool) or order not in STEP_CACHE_ORDERS:
            raise ValueError(f"StepCache order must be one of {STEP_CACHE_ORDERS}, not {order!r}")
        for name, v in (("max_run", max_run), ("warmup", warmup)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"StepCache {name} must be an integer >= 0, not {v!r}")
        self.threshold = threshold
        self.scope = scope
        self.forced = None if forced is None else [bool(v) for v in forced]
        self.forced_images = None if forced_images is None else [tuple(bool(v) for v in m) for m in forced_images]
        if order != getattr(self, "order", order):      # P and the times are kept under order 1 only: nothing to forecast from yet
            self._forget_prev()
        self.order, self.max_run, self.warmup = int(order), max_run, warmup

    @property
    def valid(self) -> bool:
        return bool(self.valid_images) and all(self.valid_images)

    @valid.setter
    def valid(self, value: bool) -> None:
        self.valid_images = [bool(value)] * (self._key[0] if self._key else 0)

    def _forget_prev(self) -> None:
        B = self._key[0] if self._key else 0
        self.has_prev, self.t_last, self.t_prev = [False] * B, [None] * B, [None] * B

    def _invalidate(self) -> None:
        """every image: nothing to reuse, nothing to forecast from, no run of reuses behind it"""
        self.valid = False
        self._forget_prev()
        self.runs = [0] * len(self.valid_images)

    def reset(self) -> None:
        self._invalidate()
        self._step = (0, None, ())      # after_first_block's (batch size of blocks 1..., computing images, compaction) for after_last_block
        self.decisions: list[StepDecision] = []
        self.reused_images: list[tuple] = []
        self.forecasts: list[tuple] = []

    def _prepare(self, B: int, Si: int, D: int, precision: str, device) -> None:
        key = (B, Si, D, str(device))
        if self._key != key:
            bf = dict(dtype=torch.bfloat16, device=device)
            self.E, self.F, self.R = (torch.empty((B, Si, D), **bf) for _ in range(3))
            self.P = None
            self.ratios = torch.empty(B, dtype=torch.float64, device=device)
            self.workspace = torch.empty(ops.stepcache_workspace_bytes(B, Si, D), dtype=torch.uint8, device=device)
            self._key = key
            self._invalidate()
        if self._precision != precision:
            self._precision = precision
            self._invalidate()
        if len(self.valid_images) != B:          # reset() before the first forward did not know B
            self._invalidate()
        if self.order == 1 and self.P is None:
            self.P = torch.empty_like(self.R)
            self._forget_prev()

    def _decide(self) -> tuple:
        """after ``stepcache_delta``: read the ratios back, record the decision, return the per-image ``reused``"""
        valid = self.valid_images
        B, n = len(valid), len(self.decisions)
        ratios = None
        if any(valid):
            ratios = tuple(r if v else None for r, v in zip(self.ratios.cpu().tolist(), valid))
        if len(self.runs) != B:
            self.runs = [0] * B
        warm = n >= self.warmup      # the limits of a threshold decision
        if self.scope == "image":
            if self.forced_images is not None and n < len(self.forced_images):
                want = self.forced_images[n]
                if len(want) != B:
                    raise ValueError(f"StepCache forced_images[{n}] has {len(want)} entries for a batch of {B}")
            elif self.forced is not None and n < len(self.forced):
                want = (self.forced[n],) * B
            else:
                want = tuple(v and ratios[b] < self.threshold for b, v in enumerate(valid))      # NaN and +inf compare False
                want = tuple(w and warm and not 0 < self.max_run <= self.runs[b] for b, w in enumerate(want))
            mask = tuple(bool(v and w) for v, w in zip(valid, want))
        else:
            if self.forced is not None and n < len(self.forced):
                want = self.forced[n]
            else:
                want = self.valid and all(r < self.threshold for r in ratios)      # NaN and +inf compare False
                want = want and warm and not 0 < self.max_run <= max(self.runs)      # one shared count: all images reuse or compute together
            mask = (bool(self.valid and want),) * B
        self.runs = [run + 1 if m else 0 for run, m in zip(self.runs, mask)]
        self.decisions.append(StepDecision(ratios, all(mask)))
        self.reused_images.append(mask)
        return mask

    def _add_residual(self, x_img, B, Si, D, x_bs, images, times, taps) -> None:
        """a reused step of ``images``: each adds its cached residual R — with order 1 and two computed steps at distinct times behind it the
        forecast R + c (R - P), else R as it is (today's launches) — and ``forecasts`` gains the forward's coefficients"""
        coefs = [None] * B
        if self.order == 1:
            for b in images:
                if self.has_prev[b]:
                    coefs[b] = forecast_coefficient(times[b], self.t_last[b], self.t_prev[b])
        self.forecasts.append(tuple(coefs))
        ahead = [b for b in images if coefs[b] is not None]
        plain = [b for b in images if coefs[b] is None]
        if len(plain) == B:
            ops.stepcache_apply(x_img, self.R, B, Si, D, x_bs, +1)
        elif plain:
            ops.stepcache_apply_images(x_img, self.R, B, Si, D, x_bs, +1, plain)
        if ahead:
            ops.stepcache_forecast_images(x_img, self.R, self.P, B, Si, D, x_bs, ahead, [coefs[b] for b in ahead])
            if taps is not None:
                taps["cache.forecast"] = (tuple(ahead), tuple(coefs[b] for b in ahead))

    def _computed(self, computing, times) -> None:
        """order 1, the images that compute this step: the time of their last computed step moves to ``t_prev`` (with ``has_prev`` where
        that step is still valid: its R has just become P), this step's becomes ``t_last``"""
        for b in computing:
            self.has_prev[b] = self.valid_images[b]
            self.t_prev[b] = self.t_last[b] if self.valid_images[b] else None
            self.t_last[b] = times[b]

    # ---- the three calls of FluxTransformerHIP.forward on its workspace: ``x`` bf16 [B, St + Si, D] (text rows first), ``mod`` bf16 [B, mod_total].
    # An image is invalid exactly while its R holds the image rows after block 0 instead of a residual: between the last two calls.
    def before_first_block(self, x, B, St, Si, D, precision, device) -> None:
        """E <- the image rows as double block 0 receives them"""
        self._prepare(B, Si, D, precision, device)
        self.E.copy_(x[:, St:])

    def after_first_block(self, x, mod, B, St, Si, D, taps: dict | None = None, times: Sequence[float] | None = None) -> int:
        """E <- block 0's residual of the image rows, its ratio against the last computed step's (F), the decision.  Returns the batch size blocks
        1... run at: 0 (all reuse), B, or on a mixed step the number of computing images, which sit in the first slots until after_last_block.
        ``times``: the B model timesteps of this forward (host floats), which order 1 needs."""
        S, LM, x_img = St + Si, mod.shape[1], x.view(-1)[St * D:]          # joint buffer, image rows of batch 0 onwards
        if self.order == 1:
            if times is None:
                raise ValueError("StepCache order 1 needs the forward's timesteps (times)")
            times = [float(t) for t in times]
            if len(times) != B:
                raise ValueError(f"StepCache times has {len(times)} entries for a batch of {B}")
        ops.stepcache_delta(x_img, self.E, self.F if any(self.valid_images) else None, self.ratios, self.workspace, B, Si, D, S * D)
        if taps is not None:
            taps["cache.delta"] = self.E.clone()
        mask = self._decide()
        if all(mask):      # add that step's residual of the remaining blocks (or its forecast) and go to the final LayerNorm; F, R and P stay
            self._add_residual(x_img, B, Si, D, S * D, list(range(B)), times, taps)
            if taps is not None:
                taps["cache.x_img"] = x[:, St:].clone()
        elif not any(mask):
            # computed step: this residual becomes F; R <- the image rows now, turned into the residual after the last block
            self.forecasts.append((None,) * B)
            self.E, self.F = self.F, self.E
            if self.order == 1:      # the last computed step's residual becomes P: a pointer swap, R is overwritten anyway
                self.R, self.P = self.P, self.R
                self._computed(range(B), times)
            self.valid = False
            self.R.copy_(x[:, St:])
            self._step = (B, None, ())
        else:
            # scope "image", some reuse: the same per image, then the computing images go to the front (whole joint rows, modulation rows)
            computing = [b for b in range(B) if not mask[b]]
            if self.order == 1:      # before R is overwritten
                ops.stepcache_copy_images(self.P, self.R, Si * D, B, Si, D, [b for b in computing if self.valid_images[b]])
                self._computed(computing, times)
            ops.stepcache_copy_images(self.F, self.E, Si * D, B, Si, D, computing)
            ops.stepcache_copy_images(self.R, x_img, S * D, B, Si, D, computing)
            self._add_residual(x_img, B, Si, D, S * D, [b for b in range(B) if mask[b]], times, taps)
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
                        forced_images: Sequence[Sequence[bool]] | None = None, order: int = 0, max_run: int = 0,
                        warmup: int = 0) -> StepCache | None:
    """the cache one pipeline call runs with: None when the mode is off (``threshold`` None or 0); else the pipeline's one StepCache (its
    buffers are kept from call to call), brought to ``threshold`` / ``forced`` / ``scope`` / ``forced_images`` / ``order`` / ``max_run`` /
    ``warmup`` and RESET, so that no state leaks between samples"""
    if threshold is None or float(threshold) == 0:
        return None
    if cache is None:
        return StepCache(threshold, forced, scope, forced_images, order, max_run, warmup)
    cache.configure(threshold, forced, scope, forced_images, order, max_run, warmup)
    cache.reset()
    return cache
