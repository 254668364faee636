"""Host side of the step cache's forecast order and reuse limits (``step_cache.StepCache(order=, max_run=, warmup=)``): the parsers and the
process defaults, ``forecast_coefficient``, the constructor's refusals, the limit logic of ``_decide`` driven without kernels (as
tests/test_step_cache_scope_host.py drives it), ``pipeline_step_cache``, the stages' flags and the two output writers (no GPU)."""
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_parsing():
    from domain_rag_amd.step_cache import parse_step_cache_order
    for default in (None, "", "  "):
        assert parse_step_cache_order(default) == 0
    assert parse_step_cache_order("0") == 0 and parse_step_cache_order("1") == 1 and parse_step_cache_order(" 1 ") == 1
    assert parse_step_cache_order(0) == 0 and parse_step_cache_order(1) == 1
    for bad in ("2", "-1", "one", "1.0", "0.5", 2):
        with pytest.raises(ValueError, match="order"):
            parse_step_cache_order(bad)


def test_limit_parsing():
    from domain_rag_amd.step_cache import parse_step_cache_count
    for default in (None, "", "  "):
        assert parse_step_cache_count(default) == 0
    assert parse_step_cache_count("0") == 0 and parse_step_cache_count("3") == 3 and parse_step_cache_count(" 12 ") == 12 and parse_step_cache_count(4) == 4
    for bad in ("-1", "two", "1.5", "inf", -2):
        with pytest.raises(ValueError, match="max_run"):
            parse_step_cache_count(bad, "max_run")
    with pytest.raises(ValueError, match="warmup"):
        parse_step_cache_count("-3", "warmup")


@pytest.mark.parametrize("var, name, value, want", [
    ("DRAG_STEP_CACHE_ORDER", "STEP_CACHE_ORDER_DEFAULT", None, "0"), ("DRAG_STEP_CACHE_ORDER", "STEP_CACHE_ORDER_DEFAULT", "", "0"),
    ("DRAG_STEP_CACHE_ORDER", "STEP_CACHE_ORDER_DEFAULT", "1", "1"), ("DRAG_STEP_CACHE_ORDER", "STEP_CACHE_ORDER_DEFAULT", "2", "raises"),
    ("DRAG_STEP_CACHE_MAX_RUN", "STEP_CACHE_MAX_RUN_DEFAULT", "", "0"), ("DRAG_STEP_CACHE_MAX_RUN", "STEP_CACHE_MAX_RUN_DEFAULT", "3", "3"),
    ("DRAG_STEP_CACHE_MAX_RUN", "STEP_CACHE_MAX_RUN_DEFAULT", "-1", "raises"),
    ("DRAG_STEP_CACHE_WARMUP", "STEP_CACHE_WARMUP_DEFAULT", "5", "5"), ("DRAG_STEP_CACHE_WARMUP", "STEP_CACHE_WARMUP_DEFAULT", "few", "raises")])
def test_environment_variables_are_read_at_start_up(var, name, value, want):
    """a fresh interpreter per value (imports only, no GPU)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRAG_STEP_CACHE")}
    if value is not None:
        env[var] = value
    r = subprocess.run([sys.executable, "-c", f"from domain_rag_amd import flux; print(repr(flux.{name}))"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    if want == "raises":
        assert r.returncode != 0 and "ValueError" in r.stderr and "step cache" in r.stderr
    else:
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want


def test_forecast_coefficient():
    from domain_rag_amd.step_cache import forecast_coefficient
    assert forecast_coefficient(0.5, 0.75, 1.0) == 1.0                  # equal spacing
    assert forecast_coefficient(0.25, 0.75, 1.0) == 2.0                 # a run of two reused steps
    assert forecast_coefficient(0.75, 0.75, 1.0) == 0.0                 # the same time again: R itself
    assert forecast_coefficient(1.0, 0.75, 0.5) == 1.0                  # the direction of time does not matter
    assert forecast_coefficient(0.625, 0.75, 1.0) == 0.5
    assert forecast_coefficient(0.7, 0.8, 0.9) == (0.7 - 0.8) / (0.8 - 0.9)
    assert forecast_coefficient(0.5, 0.75, 0.75) is None                # nothing to extrapolate along
    assert forecast_coefficient(0.5, 1.0, 1.0 + 1e-300) is None         # the same float
    assert forecast_coefficient(0.0, 1.0, 1.0 - 2.0 ** -53) == -2.0 ** 53          # large, but a finite float32
    assert forecast_coefficient(-1e30, 1.0, 1.0 + 2.0 ** -52) is None   # a quotient that is no finite float32 falls back to order 0
    assert forecast_coefficient(math.nan, 1.0, 0.5) is None


def test_constructor_refusals_and_defaults():
    from domain_rag_amd.step_cache import StepCache
    c = StepCache(0.1)
    assert (c.order, c.max_run, c.warmup, c.forecasts, c.P) == (0, 0, 0, [], None)
    c = StepCache(0.1, None, "image", None, 1, 2, 3)                    # the new keywords come after the existing ones, in this order
    assert (c.order, c.max_run, c.warmup) == (1, 2, 3)
    for bad in (2, -1, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="order"):
            StepCache(0.1, order=bad)
    for bad in (-1, 1.5, "2", None):
        with pytest.raises(ValueError, match="max_run"):
            StepCache(0.1, max_run=bad)
        with pytest.raises(ValueError, match="warmup"):
            StepCache(0.1, warmup=bad)
    with pytest.raises(ValueError, match="order"):
        c.configure(0.1, order=3)
    assert c.order == 1                                                 # a refused configure changes nothing


def _drive(cache, ratios_per_forward):
    """``_decide`` without kernels: every image is valid (a computed step leaves it valid again), the ratios are what a delta would have
    written; returns the per-image masks"""
    out = []
    for ratios in ratios_per_forward:
        cache.valid_images = [True] * len(ratios)
        cache.ratios = torch.tensor(ratios, dtype=torch.float64)
        out.append(cache._decide())
    assert cache.reused_images[-len(out):] == out
    return out


C, R = False, True


def test_max_run():
    from domain_rag_amd.step_cache import StepCache
    for scope in ("batch", "image"):
        got = _drive(StepCache(math.inf, scope=scope, max_run=2), [[0.1, 0.1]] * 7)
        # the drive has everything valid from the start, so the first forward already reuses: two reuses, then a compute, and again
        assert got == [(R, R), (R, R), (C, C), (R, R), (R, R), (C, C), (R, R)], scope
        c = StepCache(math.inf, scope=scope, max_run=2)
        c.valid_images = [False, False]
        first = c._decide()                                             # nothing valid: computes
        assert [first] + _drive(c, [[0.1, 0.1]] * 6) == [(C, C), (R, R), (R, R), (C, C), (R, R), (R, R), (C, C)], scope
        assert _drive(StepCache(math.inf, scope=scope, max_run=1), [[0.0]] * 4) == [(R,), (C,), (R,), (C,)]
        assert _drive(StepCache(math.inf, scope=scope, max_run=0), [[0.0]] * 4) == [(R,)] * 4


def test_warmup():
    from domain_rag_amd.step_cache import StepCache
    for scope in ("batch", "image"):
        assert _drive(StepCache(math.inf, scope=scope, warmup=3), [[0.1, 0.2]] * 6) == [(C, C)] * 3 + [(R, R)] * 3, scope
        # both limits: the count of a run starts after the warm-up's computed steps
        assert _drive(StepCache(math.inf, scope=scope, warmup=2, max_run=2), [[0.1]] * 7) == [(C,), (C,), (R,), (R,), (C,), (R,), (R,)], scope
        c = StepCache(math.inf, scope=scope, warmup=1)
        _drive(c, [[0.1]] * 2)
        c.reset()                                                       # the index counts from reset()
        assert _drive(c, [[0.1]] * 2) == [(C,), (R,)]


def test_scope_image_counts_per_image():
    """threshold 0.5, max_run 2: image 1's ratio forces it to compute on forward 1 while image 0's run goes on; image 0 hits the limit on
    forward 2, image 1 (whose count started anew) only on forward 4"""
    from domain_rag_amd.step_cache import StepCache
    near, far = 0.1, 0.9
    got = _drive(StepCache(0.5, scope="image", max_run=2), [[near, near], [near, far], [near, near], [near, near], [near, near], [near, near]])
    assert got == [(R, R), (R, C), (C, R), (R, R), (R, C), (C, R)]


def test_scope_batch_shares_one_count():
    """the same ratios under scope "batch": image 1's ratio makes BOTH compute on forward 1, which resets the one count"""
    from domain_rag_amd.step_cache import StepCache
    near, far = 0.1, 0.9
    got = _drive(StepCache(0.5, scope="batch", max_run=2), [[near, near], [near, far], [near, near], [near, near], [near, near], [near, near]])
    assert got == [(R, R), (C, C), (R, R), (R, R), (C, C), (R, R)]


def test_forced_patterns_are_obeyed_beyond_the_limits():
    from domain_rag_amd.step_cache import StepCache
    c = StepCache(math.inf, forced=[True] * 5, max_run=2, warmup=3)
    assert _drive(c, [[0.1, 0.1]] * 8) == [(R, R)] * 5 + [(C, C), (R, R), (R, R)]          # ... after which the run of 5 counts: compute first
    masks = [(True, False), (True, True), (True, False), (True, True)]
    c = StepCache(math.inf, scope="image", forced_images=masks, max_run=1, warmup=4)
    assert _drive(c, [[0.1, 0.1]] * 6) == masks + [(C, C), (R, R)]
    c = StepCache(math.inf, scope="image", forced=[True, True, True], max_run=1)
    assert _drive(c, [[0.1]] * 5) == [(R,)] * 3 + [(C,), (R,)]


def test_pipeline_step_cache_passes_the_three_through_and_resets():
    from domain_rag_amd.step_cache import StepCache, pipeline_step_cache
    assert pipeline_step_cache(None, None, order=1, max_run=2, warmup=3) is None          # off: the switches do nothing
    assert pipeline_step_cache(None, 0, order=1) is None
    c = pipeline_step_cache(None, 0.2, None, "image", None, 1, 2, 3)
    assert isinstance(c, StepCache) and (c.threshold, c.scope, c.order, c.max_run, c.warmup) == (0.2, "image", 1, 2, 3)
    _drive(c, [[0.1]] * 4)
    assert len(c.decisions) == 4 and len(c.forecasts) == 0 and c.runs == [1]          # three warm-up computes, one reuse
    again = pipeline_step_cache(c, 0.3, order=1, max_run=4)
    assert again is c and (c.threshold, c.scope, c.order, c.max_run, c.warmup) == (0.3, "batch", 1, 4, 0)
    assert c.decisions == [] and c.reused_images == [] and c.forecasts == [] and c.runs == [] and c.has_prev == []
    assert pipeline_step_cache(c, 0.3) is c and (c.order, c.max_run, c.warmup) == (0, 0, 0)          # the defaults come back
    with pytest.raises(ValueError, match="order"):
        pipeline_step_cache(c, 0.3, order=2)
    with pytest.raises(ValueError, match="warmup"):
        pipeline_step_cache(None, 0.3, warmup=-1)


def test_order_one_needs_the_times():
    """refused before anything is launched (no GPU here: a launch would fail differently)"""
    from domain_rag_amd.step_cache import StepCache
    c = StepCache(0.1, order=1)
    x, mod = torch.zeros(2, 5, 8, dtype=torch.bfloat16), torch.zeros(2, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="times"):
        c.after_first_block(x, mod, 2, 1, 4, 8)
    with pytest.raises(ValueError, match="times"):
        c.after_first_block(x, mod, 2, 1, 4, 8, times=[0.5])


def test_cli_parsers_accept_the_three_flags():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    for mod in (stage2_generate, stage3_outpaint):
        p = mod.build_parser()
        a = p.parse_args([])
        assert (a.step_cache_order, a.step_cache_max_run, a.step_cache_warmup) == (None, None, None)
        a = p.parse_args(["--step_cache_order", "1", "--step_cache_max_run", "2", "--step_cache_warmup", "3"])
        assert (a.step_cache_order, a.step_cache_max_run, a.step_cache_warmup) == (1, 2, 3)
        assert p.parse_args(["--step_cache_order", "0"]).step_cache_order == 0
        for bad in (["--step_cache_order", "2"], ["--step_cache_max_run", "-1"], ["--step_cache_warmup", "x"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)


def test_output_writers_name_a_switch_only_when_it_is_not_the_default_and_the_cache_is_on():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    from domain_rag_amd.cli.engine_args import pipe_step_cache_switches
    for off in (None, 0, 0.0):
        assert stage2_generate.params_txt_step_cache(off, "image", 1, 2, 3) == ""
        assert stage3_outpaint.step_cache_params(off, "image", 1, 2, 3) == {}
    for scope in ("batch", "image"):
        assert stage2_generate.params_txt_step_cache(0.08, scope, 0, 0, 0) == stage2_generate.params_txt_step_cache(0.08, scope)
        assert stage3_outpaint.step_cache_params(0.08, scope, 0, 0, 0) == stage3_outpaint.step_cache_params(0.08, scope)
    assert stage3_outpaint.step_cache_params(0.08, "batch", 1, 2, 0) == {"step_cache": 0.08, "step_cache_order": 1, "step_cache_max_run": 2}
    assert stage3_outpaint.step_cache_params(0.08, "image", 0, 0, 4) == {"step_cache": 0.08, "step_cache_scope": "image", "step_cache_warmup": 4}
    base = stage2_generate.params_txt_step_cache(0.08)
    text = stage2_generate.params_txt_step_cache(0.08, "batch", 1, 2, 0)
    assert text.startswith(base) and text.count("\n") == 3 and text.splitlines()[1].endswith(": 1") and text.splitlines()[2].endswith(": 2")
    text = stage2_generate.params_txt_step_cache(0.08, "image", 1, 2, 3)
    assert text.count("\n") == 5 and len(set(line.split(":")[0] for line in text.splitlines())) == 5

    class Pipe:
        step_cache, step_cache_scope, step_cache_order, step_cache_max_run, step_cache_warmup = 0.5, "image", 1, 2, 3
    assert pipe_step_cache_switches(Pipe()) == (0.5, "image", 1, 2, 3)
    assert pipe_step_cache_switches(object()) == (None, "batch", 0, 0, 0)
