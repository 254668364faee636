"""Host side of the step-cache switch: the CLI flags, the environment variable's parsing and the two output writers' additions (no GPU)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_parsers_accept_the_flag_and_default_to_off():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    for mod in (stage2_generate, stage3_outpaint):
        p = mod.build_parser()
        assert p.parse_args([]).step_cache is None
        assert p.parse_args(["--step_cache", "0.1"]).step_cache == 0.1
        assert p.parse_args(["--step_cache", "inf"]).step_cache == float("inf")
        assert p.parse_args(["--step_cache", "0"]).step_cache is None              # 0 means off
        for bad in ("-1", "abc", "nan"):
            with pytest.raises(SystemExit):
                p.parse_args(["--step_cache", bad])


def test_threshold_parsing():
    from domain_rag_amd.flux import parse_step_cache
    for off in (None, "", "  ", "0", "0.0"):
        assert parse_step_cache(off) is None
    assert parse_step_cache("0.08") == 0.08 and parse_step_cache("inf") == float("inf")
    for bad in ("-1", "abc", "nan", "-inf"):
        with pytest.raises(ValueError):
            parse_step_cache(bad)


@pytest.mark.parametrize("value, want", [(None, "None"), ("", "None"), ("0", "None"), ("0.25", "0.25"), ("-1", "raises"), ("abc", "raises")])
def test_environment_variable_is_read_at_start_up(value, want):
    """$DRAG_STEP_CACHE is read once, when domain_rag_amd.flux is imported: a fresh interpreter per value (imports only, no GPU)"""
    env = {k: v for k, v in os.environ.items() if k != "DRAG_STEP_CACHE"}
    if value is not None:
        env["DRAG_STEP_CACHE"] = value
    r = subprocess.run([sys.executable, "-c", "from domain_rag_amd import flux; print(repr(flux.STEP_CACHE_DEFAULT))"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    if want == "raises":
        assert r.returncode != 0 and "ValueError" in r.stderr and "step cache threshold" in r.stderr
    else:
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want


def test_output_writers_add_nothing_when_off():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    for off in (None, 0, 0.0):
        assert stage2_generate.params_txt_step_cache(off) == ""
        assert stage3_outpaint.step_cache_params(off) == {}
    line = stage2_generate.params_txt_step_cache(0.08)
    assert line.endswith("\n") and line.count("\n") == 1 and "0.08" in line
    assert stage3_outpaint.step_cache_params(0.08) == {"step_cache": 0.08}
