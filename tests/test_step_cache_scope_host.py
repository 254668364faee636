"""Host side of the step cache's scope (``step_cache.StepCache(scope=...)``): the compaction helper, the scope's parsing, the refusal of
``forced_images`` under "batch", the unchanged ``StepDecision`` and the two output writers' additions (no GPU)."""
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_pairs_exhaustively_up_to_six_images():
    from domain_rag_amd.flux import compact_pairs
    for B in range(1, 7):
        for mask in itertools.product((False, True), repeat=B):
            k, pairs = compact_pairs(mask)
            assert k == mask.count(False)
            flat = [i for p in pairs for i in p]
            assert len(set(flat)) == len(flat) and all(0 <= i < B for i in flat), (mask, pairs)
            for a, b in pairs:          # a reusing image in the front, a computing image behind it
                assert a < k <= b and mask[a] and not mask[b], (mask, pairs)
            slots = list(range(B))
            for a, b in pairs:
                slots[a], slots[b] = slots[b], slots[a]
            assert sorted(slots[:k]) == [i for i in range(B) if not mask[i]], (mask, pairs)
            for a, b in pairs:
                slots[a], slots[b] = slots[b], slots[a]
            assert slots == list(range(B))
            if all(mask) or not any(mask) or list(mask) == sorted(mask):          # all reuse, all compute, already compact
                assert pairs == [], (mask, pairs)
            # both sides in increasing order
            assert [a for a, _ in pairs] == sorted(a for a, _ in pairs) and [b for _, b in pairs] == sorted(b for _, b in pairs)


def test_scope_parsing():
    from domain_rag_amd.flux import parse_step_cache_scope
    for off in (None, "", "  "):
        assert parse_step_cache_scope(off) == "batch"
    assert parse_step_cache_scope("batch") == "batch" and parse_step_cache_scope("image") == "image"
    for bad in ("junk", "Image", "images", "0", "1"):
        with pytest.raises(ValueError, match="scope"):
            parse_step_cache_scope(bad)


@pytest.mark.parametrize("value, want", [(None, "'batch'"), ("", "'batch'"), ("batch", "'batch'"), ("image", "'image'"), ("junk", "raises")])
def test_environment_variable_is_read_at_start_up(value, want):
    """$DRAG_STEP_CACHE_SCOPE is read once, when domain_rag_amd.flux is imported: a fresh interpreter per value (imports only, no GPU)"""
    env = {k: v for k, v in os.environ.items() if k != "DRAG_STEP_CACHE_SCOPE"}
    if value is not None:
        env["DRAG_STEP_CACHE_SCOPE"] = value
    r = subprocess.run([sys.executable, "-c", "from domain_rag_amd import flux; print(repr(flux.STEP_CACHE_SCOPE_DEFAULT))"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    if want == "raises":
        assert r.returncode != 0 and "ValueError" in r.stderr and "step cache scope" in r.stderr
    else:
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want


def test_cache_arguments():
    from domain_rag_amd.flux import StepCache, pipeline_step_cache
    assert StepCache(0.1).scope == "batch" and StepCache(0.1, scope="image").scope == "image"
    with pytest.raises(ValueError, match="scope"):
        StepCache(0.1, scope="junk")
    with pytest.raises(ValueError, match="forced_images"):
        StepCache(0.1, forced_images=[(True, False)])
    with pytest.raises(ValueError, match="forced_images"):
        StepCache(0.1, scope="batch", forced_images=[(True, False)])
    c = StepCache(0.1, scope="image", forced_images=[(True, False), [0, 1]])
    assert c.forced_images == [(True, False), (False, True)] and c.forced is None
    assert c.decisions == [] and c.reused_images == [] and c.valid is False
    # the pipelines' helper carries both through, and keeps the one cache
    assert pipeline_step_cache(None, None, scope="image") is None
    again = pipeline_step_cache(c, 0.2, None, "image", [(False, False)])
    assert again is c and c.threshold == 0.2 and c.forced_images == [(False, False)]
    assert pipeline_step_cache(c, 0.2).scope == "batch" and c.forced_images is None
    with pytest.raises(ValueError, match="forced_images"):
        pipeline_step_cache(c, 0.2, None, "batch", [(False, False)])


def test_step_decision_is_still_a_pair():
    """a first forward's decision, recorded without a device: nothing valid, so no ratios are read"""
    from domain_rag_amd.flux import StepCache, StepDecision
    for scope in ("batch", "image"):
        c = StepCache(0.1, scope=scope)
        c.valid_images = [False, False, False]
        assert c._decide() == (False, False, False)
        assert c.decisions[-1] == (None, False) and isinstance(c.decisions[-1], StepDecision) and len(c.decisions[-1]) == 2
        assert c.reused_images == [(False, False, False)]


def test_cli_parsers_accept_the_scope():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    for mod in (stage2_generate, stage3_outpaint):
        p = mod.build_parser()
        assert p.parse_args([]).step_cache_scope is None
        assert p.parse_args(["--step_cache_scope", "image"]).step_cache_scope == "image"
        assert p.parse_args(["--step_cache_scope", "batch"]).step_cache_scope == "batch"
        with pytest.raises(SystemExit):
            p.parse_args(["--step_cache_scope", "junk"])


def test_output_writers_name_the_scope_only_when_it_is_image_and_the_cache_is_on():
    from domain_rag_amd.cli import stage2_generate, stage3_outpaint
    for off in (None, 0, 0.0):
        assert stage2_generate.params_txt_step_cache(off, "image") == ""
        assert stage3_outpaint.step_cache_params(off, "image") == {}
    assert stage2_generate.params_txt_step_cache(0.08, "batch") == stage2_generate.params_txt_step_cache(0.08)
    assert stage3_outpaint.step_cache_params(0.08, "batch") == {"step_cache": 0.08}
    text = stage2_generate.params_txt_step_cache(0.08, "image")
    assert text.startswith(stage2_generate.params_txt_step_cache(0.08)) and text.count("\n") == 2 and text.endswith("image\n")
    assert stage3_outpaint.step_cache_params(0.08, "image") == {"step_cache": 0.08, "step_cache_scope": "image"}
