"""The Flux DiT forward's launch sequence and weight layout, on CPU tensors (no GPU): every variant of tests/helpers/flux_trace.py against
tests/golden/flux_launch_trace.json, line for line (the fixture is what the helper's ``--write`` mode gave when the fixture was last changed on
purpose), and ``linear_locations`` against the parameters the constructor was given."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import flux_trace  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return flux_trace.load()


def test_fixture_holds_exactly_the_variants(golden):
    assert list(golden) == list(flux_trace.VARIANTS)


@pytest.mark.parametrize("name", list(flux_trace.VARIANTS))
def test_launch_trace(golden, name):
    got = json.loads(json.dumps(flux_trace.trace_variant(name)))
    want = golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} differs\n  got  {json.dumps(g, sort_keys=True)}\n  want {json.dumps(w, sort_keys=True)}"
    assert len(got) == len(want), f"{name}: {len(got)} launches, the fixture has {len(want)}"


def test_fixture_text_is_the_helpers(golden):
    """one launch per text line, in the helper's spelling: a regenerated fixture diffs line by line"""
    with open(flux_trace.FIXTURE) as f:
        assert f.read() == flux_trace.dump(golden)


def test_a_trace_is_repeatable():
    assert flux_trace.trace_variant("mxfp8-mxfp8-split") == flux_trace.trace_variant("mxfp8-mxfp8-split")


def test_exchanged_weights_change_the_trace(monkeypatch):
    """resident tensors are named by their place, not numbered: wo for cwo is another trace"""
    begin = flux_trace.TraceOps.begin

    def swapped(self, model, **inputs):
        begin(self, model, **inputs)
        blk = model.double[1]
        blk["wo"], blk["cwo"] = blk["cwo"], blk["wo"]      # (same shape: only the names tell them apart)
    want = flux_trace.trace_variant("bf16-bf16-fused")
    monkeypatch.setattr(flux_trace.TraceOps, "begin", swapped)
    got = flux_trace.trace_variant("bf16-bf16-fused")
    assert len(got) == len(want) and got != want


# ------------------------------------------------------------------ the weight layout
@pytest.fixture(scope="module", params=[True, False], ids=["guidance", "no-guidance"])
def built(request):
    from domain_rag_amd.flux import FluxTransformerHIP
    from domain_rag_amd.flux_params import init_params
    cfg = flux_trace.config(guidance_embeds=request.param)
    params = init_params(cfg, seed=1)
    return cfg, params, FluxTransformerHIP(cfg, params, "cpu")


def test_linear_locations_names_every_linear(built):
    from domain_rag_amd.flux import linear_locations
    from domain_rag_amd.flux_params import param_shapes
    cfg = built[0]
    assert set(linear_locations(cfg)) == {n for n, shape in param_shapes(cfg).items() if len(shape) == 2}


def test_row_ranges_tile_each_holder(built):
    from domain_rag_amd.flux import linear_locations
    cfg, _, model = built
    ranges: dict = {}
    for holder, row0, rows in linear_locations(cfg).values():
        ranges.setdefault(holder, []).append((row0, rows))
    for holder, rr in ranges.items():
        end = 0
        for row0, rows in sorted(rr):
            assert row0 == end and rows > 0, f"{holder}: rows {row0} follow rows ending at {end}"
            end = row0 + rows
        assert end == model._holder(holder).shape[0], holder


def test_each_range_holds_its_parameter(built):
    from domain_rag_amd.flux import linear_locations
    cfg, params, model = built
    for name, (holder, row0, rows) in linear_locations(cfg).items():
        assert torch.equal(model._holder(holder)[row0: row0 + rows], params[name]), name


def test_mod_off_agrees_with_the_modulation_rows(built):
    from domain_rag_amd.flux import linear_locations
    cfg, _, model = built
    loc = linear_locations(cfg)
    want = {(i, nm): loc[f"transformer_blocks.{i}.{nm}.linear.weight"][1] for i in range(cfg.num_layers) for nm in ("norm1", "norm1_context")}
    want.update({("s", i): loc[f"single_transformer_blocks.{i}.norm.linear.weight"][1] for i in range(cfg.num_single_layers)})
    want["out"] = loc["norm_out.linear.weight"][1]
    assert model.mod_off == want
    assert all(h == ("mod_w",) for n, (h, _, _) in loc.items() if "norm" in n and ".linear." in n)
    assert model.mod_total == model.mod_w.shape[0] == model.mod_b.shape[0]
