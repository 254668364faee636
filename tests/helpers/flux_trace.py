"""The launch trace of the Flux DiT forward, on CPU tensors: :class:`TraceOps` stands in for ``domain_rag_amd.ops`` in every module of the
package that imported it (flux, step_cache, ...), records each call as one line and returns tensors of the right shape for the calls that
allocate.  ``tests/test_flux_launch_trace.py`` compares the traces of :data:`VARIANTS` with ``tests/golden/flux_launch_trace.json``.

A line is ``[function, {parameter: value}]``: the arguments bound to the parameter names of the real ``ops`` function, those that equal
the parameter's default left out (so a keyword passed as its default is the launch it is without it); the dicts of ``gemm_pair`` are
``gemm`` keywords and are recorded the same way.  A tensor is ``"buffer+element offset:dtype"``.  Buffers: the model's resident
tensors by their place (``w[name]``, ``mod_w``, ``mod_b``, ``double[i][key]``, ``single[i][key]``, ``...[key@mx][0 | 1]``), the forward's
inputs by name, everything else (workspace, temporaries, the step cache's state) ``#bytes.n``: the size of its storage and the ordinal of
the storage's first appearance among those of that size (so a buffer that one variant adds does not renumber the others).  Every tensor
seen is kept alive: a freed storage's address would be handed out again and two buffers would share a name.

The fixture holds every distinct launch once, one per text line under a short id (a hash of the line), and each variant as its sequence of
ids: the variants share most of their launches.  A changed launch shows as one line out, one line in, and its id in the variants it is in.

    python tests/helpers/flux_trace.py --write      # a pull request that changes launches on purpose regenerates the fixture
"""
from __future__ import annotations

import contextlib
import hashlib
import inspect
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "flux_launch_trace.json")

CFG = dict(in_channels=64, num_layers=2, num_single_layers=2, num_attention_heads=2, joint_attention_dim=128, pooled_projection_dim=64)
B, LAT_H, LAT_W, ST = 2, 4, 6, 8      # h != w: the RoPE table knows which is which
TIMES = (1.0, 0.75, 0.5, 0.25)      # one per forward of a step-cache sequence (exact in binary: the forecast coefficients are too)
FORCED_IMAGES = [(False, False), (False, False), (True, False), (True, True)]      # computed, computed, mixed (compaction), all reuse


def _real_ops():
    from domain_rag_amd import ops
    return ops


_DTYPES = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.uint8: "u8"}


class TraceOps:
    def __init__(self, cost=lambda M, N, K, M2=0: M * N * K):
        self._real = _real_ops()
        self._cost = cost
        self._keep, self._named, self._ordinal, self.lines = [], {}, {}, []

    # ---- naming
    def name(self, tensor, name) -> None:
        self._keep.append(tensor)
        self._named[tensor.untyped_storage().data_ptr()] = name

    def begin(self, model, **inputs) -> None:
        """name the model's resident tensors and the forward's inputs; the trace starts here (set-up is not pinned)"""
        for k, v in model.w.items():
            self.name(v, f"w[{k}]")
        self.name(model.mod_w, "mod_w"); self.name(model.mod_b, "mod_b")
        for kind, blocks in (("double", model.double), ("single", model.single)):
            for i, blk in enumerate(blocks):
                for k, v in blk.items():
                    for j, t in enumerate(v if isinstance(v, tuple) else (v,)):
                        self.name(t, f"{kind}[{i}][{k}]" + (f"[{j}]" if isinstance(v, tuple) else ""))
        for k, v in inputs.items():
            if torch.is_tensor(v):
                self.name(v, k)
        self._ordinal, self.lines = {}, []

    def _value(self, v):
        if torch.is_tensor(v):
            self._keep.append(v)
            ptr, size = v.untyped_storage().data_ptr(), v.untyped_storage().nbytes()
            if ptr not in self._named and ptr not in self._ordinal:
                self._ordinal[ptr] = "#%d.%d" % (size, sum(n.startswith("#%d." % size) for n in self._ordinal.values()))
            return "%s+%d:%s" % (self._named.get(ptr) or self._ordinal[ptr], v.storage_offset(), _DTYPES.get(v.dtype, str(v.dtype)))
        if isinstance(v, dict):
            return {k: self._value(x) for k, x in v.items()}
        if isinstance(v, (tuple, list)):
            return [self._value(x) for x in v]
        if isinstance(v, torch.device):
            return str(v)
        return v

    def _bound(self, fn, args, kwargs) -> dict:
        """the call's arguments by parameter name of the real ``ops.fn``, without those that equal the default"""
        sig = inspect.signature(getattr(self._real, fn))
        given = sig.bind(*args, **kwargs).arguments
        return {k: self._value(v) for k, v in given.items()
                if torch.is_tensor(v) or isinstance(v, (dict, tuple, list)) or v != sig.parameters[k].default}

    def _record(self, fn, args, kwargs, **more) -> None:
        line = self._bound(fn, args, kwargs)
        line.update({k: self._value(v) for k, v in more.items()})
        self.lines.append([fn, line])

    # ---- the calls that answer or allocate
    def __getattr__(self, fn):
        if fn.startswith("_"):
            raise AttributeError(fn)
        real = getattr(self._real, fn)      # a name ops does not have is an error here too
        if not callable(real):
            return real                      # ACT_* and the like
        return lambda *a, **k: self._record(fn, a, k)

    def attention_mxfp8_supported(self, B, S, H):
        return True

    def gemm_cost(self, M, N, K, M2=0):
        return self._cost(M, N, K, M2)

    def stepcache_workspace_bytes(self, B, rows_per_batch, cols):
        return 64

    def gemm(self, a, w, out=None, **k):
        if out is None:
            out = torch.empty((k.get("M") or a.numel() // w.shape[1], w.shape[0]), dtype=torch.float32 if k.get("out_f32") else torch.bfloat16)
        self._record("gemm", (a, w, out), k)
        return out

    def gemm_pair(self, first, second):
        self.lines.append(["gemm_pair", {"first": self._bound("gemm", (), first), "second": self._bound("gemm", (), second)}])
        return first["out"], second["out"]

    def gemm_mxfp8(self, aq, ascale, wq, wscale, out=None, **k):
        if out is None:
            out = torch.empty((k.get("M") or aq.shape[0], wq.shape[0]), dtype=torch.bfloat16)
        self._record("gemm_mxfp8", (aq, ascale, wq, wscale, out), k)
        return out

    def timestep_embedding(self, t, dim):
        out = torch.empty((t.numel(), dim), dtype=torch.bfloat16)
        self._record("timestep_embedding", (t, dim), {}, **{"->": out})
        return out

    def act(self, x, kind, out=None):
        given = out is not None
        out = out if given else torch.empty_like(x)
        self._record("act", (x, kind), {"out": out} if given else {}, **({} if given else {"->": out}))
        return out

    def quantize_mxfp8(self, x, **k):
        out = k.get("out")
        if out is None:
            M, K = (k.get("M") or x.shape[0]), (k.get("K") or x.shape[-1])
            k = dict(k, out=(torch.empty((M, K), dtype=torch.uint8), torch.empty((M, K // 32), dtype=torch.uint8)))
        self._record("quantize_mxfp8", (x,), k)
        return k["out"]

    def attention_mxfp8_images(self, B, S, H, device):
        sp = (S + 127) // 128 * 128
        out = tuple(torch.empty((B, H) + shp, dtype=torch.uint8) for shp in ((sp, 128), (sp, 4), (sp, 128), (sp, 4), (128, sp), (128, sp // 32)))
        self._record("attention_mxfp8_images", (B, S, H, device), {}, **{"->": out})
        return out


@contextlib.contextmanager
def installed(trace: TraceOps, **flux_globals):
    """``trace`` in place of ``ops`` in every loaded module of the package that holds it, and ``flux``'s module switches set as given"""
    from domain_rag_amd import flux
    real = trace._real
    holders = [m for n, m in list(sys.modules.items()) if n.startswith("domain_rag_amd.") and m is not None and m.__dict__.get("ops") is real]
    saved = {k: getattr(flux, k) for k in flux_globals}
    try:
        for m in holders:
            m.ops = trace
        for k, v in flux_globals.items():
            setattr(flux, k, v)
        yield
    finally:
        for m in holders:
            m.ops = real
        for k, v in saved.items():
            setattr(flux, k, v)


def config(**over):
    from domain_rag_amd.flux_params import FluxConfig
    return FluxConfig(**dict(CFG, **over))


def inputs(cfg, guidance=True, seed=0) -> dict:
    """the forward's arguments by name (CPU tensors; ``timestep`` is set per forward)"""
    from domain_rag_amd.flux import latent_image_ids
    g = torch.Generator().manual_seed(seed)
    return dict(hidden=torch.randn(B, LAT_H * LAT_W, cfg.in_channels, generator=g).bfloat16(),
                enc=torch.randn(B, ST, cfg.joint_attention_dim, generator=g).bfloat16(),
                pooled=torch.randn(B, cfg.pooled_projection_dim, generator=g).bfloat16(),
                img_ids=latent_image_ids(LAT_H, LAT_W), txt_ids=torch.zeros(ST, 3),
                guidance=torch.full((B,), 3.5) if guidance else None)


def _cache(kind):
    from domain_rag_amd.step_cache import StepCache
    if kind is None:
        return None, TIMES[:1]
    if kind == "batch":
        return StepCache(0.1, forced=[False, True]), TIMES[:2]
    return StepCache(0.1, scope="image", forced_images=FORCED_IMAGES, order=kind), TIMES


def _stays(which):
    D = CFG["num_attention_heads"] * 128
    return frozenset({{"qkv": (3 * D, D), "mlp": (4 * D, D)}[which]})


# name -> (linear_precision, attention_precision, flux module switches, gemm_cost rule, guidance embedding, step cache)
_FUSE, _SPLIT = (lambda M, N, K, M2=0: 1), (lambda M, N, K, M2=0: N)      # one launch costs what each of two does / what its columns do
VARIANTS: dict = {}
for _lin in ("bf16", "mxfp8"):
    for _att in ("bf16", "mxfp8"):
        for _f in (True, False):
            VARIANTS[f"{_lin}-{_att}-{'fused' if _f else 'split'}"] = (_lin, _att, dict(_FUSED_QKV_MLP=_f), None, True, None)
VARIANTS.update({
    "bf16-bf16-cost-favours-fused": ("bf16", "bf16", dict(_FUSED_QKV_MLP=None), _FUSE, True, None),
    "bf16-bf16-cost-favours-split": ("bf16", "bf16", dict(_FUSED_QKV_MLP=None), _SPLIT, True, None),
    "bf16-bf16-separate-qprep": ("bf16", "bf16", dict(_FUSED_QKV_MLP=True, _SEPARATE_QPREP=True), None, True, None),
    "mxfp8-bf16-qkv-stays-bf16": ("mxfp8", "bf16", dict(_FUSED_QKV_MLP=True, _MX_STAYS_BF16=_stays("qkv")), None, True, None),
    "mxfp8-bf16-mlp-stays-bf16": ("mxfp8", "bf16", dict(_FUSED_QKV_MLP=True, _MX_STAYS_BF16=_stays("mlp")), None, True, None),
    "bf16-bf16-no-guidance": ("bf16", "bf16", dict(_FUSED_QKV_MLP=True), None, False, None),
    "step-cache-image-order0": ("bf16", "bf16", dict(_FUSED_QKV_MLP=True), None, True, 0),
    "step-cache-image-order1": ("bf16", "bf16", dict(_FUSED_QKV_MLP=True), None, True, 1),
    "step-cache-batch": ("bf16", "bf16", dict(_FUSED_QKV_MLP=True), None, True, "batch"),
})


def trace_variant(name: str) -> list:
    """the lines of variant ``name``: one model, one forward (a step cache: one per entry of its forced sequence)"""
    from domain_rag_amd.flux import FluxTransformerHIP
    from domain_rag_amd.flux_params import init_params
    lin, att, switches, cost, guided, cached = VARIANTS[name]
    cfg = config(guidance_embeds=guided)
    trace = TraceOps(cost) if cost else TraceOps()
    with installed(trace, **switches):
        model = FluxTransformerHIP(cfg, init_params(cfg, seed=1), "cpu", linear_precision=lin, attention_precision=att)
        inp = inputs(cfg, guided)
        cache, times = _cache(cached)
        trace.begin(model, **inp)
        for t in times:
            model.forward(inp["hidden"], inp["enc"], inp["pooled"], torch.full((B,), t), inp["img_ids"], inp["txt_ids"], inp["guidance"], cache=cache)
    return trace.lines


def dump(traces: dict) -> str:
    """the fixture's text: {"launches": {id: line}, one per text line in the order of first use; "variants": {name: [id, ...]}}"""
    launches, variants = {}, []
    for name, lines in traces.items():
        ids = []
        for ln in lines:
            text = json.dumps(ln, sort_keys=True)
            ids.append(hashlib.sha1(text.encode()).hexdigest()[:6])
            assert launches.setdefault(ids[-1], text) == text, f"two launches share the id {ids[-1]}: lengthen it"
        rows = [", ".join(json.dumps(i) for i in ids[k: k + 16]) for k in range(0, len(ids), 16)]
        variants.append(json.dumps(name) + ": [\n" + ",\n".join(rows) + "\n]")
    table = ",\n".join(json.dumps(i) + ": " + text for i, text in launches.items())
    return '{\n"launches": {\n' + table + '\n},\n"variants": {\n' + ",\n".join(variants) + "\n}\n}\n"


def load() -> dict:
    """the fixture as variant -> list of lines"""
    with open(FIXTURE) as f:
        g = json.load(f)
    used = {i for ids in g["variants"].values() for i in ids}
    assert used == set(g["launches"]), f"launches no variant uses: {sorted(set(g['launches']) - used)}"
    return {name: [g["launches"][i] for i in ids] for name, ids in g["variants"].items()}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    with open(FIXTURE, "w") as f:
        f.write(dump({name: trace_variant(name) for name in VARIANTS}))
    print(f"wrote {FIXTURE}")
