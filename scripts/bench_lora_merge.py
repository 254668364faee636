"""The LoRA merge on the GPU: drag_lora_merge_bf16 against a device-to-device copy of the same weight, and a whole-model load / unload.

    python scripts/bench_lora_merge.py [--rounds 5] [--iters 20] [--no-model] [--log profiles/lora_merge.log]

Kernel: in place on the headline's four weight shapes (N, K) = (3072, 3072), (9216, 3072), (21504, 3072), (3072, 15360) at R = 16, 64, 128.
The yardstick is ``copy_`` of the same N x K bf16 elements, device to device: it moves the same bytes (one read, one write) and is not code
under test.  One process, interleaved rounds (copy, then the three ranks, per shape, per round); every figure is the median over the
rounds of a device-event time over ``--iters`` back-to-back launches, after a warm-up of every launch the window uses.  The working set
cycles through enough buffers to exceed the 256 MiB Infinity Cache, so neither side is served from it.

Whole model: ``load_lora`` and ``unload_lora`` of an adapter over every Linear (rank 16) on the full-size synthetic FLUX.1-Fill DiT, host
clock around a device synchronise: the uploads of the factors and the copies of the pristine tensors are part of what a user waits for.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(3072, 3072), (9216, 3072), (21504, 3072), (3072, 15360)]
RANKS = [16, 64, 128]


def _event_ms(fn, iters: int) -> float:
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench_kernel(rounds: int, iters: int, out) -> None:
    import torch
    from domain_rag_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    cases = []
    for N, K in SHAPES:
        nbuf = max(2, -(-(512 << 20) // (N * K * 2)))                    # >= 512 MiB of weights in rotation
        ws = [(0.02 * torch.randn(N, K, generator=g, device=dev)).bfloat16() for _ in range(nbuf)]
        dst = torch.empty_like(ws[0])
        fac = {R: ((0.02 * torch.randn(N, R, generator=g, device=dev)).bfloat16(), (0.02 * torch.randn(R, K, generator=g, device=dev)).bfloat16(),
                   torch.full((R,), 1e-3, device=dev)) for R in RANKS}
        cases.append((N, K, ws, dst, fac))
    times: dict = {}
    for rnd in range(rounds + 1):                                         # round 0 is the warm-up of every launch
        for N, K, ws, dst, fac in cases:
            n = len(ws)
            t = _event_ms(lambda i: dst.copy_(ws[i % n]), iters)
            if rnd:
                times.setdefault((N, K, 0), []).append(t)
            for R in RANKS:
                up, down, sc = fac[R]
                t = _event_ms(lambda i: ops.lora_merge(ws[i % n], ws[i % n], up, down, sc), iters)
                if rnd:
                    times.setdefault((N, K, R), []).append(t)
    out(f"kernel: median of {rounds} interleaved rounds, {iters} launches per window; bytes = 2 x N x K x 2 (one read, one write)")
    out(f"{'N':>6} {'K':>6} {'R':>4} {'ms':>8} {'min':>8} {'max':>8} {'GB/s':>8} {'of copy':>8} {'TFLOP/s':>8}")
    for N, K, *_ in cases:
        tc = statistics.median(times[(N, K, 0)])
        for R in [0] + RANKS:
            v = times[(N, K, R)]
            t = statistics.median(v)
            name = "copy" if R == 0 else str(R)
            flops = f"{2.0 * N * K * R / (t * 1e-3) / 1e12:8.1f}" if R else f"{'':>8}"
            out(f"{N:>6} {K:>6} {name:>4} {t:8.4f} {min(v):8.4f} {max(v):8.4f} {4.0 * N * K / (t * 1e-3) / 1e9:8.0f} {tc / t:8.3f} {flops}")


def bench_model(out) -> None:
    import torch
    from domain_rag_amd import lora
    from domain_rag_amd.flux import FluxTransformerHIP, linear_locations
    from domain_rag_amd.flux_params import FluxConfig, init_params, param_shapes
    dev = torch.device("cuda:0")
    cfg = FluxConfig.flux_fill()
    params = init_params(cfg, seed=0, device=dev)
    model = FluxTransformerHIP(cfg, params, dev)
    del params
    torch.cuda.empty_cache()
    shapes = param_shapes(cfg)
    g = torch.Generator().manual_seed(1)
    entries = {n: ((torch.randn(16, shapes[n][1], generator=g) / shapes[n][1] ** 0.5).bfloat16(),
                   (0.01 * torch.randn(shapes[n][0], 16, generator=g)).bfloat16(), 1.0) for n in linear_locations(cfg)}
    ad = lora.Adapter(entries=entries)
    elements = sum(shapes[n][0] * shapes[n][1] for n in entries)
    out(f"whole model: FLUX.1-Fill DiT, seeded synthetic weights, {len(entries)} Linears, {elements / 1e9:.2f} G weights, rank 16 on every one")
    for rnd in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.load_lora(ad, name="bench")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.unload_lora("bench")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out(f"  round {rnd}: load_lora {t1 - t0:7.3f} s ({4.0 * elements / (t1 - t0) / 1e9:6.0f} GB/s of merge traffic), unload_lora {t2 - t1:7.3f} s")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the whole-model load / unload")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "lora_merge.log"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("bench_lora_merge: no GPU visible (there is no CPU path to time)", file=sys.stderr)
        return 2
    import __graft_entry__ as ge
    ge.build()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"scripts/bench_lora_merge.py --rounds {args.rounds} --iters {args.iters} on {torch.cuda.get_device_name(0)}")
    bench_kernel(args.rounds, args.iters, out)
    if not args.no_model:
        bench_model(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
