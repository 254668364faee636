"""drag_gemm_mxfp8 against drag_gemm_bf16 on the DiT's six headline Linear shapes (M = 42 696 rows: 8 x 5337 joint tokens), same process,
interleaved: per round one timed batch of the bf16 GEMM, of the MX GEMM and of the activation quantise pass (the weights are quantised once,
when a model is built), medians over the rounds after a warm-up of each.  Yardstick: the bf16 GEMM.  The ratio column prices the MX route
with its quantise pass: (MX GEMM + quantise) / bf16 — below 1 the route is faster; a shape at or above 1 stays on bf16 inside
linear_precision="mxfp8" (flux._MX_STAYS_BF16).

    python scripts/bench_gemm_mxfp8.py [--log profiles/mxfp8_gemm_ab.log] [--m 42696] [--rounds 7] [--iters 10]

Clock and socket power: one read-only `amd-smi metric` query per shape while the GPU is under the MX GEMM, when the tool answers."""
import argparse
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from domain_rag_amd import ops

SHAPES = [(9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288), (21504, 3072), (3072, 15360)]        # (N, K)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters          # microseconds per call


def clock_and_power():
    """(MHz, W) from one read-only query, or (None, None)"""
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", "0", "--clock", "--power"], capture_output=True, text=True, timeout=20)
        mhz = re.search(r"GFX_0:\s*\n\s*CLK:\s*(\d+)", r.stdout)
        watt = re.search(r"SOCKET_POWER:\s*(\d+)", r.stdout)
        return (int(mhz.group(1)) if mhz else None, int(watt.group(1)) if watt else None)
    except (OSError, subprocess.SubprocessError):
        return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--m", type=int, default=42696)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    M = args.m
    say(f"# scripts/bench_gemm_mxfp8.py: M = {M}, {args.rounds} interleaved rounds x {args.iters} launches, medians; bias epilogue; "
        f"{torch.cuda.get_device_name(0)}")
    say("# N K | bf16 us (TFLOP/s) | mx gemm us (TFLOP/s) | quantise us (GB/s) | (mx + quantise) / bf16 | clock MHz, socket W under the MX GEMM")
    g = torch.Generator(device=dev).manual_seed(0)
    for N, K in SHAPES:
        a = torch.randn(M, K, device=dev, generator=g).bfloat16()
        w = (torch.randn(N, K, device=dev, generator=g) * 0.02).bfloat16()
        bias = torch.randn(N, device=dev, generator=g).bfloat16()
        c_bf, c_mx = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        wq, wsc = ops.quantize_mxfp8(w)
        aq, asc = ops.quantize_mxfp8(a)
        runs = {"bf16": lambda: ops.gemm(a, w, out=c_bf, bias=bias),
                "mx": lambda: ops.gemm_mxfp8(aq, asc, wq, wsc, c_mx, bias=bias),
                "quant": lambda: ops.quantize_mxfp8(a, out=(aq, asc))}
        for fn in runs.values():           # warm-up of every shape the timed window uses
            timed(fn, 3)
        # the MX result against the bf16 one on the same seeded data: the format's own error, not a kernel check (tests/test_gpu_mxfp8.py)
        rel = ((c_mx[:2048].float() - c_bf[:2048].float()).pow(2).mean().sqrt() / c_bf[:2048].float().pow(2).mean().sqrt()).item()
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, args.iters))
        for _ in range(20):
            runs["mx"]()
        mhz, watt = clock_and_power()
        torch.cuda.synchronize()
        bf, mx_, qn = (statistics.median(t[k]) for k in ("bf16", "mx", "quant"))
        fl = 2.0 * M * N * K
        qbytes = M * K * (2 + 1 + 1 / 32)
        say(f"{N:6d} {K:6d} | {bf:8.1f} ({fl / bf / 1e6:6.0f}) | {mx_:8.1f} ({fl / mx_ / 1e6:6.0f}) | {qn:7.1f} ({qbytes / qn / 1e3:5.0f}) | "
            f"{(mx_ + qn) / bf:5.3f} | {mhz if mhz is not None else '-'} MHz, {watt if watt is not None else '-'} W | rms(mx - bf16) / rms(bf16) = {rel:.4f}")
        del a, w, c_bf, c_mx, aq, asc, wq, wsc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
