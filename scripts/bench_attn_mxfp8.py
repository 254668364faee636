"""MXFP8 attention (ops.qkv_prep_mxfp8 + ops.attention_mxfp8) against the bf16 route of the DiT (ops.k_norm_rope_vt + ops.attention_qprep), prep
passes included on both sides, same process, interleaved: per round every side gets --repeats timed windows of at least --window seconds
(device events, after a warm-up of each); the log carries each side's median and the spread (min .. max) of its own windows, TFLOP/s from
the shape-derived 4 B H S^2 128 FLOPs, and the MX kernel's registers, LDS and occupancy from the compiler's resource report.

    python scripts/bench_attn_mxfp8.py [--log profiles/attn_mxfp8_ab.log] [--rounds 2] [--repeats 2] [--window 0.5]
                                       [--resources FILE]     # a saved resource report instead of compiling csrc/attention_mxfp8.hip here

    python scripts/bench_attn_mxfp8.py --print-resources      # no GPU needed: compile for gfx950 and print the report's lines"""
import argparse
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 4608, 24), (1, 4608, 24), (1, 17625, 24), (1, 24166, 24)]        # (B, S, H): the headline step, one image, the stage-3 sizes
S_TXT = 512


def resource_report() -> list[str]:
    """the kernel-resource-usage remarks of the two MX attention sources, one line per kernel"""
    from domain_rag_amd import build
    out = []
    for src in ("attention_mxfp8.hip", "attention_prep_mxfp8.hip"):
        r = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                             os.path.join(build.CSRC, src), "-o", os.devnull], capture_output=True, text=True)
        if r.returncode != 0:
            return [f"# resource report: hipcc failed for {src}"]
        name, vals = None, {}
        for line in r.stderr.splitlines():
            m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|TotalSGPRs): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name, vals = m.group(2), {}
            else:
                vals[m.group(1)] = m.group(2)
                if m.group(1).startswith("LDS"):
                    out.append(f"# {src}: {name}: " + ", ".join(f"{k} {v}" for k, v in vals.items()))
    return out


def timed_window(fn, seconds):
    """microseconds per call over one window of at least ``seconds`` (the call count from a short probe)"""
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn(); fn()
    e.record()
    torch.cuda.synchronize()
    per = max(s.elapsed_time(e) / 2, 1e-3)                      # ms
    iters = max(3, int(math.ceil(seconds * 1e3 / per)))
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--print-resources", action="store_true")
    args = ap.parse_args()
    if args.print_resources:
        print("\n".join(resource_report()))
        return
    import torch
    from domain_rag_amd import ops
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            with open(args.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"# scripts/bench_attn_mxfp8.py: {args.rounds} interleaved rounds x {args.repeats} windows of >= {args.window} s per side, device events; "
        f"{torch.cuda.get_device_name(0)}")
    for line in (open(args.resources).read().splitlines() if args.resources else resource_report()):
        say(line)
    say("# B S H | side: median us [min .. max over its windows] (TFLOP/s of 4 B H S^2 128 over the side's total) | mxfp8 / bf16")
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1 / math.sqrt(128)
    for B, S, H in SHAPES:
        D = H * 128
        qkv0 = torch.randn(B, S, 3 * D, device=dev, generator=g).bfloat16()
        qkv = qkv0.clone()
        w = [(1 + 0.1 * torch.randn(128, device=dev, generator=g)).bfloat16() for _ in range(4)]
        ang = torch.rand(S, 64, device=dev, generator=g) * 6.28
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
        vt = torch.empty(B, H, 128, (S + 63) // 64 * 64, device=dev, dtype=torch.bfloat16)
        out_bf, out_mx = torch.empty(B, S, D, device=dev, dtype=torch.bfloat16), torch.empty(B, S, D, device=dev, dtype=torch.bfloat16)
        images = ops.attention_mxfp8_images(B, S, H, dev)
        # (the bf16 prep pass works in place: its timed repeats re-normalise prepared rows, the same memory traffic and arithmetic)
        runs = {"bf16 prep": lambda: ops.k_norm_rope_vt(qkv, vt, w[1], w[3], cos, sin, B, S, H, 3 * D, S_TXT),
                "bf16 attn": lambda: ops.attention_qprep(qkv, qkv.view(-1)[D:], vt, out_bf, B, S, H, 3 * D, S * 3 * D, D, S * D, scale,
                                                         w[0], w[2], cos, sin, S_TXT),
                "mx prep": lambda: ops.qkv_prep_mxfp8(qkv0, images, w[0], w[1], w[2], w[3], cos, sin, B, S, H, 3 * D, S_TXT),
                "mx attn": lambda: ops.attention_mxfp8(images, out_mx, B, S, H, D, S * D, scale)}
        for fn in runs.values():
            fn(); fn()
        torch.cuda.synchronize()
        # one consistent evaluation of both routes on the same projection: the format's own distance, not a kernel check
        qkv.copy_(qkv0); runs["bf16 prep"](); runs["bf16 attn"](); runs["mx prep"](); runs["mx attn"]()
        rel = ((out_mx[0, :1024].float() - out_bf[0, :1024].float()).pow(2).mean().sqrt() / out_bf[0, :1024].float().pow(2).mean().sqrt()).item()
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                for _ in range(args.repeats):
                    t[k].append(timed_window(fn, args.window))
        med = {k: statistics.median(v) for k, v in t.items()}
        fl = 4.0 * B * H * S * S * 128
        say(f"{B} {S} {H}")
        for k in runs:
            say(f"    {k:9s}: {med[k]:9.1f} us [{min(t[k]):9.1f} .. {max(t[k]):9.1f}]")
        bf, mx_ = med["bf16 prep"] + med["bf16 attn"], med["mx prep"] + med["mx attn"]
        say(f"    bf16 route {bf:9.1f} us ({fl / bf / 1e6:6.0f} TFLOP/s; kernel alone {fl / med['bf16 attn'] / 1e6:6.0f}) | mxfp8 route {mx_:9.1f} us "
            f"({fl / mx_ / 1e6:6.0f} TFLOP/s; kernel alone {fl / med['mx attn'] / 1e6:6.0f}) | mxfp8 / bf16 = {mx_ / bf:5.3f} | "
            f"rms(mx - bf16) / rms(bf16) = {rel:.4f}")
        del qkv, qkv0, vt, out_bf, out_mx, images
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
