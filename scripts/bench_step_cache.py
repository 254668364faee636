"""What the first-block step cache (flux.StepCache) costs and saves on the headline workload: SyntheticFillJob (B = 8, 1024^2, 30 Flux-Fill
steps), one process, the passes interleaved round by round:

  off                the product's default path (hipGraph replay, no cache)
  compute_every      cache on, ``forced`` = compute every step: the cache's own overhead (eager forward, two copies, delta, capture, one sync)
  compute_every_2nd  ``forced`` = compute steps 0, 2, 4, ...; reuse the others
  compute_every_3rd  ``forced`` = compute steps 0, 3, 6, ...
  inf                threshold inf: 1 computed step + 29 reused

Per pass: wall time per batch, GPU time of a computed and of a reused step (events after every step's Euler update), the per-step ratio
trace, and the distance of its result from the off pass (rms of the final packed latents, mean absolute uint8 level).  The two kernels are
also timed alone at the workload's shape.  The weights are seeded random: the ratios and distances say nothing about real checkpoints.

    python scripts/bench_step_cache.py [--out-dir profiles]      # writes step_cache.json and step_cache.log there"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from domain_rag_amd import ops  # noqa: E402
from domain_rag_amd.fill_pipeline import SyntheticFillJob  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--denoise-steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2, help="timed rounds; every round runs each pass once, in order (one warm-up round first)")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    n = args.denoise_steps
    job = SyntheticFillJob(batch=args.batch, res=args.res, denoise_steps=n, device=dev)
    # (threshold, forced): forced[i] is the value `reused` takes in step i
    passes = {"off": (None, None),
              "compute_every": (math.inf, [False] * n),
              "compute_every_2nd": (math.inf, [i % 2 != 0 for i in range(n)]),
              "compute_every_3rd": (math.inf, [i % 3 != 0 for i in range(n)]),
              "inf": (math.inf, None)}
    os.makedirs(args.out_dir, exist_ok=True)
    log = open(os.path.join(args.out_dir, "step_cache.log"), "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n"); log.flush()

    def run(name):
        thr, forced = passes[name]
        job.fill.step_cache, job.fill.step_cache_forced = thr, forced
        marks, last = [], {}

        def on_step(i, latents):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append(ev)
            last["latents"] = latents
        pe, pp = job.prior(job.bg, job.t5, job.pooled, [job.ips], [1.0], group=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = job.fill(job.image, job.mask, pe, pp, guidance_scale=job.guidance, num_inference_steps=n, strength=job.strength,
                       enc_noise=job.enc_noise, masked_enc_noise=job.menc_noise, noise_tokens=job.noise_tokens,
                       on_step=on_step)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        # step i's GPU time = from the mark after step i - 1 to the mark after step i (step 0 also holds the VAE encodes: left out)
        step_ms = [None] + [marks[i - 1].elapsed_time(marks[i]) for i in range(1, len(marks))]
        dec = job.fill.last_step_decisions
        return dict(wall_s=wall, step_ms=step_ms, decisions=dec, out=out, latents=last["latents"])

    say(f"# bench_step_cache: B = {args.batch}, {args.res}^2, {n} steps, {args.rounds} timed rounds after one warm-up round; seeded random weights")
    say(f"# device: {torch.cuda.get_device_name(0)}")
    results = {k: [] for k in passes}
    for rnd in range(args.rounds + 1):
        for name in passes:
            r = run(name)
            if rnd == 0:
                continue
            results[name].append(r)
            reused = [bool(d.reused) for d in r["decisions"]] if r["decisions"] else [False] * n
            comp = [t for t, u in zip(r["step_ms"], reused) if t is not None and not u]
            reu = [t for t, u in zip(r["step_ms"], reused) if t is not None and u]
            say(f"round {rnd} {name:18s} wall {r['wall_s']:7.3f} s/batch  computed steps {len(comp) + (0 if reused[0] else 1):2d}"
                f" ({statistics.median(comp) if comp else float('nan'):8.2f} ms median)  reused steps {len(reu):2d}"
                f" ({statistics.median(reu) if reu else float('nan'):8.2f} ms median)")

    # ---- the two kernels alone at the workload's shape (the joint buffer's addressing: text rows in front)
    B, Si, St, D = args.batch, job.Si, job.St, job.cfg.dim
    S = St + Si
    x = torch.randn((B, S, D), device=dev).bfloat16()
    E, F, R = (torch.randn((B, Si, D), device=dev).bfloat16() for _ in range(3))
    ratios = torch.empty(B, dtype=torch.float64, device=dev)
    wsp = torch.empty(ops.stepcache_workspace_bytes(B, Si, D), dtype=torch.uint8, device=dev)
    x_img = x.view(-1)[St * D:]

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    mb = B * Si * D * 2 / 1e6
    kern = {"stepcache_delta (with ratio: reads x, e, f, writes e)": (timed(lambda: ops.stepcache_delta(x_img, E, F, ratios, wsp, B, Si, D, S * D)), 4 * mb),
            "stepcache_delta (f = null: reads x, e, writes e)": (timed(lambda: ops.stepcache_delta(x_img, E, None, None, None, B, Si, D, S * D)), 3 * mb),
            "stepcache_apply +1 (reads x, r, writes x)": (timed(lambda: ops.stepcache_apply(x_img, R, B, Si, D, S * D, +1)), 3 * mb),
            "stepcache_apply -1 (reads x, r, writes r)": (timed(lambda: ops.stepcache_apply(x_img, R, B, Si, D, S * D, -1)), 3 * mb)}
    say()
    say(f"# kernels alone, B = {B}, {Si} x {D} image rows per batch inside [{B}, {S}, {D}] ({mb:.0f} MB per operand)")
    for k, (ms, traffic) in kern.items():
        say(f"{k:58s} {ms:7.4f} ms  {traffic / ms / 1e3:6.2f} TB/s")

    # ---- summary
    def med(name, key):
        return statistics.median(r[key] for r in results[name])
    off = results["off"][-1]
    summary = {"config": dict(batch=B, res=args.res, denoise_steps=n, rounds=args.rounds, device=torch.cuda.get_device_name(0), weights="seeded random"),
               "kernels_ms": {k: v[0] for k, v in kern.items()}, "passes": {}}
    say()
    say("# per pass: median wall per batch; distance of the last round's result from the off pass")
    for name in passes:
        r = results[name][-1]
        reused = [bool(d.reused) for d in r["decisions"]] if r["decisions"] else [False] * n
        comp = [t for rr in results[name] for t, u in zip(rr["step_ms"], reused) if t is not None and not u]
        reu = [t for rr in results[name] for t, u in zip(rr["step_ms"], reused) if t is not None and u]
        dl = (r["latents"].double() - off["latents"].double())
        lat_rms = dl.pow(2).mean().sqrt().item()
        lat_rel = lat_rms / off["latents"].double().pow(2).mean().sqrt().item()
        lvl = (r["out"].float() - off["out"].float()).abs().mean().item()
        trace = None if r["decisions"] is None else [None if d.ratios is None else [float(v) for v in d.ratios] for d in r["decisions"]]
        summary["passes"][name] = dict(wall_s_per_batch=[rr["wall_s"] for rr in results[name]], wall_s_median=med(name, "wall_s"),
                                       images_per_s=B / med(name, "wall_s"), computed_steps=reused.count(False), reused_steps=reused.count(True),
                                       computed_step_ms_median=statistics.median(comp) if comp else None,
                                       reused_step_ms_median=statistics.median(reu) if reu else None,
                                       final_latents_rms_vs_off=lat_rms, final_latents_rms_rel_vs_off=lat_rel, mean_abs_uint8_level_vs_off=lvl,
                                       ratio_trace=trace)
        say(f"{name:18s} {med(name, 'wall_s'):7.3f} s/batch ({B / med(name, 'wall_s'):.4f} images/s, {med(name, 'wall_s') / med('off', 'wall_s'):.3f} x off)"
            f"  latents rms vs off {lat_rms:.4e} (relative {lat_rel:.4e})  mean |uint8 level| vs off {lvl:.3f}")
    say()
    say("# per-step ratio trace (maximum over the batch), last round")
    for name in passes:
        d = results[name][-1]["decisions"]
        if d:
            say(f"{name:18s} " + " ".join("  -  " if x.ratios is None else f"{max(x.ratios):5.3f}" for x in d))
    with open(os.path.join(args.out_dir, "step_cache.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    log.close()


if __name__ == "__main__":
    main()
