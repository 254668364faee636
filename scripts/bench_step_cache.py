"""What the first-block step cache (step_cache.StepCache) costs and saves on the headline workload: SyntheticFillJob (B = 8, 1024^2, 30 Flux-Fill
steps), one process, the passes interleaved round by round:

  off                the product's default path (hipGraph replay, no cache)
  compute_every      cache on, ``forced`` = compute every step: the cache's own overhead (eager forward, two copies, delta, capture, one sync)
  compute_every_2nd  ``forced`` = compute steps 0, 2, 4, ...; reuse the others
  compute_every_3rd  ``forced`` = compute steps 0, 3, 6, ...
  inf                threshold inf: 1 computed step + 29 reused

Per pass: wall time per batch, GPU time of a computed and of a reused step (events after every step's Euler update), the per-step ratio
trace, and the distance of its result from the off pass (rms of the final packed latents, mean absolute uint8 level).  The two kernels are
also timed alone at the workload's shape.  The weights are seeded random: the ratios and distances say nothing about real checkpoints.

    python scripts/bench_step_cache.py [--out-dir profiles]      # writes step_cache.json and step_cache.log there

``--scope image`` measures the cache's scope "image" instead (every image decides for itself; a step on which k of B images compute runs
the remaining blocks at batch k): per step, a forced pattern in which the LAST k images compute (the most swaps) under scope "image"
against the same pattern under scope "batch", where any computing image makes all B compute.  Passes k = 0, B/4, B/2, 3B/4, B under
"image" and k = 0, B under "batch", interleaved round by round in one process; the swaps and list kernels of a mixed step are also timed
alone.  Writes step_cache_image.json and step_cache_image.log.

``--order 1`` measures the first-order forecast of a reused step (``StepCache(order=1)``) against order 0: the forced patterns "every 2nd"
and "every 3rd step computed", each at order 0 and order 1, and the off pass, interleaved round by round in one process — wall per
batch, the reused step's GPU time, the distance of the final latents from the off pass — and the forecast kernel next to ``apply(+1)``
alone.  Writes step_cache_forecast.json and step_cache_forecast.log."""
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
    ap.add_argument("--scope", choices=["batch", "image"], default="batch", help="image: measure mixed steps of the cache's scope \"image\"")
    ap.add_argument("--order", type=int, choices=[0, 1], default=0, help="1: measure the first-order forecast of a reused step against order 0")
    args = ap.parse_args(argv)
    if args.order == 1:
        return main_order(args)
    if args.scope == "image":
        return main_image(args)
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


def main_image(args):
    from domain_rag_amd.flux import compact_pairs
    dev = torch.device("cuda:0")
    n, B = args.denoise_steps, args.batch
    job = SyntheticFillJob(batch=B, res=args.res, denoise_steps=n, device=dev)
    ks = sorted({0, B // 4, B // 2, 3 * B // 4, B})
    # pass -> (scope, k): from step 1 on the last k images compute; under "batch" any computing image makes all compute
    passes = {"batch_k0": ("batch", 0), f"batch_k{B}": ("batch", B)}
    passes.update({f"image_k{k}": ("image", k) for k in ks})
    os.makedirs(args.out_dir, exist_ok=True)
    log = open(os.path.join(args.out_dir, "step_cache_image.log"), "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n"); log.flush()

    def run(name):
        scope, k = passes[name]
        mask = tuple(b < B - k for b in range(B))          # True = reuses
        job.fill.step_cache, job.fill.step_cache_scope = math.inf, scope
        job.fill.step_cache_forced = [False] + [k == 0] * (n - 1) if scope == "batch" else None
        job.fill.step_cache_forced_images = [(False,) * B] + [mask] * (n - 1) if scope == "image" else None
        marks = []

        def on_step(i, latents):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append(ev)
        pe, pp = job.prior(job.bg, job.t5, job.pooled, [job.ips], [1.0], group=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job.fill(job.image, job.mask, pe, pp, guidance_scale=job.guidance, num_inference_steps=n, strength=job.strength,
                 enc_noise=job.enc_noise, masked_enc_noise=job.menc_noise, noise_tokens=job.noise_tokens, on_step=on_step)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        got = job.fill.last_step_reused_images
        want = [(False,) * B] + [mask if scope == "image" else (k == 0,) * B] * (n - 1)
        assert got == want, (name, got)
        # steps 2 ... n - 1: the forced pattern in its steady state (step 0 also holds the VAE encodes, step 1 follows the all-compute step)
        return dict(wall_s=wall, step_ms=[marks[i - 1].elapsed_time(marks[i]) for i in range(2, len(marks))])

    say(f"# bench_step_cache --scope image: B = {B}, {args.res}^2, {n} steps, {args.rounds} timed rounds after one warm-up round; seeded random weights")
    say(f"# device: {torch.cuda.get_device_name(0)}")
    say("# per pass and round: median GPU time of a step of the forced pattern (steps 2 ... n - 1), wall per batch")
    results = {name: [] for name in passes}
    for rnd in range(args.rounds + 1):
        for name in passes:
            r = run(name)
            if rnd == 0:
                continue
            results[name].append(r)
            say(f"round {rnd} {name:10s} step {statistics.median(r['step_ms']):8.2f} ms median (min {min(r['step_ms']):8.2f}, max {max(r['step_ms']):8.2f})"
                f"  wall {r['wall_s']:7.3f} s/batch")

    # ---- the swaps and list kernels of one mixed step alone, at the workload's shape
    Si, St, D, LM = job.Si, job.St, job.cfg.dim, job.fill.tr.mod_total
    S = St + Si
    x = torch.randn((B, S, D), device=dev).bfloat16()
    mod = torch.randn((B, LM), device=dev).bfloat16()
    E, F, R = (torch.randn((B, Si, D), device=dev).bfloat16() for _ in range(3))
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
        return e0.elapsed_time(e1) / reps * 1e3
    kern = {}
    say()
    say(f"# kernels of a mixed step alone (us), B = {B}, {Si} x {D} image rows + {St} text rows per image, modulation rows of {LM}")
    for k in [k for k in ks if 0 < k < B]:
        mask = tuple(b < B - k for b in range(B))
        C, U = [b for b in range(B) if not mask[b]], [b for b in range(B) if mask[b]]
        _, pairs = compact_pairs(mask)
        kern[k] = {"copy_images E -> F (computing)": timed(lambda: ops.stepcache_copy_images(F, E, Si * D, B, Si, D, C)),
                   "copy_images x_img -> R (computing)": timed(lambda: ops.stepcache_copy_images(R, x_img, S * D, B, Si, D, C)),
                   "apply_images +1 (reusing)": timed(lambda: ops.stepcache_apply_images(x_img, R, B, Si, D, S * D, +1, U)),
                   "swap x, joint rows": timed(lambda: ops.stepcache_swap(x, B, S, D, S * D, pairs)),
                   "swap mod (twice per step)": timed(lambda: ops.stepcache_swap(mod, B, 1, LM, LM, pairs)),
                   "swap x back, image rows": timed(lambda: ops.stepcache_swap(x_img, B, Si, D, S * D, pairs)),
                   "apply_images -1 (computing)": timed(lambda: ops.stepcache_apply_images(x_img, R, B, Si, D, S * D, -1, C))}
        total = sum(kern[k].values()) + kern[k]["swap mod (twice per step)"]
        kern[k]["total per mixed step"] = total
        say(f"k = {k} ({len(pairs)} pairs): " + "; ".join(f"{name} {us:.1f}" for name, us in kern[k].items()))
    whole = {"R.copy_(x_img) of a computed step": timed(lambda: R.copy_(x[:, St:])),
             "apply -1 of a computed step": timed(lambda: ops.stepcache_apply(x_img, R, B, Si, D, S * D, -1)),
             "apply +1 of a reused step": timed(lambda: ops.stepcache_apply(x_img, R, B, Si, D, S * D, +1))}
    say("whole-batch counterparts: " + "; ".join(f"{name} {us:.1f}" for name, us in whole.items()))

    # ---- summary
    def steps(name):
        return [t for r in results[name] for t in r["step_ms"]]
    summary = {"config": dict(batch=B, res=args.res, denoise_steps=n, rounds=args.rounds, device=torch.cuda.get_device_name(0), weights="seeded random"),
               "passes": {name: dict(scope=passes[name][0], computing_images=passes[name][1], step_ms_median_per_round=[statistics.median(r["step_ms"]) for r in results[name]],
                                     step_ms_median=statistics.median(steps(name)), step_ms_min=min(steps(name)), step_ms_max=max(steps(name)),
                                     wall_s_per_batch=[r["wall_s"] for r in results[name]]) for name in passes},
               "mixed_step_kernels_us": {str(k): v for k, v in kern.items()}, "whole_batch_kernels_us": whole}
    say()
    say("# summary: median step over all timed rounds; image_k vs the all-compute step of scope batch, round by round")
    full = f"batch_k{B}"
    for name in passes:
        per_round = [statistics.median(r["step_ms"]) / statistics.median(f["step_ms"]) for r, f in zip(results[name], results[full])]
        summary["passes"][name]["vs_all_compute_per_round"] = per_round
        say(f"{name:10s} {statistics.median(steps(name)):8.2f} ms  (x all-compute, per round: " + ", ".join(f"{v:.3f}" for v in per_round) + ")")
    with open(os.path.join(args.out_dir, "step_cache_image.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    log.close()


def main_order(args):
    dev = torch.device("cuda:0")
    n, B = args.denoise_steps, args.batch
    job = SyntheticFillJob(batch=B, res=args.res, denoise_steps=n, device=dev)
    # pass -> (order, forced): forced[i] is the value `reused` takes in step i; None = the cache is off
    patterns = {"every_2nd": [i % 2 != 0 for i in range(n)], "every_3rd": [i % 3 != 0 for i in range(n)]}
    passes = {"off": (0, None)}
    for pname, forced in patterns.items():
        for order in (0, 1):
            passes[f"{pname}_order{order}"] = (order, forced)
    os.makedirs(args.out_dir, exist_ok=True)
    log = open(os.path.join(args.out_dir, "step_cache_forecast.log"), "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n"); log.flush()

    def run(name):
        order, forced = passes[name]
        job.fill.step_cache, job.fill.step_cache_forced = (None if forced is None else math.inf), forced
        job.fill.step_cache_scope, job.fill.step_cache_forced_images, job.fill.step_cache_order = "batch", None, order
        marks, last = [], {}

        def on_step(i, latents):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append(ev)
            last["latents"] = latents
        pe, pp = job.prior(job.bg, job.t5, job.pooled, [job.ips], [1.0], group=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        job.fill(job.image, job.mask, pe, pp, guidance_scale=job.guidance, num_inference_steps=n, strength=job.strength,
                 enc_noise=job.enc_noise, masked_enc_noise=job.menc_noise, noise_tokens=job.noise_tokens, on_step=on_step)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        step_ms = [None] + [marks[i - 1].elapsed_time(marks[i]) for i in range(1, len(marks))]
        reused = [False] * n if forced is None else [bool(d.reused) for d in job.fill.last_step_decisions]
        fc = job.fill.last_step_forecasts
        return dict(wall_s=wall, reused_ms=[t for t, u in zip(step_ms, reused) if t is not None and u], latents=last["latents"],
                    forecast_steps=0 if fc is None else sum(1 for f in fc if f[0] is not None),
                    coefficients=None if fc is None else [f[0] for f in fc])

    say(f"# bench_step_cache --order 1: B = {B}, {args.res}^2, {n} steps, {args.rounds} timed rounds after one warm-up round; seeded random weights")
    say(f"# device: {torch.cuda.get_device_name(0)}")
    results = {k: [] for k in passes}
    for rnd in range(args.rounds + 1):
        for name in passes:
            r = run(name)
            if rnd == 0:
                continue
            results[name].append(r)
            ru = r["reused_ms"]
            say(f"round {rnd} {name:18s} wall {r['wall_s']:7.3f} s/batch  reused steps {len(ru):2d} (forecast on {r['forecast_steps']:2d})"
                + (f"  median {statistics.median(ru):7.3f} ms (min {min(ru):7.3f}, max {max(ru):7.3f})" if ru else ""))

    # ---- the forecast kernel next to apply(+1), alone, at the workload's shape (the joint buffer's addressing: text rows in front)
    Si, St, D = job.Si, job.St, job.cfg.dim
    S = St + Si
    x = torch.randn((B, S, D), device=dev).bfloat16()
    R, P = (torch.randn((B, Si, D), device=dev).bfloat16() for _ in range(2))
    x_img = x.view(-1)[St * D:]
    every, coefs = list(range(B)), [1.0 + 0.125 * b for b in range(B)]

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
    kern = {}
    for rep in range(3):          # three alternating measurements of each
        for k, fn, traffic in (("stepcache_apply +1 (reads x, r, writes x)", lambda: ops.stepcache_apply(x_img, R, B, Si, D, S * D, +1), 3 * mb),
                               ("stepcache_forecast_images (reads x, r, p, writes x)",
                                lambda: ops.stepcache_forecast_images(x_img, R, P, B, Si, D, S * D, every, coefs), 4 * mb)):
            x.normal_()           # keep x finite over the repetitions
            kern.setdefault(k, dict(ms=[], traffic_mb=traffic))["ms"].append(timed(fn))
    say()
    say(f"# kernels alone, B = {B}, {Si} x {D} image rows per batch inside [{B}, {S}, {D}] ({mb:.0f} MB per operand), 3 x 20 launches each")
    for k, v in kern.items():
        ms = statistics.median(v["ms"])
        say(f"{k:54s} {ms:7.4f} ms median (min {min(v['ms']):.4f}, max {max(v['ms']):.4f})  {v['traffic_mb'] / ms / 1e3:6.2f} TB/s")
    ka, kf = (statistics.median(v["ms"]) for v in kern.values())
    say(f"forecast / apply: {kf / ka:.3f} (4/3 by the operands read and written)")

    # ---- summary: order 1 against the order-0 pass of the same run; distances from the off pass, recorded without a claim
    off = results["off"][-1]["latents"].double()
    off_rms = off.pow(2).mean().sqrt().item()
    summary = {"config": dict(batch=B, res=args.res, denoise_steps=n, rounds=args.rounds, device=torch.cuda.get_device_name(0), weights="seeded random"),
               "kernels_ms": {k: v["ms"] for k, v in kern.items()}, "forecast_over_apply": kf / ka, "passes": {}}
    say()
    say("# per pass: wall per batch and reused step over all timed rounds; rms distance of the last round's final latents from the off pass, relative")
    for name in passes:
        rs = results[name]
        walls = [r["wall_s"] for r in rs]
        ru = [t for r in rs for t in r["reused_ms"]]
        rel = (rs[-1]["latents"].double() - off).pow(2).mean().sqrt().item() / off_rms
        summary["passes"][name] = dict(order=passes[name][0], wall_s_per_batch=walls, wall_s_median=statistics.median(walls), wall_s_min=min(walls),
                                       wall_s_max=max(walls), reused_steps=len(rs[-1]["reused_ms"]), forecast_steps=rs[-1]["forecast_steps"],
                                       reused_step_ms_median=statistics.median(ru) if ru else None, reused_step_ms_min=min(ru) if ru else None,
                                       reused_step_ms_max=max(ru) if ru else None, final_latents_rms_rel_vs_off=rel, coefficients=rs[-1]["coefficients"])
        say(f"{name:18s} wall {statistics.median(walls):7.3f} s/batch (min {min(walls):7.3f}, max {max(walls):7.3f})"
            + (f"  reused step {statistics.median(ru):7.3f} ms (min {min(ru):7.3f}, max {max(ru):7.3f})" if ru else " " * 53)
            + f"  latents rms vs off, relative {rel:.4e}")
    say()
    say("# order 1 - order 0, same pattern, same run (the order-0 pass is the reference; its own min-max spread next to it)")
    for pname in patterns:
        a, b = summary["passes"][f"{pname}_order0"], summary["passes"][f"{pname}_order1"]
        d_wall, d_step = b["wall_s_median"] - a["wall_s_median"], b["reused_step_ms_median"] - a["reused_step_ms_median"]
        spread_wall, spread_step = a["wall_s_max"] - a["wall_s_min"], a["reused_step_ms_max"] - a["reused_step_ms_min"]
        summary["passes"][f"{pname}_order1"]["vs_order0"] = dict(wall_s=d_wall, wall_s_spread_of_order0=spread_wall, reused_step_ms=d_step,
                                                               reused_step_ms_spread_of_order0=spread_step)
        say(f"{pname:10s} wall {d_wall:+8.4f} s/batch (order 0 spread {spread_wall:.4f})  reused step {d_step:+8.4f} ms (order 0 spread {spread_step:.4f})"
            f"  {'within' if abs(d_wall) <= spread_wall else 'OUTSIDE'} the wall spread, {'within' if abs(d_step) <= spread_step else 'OUTSIDE'} the step spread")
    say()
    say("# the weights are seeded random and adjacent steps differ by first-block ratios of 0.4 - 0.6: the distances above say nothing about real checkpoints")
    with open(os.path.join(args.out_dir, "step_cache_forecast.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    log.close()


if __name__ == "__main__":
    main()
