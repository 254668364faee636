"""stage 3's per-sample wall clock with --pictures host against --pictures device, in one process on one tiny engine (seeded weights),
alternating passes over a synthetic mini dataset: every sample has --bgs backgrounds of --bg_size pixels written by the GPU PNG
encoder (what stage 2 leaves with --png gpu) and an original that is upscaled, so both the background decode and the resize back are
on the path.  The first pass of each setting is a warm-up and is not counted.  Prints one JSON line per pass and a summary line; the
rule for stage3_outpaint.PICTURES_DEFAULT reads the summary.
    python scripts/bench_stage3_pictures.py [--samples 4] [--bgs 5] [--bg_size 1024] [--passes 4] [--log profiles/stage3_pictures.log]"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 80 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--bgs", type=int, default=5)
    ap.add_argument("--bg_size", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=4, help="counted passes per setting (one more, uncounted, warms up)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    log_path = os.path.abspath(a.log) if a.log else None
    ge.build()
    from domain_rag_amd import png
    from domain_rag_amd.cli import stage3_outpaint as s3
    from domain_rag_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage3_pictures.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="stage3_pictures_")
    os.chdir(root)
    ds = "DIOR"
    os.makedirs(f"datasets/{ds}/annotations"); os.makedirs(f"datasets/{ds}/train")
    images, anns, sdirs = [], [], {}
    for i in range(a.samples):
        name = f"s_{i}"
        Image.fromarray(photo(48, 72, i)).save(f"datasets/{ds}/train/{name}.jpg")
        images.append({"id": i + 1, "file_name": f"{name}.jpg", "width": 72, "height": 48})
        anns.append({"id": i + 1, "image_id": i + 1, "bbox": [10, 8, 20, 16], "category_id": 1})
        sdirs[name] = f"result/{ds}_1shot_retrieval/results_x/{name}"
        os.makedirs(sdirs[name])
        for r in range(a.bgs):
            with open(f"{sdirs[name]}/generated_image_rank{r + 1}.png", "wb") as f:
                f.write(png.encode(torch.from_numpy(photo(a.bg_size, a.bg_size, 100 * i + r)).to(dev))[0])
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "airplane"}]}, open(f"datasets/{ds}/annotations/1_shot.json", "w"))
    engine = Engine("fill", synthetic=True, tiny=True, device=dev)
    times = {"host": [], "device": []}
    out = open(log_path, "a") if log_path else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n"); out.flush()

    for p in range(a.passes + 1):
        for setting in (("host", "device") if p % 2 == 0 else ("device", "host")):          # alternate, and alternate who goes first
            args = s3.build_parser().parse_args(["--dataset", ds, "--shot", "1", "--synthetic-weights", "--tiny", "--num_inference_steps", "2",
                                                 "--io_workers", "0", "--pictures", setting])
            rng = random.Random(5)
            per = []
            for name in sorted(sdirs):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    lg = s3.process_sample(engine, args, ds, name, sdirs[name], 1, f"{setting}{p}", rng, None)
                torch.cuda.synchronize(); per.append(time.perf_counter() - t0)
                assert lg["status"] == "completed", lg.get("error")
            if p > 0:
                times[setting] += per
            emit({"pass": p, "counted": p > 0, "pictures": setting, "ms_per_sample": [round(v * 1e3, 2) for v in per]})
    emit({"summary": True, "samples": a.samples, "bgs": a.bgs, "bg_size": a.bg_size, "passes": a.passes,
          "host_ms_per_sample_median": round(statistics.median(times["host"]) * 1e3, 2), "device_ms_per_sample_median": round(statistics.median(times["device"]) * 1e3, 2),
          "host_ms_per_sample_mean": round(statistics.mean(times["host"]) * 1e3, 2), "device_ms_per_sample_mean": round(statistics.mean(times["device"]) * 1e3, 2)})


if __name__ == "__main__":
    main()
