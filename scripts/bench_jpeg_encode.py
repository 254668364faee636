"""GPU JPEG encoder (`jpeg.encode`) against the route it replaces in stage 0: `frame.cpu()` -> `Image.fromarray` -> `save` to BytesIO
(Pillow / libjpeg-turbo on one core).  Both routes start from a uint8 frame on the device and end in host bytes; both are warmed
up, interleaved in one process, and reported as the median of --reps repeats.  The files are compared byte for byte first.
    python scripts/bench_jpeg_encode.py [--sizes 504x376 512x512 1024x768 2096x2800] [--batches 1 8] [--reps 20]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def host_route(frames):
    """the parent's route: copy to the host, Pillow compresses image after image"""
    arr = frames.cpu().numpy()
    out = []
    for a in arr:
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, "JPEG")
        out.append(bio.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["504x376", "512x512", "1024x768", "2096x2800"], help="WxH")
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    ge.build()
    from domain_rag_amd import jpeg
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for s in args.sizes:
        w, h = (int(v) for v in s.split("x"))
        for n in args.batches:
            frames = torch.from_numpy(np.stack([photo(h, w, i) for i in range(n)])).to(dev)
            same = jpeg.encode(frames) == host_route(frames)          # (also the warm-up of both routes)
            jpeg.encode(frames); host_route(frames)
            t_gpu, t_host = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize(); t = time.perf_counter(); files = jpeg.encode(frames); t_gpu.append(time.perf_counter() - t)
                torch.cuda.synchronize(); t = time.perf_counter(); host_route(frames); t_host.append(time.perf_counter() - t)
            g, p = statistics.median(t_gpu) / n * 1e3, statistics.median(t_host) / n * 1e3
            print(json.dumps({"size": f"{w}x{h}", "batch": n, "identical": same, "gpu_ms_per_image": round(g, 3), "host_ms_per_image": round(p, 3),
                              "gpu_min_ms": round(min(t_gpu) / n * 1e3, 3), "host_min_ms": round(min(t_host) / n * 1e3, 3),
                              "speedup": round(p / g, 2), "file_kb": round(len(files[0]) / 1e3, 1), "reps": args.reps}), flush=True)


if __name__ == "__main__":
    main()
