"""The time from PNG file bytes on the host to RGB pixels on the device, on two routes: `png.decode_files` (csrc/png_dec.hip) and
`Image.open(...).convert("RGB")` + upload (Pillow / libpng + zlib on one core).  Inputs are the GPU encoder's own files of a
photographic test image (`png.encode`: what stages 2 and 3 write with --png gpu).  The routes are warmed up, interleaved in one process
and reported as the median (and the minimum) of --reps repeats, each ending in a device synchronise; the outputs are compared for
identity on every repeat, and every file must have taken the device route.
    python scripts/bench_png_decode.py [--sizes 1024x1024 2048x2048] [--batches 1 5] [--reps 20] [--log profiles/png_decode.log]"""
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
    """smooth colour fields, edges and sensor-like noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 80 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], axis=-1)
    base += 40 * ((xx // 64 + yy // 48) % 2)[..., None]
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1024x1024", "2048x2048"], help="WxH")
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 5])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    ge.build()
    from domain_rag_amd import png
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_decode.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    log = open(args.log, "a") if args.log else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if log:
            log.write(line + "\n"); log.flush()

    emit(dict(zip(("subseq_bytes", "subseqs_per_workgroup", "round_cap", "band_rows"), png.decode_geometry())))

    def pil_route(files):
        return [torch.from_numpy(np.array(Image.open(io.BytesIO(f)).convert("RGB"))).to(dev) for f in files]

    for s in args.sizes:
        w, h = (int(v) for v in s.split("x"))
        nmax = max(args.batches)
        distinct = []
        for i in range(nmax):
            distinct += png.encode(torch.from_numpy(photo(h, w, i)).to(dev))
        for n in args.batches:
            files = distinct[:n]
            for _ in range(3):                                         # warm-up of both (buffers grown, kernels loaded)
                pil_route(files); png.decode_files(files, dev)
            t = {"device": [], "pil": []}
            same, routes, rounds = True, set(), 0
            for _ in range(args.reps):
                torch.cuda.synchronize(); t0 = time.perf_counter(); b = png.decode_files(files, dev); torch.cuda.synchronize(); t["device"].append(time.perf_counter() - t0)
                torch.cuda.synchronize(); t0 = time.perf_counter(); pil = pil_route(files); torch.cuda.synchronize(); t["pil"].append(time.perf_counter() - t0)
                same = same and all(x is not None and torch.equal(x, y) for x, y in zip(b.images, pil))
                routes |= set(b.route)
                rounds = max(rounds, max(q["rounds"] for q in b.stats))
            emit({"size": f"{w}x{h}", "batch": n, "identical": bool(same), "routes": sorted(routes), "file_mb": round(len(files[0]) / 1e6, 2),
                  "device_ms_per_file": round(statistics.median(t["device"]) / n * 1e3, 3), "pil_upload_ms_per_file": round(statistics.median(t["pil"]) / n * 1e3, 3),
                  "device_min_ms": round(min(t["device"]) / n * 1e3, 3), "pil_min_ms": round(min(t["pil"]) / n * 1e3, 3),
                  "rounds_max": rounds, "subseqs_per_file": b.stats[0]["subsequences"], "reps": args.reps})


if __name__ == "__main__":
    main()
