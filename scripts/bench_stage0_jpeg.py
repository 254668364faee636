"""Stage 0's per-image wall clock with `--jpeg host` against `--jpeg gpu` (cli/stage0_lama.process_dataset on a synthetic k-shot
dataset of same-size JPEG frames, big-lama architecture with seeded weights): the number that decides the flag's default.  The two
routes alternate in one process, pass after pass; the first pass of each is the warm-up and is not counted.  The files of the two
routes are compared byte for byte.  A second JSON line times the steps of one image on their own (median of --reps, each ending in a
device synchronise): reading the source (PIL + upload, what stage 0 does | jpeg.decode_files on one file and on all --images files at once, which stage 0 does not use: this is the record of why), the generator (device call | PIL in / PIL out), writing
(device encode + write | copy back + Image.save).  With `--source gpu` a third route joins the alternating passes: `--jpeg gpu --source gpu`
(the source decoded on the device by the parallel entropy route), compared with `--jpeg gpu --source host` under the same rule.
    python scripts/bench_stage0_jpeg.py [--size 504x376] [--images 16] [--passes 4] [--tiny] [--source gpu]"""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def photo(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 37.0 + k) * np.cos(yy / 23.0 - k) for k in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="504x376", help="WxH")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4, help="timed passes per route (one more, the first, is the warm-up)")
    ap.add_argument("--reps", type=int, default=20, help="repeats per step of the breakdown")
    ap.add_argument("--tiny", action="store_true", help="tiny generator (rehearsal)")
    ap.add_argument("--source", choices=["host", "gpu"], default="host", help="gpu: also time --jpeg gpu --source gpu in the alternating passes")
    args = ap.parse_args()
    ge.build()
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("bench_stage0_jpeg.py measures on the GPU; none is visible")
    os.environ["DRAG_SYNTHETIC_WEIGHTS"] = "1"
    if args.tiny:
        os.environ["DRAG_TINY"] = "1"
    from domain_rag_amd.cli import stage0_lama as s0
    from domain_rag_amd.lama import SimpleLama
    w, h = (int(v) for v in args.size.split("x"))
    ds = "bench"
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "lama_inpaint"))
        os.makedirs(os.path.join(root, "datasets", ds, "annotations"))
        os.makedirs(os.path.join(root, "datasets", ds, "train"))
        images, anns = [], []
        for i in range(args.images):
            name = f"img_{i:03d}.jpg"
            Image.fromarray(photo(h, w, i)).save(os.path.join(root, "datasets", ds, "train", name), quality=90)
            images.append({"id": i + 1, "file_name": name, "width": w, "height": h})
            anns.append({"id": i + 1, "image_id": i + 1, "bbox": [w // 4, h // 4, w // 3, h // 3], "category_id": 1})
        with open(os.path.join(root, "datasets", ds, "annotations", "1_shot.json"), "w") as f:
            json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "thing"}]}, f)
        os.chdir(os.path.join(root, "lama_inpaint"))
        logger = logging.getLogger("bench_stage0_jpeg"); logger.addHandler(logging.NullHandler()); logger.propagate = False
        model = SimpleLama()
        out_dir = os.path.join(root, "lamainpaint", ds, "1_shot")
        routes = {"host": ("host", "host"), "gpu": ("gpu", "host")}              # name -> (--jpeg, --source)
        if args.source == "gpu":
            routes["gpu_source_gpu"] = ("gpu", "gpu")
        times = {r: [] for r in routes}
        files = {}
        for p in range(args.passes + 1):
            for route, (jpeg_route, source_route) in routes.items():
                torch.cuda.synchronize(); t = time.perf_counter()
                done, failed = s0.process_dataset(ds, "1", logger, model, jpeg=jpeg_route, source=source_route)
                torch.cuda.synchronize(); dt = time.perf_counter() - t
                assert (done, failed) == (args.images, 0), (route, done, failed)
                files[route] = {n: open(os.path.join(out_dir, n), "rb").read() for n in sorted(os.listdir(out_dir))}
                if p > 0:
                    times[route].append(dt / args.images * 1e3)
        # the steps of one image, each on its own
        import io
        from domain_rag_amd import hostlogic as H, jpeg
        dev = model.device
        src = os.path.join(root, "datasets", ds, "train", images[0]["file_name"])
        data = open(src, "rb").read()
        all_data = [open(os.path.join(root, "datasets", ds, "train", im["file_name"]), "rb").read() for im in images]
        mask = H.inpaint_mask_array(w, h, [anns[0]["bbox"]])
        tmp_out = os.path.join(root, "step.jpg")

        def med(fn):
            fn(); fn()
            v = []
            for _ in range(args.reps):
                torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); v.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(v), 3)

        def read_pil():
            return torch.from_numpy(np.array(Image.open(src).convert("RGB"))).to(dev)

        def write_device():
            with open(tmp_out, "wb") as f:
                f.write(jpeg.encode(frame)[0])

        img_dev, mask_dev = read_pil(), torch.from_numpy(mask).to(dev)
        frame = model.model(img_dev, mask_dev)
        pil_img, pil_mask = Image.open(src).convert("RGB"), Image.fromarray(mask, mode="L")
        steps = {"read_pil_open_upload_ms": med(read_pil),
                 "read_device_decode_ms": med(lambda: jpeg.decode_files([data], dev).image(0)),
                 "read_device_decode_batch_ms_per_file": round(med(lambda: jpeg.decode_files(all_data, dev)) / len(all_data), 3),
                 "read_device_decode_parallel_ms": med(lambda: jpeg.decode_files([data], dev, entropy="parallel").image(0)),
                 "read_stage_paths_decode_parallel_ms": med(lambda: jpeg.decode_files(jpeg.stage_paths([src], dev), dev, entropy="parallel").image(0)),
                 "mask_build_upload_ms": med(lambda: torch.from_numpy(H.inpaint_mask_array(w, h, [anns[0]["bbox"]])).to(dev)),
                 "lama_device_in_device_out_ms": med(lambda: model.model(img_dev, mask_dev)),
                 "lama_pil_in_pil_out_ms": med(lambda: model(pil_img, pil_mask)),
                 "write_device_encode_ms": med(write_device),
                 "write_copy_back_pil_save_ms": med(lambda: Image.fromarray(frame.cpu().numpy()).save(tmp_out))}
        os.chdir("/")
    host, gpu = statistics.median(times["host"]), statistics.median(times["gpu"])
    line = {"size": f"{w}x{h}", "images": args.images, "passes": args.passes, "tiny": args.tiny, "identical": all(f == files["host"] for f in files.values()),
            "host_ms_per_image": round(host, 3), "gpu_ms_per_image": round(gpu, 3),
            "host_all": [round(v, 3) for v in times["host"]], "gpu_all": [round(v, 3) for v in times["gpu"]],
            "default_gpu_allowed": gpu <= host}
    if "gpu_source_gpu" in times:                  # --source's rule is --jpeg's: gpu only if its wall clock is not above host's in the same run
        sg = statistics.median(times["gpu_source_gpu"])
        line.update({"source_gpu_ms_per_image": round(sg, 3), "source_gpu_all": [round(v, 3) for v in times["gpu_source_gpu"]],
                     "source_default_gpu_allowed": sg <= gpu})
    print(json.dumps(line), flush=True)
    print(json.dumps({"size": f"{w}x{h}", "reps": args.reps, "decode_batch": len(all_data), "source_file_kb": round(len(data) / 1e3, 1), **steps}), flush=True)


if __name__ == "__main__":
    main()
