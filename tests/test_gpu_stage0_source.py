"""Stage 0 with ``--source gpu`` (a .jpg source is decoded on the device by the parallel entropy route and handed to LamaHIP without
leaving it) against ``--source host`` (PIL opens every file: the reference's lama_inpaint/lama_inpaint.py:159-170): the same files, byte
for byte, and every source on the route the CLI documents for it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = "ArTaxOr"


def _run_stage0(cwd, extra):
    env = dict(os.environ, PYTHONPATH=ROOT, DRAG_TIMESTAMP="20260101_000000")
    r = subprocess.run([sys.executable, "-m", "domain_rag_amd.cli.stage0_lama", "--datasets", DS, "--shots", "1", "--synthetic-weights", "--tiny"] + extra,
                       cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr                                   # stage 0 logs through `logging` (stderr)


def _mini_dataset(root):
    """-> (expected output names, the names the device route must decode)"""
    from PIL import Image
    rng = np.random.default_rng(0)
    (root / "lama_inpaint").mkdir(parents=True)
    (root / "datasets" / DS / "annotations").mkdir(parents=True)
    train = root / "datasets" / DS / "train"
    (train / "sub").mkdir(parents=True)
    images, anns = [], []

    def add(name, w, h, boxes):
        images.append({"id": len(images) + 1, "file_name": name, "width": w, "height": h})
        for b in boxes:
            anns.append({"id": len(anns) + 1, "image_id": len(images), "bbox": b, "category_id": 1})

    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "beetle_01.jpg")
    add("beetle_01.jpg", 72, 48, [[10, 8, 20, 16]])                                   # a JPEG at the annotated size: the device decodes it
    Image.fromarray(rng.integers(0, 256, (45, 70, 3), dtype=np.uint8)).save(train / "sub" / "odd_02.JPG", quality=90, subsampling=0)
    add("sub/odd_02.JPG", 70, 45, [[5, 5, 30, 20], [40, 10, 20, 30]])                 # odd size, 4:4:4, two boxes: the device decodes it
    Image.fromarray(rng.integers(0, 256, (45, 70), dtype=np.uint8)).save(train / "grey_03.jpeg")
    add("grey_03.jpeg", 70, 45, [[20, 10, 25, 25]])                                   # one component: the decoder replicates it like convert("RGB")
    Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(train / "fly_04.jpg")
    add("fly_04.jpg", 72, 48, [[10, 8, 20, 16]])                                      # annotated size differs from the file's: PIL resizes
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "leaf_05.png")
    add("leaf_05.png", 72, 48, [[12, 8, 20, 16]])                                     # not a JPEG name: PIL
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "wasp_06.jpg", format="PNG")
    add("wasp_06.jpg", 72, 48, [[30, 20, 20, 16]])                                    # PNG bytes under a .jpg name: the device parser refuses, PIL
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).convert("CMYK").save(train / "cmyk_07.jpg")
    add("cmyk_07.jpg", 72, 48, [[30, 20, 20, 16]])                                    # a mode the decoder hands back: PIL
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "prog_08.jpg", progressive=True)
    add("prog_08.jpg", 72, 48, [[8, 8, 20, 16]])                                      # progressive: decoded on the device by the lane kernel
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "Coleoptera"}]},
              open(root / "datasets" / DS / "annotations" / "1_shot.json", "w"))
    return sorted(im["file_name"] for im in images), {"beetle_01.jpg", "sub/odd_02.JPG", "grey_03.jpeg", "prog_08.jpg"}


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            full = os.path.join(dp, f)
            out[os.path.relpath(full, base)] = open(full, "rb").read()
    return out


def test_gpu_and_host_sources_write_the_same_files(gpu, tmp_path):
    trees = {}
    for route in ("host", "gpu"):
        root = tmp_path / route
        names, on_device = _mini_dataset(root)
        log = _run_stage0(root / "lama_inpaint", ["--source", route])
        assert f"完成 {len(names)} 个图像, 失败 0 个" in log, log[-2000:]
        assert "GPU JPEG" not in log                              # neither the device decoder nor the encoder fell back with a warning
        took = {ln.split("设备读取 ")[1].split(":")[0] for ln in log.splitlines() if "设备读取 " in ln}
        assert took == (set() if route == "host" else on_device), took
        trees[route] = _tree(root / "lamainpaint" / DS / "1_shot")
        assert sorted(trees[route]) == names
    for name, data in trees["host"].items():
        assert trees["gpu"][name] == data, name
    # --source gpu with --jpeg host: the frame decoded on the device leaves through PIL, the same bytes again
    root = tmp_path / "mixed"
    names, on_device = _mini_dataset(root)
    log = _run_stage0(root / "lama_inpaint", ["--source", "gpu", "--jpeg", "host"])
    assert f"完成 {len(names)} 个图像, 失败 0 个" in log and "设备路径 " not in log
    assert _tree(root / "lamainpaint" / DS / "1_shot") == trees["host"]
    from domain_rag_amd.cli import stage0_lama as s0
    assert s0.build_parser().parse_args([]).source == "host"
    with pytest.raises(SystemExit):
        s0.build_parser().parse_args(["--source", "nvjpeg"])
    with pytest.raises(ValueError, match="source"):
        s0.process_dataset(DS, "1", None, None, source="nvjpeg")
