"""Stage 0 with ``--jpeg gpu`` (the inpainted frame stays on the device up to the finished .jpg bytes: LamaHIP -> jpeg.encode)
against ``--jpeg host`` (PIL in, PIL out: the reference's lama_inpaint/lama_inpaint.py:159-211): the same files, byte for byte.
The stage-0 files are what stages 1 and 2 read, so "the same pixels" would not be enough."""
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
    """the mini dataset of tests/test_gpu_cli.py plus inputs of other kinds (sub-directory, odd size, grey, PNG, a size to resize from): -> the expected output names"""
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

    for i, name in enumerate(["beetle_01.jpg", "moth_02.jpg"]):                       # 72 x 48
        Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / name)
        add(name, 72, 48, [[10 + i, 8, 20, 16]])
    Image.fromarray(rng.integers(0, 256, (45, 70, 3), dtype=np.uint8)).save(train / "sub" / "odd_03.JPG", quality=90, subsampling=0)
    add("sub/odd_03.JPG", 70, 45, [[5, 5, 30, 20], [40, 10, 20, 30]])                 # odd size (the frame is padded to 72 x 48), two boxes, 4:4:4
    Image.fromarray(rng.integers(0, 256, (45, 70), dtype=np.uint8)).save(train / "grey_04.jpeg")
    add("grey_04.jpeg", 70, 45, [[20, 10, 25, 25]])                                   # a one-component file
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "leaf_05.png")
    add("leaf_05.png", 72, 48, [[12, 8, 20, 16]])                                     # a PNG in, a PNG out: PIL on both ends
    Image.fromarray(rng.integers(0, 256, (48, 72, 3), dtype=np.uint8)).save(train / "wasp_06.jpg", format="PNG")
    add("wasp_06.jpg", 72, 48, [[30, 20, 20, 16]])                                    # PNG bytes under a .jpg name: a JPEG out
    Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(train / "fly_07.jpg")
    add("fly_07.jpg", 72, 48, [[10, 8, 20, 16]])                                      # annotated size differs from the file's: image.resize
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "Coleoptera"}]},
              open(root / "datasets" / DS / "annotations" / "1_shot.json", "w"))
    return sorted(im["file_name"] for im in images)


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            full = os.path.join(dp, f)
            out[os.path.relpath(full, base)] = open(full, "rb").read()
    return out


def test_gpu_and_host_routes_write_the_same_files(gpu, tmp_path):
    from PIL import Image
    trees = {}
    for route in ("host", "gpu"):
        root = tmp_path / route
        names = _mini_dataset(root)
        log = _run_stage0(root / "lama_inpaint", ["--jpeg", route])
        assert f"完成 {len(names)} 个图像, 失败 0 个" in log, log[-2000:]
        assert "GPU JPEG" not in log                              # the device encoder did not fall back to Pillow with a warning
        # positive evidence of the route each file took: one line per file the device wrote, none on the host route
        took = {ln.split("设备路径 ")[1].split(":")[0]: ln.split(": ", 1)[1].strip() for ln in log.splitlines() if "设备路径 " in ln}
        jpeg_names = [n for n in names if not n.endswith(".png")]
        assert len(jpeg_names) == 6
        assert took == ({} if route == "host" else {n: "JPEG 写入 device" for n in jpeg_names}), took       # (leaf_05.png: PIL on both routes)
        trees[route] = _tree(root / "lamainpaint" / DS / "1_shot")
        assert sorted(trees[route]) == names
    for name, data in trees["host"].items():
        assert trees["gpu"][name] == data, name
        assert Image.open(tmp_path / "gpu" / "lamainpaint" / DS / "1_shot" / name).size == (72, 48)
    # the flag's default is one of the two routes, and a route that does not exist is refused
    from domain_rag_amd.cli import stage0_lama as s0
    assert s0.build_parser().parse_args([]).jpeg in ("gpu", "host")
    with pytest.raises(SystemExit):
        s0.build_parser().parse_args(["--jpeg", "nvjpeg"])
