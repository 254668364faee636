"""stage3_outpaint --pictures device|host on a synthetic mini dataset (tiny architectures, seeded weights): the device route decodes the
backgrounds with png.decode_paths, feeds the Redux prior from the decoded tensors and, with --png gpu, resizes the results back on
the device — and must write byte-identical files.  One sample is upscaled (short side < 64), one needs no resize, one has a
Pillow-written background (LZ77: the "pil" route inside the device run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORED_PARAMS = ("process_id", "copied_bg_path")          # they carry the run's own process id


def _run(mod, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, DRAG_TIMESTAMP="20260101_000000")
    r = subprocess.run([sys.executable, "-m", mod] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _mini_dataset(root, gpu):
    from PIL import Image
    from domain_rag_amd import png
    rng = np.random.default_rng(4)
    ds = "DIOR"
    (root / "datasets" / ds / "annotations").mkdir(parents=True); (root / "datasets" / ds / "train").mkdir(parents=True)
    samples = {"up_1": (40, 56), "same_2": (80, 96), "pil_3": (48, 64)}         # H, W of the original: upscaled | untouched | upscaled
    images, anns = [], []
    for i, (name, (h, w)) in enumerate(samples.items()):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "datasets" / ds / "train" / f"{name}.jpg")
        images.append({"id": i + 1, "file_name": f"{name}.jpg", "width": w, "height": h})
        anns.append({"id": i + 1, "image_id": i + 1, "bbox": [8, 6, 20, 14], "category_id": 1})
        sdir = root / "result" / f"{ds}_1shot_retrieval" / "results_x" / name
        sdir.mkdir(parents=True)
        for r in (1, 2):
            bg = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
            if name == "pil_3" and r == 1:          # Pillow's own file of a picture with repeats: LZ77 matches, so the device declines it
                Image.fromarray(np.tile(bg[:8, :8], (8, 8, 1))).save(sdir / f"generated_image_rank{r}.png")
            else:                                   # what stage 2 writes with --png gpu
                (sdir / f"generated_image_rank{r}.png").write_bytes(png.encode(torch.from_numpy(bg).to(gpu))[0])
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "airplane"}]},
              open(root / "datasets" / ds / "annotations" / "1_shot.json", "w"))
    return ds, list(samples)


def test_pictures_device_writes_the_files_of_pictures_host(gpu, tmp_path):
    root = tmp_path
    ds, names = _mini_dataset(root, gpu)
    common = ["--dataset", ds, "--shot", "1", "--synthetic-weights", "--tiny", "--num_inference_steps", "2", "--seed", "5"]
    out_h = _run("domain_rag_amd.cli.stage3_outpaint", ["--process_id", "h", "--pictures", "host"] + common, cwd=root)
    out_d = _run("domain_rag_amd.cli.stage3_outpaint", ["--process_id", "d", "--pictures", "device"] + common, cwd=root)
    for name in names:
        assert f"样本 {name} 处理完成" in out_h and f"样本 {name} 处理完成" in out_d
    # the device run says how many backgrounds went each route
    assert "样本 up_1 背景解码: device 2, pil 0" in out_d and "样本 same_2 背景解码: device 2, pil 0" in out_d
    assert "样本 pil_3 背景解码: device 1, pil 1" in out_d and "背景解码" not in out_h
    compared = 0
    for name in names:
        dh, dd = (root / "outpaint_hires" / f"process_{p}" / ds / "1_shot" / name for p in "hd")
        files = sorted(os.listdir(dh))
        assert files == sorted(os.listdir(dd)) and len(files) >= 12
        for f in files:
            if f.endswith(".json"):
                a, b = json.load(open(dh / f)), json.load(open(dd / f))
                assert {k: v for k, v in a.items() if k not in IGNORED_PARAMS} == {k: v for k, v in b.items() if k not in IGNORED_PARAMS}, f
            else:
                assert (dh / f).read_bytes() == (dd / f).read_bytes(), f
                compared += 1
        pre = f"{ds}_{name}_1shot"
        for kind in ("hires_result", "final_result", "mask", "bg"):
            assert any(f.startswith(f"{pre}_{kind}_") for f in files), kind
    assert compared >= 3 * 10
    from PIL import Image
    up = root / "outpaint_hires" / "process_d" / ds / "1_shot" / "up_1"
    assert Image.open(up / f"{ds}_up_1_1shot_hires_result_1.png").size != Image.open(up / f"{ds}_up_1_1shot_final_result_1.png").size      # resized back
    same = root / "outpaint_hires" / "process_d" / ds / "1_shot" / "same_2"
    assert (same / f"{ds}_same_2_1shot_hires_result_1.png").read_bytes() == (same / f"{ds}_same_2_1shot_final_result_1.png").read_bytes()


def test_prior_embeds_device_equals_prior_embeds(gpu):
    from PIL import Image
    from domain_rag_amd.engine import Engine
    eng = Engine("fill", synthetic=True, tiny=True, device=gpu)
    pic = np.random.default_rng(9).integers(0, 256, (70, 90, 3), dtype=np.uint8)
    a = eng.prior_embeds([Image.fromarray(pic)], "", [1.0], [1.0])
    b = eng.prior_embeds_device([torch.from_numpy(pic).to(gpu)], "", [1.0], [1.0])
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    with pytest.raises(ValueError, match="uint8"):
        eng.prior_embeds_device([torch.from_numpy(pic).to(gpu).float()], "", [1.0], [1.0])
