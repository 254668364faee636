"""Stage 0 — drop-in for ``lama_inpaint/lama_inpaint.py`` (flags :227-233, paths :82-99, loop :139-215): erase the annotated
objects of every k-shot training image with LaMa and write ``../lamainpaint/<dataset>/<k>_shot/<file_name>``.

    cd lama_inpaint && python -m domain_rag_amd.cli.stage0_lama --datasets ArTaxOr --shots 1

The generator runs on the HIP path (domain-rag_amd/lama.py); the model is loaded once for all datasets.  Under
torch.distributed.run (RANK / WORLD_SIZE) the images of a dataset are sharded with the reference's contiguous rule — no
collective is needed, every rank writes its own files and logs its own counters.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import time
from collections import defaultdict
from datetime import datetime

from .. import hostlogic as H

JPEG_SUFFIXES = (".jpg", ".jpeg", ".jpe", ".jfif")                # the names Pillow's `save(path)` writes as JPEG
# --jpeg: who compresses a .jpg result.  Both routes write the same bytes (tests/test_gpu_stage0_jpeg.py).  Measured on an MI355X
# (scripts/bench_stage0_jpeg.py, 16 frames of 504 x 376, two runs of 5 alternating passes; DESIGN.md kernel table): 11.49 / 11.52 ms per
# image on the device route against 11.90 / 11.93 ms on the host route, every device pass below every host pass: the device route
JPEG_DEFAULT = "gpu"
# --source: who decodes a .jpg source.  Both routes hand the model the same pixels (tests/test_gpu_stage0_source.py).  "host" until a
# measurement says otherwise; the rule is --jpeg's: "gpu" only if its per-image wall clock is not above "host"'s in the same run
# (scripts/bench_stage0_jpeg.py --source gpu).
SOURCE_DEFAULT = "host"


def setup_logger():
    log_dir = "../lamainpaint/logs"
    os.makedirs(log_dir, exist_ok=True)
    stamp = os.environ.get("DRAG_TIMESTAMP") or datetime.now().strftime("%Y%m%d_%H%M%S")
    rank = os.environ.get("RANK")
    log_file = os.path.join(log_dir, f"lama_inpaint_{stamp}{'_rank' + rank if rank else ''}.log")
    logger = logging.getLogger("domain_rag_amd.lama")
    logger.setLevel(logging.INFO)
    logger.handlers.clear()
    fmt = logging.Formatter("%(asctime)s - %(levelname)s - %(message)s")
    for h in (logging.FileHandler(log_file), logging.StreamHandler()):
        h.setFormatter(fmt)
        logger.addHandler(h)
    logger.propagate = False
    return logger


def build_parser():
    p = argparse.ArgumentParser(description="LaMa Inpainting for Multiple Datasets (MI355X)")
    p.add_argument("--datasets", nargs="+", default=["ArTaxOr", "clipart1k", "DIOR", "FISH", "NEU-DET"], help="要处理的数据集列表")
    p.add_argument("--shots", nargs="+", default=["1", "2", "3", "5", "10"], help="每个数据集要处理的shot数量")
    p.add_argument("--fix-channels", action="store_true", help="修复通道不匹配问题")          # parsed and unused in the reference too
    # additions
    p.add_argument("--lama-model", type=str, default=None, help="big-lama.pt (default: $LAMA_MODEL or ./model/big-lama.pt)")
    p.add_argument("--synthetic-weights", action="store_true")
    p.add_argument("--tiny", action="store_true", help="test hook: tiny generator")
    p.add_argument("--jpeg", choices=["gpu", "host"], default=JPEG_DEFAULT,
                   help="gpu: .jpg results stay on the device and are compressed there (jpeg.encode: Pillow's bytes); host: Pillow's Image.save")
    p.add_argument("--source", choices=["gpu", "host"], default=SOURCE_DEFAULT,
                   help="gpu: a .jpg source the device parser accepts at the annotated size is decoded on the device "
                        "(jpeg.decode_files(entropy='parallel'): Pillow's bytes); host: Pillow's Image.open")
    return p


def _annotation_index(annotation_file):
    """-> (image_id -> {file_name, width, height}, image_id -> [annotations] in file order, category_id -> name)"""
    with open(annotation_file, "r") as f:
        data = json.load(f)
    info_of = {im["id"]: {k: im[k] for k in ("file_name", "width", "height")} for im in data.get("images", [])}
    anns_of = defaultdict(list)
    for ann in data.get("annotations", []):
        anns_of[ann["image_id"]].append(ann)
    names = {c["id"]: c["name"] for c in data.get("categories", [])}
    return info_of, anns_of, names, len(data.get("annotations", []))


def _open_rgb(image_path, size):
    """the image as the loop reads it (:159-170): RGB, at the annotated size (PIL's default bicubic resize if the file differs)"""
    from PIL import Image
    image = Image.open(image_path)
    if image.mode != "RGB":
        image = image.convert("RGB")
    if image.size != size:
        image = image.resize(size)
    return image


def _inpaint_one(simple_lama, image_path, info, boxes):
    """one image of the loop (:159-215): RGB, annotated size, union mask"""
    from PIL import Image
    size = (info["width"], info["height"])
    mask = Image.fromarray(H.inpaint_mask_array(size[0], size[1], boxes), mode="L")
    return simple_lama(_open_rgb(image_path, size), mask)


def _decode_source_on_device(simple_lama, image_path, size, logger):
    """``--source gpu``: the file -> uint8 [H, W, 3] on the device through ``jpeg.stage_paths`` / ``decode_files(entropy="parallel")``
    (Pillow's bytes: tests/test_gpu_jpeg_parallel.py), or None when the caller has to read it with ``_open_rgb``: a file the device
    parser does not accept (CMYK, arithmetic coding, ...: status != 0, or entropy data that does not end at EOI), a size that differs
    from the annotation (PIL resizes those), a file that cannot be read (``_open_rgb`` raises the error the loop logs), and any
    exception of the device route (logged)."""
    from .. import jpeg
    try:
        staged = jpeg.stage_paths([image_path], simple_lama.device)
        if staged.errors:
            return None
        batch = jpeg.decode_files(staged, simple_lama.device, entropy="parallel")
        if int(batch.status[0]) != 0 or (int(batch.width[0]), int(batch.height[0])) != tuple(size):
            return None
        return batch.image(0)
    except Exception as e:
        logger.warning(f"GPU JPEG 解码失败 ({e}), 改用 Pillow: {image_path}")
        return None


def _inpaint_one_on_device(simple_lama, image_path, info, boxes, image_dev=None):
    """``_inpaint_one`` for the HIP model without the trip of the RESULT through the host: -> the uint8 frame on the device.
    ``image_dev``: the source already on the device (``_decode_source_on_device``); without it the source is read by PIL as on the
    host route and uploaded (measurements of both: DESIGN.md (f), scripts/bench_jpeg_decode_single.py)."""
    import numpy as np
    import torch
    size = (info["width"], info["height"])
    if image_dev is None:
        image_dev = torch.from_numpy(np.array(_open_rgb(image_path, size))).to(simple_lama.device)
    mask_dev = torch.from_numpy(H.inpaint_mask_array(size[0], size[1], boxes)).to(simple_lama.device)
    return simple_lama.model(image_dev, mask_dev)


def _save_frame(frame, out_name, logger):
    """a device frame -> ``out_name`` (a JPEG name): compressed on the device; if the encoder raises, Pillow writes the file
    (the same bytes).  -> who wrote it: "device" | "PIL" """
    from .. import jpeg
    try:
        data = jpeg.encode(frame)[0]
    except Exception as e:
        logger.warning(f"GPU JPEG 编码失败 ({e}), 改用 Pillow: {out_name}")
        from PIL import Image
        Image.fromarray(frame.cpu().numpy()).save(out_name)
        return "PIL"
    with open(out_name, "wb") as f:
        f.write(data)
    return "device"


def process_dataset(dataset_name, shot_count, logger, simple_lama, rank: int = 0, world: int = 1, jpeg: str = JPEG_DEFAULT,
                    source: str = SOURCE_DEFAULT):
    """process_dataset (:78-224) -> (processed, errors).  ``simple_lama`` is the model object: (PIL RGB, PIL L) -> PIL.
    ``jpeg``: "gpu" keeps a .jpg result of the HIP ``SimpleLama`` on the device up to the finished file's bytes; "host", any other
    model object and any other file type go through PIL.  ``source``: "gpu" decodes a .jpg source of the HIP ``SimpleLama`` on the
    device (``_decode_source_on_device`` says which files); "host", any other model object and every other file are opened by PIL.
    Both settings of both switches write the same files."""
    if jpeg not in ("gpu", "host"):
        raise ValueError(f"process_dataset: jpeg must be 'gpu' or 'host', got {jpeg!r}")
    if source not in ("gpu", "host"):
        raise ValueError(f"process_dataset: source must be 'gpu' or 'host', got {source!r}")
    on_device = source_on_device = False
    if jpeg == "gpu" or source == "gpu":
        from ..lama import SimpleLama
        on_device = jpeg == "gpu" and isinstance(simple_lama, SimpleLama)
        source_on_device = source == "gpu" and isinstance(simple_lama, SimpleLama)
    logger.info(f"数据集 {dataset_name} / {shot_count}-shot: 开始")
    dataset_path = os.path.join("../datasets", dataset_name)
    train_images_dir = os.path.join(dataset_path, "train")
    for need, what in ((dataset_path, "数据集目录"), (train_images_dir, "训练图像目录")):
        if not os.path.exists(need):
            logger.error(f"{what}不存在: {need}")
            return 0, 0
    annotation_file = os.path.join(dataset_path, "annotations", f"{shot_count}_shot.json")
    output_dir = H.lama_output_dir(dataset_name, shot_count)
    os.makedirs(output_dir, exist_ok=True)
    logger.info(f"结果写入 {output_dir}")
    try:
        info_of, anns_of, names, n_ann = _annotation_index(annotation_file)
    except Exception as e:
        logger.error(f"读取注释文件 {annotation_file} 失败: {e}")
        return 0, 0
    logger.info(f"注释文件 {annotation_file}: {len(info_of)} 个图像, {n_ann} 个注释, {len(anns_of)} 个图像带有bbox")
    work = list(anns_of.items())                                  # annotation order (dict insertion), like the reference's loop
    if world > 1:
        work = H.split_samples_for_gpus(work, world)[rank]
    done = failed = multi = 0
    for image_id, anns in work:
        info = info_of.get(image_id)
        if info is None:
            logger.warning(f"注释引用了未知的图像ID {image_id}, 跳过")
            continue
        image_path = os.path.join(train_images_dir, info["file_name"])
        if len(anns) > 1:
            multi += 1
            cats = ", ".join("{}(ID:{})".format(names.get(a["category_id"], "未知类别 {}".format(a["category_id"])), a["category_id"]) for a in anns)
            logger.info(f"多bbox图像 {info['file_name']}: {len(anns)} 个bbox, 类别: {cats}")
        try:
            out_name = os.path.join(output_dir, info["file_name"])
            boxes = [a["bbox"] for a in anns]
            image_dev = None
            if source_on_device and image_path.lower().endswith(JPEG_SUFFIXES):
                image_dev = _decode_source_on_device(simple_lama, image_path, (info["width"], info["height"]), logger)
                if image_dev is not None:
                    logger.info(f"设备读取 {info['file_name']}: JPEG 解码于 device")
            device_out = on_device and out_name.lower().endswith(JPEG_SUFFIXES)
            if device_out or image_dev is not None:
                frame = _inpaint_one_on_device(simple_lama, image_path, info, boxes, image_dev)
                os.makedirs(os.path.dirname(out_name), exist_ok=True)
                if device_out:
                    writer = _save_frame(frame, out_name, logger)
                    logger.info(f"设备路径 {info['file_name']}: JPEG 写入 {writer}")
                else:                                              # what SimpleLama.__call__ hands back, saved as on the host route
                    from PIL import Image
                    Image.fromarray(frame.cpu().numpy()).save(out_name)
            else:
                result = _inpaint_one(simple_lama, image_path, info, boxes)
                os.makedirs(os.path.dirname(out_name), exist_ok=True)
                result.save(out_name)
            done += 1
        except Exception as e:                                     # reference convention: log, count, continue
            logger.error(f"图像 {image_path} 处理失败: {e}")
            failed += 1
    logger.info(f"数据集 {dataset_name} / {shot_count}-shot: 完成 {done} 个图像, 失败 {failed} 个, 其中多bbox图像 {multi} 个")
    return done, failed


def main(argv=None):
    args = build_parser().parse_args(argv)
    logger = setup_logger()
    logger.info(f"LaMa stage: 数据集 {', '.join(args.datasets)}; shots {', '.join(args.shots)}")
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    if args.synthetic_weights:
        os.environ["DRAG_SYNTHETIC_WEIGHTS"] = "1"
    if args.tiny:
        os.environ["DRAG_TINY"] = "1"
    if args.lama_model:
        os.environ["LAMA_MODEL"] = args.lama_model
    from ..lama import SimpleLama
    simple_lama = SimpleLama()                                     # once, not per dataset (:104) — same outputs
    t_start = time.time()
    totals = [0, 0]
    for ds in args.datasets:
        for shot in args.shots:
            try:
                for i, v in enumerate(process_dataset(ds, shot, logger, simple_lama, rank, world, jpeg=args.jpeg, source=args.source)):
                    totals[i] += v
            except Exception as e:
                logger.error(f"数据集 {ds} / {shot}-shot 中断: {e}")
    elapsed = time.time() - t_start
    logger.info(f"全部完成: {totals[0]} 个图像成功, {totals[1]} 个失败, 用时 {int(elapsed // 3600)}:{int(elapsed % 3600 // 60):02d}:{elapsed % 60:05.2f}")
    return tuple(totals)


if __name__ == "__main__":
    main()
