"""One process, two devices: every kernel that takes more dynamic LDS than the default limit needs the permission on EACH device it runs
on (csrc/drag_launch.h keeps it per device and kernel), and a persistent grid is sized by the CURRENT device's CU count.  Each case runs
on cuda:0 and then on cuda:1 and must give the same bytes.  Skipped on a machine with one device."""
import io
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).bfloat16()


def _gemm(kernel):
    def run(dev):
        from domain_rag_amd import ops
        a, w = _randn((256, 256), 1).to(dev), _randn((256, 256), 2, 0.05).to(dev)
        with ops.options(gemm_kernel=kernel):
            return ops.gemm(a, w).cpu()
    return run


def _attention(dev):
    from domain_rag_amd import ops
    B, H, S = 1, 8, 1024
    D = H * 128
    qkv, vt = _randn((B, S, 3 * D), 3).to(dev), _randn((B, H, 128, S), 4).to(dev)
    out = torch.full((B, S, D), float("nan"), dtype=torch.bfloat16, device=dev)
    with ops.options(attn_q64=1):
        ops.attention(qkv, qkv.view(-1)[D:], vt, out, B, S, H, 3 * D, S * 3 * D, D, S * D, 1 / math.sqrt(128))
    return out.cpu()


def _topk(dev):
    from domain_rag_amd import ops
    g = torch.Generator().manual_seed(5)
    corpus = torch.nn.functional.normalize(torch.randn((4096, 768), generator=g), dim=1)
    queries = corpus[:16] + 0.1 * torch.randn((16, 768), generator=g)
    D, I = ops.cosine_topk(corpus.to(dev), queries.to(dev), 10)      # d = 768: 81 920 bytes of dynamic LDS
    return torch.cat([D.cpu().view(torch.int32).long(), I.cpu()], dim=1)


def _jpeg(dev):
    from PIL import Image
    from domain_rag_amd import jpeg
    rng = np.random.default_rng(6)
    blobs = []
    for progressive in (False, True):
        bio = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(bio, "JPEG", quality=80, progressive=progressive)
        blobs.append(bio.getvalue())
    batch = jpeg.decode_files(blobs, dev)
    assert (batch.status == 0).all()
    return torch.stack([batch.image(i).cpu() for i in range(2)])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices in one process")
@pytest.mark.parametrize("case", [_gemm(3), _gemm(143), _attention, _topk, _jpeg], ids=["gemm_w4p", "gemm_deep_143", "attention_q64", "topk_d768", "jpeg"])
def test_second_device_gives_the_first_device_s_bytes(gpu, case):
    outs = []
    for idx in (0, 1):
        with torch.cuda.device(idx):
            outs.append(case(torch.device("cuda", idx)))
            torch.cuda.synchronize()
    assert outs[0].dtype == outs[1].dtype and torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0].float()).all()
