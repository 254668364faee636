"""The arithmetic of ``drag_stepcache_forecast_images_bf16`` (csrc/stepcache.hip) restated in numpy float32, one operation per line: numpy
rounds every float32 operation by itself and cannot fuse a multiply into an add, which is exactly what the kernel promises.  The last step,
float32 -> bf16 round-to-nearest-even, goes through torch's cast (the rule the library's other bf16 kernels are held to).

``forecast(x, r, p, c)``: bf16 tensors of one shape and one coefficient -> the bf16 tensor the kernel leaves in ``x``."""
import numpy as np
import torch


def _f32(t: torch.Tensor) -> np.ndarray:
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().float().numpy()          # bf16 -> float32 is exact


def forecast(x: torch.Tensor, r: torch.Tensor, p: torch.Tensor, c: float) -> torch.Tensor:
    xf, rf, pf = _f32(x), _f32(r), _f32(p)
    cf = np.float32(c)                               # the coefficient travels as float32
    with np.errstate(all="ignore"):                  # inf - inf, 0 * inf, overflow: IEEE results, as on the device
        d = rf - pf
        m = cf * d
        f = m + rf
        s = xf + f
    assert d.dtype == m.dtype == f.dtype == s.dtype == np.float32
    return torch.from_numpy(s).bfloat16()            # round to nearest even
