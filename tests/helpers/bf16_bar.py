"""The bar that a bf16 kernel is held to against a float64 restatement with the kernel's own rounding points (tests/test_gpu_textenc.py,
tests/test_gpu_elementwise_exact.py, tests/test_elementwise_restatements_host.py)."""
import torch


def ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """distance in bf16 ulps between two bf16 tensors (ordered integer images of the bit patterns)"""
    def ordered(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -32768 - i, i)
    return (ordered(a.cpu()) - ordered(b.cpu())).abs()


def bar(got, want, what, frac=0.99):
    """equal on >= 99 % of the elements; every other one within 1 bf16 ulp, or — an output that cancels to near zero, where the kernel's fp32
    accumulation and the float64 restatement part by more ulps than they part in value — within 2^-8 of the largest output"""
    got, want = got.cpu(), want.cpu()
    d = ulps(got, want)
    eq = (d == 0).float().mean().item()
    err = (got.float() - want.float()).abs()
    tol = 2.0 ** -8 * want.float().abs().max().item()
    bad = (d > 1) & (err > tol)
    assert eq >= frac and not bad.any(), f"{what}: {eq:.4%} equal, max {d.max().item()} ulp, worst abs err {err.max().item():.3e} (tol {tol:.3e})"
    return eq


def bar_rows(got, want, what, frac=0.99):
    """``bar`` for [rows, D] outputs whose rows differ in size, and for rows that hold NaN or inf: the 2^-8 allowance is of each ROW's largest
    finite output, a NaN is met by a NaN and an inf by the same inf (neither has a distance in ulps).  Returns the equal share."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dim() == 2, f"{what}: shapes {tuple(got.shape)} / {tuple(want.shape)}"
    g, w = got.float(), want.float()
    special = ~torch.isfinite(w) | ~torch.isfinite(g)
    same_special = (torch.isnan(g) & torch.isnan(w)) | (g == w)
    assert bool((same_special | ~special).all()), f"{what}: {int((special & ~same_special).sum())} NaN / inf outputs differ from the restatement"
    d = torch.where(special, torch.zeros((), dtype=torch.int32), ulps(got, want))
    err = torch.where(special, torch.zeros(()), (g - w).abs())
    tol = 2.0 ** -8 * torch.where(special, torch.zeros(()), w.abs()).amax(dim=1, keepdim=True)
    eq = (d == 0).float().mean().item()
    bad = (d > 1) & (err > tol)
    assert eq >= frac and not bad.any(), (f"{what}: {eq:.4%} equal, max {d.max().item()} ulp, {int(bad.sum())} elements past 1 ulp and their row's "
                                          f"allowance, worst abs err {err.max().item():.3e}")
    return eq
