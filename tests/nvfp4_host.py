"""TEST INFRASTRUCTURE: torch restatements of the three static-NVFP4 entries of include/moquant.h.

Elementwise torch ops only (one rounding per op, no contraction), so the same code runs on CPU tensors -- where it is
checked bit for bit against the reference's own Triton kernels run by the Triton interpreter
(tests/golden/nvfp4_static.npz) -- and on the GPU, where it checks the kernels on Llama-size weights.

  static_qdq       static_blockwise_fp4_fake_quant (gemm/fp4_kernel.py:281-318) with the scales of compute_fp4_scales
  sweep            _fp8_scale_sweep_kernel (gemm/nvfp4_fp8_sweep.py:59-124)
  sweep_hessian    _fp8_scale_sweep_hessian_kernel (:174-226) with the defined order of moq_nvfp4_fp8_sweep_hessian:
                   (dw H)_j as an fmaf chain over k = 0,4,8,12, 1,5,9,13, 2,6,10,14, 3,7,11,15 (the reference's tl.dot
                   is a BLAS call in the interpreter: same values up to summation order)
"""

from __future__ import annotations

import ctypes

import numpy as np
import torch

K_ORDER = [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]


def candidates(device="cpu") -> torch.Tensor:
    """The 126 positive finite E4M3 values / 448, ascending (_fp8_scale_candidates.py)."""
    v = torch.arange(1, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    return (v / 448.0).to(device)


def _div(a: torch.Tensor, b: float) -> torch.Tensor:
    """a / b correctly rounded on every device: PyTorch's GPU division by a Python number multiplies by its reciprocal
    (two roundings), so the divisor goes in as a tensor."""
    return a / torch.full_like(a, b)


def fp4_round(r: torch.Tensor) -> torch.Tensor:
    """fp4_round_magnitude (common/nvfp4_quant.py): a NaN falls through every test and gives 6."""
    w = torch.where
    return w(r <= 0.25, 0.0, w(r < 0.75, 0.5, w(r <= 1.25, 1.0, w(r < 1.75, 1.5, w(r <= 2.5, 2.0, w(
        r < 3.5, 3.0, w(r <= 5.0, 4.0, 6.0))))))).to(torch.float32)


def fp8_eager(v: torch.Tensor, amax: torch.Tensor) -> torch.Tensor:
    """_fp8_eager (tensor_quant.py:46-59) for fp32 v: `448.0 / t` is t.reciprocal() * 448 there (two roundings)."""
    amax = amax.float()
    safe = torch.where(amax <= 1.0 / (1 << 24), torch.ones_like(amax), amax)
    scale = torch.reciprocal(safe) * 448.0
    inv = torch.reciprocal(scale)
    return (v.float() * scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * inv


def block_scales(amax: torch.Tensor, global_amax: torch.Tensor) -> torch.Tensor:
    """compute_fp4_scales(amax, global_amax, quantize_block_scales=True) (gemm/fp4_kernel.py:235-278)."""
    g = global_amax.float().reshape(())
    return fp8_eager(_div(amax.float(), 6.0), _div(g, 6.0))


def static_qdq(x: torch.Tensor, amax: torch.Tensor, global_amax: torch.Tensor) -> torch.Tensor:
    xb = x.reshape(-1, 16).float()
    s = block_scales(amax.reshape(-1, 1), global_amax)
    zero = s == 0
    safe = torch.where(zero | torch.isnan(s) | torch.isinf(s), torch.ones_like(s), s)
    m = fp4_round(xb.abs() / safe) * safe
    y = torch.where(xb >= 0, m, -m)
    y = torch.where(zero, torch.zeros_like(y), y)
    return y.to(x.dtype).reshape(x.shape)


def sum16(p: torch.Tensor) -> torch.Tensor:
    """numpy's pairwise order for a contiguous 16-term float32 row sum (np.sum: 8 partial sums, then a tree)."""
    r = p[:, :8] + p[:, 8:]
    return ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))


def _argmin_strict(losses):
    best = torch.full_like(losses[0], float("inf"))
    idx = torch.zeros(best.shape, dtype=torch.int64, device=best.device)
    for k, loss in enumerate(losses):
        better = loss < best
        best = torch.where(better, loss, best)
        idx = torch.where(better, torch.full_like(idx, k), idx)
    return idx


def sweep(x: torch.Tensor, global_amax: torch.Tensor) -> torch.Tensor:
    a = x.reshape(-1, 16).float().abs()
    g = global_amax.float().reshape(())
    c = candidates(x.device)
    losses = []
    for k in range(c.numel()):
        s = _div(c[k] * g, 6.0)
        s = torch.where(s == 0, torch.ones_like(s), s)
        d = a - fp4_round(a / s) * s
        losses.append(sum16(d * d))
    return g * c[_argmin_strict(losses)]


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fl32(a * b + c) with one rounding: the float64 product is exact, the float64 sum is rounded to odd (TwoSum
    error term), and round-to-odd with 29 spare bits then rounds to float32 exactly as a fused multiply-add would."""
    p = a.double() * b.double()
    cd = c.double()
    s = p + cd
    bb = s - p
    err = (p - (s - bb)) + (cd - bb)
    odd = (s.view(torch.int64) & 1) == 1
    fix = (err != 0) & ~odd & torch.isfinite(s)
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where(fix, torch.nextafter(s, toward), s)
    return s.float()


def sweep_hessian(x: torch.Tensor, global_amax: torch.Tensor, hessian: torch.Tensor) -> torch.Tensor:
    w = x.reshape(-1, 16).float()
    a = w.abs()
    sign = torch.where(w >= 0, 1.0, -1.0)
    ncb = hessian.shape[0]
    h = hessian.float().reshape(ncb, 16, 16)[torch.arange(w.shape[0], device=w.device) % ncb]  # [n_blocks, 16, 16]
    g = global_amax.float().reshape(())
    c = candidates(x.device)
    amaxes = c * g
    scales = block_scales(amaxes, g)
    losses = []
    for k in range(c.numel()):
        s = scales[k]
        s = torch.where(s == 0, torch.ones_like(s), s)
        dw = sign * (a - fp4_round(a / s) * s)
        acc = torch.zeros_like(dw)
        for kk in K_ORDER:
            acc = fma32(dw[:, kk:kk + 1], h[:, kk, :], acc)
        losses.append(sum16(acc * dw))
    return amaxes[_argmin_strict(losses)]


# ----------------------------------------------------------------------------------------------- hostmem twins
_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


def _addr(p) -> int:
    if p is None:
        return 0
    return (p.value or 0) if isinstance(p, ctypes.c_void_p) else int(p)


def _host(p, n, dtype) -> torch.Tensor:
    """A torch view of host memory handed over as a raw pointer (CPU tier only)."""
    nbytes = int(n) * torch.tensor([], dtype=dtype).element_size()
    buf = (ctypes.c_uint8 * nbytes).from_address(_addr(p))
    return torch.frombuffer(buf, dtype=torch.uint8).view(dtype)


def install(fake) -> None:
    """Give the host-memory stand-in of libmoquant (tests/hostmem_backend.py) these restatements as the three entries."""

    def qdq(x, y, amax, ga, n_blocks, block, dt, stream):
        if block != 16:
            return -2
        xt = _host(x, n_blocks * 16, _DT[dt])
        _host(y, n_blocks * 16, _DT[dt]).copy_(static_qdq(xt, _host(amax, n_blocks, torch.float32),
                                                          _host(ga, 1, torch.float32)))
        return 0

    def sw(x, ga, best, n_blocks, block, dt, stream):
        if block != 16:
            return -2
        _host(best, n_blocks, torch.float32).copy_(sweep(_host(x, n_blocks * 16, _DT[dt]), _host(ga, 1, torch.float32)))
        return 0

    def swh(x, h, ga, best, n_blocks, ncb, block, dt, stream):
        if block != 16 or n_blocks % ncb:
            return -2
        hh = _host(h, ncb * 256, torch.float32).reshape(ncb, 16, 16)
        _host(best, n_blocks, torch.float32).copy_(
            sweep_hessian(_host(x, n_blocks * 16, _DT[dt]), _host(ga, 1, torch.float32), hh))
        return 0

    fake.moq_nvfp4_static_qdq = qdq
    fake.moq_nvfp4_fp8_sweep = sw
    fake.moq_nvfp4_fp8_sweep_hessian = swh


def as_np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------- fixture access
def fixture():
    """(npz, cases) of tests/golden/nvfp4_static.npz (tests/golden/gen_nvfp4_static.py)."""
    import json
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nvfp4_static.npz"))
    return z, json.loads(str(z["cases"]))


def case_x(z, k, c) -> torch.Tensor:
    a = z[f"{k}_x"]
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[c["dtype"]]
    t = torch.from_numpy(a.copy()) if dt == torch.float32 else torch.from_numpy(a.view(np.int16).copy()).view(dt)
    return t.reshape(c["shape"])


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def hessian_loss64(x: torch.Tensor, global_amax: torch.Tensor, hessian: torch.Tensor, amax: torch.Tensor):
    """fp64 re-score dw^T H dw of the block amax `amax` (one of the candidate amaxes) -- for the stated tolerance
    against the interpreter fixture, whose [rows, 16] x [16, 16] product is a BLAS call."""
    w = x.reshape(-1, 16).float()
    g = global_amax.float().reshape(())
    s = block_scales(amax.float(), g)
    s = torch.where(s == 0, torch.ones_like(s), s).reshape(-1, 1)
    dw = (torch.where(w >= 0, 1.0, -1.0) * (w.abs() - fp4_round(w.abs() / s) * s)).double()
    ncb = hessian.shape[0]
    h = hessian.double().reshape(ncb, 16, 16)[torch.arange(w.shape[0], device=w.device) % ncb]
    return torch.einsum("bi,bij,bj->b", dw, h, dw)
