"""TEST INFRASTRUCTURE: torch restatement of moq_hadamard / moq_hadamard_mx_qdq (include/moquant.h).

The definition, stated once more in torch ops that are exact IEEE fp32 on every device: the block in fp32; for
h = 1, 2, 4, ..., B / 2 in this order, (v[i], v[i+h]) <- (v[i] + v[i+h], v[i] - v[i+h]) for every i with (i & h) == 0,
as one reshape / add / sub per stride; times torch.tensor(B ** -0.5, dtype=float32); `.to(dtype)`.  On CPU tensors it
stands in for libmoquant in the `-m "not gpu"` tier (install), on the GPU it is what the kernels are compared with.
"""

from __future__ import annotations

import ctypes

import torch

_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}


def fwht(x: torch.Tensor, block: int) -> torch.Tensor:
    """scale * H_block * x per block of the last dim, in the dtype of x."""
    shape, dtype = x.shape, x.dtype
    v = x.to(torch.float32).reshape(-1, block)
    rows = v.shape[0]
    h = 1
    while h < block:
        v = v.reshape(rows, block // (2 * h), 2, h)
        a, b = v[:, :, 0, :], v[:, :, 1, :]
        v = torch.stack((a + b, a - b), dim=2).reshape(rows, block)
        h *= 2
    v = v * torch.tensor(block ** -0.5, dtype=torch.float32, device=x.device)
    return v.to(dtype).reshape(shape)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal NaN positions, every other element equal as a bit pattern (so -0 != +0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(iv)[~na], b.contiguous().view(iv)[~nb])


# ----------------------------------------------------------------------------------------------- hostmem twin
def _addr(p) -> int:
    if p is None:
        return 0
    return (p.value or 0) if isinstance(p, ctypes.c_void_p) else int(p)


def _host(p, n, dtype) -> torch.Tensor:
    nbytes = int(n) * torch.tensor([], dtype=dtype).element_size()
    buf = (ctypes.c_uint8 * nbytes).from_address(_addr(p))
    return torch.frombuffer(buf, dtype=torch.uint8).view(dtype)


def _bad(rows, cols, block):
    if rows < 0 or cols < 0 or block < 2 or block & (block - 1) or cols % block:
        return -1
    return -2 if block > 16384 else 0


def install(fake) -> None:
    """Give the host-memory stand-in of libmoquant (tests/hostmem_backend.py) the two entries."""

    def hadamard(x, y, rows, cols, block, scale, dt, running_amax, stream):
        rc = _bad(rows, cols, block)
        if rc or rows * cols == 0:
            return rc
        assert scale == float(torch.tensor(block ** -0.5, dtype=torch.float32))
        out = fwht(_host(x, rows * cols, _DT[dt]).clone(), block)
        _host(y, rows * cols, _DT[dt]).copy_(out)
        if _addr(running_amax):
            r = _host(running_amax, 1, torch.float32)
            m = out.abs().amax().float().reshape(1)  # (amax propagates NaN, and torch.maximum does)
            r.copy_(torch.maximum(r, m))
        return 0

    def hadamard_mx_qdq(x, y, rows, cols, rot_block, scale, block, dt, fmt, scale_fmt, global_amax, rotate_back, stream):
        rc = _bad(rows, cols, rot_block)
        if rc:
            return rc
        vec = 4 if dt == 0 else 8
        lpg = block // vec
        if (rot_block > 64 * vec or rot_block % block or block % vec or lpg & (lpg - 1)
                or lpg > (64 if scale_fmt == 9 else 8)):
            return -2
        hadamard(x, y, rows, cols, rot_block, scale, dt, None, stream)
        fake.moq_mx_fused_amax_convert(y, y, rows, cols, block, dt, fmt, scale_fmt, global_amax, stream)
        if rotate_back:
            hadamard(y, y, rows, cols, rot_block, scale, dt, None, stream)
        return 0

    fake.moq_hadamard = hadamard
    fake.moq_hadamard_mx_qdq = hadamard_mx_qdq
