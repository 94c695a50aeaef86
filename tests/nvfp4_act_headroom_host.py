"""TEST INFRASTRUCTURE: torch restatement of moq_block_amax_log2_hist (include/moquant.h) and access to
tests/golden/nvfp4_act_headroom.npz (tests/golden/gen_nvfp4_act_headroom.py).

The restatement takes what the C-ABI entry takes -- the tensor and the table of bin edges -- and uses torch ops that are
exact on every device (abs, max, comparisons of the table by searchsorted, bincount): on CPU tensors it stands in for
libmoquant in the `-m "not gpu"` tier, on the GPU it checks the kernel on Llama-size activations.  No logarithm here:
that the table reproduces the reference's log2 expression is what tests/test_nvfp4_act_headroom_cpu.py checks first.
"""

from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HERE = os.path.dirname(os.path.abspath(__file__))


def block_hist(x: torch.Tensor, thresholds: torch.Tensor, block: int = 16, chunk_rows: int | None = None):
    """(counts int64 [bins], running max f32 0-dim, bad int) of a tensor whose last dim is a multiple of `block`."""
    bins = thresholds.numel() + 1
    amax = x.reshape(-1, block).abs().amax(dim=1).float()
    nan, inf = torch.isnan(amax), torch.isinf(amax)
    bad = int(nan.any()) | (int(inf.any()) << 1)
    good = amax[~(nan | inf)]
    live = good[good > 0]
    rmax = good.max() if good.numel() else torch.zeros((), device=x.device)
    idx = torch.searchsorted(thresholds.to(x.device), live, right=True)
    return torch.bincount(idx, minlength=bins), rmax.reshape(()), bad


def block_hist_big(x: torch.Tensor, thresholds: torch.Tensor, rows_per_step: int = 1 << 24):
    """The same for multi-GB tensors: slabs of blocks, so the temporaries stay small."""
    flat = x.reshape(-1, 16)
    counts = torch.zeros(thresholds.numel() + 1, dtype=torch.int64, device=x.device)
    rmax, bad = torch.zeros((), device=x.device), 0
    for r in range(0, flat.shape[0], rows_per_step):
        c, m, b = block_hist(flat[r:r + rows_per_step], thresholds)
        counts += c
        rmax = torch.maximum(rmax, m)
        bad |= b
    return counts, rmax, bad


# ----------------------------------------------------------------------------------------------- hostmem twin
def _addr(p) -> int:
    if p is None:
        return 0
    return (p.value or 0) if isinstance(p, ctypes.c_void_p) else int(p)


def _host(p, n, dtype) -> torch.Tensor:
    nbytes = int(n) * torch.tensor([], dtype=dtype).element_size()
    buf = (ctypes.c_uint8 * nbytes).from_address(_addr(p))
    return torch.frombuffer(buf, dtype=torch.uint8).view(dtype)


def install(fake) -> None:
    """Give the host-memory stand-in of libmoquant (tests/hostmem_backend.py) the entry."""

    def entry(x, rows, cols, dt, block, thresholds, bins, counts, running_max, bad, stream):
        if block != 16 or cols % 16:
            return -2
        if rows * cols == 0:
            return 0
        c, m, b = block_hist(_host(x, rows * cols, _DT[dt]), _host(thresholds, bins - 1, torch.float32))
        _host(counts, bins, torch.int64).add_(c)
        rm = _host(running_max, 1, torch.float32)
        rm.copy_(torch.maximum(rm, m.reshape(1)))
        _host(bad, 1, torch.int32).bitwise_or_(torch.tensor([b], dtype=torch.int32))
        return 0

    fake.moq_block_amax_log2_hist = entry


# ----------------------------------------------------------------------------------------------- fixture access
def fixture():
    z = np.load(os.path.join(HERE, "golden", "nvfp4_act_headroom.npz"))
    return z, json.loads(str(z["cases"]))


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


def all_patterns(dtype) -> torch.Tensor:
    """Block b holds the positive finite 16-bit pattern b + 1 at position b % 16 (odd blocks negated), zeros elsewhere."""
    top = 0x7F80 if dtype == torch.bfloat16 else 0x7C00
    n = top - 1
    x = torch.zeros(n, 16, dtype=torch.int32)
    b = torch.arange(n)
    x[b, b % 16] = (b + 1).to(torch.int32) | ((b % 2) << 15).to(torch.int32)
    return x.to(torch.int16).view(dtype)


def case_tensors(z, k, c) -> list:
    dt = DT[c["dtype"]]
    if c.get("allpatterns"):
        return [all_patterns(dt)]
    return [from_bits(z[f"{k}_x{i}"], dt).reshape(s) for i, s in enumerate(c["shapes"])]


def case_hist(z, k) -> torch.Tensor:
    """The reference's `_hist`; zeros where it stayed None."""
    return torch.from_numpy(z[f"{k}_hist"].copy()) if f"{k}_hist" in z.files else torch.zeros(512, dtype=torch.int64)


def padded(t: torch.Tensor) -> torch.Tensor:
    rem = t.shape[-1] % 16
    return torch.nn.functional.pad(t, (0, 16 - rem)) if rem else t


def neighbours(thresholds: torch.Tensor, dtype) -> torch.Tensor:
    """[n, 16] in `dtype`: every table entry rounded to the dtype, that value and its neighbours one representable value
    below and above, each as the abs-max of a block of its own (position and sign vary)."""
    t = thresholds[torch.isfinite(thresholds)]
    if dtype == torch.float32:
        base = t.view(torch.int32).to(torch.int64)
        pats = torch.cat([base + d for d in (-1, 0, 1)]).clamp(1, 0x7F7FFFFF)
        vals = pats.to(torch.int32).view(torch.float32)
    else:
        top = 0x7F7F if dtype == torch.bfloat16 else 0x7BFF
        base = t.to(dtype).view(torch.int16).to(torch.int64)
        pats = torch.cat([base + d for d in (-1, 0, 1)]).clamp(1, top)
        vals = pats.to(torch.int16).view(dtype)
    n = vals.numel()
    x = torch.zeros(n, 16, dtype=dtype)
    i = torch.arange(n)
    x[i, i % 16] = torch.where(i % 2 == 0, vals, -vals)
    x[i, (i + 5) % 16] = (vals.float() * 0.5).to(dtype)  # a smaller companion in the block
    return x


def build_llama(cfgd, device="cpu"):
    """The tiny bf16 Llama the flow case was made from: the `orig/*` weights of export_llama.npz."""
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(HERE, "golden", "export_llama.npz"))
    with torch.device("cpu"):
        model = LlamaForCausalLM(LlamaConfig(architectures=["LlamaForCausalLM"], **cfgd)).to(torch.bfloat16)
    sd = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.to(device).eval()


def input_amaxes(model) -> dict:
    return {n: m.amax.detach().float().reshape(()).cpu() for n, m in model.named_modules()
            if n.endswith("input_quantizer") and m.is_enabled and getattr(m, "amax", None) is not None}
