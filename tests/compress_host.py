"""TEST INFRASTRUCTURE: torch restatements of moq_int8_pack / moq_int8_unpack / moq_wq_linear (include/moquant.h), their
twins for the host-memory stand-in of libmoquant (tests/hostmem_backend.py), and access to the compress fixture
(tests/golden/compress.npz + its compress_p*.npz shards, tests/golden/gen_compress.py).

Elementwise torch ops only, every division with a tensor divisor, so the same code runs on CPU tensors -- where it is pinned
bit for bit to what the reference's INT8QTensor computed on CPU -- and on the GPU, where it checks the kernels.
"""

from __future__ import annotations

import ctypes
import glob
import json
import os

import numpy as np
import torch

_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TD = {"torch.bfloat16": torch.bfloat16, "torch.float32": torch.float32, "torch.uint8": torch.uint8, "torch.int8": torch.int8,
      "torch.float16": torch.float16, "torch.float8_e4m3fn": torch.float8_e4m3fn}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ----------------------------------------------------------------------------------------------- INT8 restatements
def _expand(scales: torch.Tensor, n: int, mode: int, axis_size: int, inner: int) -> torch.Tensor:
    s = scales.reshape(-1)
    if mode == 0:
        return s[:1].expand(n)
    idx = (torch.arange(n, device=s.device) // inner) % axis_size
    return s[idx]


def int8_pack(x: torch.Tensor, scales: torch.Tensor, mode: int, axis_size: int, inner: int) -> torch.Tensor:
    """int8 of the flat tensor: the quotient in x's dtype (one rounding), round half to even, clamp, NaN -> 0."""
    q = (x.reshape(-1) / _expand(scales.to(x.dtype), x.numel(), mode, axis_size, inner)).round().clamp(-128, 127)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).to(torch.int8)


def int8_unpack(q: torch.Tensor, scales: torch.Tensor, dtype, mode: int, axis_size: int, inner: int) -> torch.Tensor:
    return q.reshape(-1).view(torch.int8).to(dtype) * _expand(scales.to(dtype), q.numel(), mode, axis_size, inner)


def layout(shape, sshape):
    """(mode, axis_size, inner) as the C-ABI takes it, from the shapes INT8QTensor works with."""
    n, ns = int(np.prod(shape)), int(np.prod(sshape))
    if ns == 1:
        return 0, 1, 1
    if tuple(sshape[:-1]) == tuple(shape[:-1]) and sshape[-1] != 1:
        return 1, ns, shape[-1] // sshape[-1]
    d = max(i for i, v in enumerate(sshape) if v != 1)
    return 1, ns, int(np.prod(shape[d + 1:]))


# ----------------------------------------------------------------------------------------------- fused linear restatement
_E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def int4_unpack(packed: torch.Tensor, scales: torch.Tensor, g: int) -> torch.Tensor:
    """[N, K] in the scale dtype: ((byte >> 4) - 8) / scale, ((byte & 15) - 8) / scale -- the high nibble is the even element."""
    p = packed.reshape(-1, 1).to(torch.int32)
    nib = torch.cat([p >> 4, p & 15], dim=1).reshape(-1, g) - 8
    out = nib.to(scales.dtype) / scales.reshape(-1, 1)
    return out.reshape(packed.shape[0], -1)


def nvfp4_unpack(packed: torch.Tensor, sb: torch.Tensor, scale_2: torch.Tensor, dtype) -> torch.Tensor:
    p = packed.reshape(-1, 1)
    nib = torch.cat([p & 0xF, p >> 4], dim=1).reshape(-1, 16).long()
    vals = torch.tensor(_E2M1, dtype=torch.float32, device=packed.device)[nib]
    d = sb.reshape(-1).view(torch.float8_e4m3fn).float() * scale_2.float().reshape(()).to(packed.device)
    return (vals * d.reshape(-1, 1)).to(dtype).reshape(packed.shape[0], -1)


def wq_linear(x: torch.Tensor, w_hat: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """The kernel's contract with ANOTHER summation order: exact fp32 products of the decoded weights, fp32 sums, the bias
    added in fp32, one rounding to x's dtype (float64 here: the order does not matter where the test demands equality)."""
    y = x.double() @ w_hat.double().T
    if bias is not None:
        y = y + bias.double()
    return y.to(x.dtype)


# ----------------------------------------------------------------------------------------------- hostmem twins
def _addr(p) -> int:
    if p is None:
        return 0
    return (p.value or 0) if isinstance(p, ctypes.c_void_p) else int(p)


def _host(p, n, dtype) -> torch.Tensor:
    nbytes = int(n) * torch.tensor([], dtype=dtype).element_size()
    buf = (ctypes.c_uint8 * nbytes).from_address(_addr(p))
    return torch.frombuffer(buf, dtype=torch.uint8).view(dtype)


def install(fake) -> None:
    """Give the host-memory stand-in of libmoquant the new entries."""

    def n_scales(mode, axis_size):
        return axis_size if mode == 1 else 1

    def pk(x, scales, out, n, dt, mode, axis_size, inner, stream):
        if n:
            q = int8_pack(_host(x, n, _DT[dt]), _host(scales, n_scales(mode, axis_size), _DT[dt]), mode, axis_size, inner)
            _host(out, n, torch.int8).copy_(q)
        return 0

    def un(q, scales, out, n, dt, mode, axis_size, inner, stream):
        if n:
            y = int8_unpack(_host(q, n, torch.int8), _host(scales, n_scales(mode, axis_size), _DT[dt]), _DT[dt], mode,
                            axis_size, inner)
            _host(out, n, _DT[dt]).copy_(y)
        return 0

    def wq(x, packed, scales, scale_2, bias, y, t, n, k, g, fmt, dt, stream):
        if t > 32 or t <= 0 or k % 32 or dt == 0:
            return -2
        xt = _host(x, t * k, _DT[dt]).reshape(t, k)
        pt = _host(packed, n * k // 2, torch.uint8).reshape(n, k // 2)
        if fmt == 0:
            w_hat = int4_unpack(pt, _host(scales, n * k // g, _DT[dt]), g)
        else:
            w_hat = nvfp4_unpack(pt, _host(scales, n * k // 16, torch.uint8), _host(scale_2, 1, torch.float32), _DT[dt])
        b = _host(bias, n, _DT[dt]) if _addr(bias) else None
        _host(y, t * n, _DT[dt]).copy_(wq_linear(xt, w_hat, b).reshape(-1))
        return 0

    fake.moq_int8_pack = pk
    fake.moq_int8_unpack = un
    fake.moq_wq_linear = wq


# ----------------------------------------------------------------------------------------------- fixture access
class _Fixture(dict):
    files = property(lambda self: list(self))


def fixture():
    """(arrays, cases): compress.npz's `cases` and the arrays of every compress_p*.npz shard as one mapping."""
    cases = json.loads(str(np.load(os.path.join(GOLDEN, "compress.npz"))["cases"]))
    z = _Fixture()
    for path in sorted(glob.glob(os.path.join(GOLDEN, "compress_p*.npz"))):
        with np.load(path) as shard:
            for k in shard.files:
                z[k] = shard[k]
    missing = set(cases["shard_of"]) - set(z)
    assert not missing, f"compress fixture: arrays missing from the shards: {sorted(missing)[:3]}"
    return z, cases


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    if dtype in (torch.float8_e4m3fn, torch.int8):
        return torch.from_numpy(a.copy()).view(dtype)
    return torch.from_numpy(a.copy())


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.detach().cpu(), b.detach().cpu()
    return (a.dtype == b.dtype and a.shape == b.shape
            and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


def build_llama(cases, device="cpu", seed=None):
    """The tiny bf16 Llama the fixture was made from (the `orig/*` weights of export_llama.npz); with `seed`, the same
    architecture under other weights."""
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(architectures=["LlamaForCausalLM"], **cases["config"])
    with torch.device("cpu"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    if seed is None:
        base = np.load(os.path.join(GOLDEN, "export_llama.npz"))
        sd = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
        assert not model.load_state_dict(sd, strict=False).unexpected_keys
    else:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in model.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(p.dtype))
    return model.to(device).eval()


def preset_config(moa, cases, preset):
    """This package's preset as the fixture ran it: weight-only where the reference's CPU run had to be."""
    import copy

    cfg = copy.deepcopy(getattr(moa.model_quant, preset))
    if cases["presets"][preset].get("weight_only"):
        cfg["quant_cfg"]["*input_quantizer"] = {"enable": False}
    return cfg


def quantize_and_compress(moa, z, cases, preset, device="cpu", pattern=None, quant_gemm=False, model=None):
    tokens = torch.from_numpy(z["tokens"]).to(device)
    model = build_llama(cases, device) if model is None else model
    with torch.no_grad():
        moa.quantize(model, preset_config(moa, cases, preset), forward_loop=lambda m: [m(t) for t in tokens])
        was = moa.is_real_quantized(model)
        moa.compress(model, {"compress": pattern or {"default": True}, "quant_gemm": quant_gemm})
    return model, was


def logits_of(model, z, device="cpu"):
    with torch.no_grad():
        return model(torch.from_numpy(z["batch"]).to(device)).logits


def compare_packed(model, z, cases, preset):
    """Packed bytes, scale buffers and wrapper metadata of every linear against the fixture."""
    from model_optimizer_amd.qtensor import QTensorWrapper

    want = cases["presets"][preset]["linears"]
    got = {n for n, m in model.named_modules() if isinstance(getattr(m, "weight", None), QTensorWrapper)}
    assert got == set(want), f"{preset}: compressed linears {sorted(got ^ set(want))[:4]} differ from the reference's"
    for n, rec in want.items():
        m = model.get_submodule(n)
        w, wq = m.weight, m.weight_quantizer
        assert list(w.metadata["shape"]) == rec["shape"] and str(w.metadata["dtype"]) == rec["dtype"], f"{preset} {n}: metadata"
        assert w.metadata["qtensor_class"].__name__ == rec["qtensor_class"], f"{preset} {n}: {w.metadata['qtensor_class']}"
        assert list(w.data.shape) == rec["packed_shape"] and str(w.data.dtype) == rec["packed_dtype"], \
            f"{preset} {n}: packed {tuple(w.data.shape)} {w.data.dtype} vs {rec['packed_shape']} {rec['packed_dtype']}"
        ref = torch.from_numpy(z[f"{preset}/{n}.weight"].copy())
        bad = (w.data.detach().cpu().contiguous().view(torch.uint8) != ref).sum().item()
        assert bad == 0, f"{preset} {n}: {bad} of {ref.numel()} packed bytes differ from the reference's"
        held = {k for k in ("_scale", "_double_scale", "_scale_zeros") if getattr(wq, k, None) is not None}
        assert held == set(rec["scales"]), f"{preset} {n}: scale buffers {held} vs {set(rec['scales'])}"
        for key, srec in rec["scales"].items():
            s = getattr(wq, key).detach().cpu()
            sw = from_bits(z[f"{preset}/{n}.{key}"], TD[srec["dtype"]]).reshape(srec["shape"])
            assert bits_equal(s, sw), f"{preset} {n}.{key}: {s.dtype} {tuple(s.shape)} vs {sw.dtype} {tuple(sw.shape)}, or bits"
