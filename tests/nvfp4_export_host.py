"""TEST INFRASTRUCTURE: torch restatements of moq_nvfp4_pack / moq_nvfp4_unpack (include/moquant.h).

Elementwise torch ops only, every division with a tensor divisor (one IEEE rounding per operation on every device), so
the same code runs on CPU tensors -- where it is pinned bit for bit to what the reference's NVFP4QTensor wrote on CPU
(tests/golden/export_llama_nvfp4.npz) -- and on the GPU, where it checks the kernels on Llama-size weights.  Nothing here
is taken from the reference: the E2M1 cast is restated as a chain of comparisons, not its searchsorted.
"""

from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _div(a: torch.Tensor, b) -> torch.Tensor:
    b = b if isinstance(b, torch.Tensor) else torch.full_like(a, b)
    return a / b


def scale_2_of(global_amax: torch.Tensor) -> torch.Tensor:
    return _div(global_amax.float().reshape(()), 2688.0)


def scale_bytes(s: torch.Tensor) -> torch.Tensor:
    """e4m3_rne(clamp(s, 2^-9, 448)) as bytes."""
    return s.clamp(min=2.0 ** -9, max=448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def static_scales(amax: torch.Tensor, global_amax: torch.Tensor) -> torch.Tensor:
    s = _div(amax.float().reshape(-1), 6.0)
    s = torch.where(s == 0, torch.ones_like(s), s)
    return scale_bytes(_div(s * 448.0, _div(global_amax.float().reshape(()), 6.0)))


def dynamic_scales(x: torch.Tensor, scale_2: torch.Tensor) -> torch.Tensor:
    a = x.reshape(-1, 16).abs().amax(dim=1).float()
    s = _div(a, 6.0 * scale_2.float().reshape(()))
    return scale_bytes(torch.where(s == 0, torch.ones_like(s), s))


def e2m1_codes(q: torch.Tensor) -> torch.Tensor:
    """(q < 0) << 3 | round-half-even magnitude code; a NaN falls through every test and gives 7."""
    a = q.abs()
    w = torch.where
    i8 = lambda v: torch.full(a.shape, v, dtype=torch.uint8, device=a.device)  # noqa: E731
    code = w(a <= 0.25, i8(0), w(a < 0.75, i8(1), w(a <= 1.25, i8(2), w(a < 1.75, i8(3), w(a <= 2.5, i8(4), w(
        a < 3.5, i8(5), w(a <= 5.0, i8(6), i8(7))))))))
    return code | ((q < 0).to(torch.uint8) << 3)


def pack(x: torch.Tensor, amax=None, global_amax=None, scale_2=None, scale=None):
    """(packed uint8 [..., cin / 2], scale bytes uint8 [n_blocks], scale_2 f32 0-dim) -- moq_nvfp4_pack."""
    if scale_2 is None:
        scale_2 = scale_2_of(global_amax if global_amax is not None else x.abs().max())
    s2 = scale_2.float().reshape(()).to(x.device)
    if scale is not None:
        sb = scale.reshape(-1).view(torch.uint8)
    elif amax is not None:
        sb = static_scales(amax.to(x.device), global_amax.to(x.device))
    else:
        sb = dynamic_scales(x, s2)
    d = sb.view(torch.float8_e4m3fn).float() * s2
    q = x.reshape(-1, 16).float() / d.reshape(-1, 1)
    nib = e2m1_codes(q).reshape(-1, 2)
    packed = (nib[:, 1] << 4) | nib[:, 0]
    return packed.reshape(*x.shape[:-1], x.shape[-1] // 2), sb, s2


_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def unpack(packed: torch.Tensor, sb: torch.Tensor, scale_2: torch.Tensor, dtype) -> torch.Tensor:
    p = packed.reshape(-1, 1)
    nib = torch.cat([p & 0xF, p >> 4], dim=1).reshape(-1, 16).long()
    vals = torch.tensor(_VALUES, dtype=torch.float32, device=packed.device)[nib]
    d = sb.reshape(-1).view(torch.float8_e4m3fn).float() * scale_2.float().reshape(()).to(packed.device)
    return (vals * d.reshape(-1, 1)).to(dtype).reshape(*packed.shape[:-1], packed.shape[-1] * 2)


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
    """Give the host-memory stand-in of libmoquant (tests/hostmem_backend.py) the two entries."""

    def pk(x, amax, ga, s2, packed, scale, given, n_blocks, block, dt, stream):
        if block != 16:
            return -2
        if n_blocks == 0:
            return 0
        xt = _host(x, n_blocks * 16, _DT[dt]).reshape(-1, 16)
        sc = _host(scale, n_blocks, torch.uint8)
        p, sb, _ = pack(xt, amax=_host(amax, n_blocks, torch.float32) if _addr(amax) and not given else None,
                        global_amax=_host(ga, 1, torch.float32) if _addr(ga) else None,
                        scale_2=_host(s2, 1, torch.float32), scale=sc.clone() if given else None)
        _host(packed, n_blocks * 8, torch.uint8).copy_(p.reshape(-1))
        if not given:
            sc.copy_(sb)
        return 0

    def un(packed, scale, s2, out, n_blocks, block, dt, stream):
        if block != 16:
            return -2
        if n_blocks == 0:
            return 0
        y = unpack(_host(packed, n_blocks * 8, torch.uint8).reshape(-1, 8), _host(scale, n_blocks, torch.uint8),
                   _host(s2, 1, torch.float32), _DT[dt])
        _host(out, n_blocks * 16, _DT[dt]).copy_(y.reshape(-1))
        return 0

    fake.moq_nvfp4_pack = pk
    fake.moq_nvfp4_unpack = un


# ----------------------------------------------------------------------------------------------- fixture access
def fixture():
    """(npz, cases) of tests/golden/export_llama_nvfp4.npz (tests/golden/gen_nvfp4_export.py)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_llama_nvfp4.npz"))
    return z, json.loads(str(z["cases"]))


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    if dtype == torch.float8_e4m3fn:
        return torch.from_numpy(a.copy()).view(dtype)
    return torch.from_numpy(a.copy())


def case_x(z, k, c) -> torch.Tensor:
    if c.get("allbf16"):
        return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(c["shape"])
    return from_bits(z[f"{k}_x"], DT[c["dtype"]]).reshape(c["shape"])


def case_inputs(z, k, c, device="cpu"):
    """kwargs for ops.nvfp4_quantize / pack(): the block amax and global amax of a static case."""
    if c["kind"] != "static":
        return {}
    return {"amax": torch.from_numpy(z[f"{k}_amax"].copy()).to(device),
            "global_amax": torch.from_numpy(z[f"{k}_g"].copy()).to(device)}


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return (a.dtype == b.dtype and a.shape == b.shape
            and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


_TD = {"torch.bfloat16": torch.bfloat16, "torch.float32": torch.float32, "torch.uint8": torch.uint8,
       "torch.float16": torch.float16, "torch.float8_e4m3fn": torch.float8_e4m3fn}


def build_llama(cases, device="cpu"):
    """The tiny bf16 Llama the fixture was made from: the `orig/*` weights of export_llama.npz."""
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_llama.npz"))
    cfg = LlamaConfig(architectures=["LlamaForCausalLM"], **cases["config"])
    with torch.device("cpu"):
        model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    sd = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    return model.to(device).eval(), sd


def expected_tensor(z, cases, orig, key) -> torch.Tensor:
    dt = _TD[cases["dtypes"][key]]
    if key in cases["copied"]:
        return orig[key]
    return from_bits(z[f"exp/{key}"], dt).reshape(cases["shapes"][key])


def set_fixture_state(moa, model, z, cases, device="cpu"):
    """Convert `model` with the static-NVFP4 preset's quantizer layout and SET the fixture's calibrated state."""
    mq = moa.model_quant
    moa.nn.replace_quant_module(model)
    mq.set_quantizer_by_cfg(model, mq.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG["quant_cfg"])
    mods = dict(model.named_modules())
    for n in cases["linears"]:
        m = mods[n]
        m.weight_quantizer.amax = torch.from_numpy(z[f"pre/{n}.amax"].copy()).reshape(-1, 1).to(device)
        m.weight_quantizer.promote_static_block()
        m.weight_quantizer.global_amax = torch.from_numpy(z[f"pre/{n}.global_amax"].copy()).reshape(()).to(device)
        m.input_quantizer.amax = torch.from_numpy(z[f"pre/{n}.in_amax"].copy()).reshape(()).to(device)
    return model


def compare_state(state, z, cases, orig):
    for key in cases["dtypes"]:
        assert key in state, f"{key} missing from the export"
        want = expected_tensor(z, cases, orig, key)
        got = state[key].detach().cpu()
        assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), \
            f"{key}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
        assert bits_equal(got, want), f"{key}: bytes differ from the reference's export"
    extra = set(state) - set(cases["dtypes"])
    assert not extra, f"the export has tensors the reference does not: {sorted(extra)[:5]}"
