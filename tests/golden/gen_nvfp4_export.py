"""Generate tests/golden/export_llama_nvfp4.npz by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference checkout):  python tests/golden/gen_nvfp4_export.py

Model part.  The tiny bf16 Llama of export_llama.npz (its `orig/*` weights are read from there, not stored again) is
converted by the reference with the quantizer layout of NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG.  The reference's static
NVFP4 fake quant needs Triton on CUDA, so the calibrated state is SET, not calibrated: every weight quantizer gets a
per-block `_amax` = (the global amax of its q/k/v or gate/up group) x (an E4M3 candidate / 448, drawn from a numpy Philox
stream), is promoted with NVFP4StaticQuantizer.from_tensor_quantizer, and every input quantizer gets an amax of its own
(the exporter then unifies those of fused siblings).  export_hf_checkpoint writes the checkpoint.
  pre/<linear>.amax [n_blocks] f32, .global_amax [1] f32, .in_amax [1] f32
  exp/<key>  bits of every exported tensor that is not a bit copy of orig/<key> (those are listed in `copied`)
  cases: config, linears, dtypes + shapes of every exported key, copied, hf_quant_config, quantization_config

Kernel part (`kcases`), from NVFP4QTensor directly -- get_weights_scaling_factor_from_quantizer / quantize / dequantize for
static cases, quantize / dequantize for dynamic ones: k_x (bits; absent for "allbf16" cases, whose x is every bf16 pattern
in order), k_amax + k_g (static), k_packed, k_scale (E4M3 bytes), k_s2 (f32), k_deq (bits of the dequantized tensor in x's
dtype; some cases).
"""

import copy
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()

import modelopt.torch.quantization as mtq  # noqa: E402
from modelopt.torch.quantization.config import QuantizerAttributeConfig  # noqa: E402
from modelopt.torch.quantization.nn import NVFP4StaticQuantizer, TensorQuantizer  # noqa: E402
from modelopt.torch.quantization.qtensor.nvfp4_tensor import NVFP4QTensor  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GROUPS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    if t.dtype == torch.float8_e4m3fn:
        return t.view(torch.uint8).numpy().copy()
    return t.numpy().copy()


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


def candidates() -> torch.Tensor:
    return torch.arange(1, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).float() / 448.0


def static_quantizer(amax: torch.Tensor, g: torch.Tensor):
    q = TensorQuantizer(QuantizerAttributeConfig(num_bits=(2, 1), block_sizes={-1: 16, "type": "static", "scale_bits": (4, 3)}))
    q.amax = amax.float().reshape(-1, 1)
    return NVFP4StaticQuantizer.from_tensor_quantizer(q, global_amax=g.float().reshape(()))


def gen_model(out, rng):
    from modelopt.torch.export import export_hf_checkpoint
    from safetensors import safe_open
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(HERE, "export_llama.npz"))
    cfgd = json.loads(str(base["cases"]))["config"]
    model = LlamaForCausalLM(LlamaConfig(architectures=["LlamaForCausalLM"], **cfgd)).to(torch.bfloat16)
    orig = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    assert not model.load_state_dict(orig, strict=False).unexpected_keys
    cfg = copy.deepcopy(mtq.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
    cfg["algorithm"] = None  # convert only
    q = mtq.quantize(model, cfg, forward_loop=None)
    mods = {n: m for n, m in q.named_modules() if hasattr(m, "weight_quantizer") and m.weight_quantizer.is_enabled}
    group_g = {}
    for n, m in mods.items():
        parent, _, leaf = n.rpartition(".")
        key = next(((parent, i) for i, grp in enumerate(GROUPS) if leaf in grp), n)
        a = m.weight.detach().float().abs().max()
        group_g[key] = torch.maximum(group_g[key], a) if key in group_g else a
    cand = candidates()
    linears = []
    for i, (n, m) in enumerate(mods.items()):
        parent, _, leaf = n.rpartition(".")
        g = group_g[next(((parent, j) for j, grp in enumerate(GROUPS) if leaf in grp), n)]
        idx = torch.from_numpy(rng.integers(0, 126, size=m.weight.numel() // 16).astype(np.int64))
        amax = g * cand[idx]
        m.weight_quantizer.amax = amax.reshape(-1, 1)
        NVFP4StaticQuantizer.from_tensor_quantizer(m.weight_quantizer, global_amax=g)
        in_amax = torch.tensor(2.0 + 0.375 * i)
        m.input_quantizer.amax = in_amax
        linears.append(n)
        out[f"pre/{n}.amax"] = amax.numpy().copy()
        out[f"pre/{n}.global_amax"] = g.reshape(1).numpy().copy()
        out[f"pre/{n}.in_amax"] = in_amax.reshape(1).numpy().copy()
    with tempfile.TemporaryDirectory() as d:
        export_hf_checkpoint(q, export_dir=d)
        dtypes, shapes, copied = {}, {}, []
        with safe_open(os.path.join(d, "model.safetensors"), "pt") as f:
            for k in f.keys():
                t = f.get_tensor(k)
                dtypes[k], shapes[k] = str(t.dtype), list(t.shape)
                if k in orig and t.dtype == orig[k].dtype and np.array_equal(bits(t), bits(orig[k])):
                    copied.append(k)
                else:
                    out[f"exp/{k}"] = bits(t)
        quant_cfg = json.load(open(os.path.join(d, "hf_quant_config.json")))
        qc = json.load(open(os.path.join(d, "config.json")))["quantization_config"]
    return dict(config=cfgd, linears=linears, dtypes=dtypes, shapes=shapes, copied=copied, hf_quant_config=quant_cfg,
                quantization_config=qc)


def gen_kernel_cases(out, rng):
    kc = {}
    cand = candidates()

    def put(k, kind, x, amax=None, g=None, deq=False, allbf16=False):
        c = {"kind": kind, "dtype": {v: n for n, v in DT.items()}[x.dtype], "shape": list(x.shape)}
        if allbf16:
            c["allbf16"] = True
        else:
            out[f"{k}_x"] = bits(x)
        if kind == "static":
            qz = static_quantizer(amax, g)
            wsf, wsf2 = NVFP4QTensor.get_weights_scaling_factor_from_quantizer(qz, x)
            qt, _, _ = NVFP4QTensor.quantize(x.clone(), 16, wsf, wsf2)
            out[f"{k}_amax"] = amax.float().reshape(-1).numpy().copy()
            out[f"{k}_g"] = g.float().reshape(1).numpy().copy()
        else:
            qt, wsf, wsf2 = NVFP4QTensor.quantize(x.clone(), 16)
        assert wsf.dtype == torch.float8_e4m3fn and qt._quantized_data.dtype == torch.uint8
        out[f"{k}_packed"] = qt._quantized_data.numpy().copy()
        out[f"{k}_scale"] = bits(wsf)
        out[f"{k}_s2"] = wsf2.float().reshape(1).numpy().copy()
        if deq:
            c["deq"] = True
            out[f"{k}_deq"] = bits(qt.dequantize(scale=wsf, double_scale=wsf2, block_sizes={-1: 16}))
        kc[k] = c

    def pick(n):
        return cand[torch.from_numpy(rng.integers(0, 126, size=n).astype(np.int64))]

    # every bf16 pattern (NaN and inf included) under several tensor-wide scales; block amax = g x candidate
    xall = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(-1, 16)
    for i, gv in enumerate((3.0, 0.0421, 1.7e-4, 900.0)):
        g = torch.tensor(gv)
        am = g * pick(xall.shape[0])
        am[5::37] = 0.0  # zero block amax: s = 1 before the rescale
        put(f"all_bf16_{i}", "static", xall, am, g, deq=i == 0, allbf16=True)
    # the same patterns with each block scaled by its own abs-max
    finite = xall.clone()
    finite[~torch.isfinite(finite.float())] = 0
    put("all_bf16_dyn", "dynamic", finite, deq=True)

    # quotients on and around the seven E2M1 bounds: f32 x = bound * d moved by -2..2 ulp, both signs, d the divisor the
    # packer forms (float(scale byte) * scale_2) for several block amax / global amax pairs
    bounds = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    rows, amaxes = [], []
    for gv in (1.0, 0.3, 2.7182817, 6.1e-3, 53.0):
        g = torch.tensor(gv)
        for ci in (10, 57, 83, 100, 125):
            am = g * cand[ci]
            wsf, wsf2 = NVFP4QTensor.get_weights_scaling_factor_from_quantizer(static_quantizer(am.reshape(1), g),
                                                                               torch.zeros(1, 16))
            d = (wsf.float() * wsf2).reshape(())
            vals = []
            for t in bounds:
                a = torch.tensor(t) * d
                for step in (-2, -1, 0, 1, 2):
                    v = a.clone()
                    for _ in range(abs(step)):
                        v = torch.nextafter(v, torch.tensor(float("inf") if step > 0 else 0.0))
                    vals += [v, -v]
            vals = torch.stack(vals)
            pad = (-vals.numel()) % 16
            vals = torch.cat([vals, torch.zeros(pad)]).reshape(-1, 16)
            rows.append((vals, am, g))
    for j, gv in enumerate((1.0, 0.3, 2.7182817, 6.1e-3, 53.0)):
        sel = [r for r in rows if float(r[2]) == float(torch.tensor(gv))]
        x = torch.cat([r[0] for r in sel])
        am = torch.cat([r[1].reshape(1).expand(r[0].shape[0]) for r in sel])
        put(f"bounds_f32_{j}", "static", x, am, torch.tensor(gv), deq=j == 0)

    # zero blocks, the clamp at 448 (small global amax under a zero block amax) and at 2^-9 (block amax far below global)
    xz = (torch.randn(8, 64) * 0.05).to(torch.bfloat16)
    xz[1] = 0
    xz[3, :16] = 0
    am = xz.float().reshape(-1, 16).abs().amax(1)
    put("zeros_bf16", "static", xz, am, am.max(), deq=True)
    put("zeros_bf16_dyn", "dynamic", xz, deq=True)
    xs = (torch.randn(4, 64) * 1e-7).float()
    ams = xs.reshape(-1, 16).abs().amax(1)
    ams[::3] = 0.0
    put("clamp448_f32", "static", xs, ams, torch.tensor(1e-6))
    xl = (torch.randn(4, 64) * 1e-4).to(torch.bfloat16)
    aml = xl.float().reshape(-1, 16).abs().amax(1)
    put("clamp_min_bf16", "static", xl, aml, torch.tensor(4096.0), deq=True)
    put("all_zero_g0", "static", torch.zeros(2, 32, dtype=torch.bfloat16), torch.zeros(4), torch.tensor(0.0))
    put("all_zero_dyn", "dynamic", torch.zeros(2, 32, dtype=torch.bfloat16))
    # negative values that round to zero (nibble 8) next to -0.0 (nibble 0)
    xn = torch.tensor([-1e-3, -0.0, 0.0, -0.12, 0.12, -0.13, 1.0, -1.0] * 2).reshape(1, 16)
    put("neg_to_zero_f32", "static", xn, torch.tensor([3.0]), torch.tensor(3.0), deq=True)
    # f16 / f32 / bf16 weights, static (candidate amax) and dynamic
    for dn in ("f16", "f32", "bf16"):
        w = (torch.randn(64, 128) * 0.03).to(DT[dn])
        w[2, 5] = 0.9
        g = w.float().abs().max()
        put(f"rand_{dn}", "static", w, g * pick(w.numel() // 16), g, deq=True)
        put(f"rand_{dn}_dyn", "dynamic", w, deq=True)
    # values far outside the block amax (saturation at 6) and non-finite inputs in f32
    xo = torch.randn(4, 32)
    xo[0, 0], xo[1, 1], xo[2, 2], xo[3, 3] = float("inf"), float("-inf"), float("nan"), 1e30
    put("nonfinite_f32", "static", xo, torch.full((8,), 0.5), torch.tensor(2.0))
    return kc


def main():
    torch.manual_seed(20261016)
    rng = np.random.Generator(np.random.Philox(20261016))
    out = {}
    cases = gen_model(out, rng)
    cases["kcases"] = gen_kernel_cases(out, rng)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "export_llama_nvfp4.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases['linears'])} linears, {len(cases['kcases'])} kernel cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
