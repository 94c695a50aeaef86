"""Generate tests/golden/hadamard_rotate.npz by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference checkout):  python tests/golden/gen_hadamard_rotate.py

The reference's rotation, normalized_hadamard_transform (nn/functional.py:81-138), only forwards to the CUDA-only package
fast_hadamard_transform, which does not exist on ROCm or on this host.  So the name TensorQuantizer calls is replaced by
the torch restatement of tests/hadamard_host.py -- the way the
reference's unit tests replace it (tests/unit/torch/quantization/test_tensor_quant_cpu.py:124, :198, :270).  Everything
else -- the order of pre_quant_scale, rotation, block reshape, collect, fake quant, rotate_back, the calibrators, the
attention wrappers -- is the reference's code.

(a) `qcases`: per case k a reference TensorQuantizer on one input: k_x (bits), k_cal (what the calibration-mode call
    returned), k_amax (f32, the calibrated amax in the buffer's shape), k_y (the quantized forward).  INT8 / FP8 per tensor,
    INT8 / FP8 per channel (axis 0), static INT4 blocks of 16; rotate = True, mode rotate_back, rotate_fp32, block_size 8;
    bf16 / f16 / f32; inputs of 4 x 96.
(b) `llama_fp8`: the tiny bf16 Llama of export_llama.npz (`orig/*` and tokens read from there) under FP8 weights and
    inputs, the weight quantizers with rotate {"enable": True, "mode": "rotate_back", "block_size": 16}, `*[qk]_bmm_quantizer`
    rotating (k FP8 per tensor, q disabled), the embedding table's quantizer off: every `_amax` (llama_fp8/<quantizer>)
    and the logits of the first batch.  The reference cannot fake-quantize dynamic NVFP4 on CPU, hence FP8 here.
(c) `llama_kv`: the same model calibrated -- no forward under quantization -- under the reference's NVFP4_KV_ROTATE_CFG behind
    a disable-all entry: every bmm-quantizer amax (llama_kv/<quantizer>).
(d) `presets`: the reference's NVFP4_KV_CFG and NVFP4_KV_ROTATE_CFG dicts as JSON.
"""

import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402

ref_shim.install()

import hadamard_host  # noqa: E402
import modelopt.torch.quantization as mtq  # noqa: E402
from modelopt.torch.quantization.config import QuantizerAttributeConfig  # noqa: E402
from modelopt.torch.quantization.nn import TensorQuantizer  # noqa: E402
from modelopt.torch.quantization.nn.modules import tensor_quantizer as tq_mod  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def rotate_fn(inputs, rotate_fp32=False, block_size=None):
    """normalized_hadamard_transform with the kernel call replaced by the restatement (fp32 arithmetic, one rounding to
    inputs.dtype: with rotate_fp32 or without); block_size None = the largest power-of-two divisor of the last dim.  Only
    valid sizes reach this generator."""
    dim = inputs.shape[-1]
    return hadamard_host.fwht(inputs, block_size or dim & -dim)


tq_mod.normalized_hadamard_transform = rotate_fn


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


FORMATS = {"int8": {"num_bits": 8, "axis": None}, "fp8": {"num_bits": (4, 3), "axis": None},
           "int8_pc": {"num_bits": 8, "axis": 0}, "fp8_pc": {"num_bits": (4, 3), "axis": 0},
           "int4_g16": {"num_bits": 4, "block_sizes": {-1: 16, "type": "static"}}}
ROTATES = {"rot": True, "back": {"enable": True, "mode": "rotate_back"}, "fp32": {"enable": True, "rotate_fp32": True},
           "b8": {"enable": True, "block_size": 8}}


def gen_quantizer_cases(out, rng):
    cases = {}
    for dn, dt in DT.items():
        x = (torch.from_numpy(rng.standard_normal(size=(4, 96)).astype(np.float32))
             * torch.exp2(torch.from_numpy(rng.integers(-6, 3, size=(4, 96)).astype(np.float32)))).to(dt)
        for fn, fmt in FORMATS.items():
            for rn, rot in ROTATES.items():
                k = f"{fn}_{rn}_{dn}"
                q = TensorQuantizer(QuantizerAttributeConfig(**copy.deepcopy(fmt), rotate=copy.deepcopy(rot)))
                q.enable_calib()
                q.disable_quant()
                cal = q(x)
                q.load_calib_amax()
                q.enable_quant()
                q.disable_calib()
                y = q(x)
                assert y.dtype == dt and cal.dtype == dt
                out[f"{k}_x"], out[f"{k}_cal"], out[f"{k}_y"] = bits(x), bits(cal), bits(y)
                out[f"{k}_amax"] = q._amax.detach().float().numpy().copy()
                cases[k] = {"dtype": dn, "format": fn, "rotate": rn, "amax_shape": list(q._amax.shape), "repr": q.extra_repr()}
    return cases


def _llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(HERE, "export_llama.npz"))
    c = json.loads(str(base["cases"]))
    orig = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    tokens = [torch.from_numpy(base[f"tokens{i}"].copy()) for i in range(c["n_batches"])]
    model = LlamaForCausalLM(LlamaConfig(architectures=["LlamaForCausalLM"], **c["config"])).to(torch.bfloat16).eval()
    assert not model.load_state_dict(orig, strict=False).unexpected_keys
    return model, tokens, c["config"]


LLAMA_FP8_ENTRIES = [
    {"quantizer_name": "*weight_quantizer",
     "cfg": {"num_bits": (4, 3), "axis": None, "rotate": {"enable": True, "mode": "rotate_back", "block_size": 16}}},
    {"quantizer_name": "*q_bmm_quantizer", "cfg": {"rotate": True}, "enable": False},
    {"quantizer_name": "*k_bmm_quantizer", "cfg": {"num_bits": (4, 3), "axis": None, "rotate": True}},
    # (the reference also wraps nn.Embedding; this package converts linears and attention only, so the table stays out)
    {"quantizer_name": "*embed_tokens*", "enable": False},
]


def gen_llama(out):
    info = {}
    model, tokens, cfgd = _llama()
    info["config"], info["n_batches"] = cfgd, len(tokens)
    cfg = copy.deepcopy(mtq.FP8_DEFAULT_CFG)
    assert isinstance(cfg["quant_cfg"], list)
    cfg["quant_cfg"] = list(cfg["quant_cfg"]) + copy.deepcopy(LLAMA_FP8_ENTRIES)
    cfg["algorithm"] = "max"
    with torch.no_grad():
        q = mtq.quantize(model, cfg, forward_loop=lambda m: [m(t) for t in tokens])
        names = []
        for n, m in q.named_modules():
            if isinstance(m, TensorQuantizer) and getattr(m, "_amax", None) is not None:
                out[f"llama_fp8/{n}"] = m._amax.detach().float().reshape(-1).numpy().copy()
                names.append(n)
        rotating = sorted(n for n, m in q.named_modules() if isinstance(m, TensorQuantizer) and m.rotate_is_enabled)
        out["llama_fp8_logits"] = bits(q(tokens[0]).logits)
    info["fp8_amax"], info["fp8_rotating"] = names, rotating
    assert any(n.endswith("k_bmm_quantizer") for n in names) and any(n.endswith("q_bmm_quantizer") for n in rotating)

    model, tokens, _ = _llama()
    cfg = {"quant_cfg": [{"quantizer_name": "*", "enable": False}] + copy.deepcopy(mtq.NVFP4_KV_ROTATE_CFG["quant_cfg"]),
           "algorithm": "max"}
    with torch.no_grad():
        q = mtq.quantize(model, cfg, forward_loop=lambda m: [m(t) for t in tokens])
    names = []
    for n, m in q.named_modules():
        if isinstance(m, TensorQuantizer) and n.endswith("bmm_quantizer") and getattr(m, "_amax", None) is not None:
            out[f"llama_kv/{n}"] = m._amax.detach().float().reshape(-1).numpy().copy()
            names.append(n)
    info["kv_amax"] = names
    assert len(names) == 2 * cfgd["num_hidden_layers"]
    return info


def main():
    torch.manual_seed(20261018)
    rng = np.random.Generator(np.random.Philox(20261018))
    out = {}
    cases = {"qcases": gen_quantizer_cases(out, rng), "llama": gen_llama(out),
             "llama_fp8_entries": LLAMA_FP8_ENTRIES,
             "presets": {n: getattr(mtq, n) for n in ("NVFP4_KV_CFG", "NVFP4_KV_ROTATE_CFG")}}
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "hadamard_rotate.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases['qcases'])} quantizer cases, {len(cases['llama']['fp8_amax'])} + "
          f"{len(cases['llama']['kv_amax'])} llama amax, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
