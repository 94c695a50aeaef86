"""Generate tests/golden/compress.npz (+ compress_p*.npz shards) by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference checkout):  python tests/golden/gen_compress.py

Model part.  The tiny bf16 Llama of export_llama.npz (its `orig/*` weights are read from there, not stored again) goes
through `mtq.quantize(model, PRESET, forward_loop)` and `mtq.compress(model, {"compress": ..., "quant_gemm": False})` for
every preset of PRESETS, the calibration data being a numpy Philox stream of token ids stored as `tokens`.
  <preset>/<linear>.weight   the packed bytes of the QTensorWrapper (uint8 view)
  <preset>/<linear>._scale, ._double_scale   the weight quantizer's scale buffers (bits; fp8 as bytes)
  <preset>/logits, <preset>/mlp/logits       bf16 bits of model(batch).logits after compress({"default": True}) and after
                                             compress({"*mlp*": False, "default": True})
  cases: config, presets -> {linears -> {shape, dtype, qtensor_class, packed_shape, packed_dtype, scale dtypes}, mlp_compressed}
A preset whose ACTIVATION fake quantization does not run on the reference's CPU path (MXFP4, NVFP4: dynamic blocks need its
CUDA extension) is pinned weight-only, `weight_only` holding the reason, and without the `*mlp*` variant, whose mlp weights
would be fake-quantized by the same extension (`mlp_dropped`); a preset that still fails is left out, see `dropped`.

INT8QTensor part (`icases`): i_x (bits), optional i_scales_in, i_q (int8), i_scales (bits), i_deq (bits).

No single committed file may pass 1 MiB, so the arrays are spread over compress_p00.npz, compress_p01.npz, ...; compress.npz
holds `cases` with the shard of every key (tests/compress_host.py: fixture() puts them together again).
"""

import copy
import glob
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()

import modelopt.torch.quantization as mtq  # noqa: E402
from modelopt.torch.quantization.qtensor import QTensorWrapper  # noqa: E402
from modelopt.torch.quantization.qtensor.int8_tensor import INT8QTensor  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PRESETS = ("INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "INT4_AWQ_CFG", "FP8_DEFAULT_CFG", "INT8_DEFAULT_CFG", "MXFP4_DEFAULT_CFG",
           "NVFP4_DEFAULT_CFG")
SHARD_BYTES = 880 * 1024


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    if t.dtype in (torch.float8_e4m3fn, torch.int8):
        return t.view(torch.uint8).numpy().copy()
    return t.numpy().copy()


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


def gen_models(out, rng):
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(HERE, "export_llama.npz"))
    cfgd = json.loads(str(base["cases"]))["config"]
    orig = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    tokens = torch.from_numpy(rng.integers(0, cfgd["vocab_size"], size=(2, 2, 12)).astype(np.int64))
    batch = torch.from_numpy(rng.integers(0, cfgd["vocab_size"], size=(2, 9)).astype(np.int64))
    out["tokens"], out["batch"] = tokens.numpy().copy(), batch.numpy().copy()

    def fresh():
        model = LlamaForCausalLM(LlamaConfig(architectures=["LlamaForCausalLM"], **cfgd)).to(torch.bfloat16).eval()
        assert not model.load_state_dict(orig, strict=False).unexpected_keys
        return model

    def loop(m):
        for t in tokens:
            m(t)

    presets, dropped = {}, {}
    for preset in PRESETS:
        entry = {}
        cfg = copy.deepcopy(getattr(mtq, preset))
        try:  # the dynamic-block fake quantization of an ACTIVATION needs the reference's CUDA extension: such a preset is
            with torch.no_grad():  # pinned weight-only (input quantizers off), which leaves the compress branch as it is
                mtq.quantize(fresh(), copy.deepcopy(cfg), forward_loop=loop)(batch)
        except (AssertionError, RuntimeError) as e:
            entry["weight_only"] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
            cfg["quant_cfg"] = list(cfg["quant_cfg"]) + [{"quantizer_name": "*input_quantizer", "enable": False}]
        for variant, pattern in (("", {"default": True}), ("mlp/", {"*mlp*": False, "default": True})):
            part = {}
            try:
                with torch.no_grad():
                    q = mtq.quantize(fresh(), copy.deepcopy(cfg), forward_loop=loop)
                    mtq.compress(q, {"compress": pattern, "quant_gemm": False})
                    logits = q(batch).logits
            except Exception as e:  # this flow does not run on the reference's CPU path
                reason = f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"
                if variant:  # (the mlp linears stay fake-quantized: dynamic-block WEIGHT fake quantization, CUDA again)
                    entry["mlp_dropped"] = reason
                else:
                    dropped[preset] = reason
                break
            assert torch.isfinite(logits.float()).all()
            part[f"{preset}/{variant}logits"] = bits(logits)
            packed = [n for n, m in q.named_modules() if isinstance(getattr(m, "weight", None), QTensorWrapper)]
            if variant:
                assert packed and not any("mlp" in n for n in packed)
                entry["mlp_compressed"] = packed
                out.update(part)
                continue
            linears = {}
            for n in packed:
                m = q.get_submodule(n)
                w, wq = m.weight, m.weight_quantizer
                part[f"{preset}/{n}.weight"] = w.data.contiguous().view(torch.uint8).numpy().copy()
                rec = {"shape": list(w.metadata["shape"]), "dtype": str(w.metadata["dtype"]),
                       "qtensor_class": w.metadata["qtensor_class"].__name__, "packed_shape": list(w.data.shape),
                       "packed_dtype": str(w.data.dtype), "scales": {}}
                for key in ("_scale", "_double_scale", "_scale_zeros"):
                    s = getattr(wq, key, None)
                    if s is not None:
                        part[f"{preset}/{n}.{key}"] = bits(s)
                        rec["scales"][key] = {"dtype": str(s.dtype), "shape": list(s.shape)}
                linears[n] = rec
            entry["linears"] = linears
            out.update(part)
        if preset not in dropped:
            presets[preset] = entry
            print(f"{preset}: {len(entry['linears'])} linears, {entry.get('weight_only')}, {entry.get('mlp_dropped')}")
    return dict(config=cfgd, presets=presets, dropped=dropped)


def gen_int8_cases(out, rng):
    ic = {}

    def put(k, x, axis=None, block_sizes=None, scales=None):
        qt, sc = INT8QTensor.quantize(x.clone(), scales=None if scales is None else scales.clone(), axis=axis,
                                      block_sizes=block_sizes)
        deq = qt.dequantize(scale=sc, block_sizes=block_sizes)
        out[f"{k}_x"], out[f"{k}_q"], out[f"{k}_scales"], out[f"{k}_deq"] = bits(x), bits(qt._quantized_data), bits(sc), bits(deq)
        if scales is not None:
            out[f"{k}_scales_in"] = bits(scales)
        ic[k] = {"dtype": {v: n for n, v in DT.items()}[x.dtype], "shape": list(x.shape), "axis": axis,
                 "block": None if block_sizes is None else block_sizes[-1], "scales_shape": list(sc.shape),
                 "q_shape": list(qt._quantized_data.shape), "given": scales is not None}

    for dn, dt in DT.items():
        for shape in ((7, 48), (1, 16), (40, 96)):
            x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dt)
            # amax 127 -> scale exactly 1: ties at .5 (round half to even), both signs
            ties = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 63.5, -63.5, 126.5, -126.5, 127.0, -127.0], dtype=dt)
            xt = x.clone()
            xt.view(-1)[: min(12, xt.numel())] = ties[: min(12, xt.numel())]
            xt.view(-1)[-1] = 127.0
            put(f"i_{dn}_{shape[0]}x{shape[1]}_pt", xt)
            put(f"i_{dn}_{shape[0]}x{shape[1]}_ax0", x, axis=0)
            put(f"i_{dn}_{shape[0]}x{shape[1]}_b32", x, block_sizes={-1: 32})
            # given scales far below amax / 127: quotients beyond +-127.5 saturate, ties at +-127.5 and +-128.5 included
            sg = torch.full((shape[0], 1), 0.0078125, dtype=dt)
            xs = x.clone()
            xs.view(-1)[:6] = torch.tensor([127.5, -127.5, 128.5, -128.5, 300.0, -300.0], dtype=dt) * 0.0078125
            put(f"i_{dn}_{shape[0]}x{shape[1]}_given", xs, axis=0, scales=sg)
    return ic


def main():
    warnings.simplefilter("ignore")
    torch.manual_seed(20261019)
    rng = np.random.Generator(np.random.Philox(20261019))
    out = {}
    cases = gen_models(out, rng)
    cases["icases"] = gen_int8_cases(out, rng)
    for old in glob.glob(os.path.join(HERE, "compress_p*.npz")):
        os.unlink(old)
    shards, where, size = [{}], {}, 0
    for k, a in out.items():
        if size and size + a.nbytes > SHARD_BYTES:
            shards.append({})
            size = 0
        shards[-1][k] = a
        where[k] = len(shards) - 1
        size += a.nbytes
    cases["shard_of"] = where
    np.savez_compressed(os.path.join(HERE, "compress.npz"), cases=np.array(json.dumps(cases)))
    for i, s in enumerate(shards):
        p = os.path.join(HERE, f"compress_p{i:02d}.npz")
        np.savez_compressed(p, **s)
        print(f"wrote {p}: {os.path.getsize(p)} bytes")
    print(f"{len(cases['presets'])} presets, dropped {cases['dropped']}, {len(cases['icases'])} INT8 cases")


if __name__ == "__main__":
    main()
