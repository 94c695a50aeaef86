"""Generate tests/golden/nvfp4_act_headroom.npz by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference checkout):  python tests/golden/gen_nvfp4_act_headroom.py

Calibrator cases (`kcases`), from the reference's NVFP4ActHeadroomCalibrator on CPU tensors.  Per case k:
  k_x<i>     bits of the i-th collected tensor (absent for "allpatterns" cases: block b of the one tensor holds the 16-bit
             pattern b + 1 of the case's dtype at position b % 16, sign alternating, zeros elsewhere -- every positive finite
             value of the dtype is one block amax, the neighbours of every bin edge among them)
  k_hist     int64 [512] (absent when the reference's `_hist` stayed None), k_rmax f32 [1]
  k_amax     f32 [n_triples] compute_amax() per (anchor_percentile, upper_percentile, rho) of `triples` (NaN = None)
  case entry: dtype, shapes, triples, warn (per triple: "", "lower" or "range" -- which wording of the no-headroom warning)

Flow case.  The tiny bf16 Llama of export_llama.npz (`orig/*` read from there) quantized by the reference's mtq.quantize
with the quantizer layout of NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG and algorithm {"method": "nvfp4_act_headroom"} (weights
at max), on CPU: statistics collection does no fake quant, so no step had to be set by hand.
  flow_tokens int64 [batches, B, S];  flow/<input quantizer>.amax f32 [1];  flow_max/<...>.amax the same model under plain
  max calibration (what the headroom amax must differ from);  flow_in/<owner>/<batch> bits of the activation a linear saw in
  that batch, stored once per distinct tensor (`alias`: linear -> the linear it is stored under; q / k / v and gate / up read
  one tensor) -- for the replay of linears whose input the CPU forward of another torch build would not reproduce.
"""

import copy
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
from modelopt.torch.quantization.calib import NVFP4ActHeadroomCalibrator  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TRIPLES = [(1.0, 99.99, 16384.0), (1.0, 100.0, 16384.0), (5.0, 99.0, 1024.0), (50.0, 100.0, 2.0), (0.01, 99.99, 28000.0)]


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().contiguous()
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def from_bits(a: np.ndarray, dtype) -> torch.Tensor:
    if dtype in (torch.bfloat16, torch.float16):
        return torch.from_numpy(a.view(np.int16).copy()).view(dtype)
    return torch.from_numpy(a.copy())


def all_patterns(dtype) -> torch.Tensor:
    """Block b holds the positive finite pattern b + 1 at position b % 16 (odd blocks negated), zeros elsewhere."""
    top = 0x7F80 if dtype == torch.bfloat16 else 0x7C00
    n = top - 1
    x = torch.zeros(n, 16, dtype=torch.int32)
    b = torch.arange(n)
    x[b, b % 16] = (b + 1).to(torch.int32) | ((b % 2) << 15).to(torch.int32)
    return x.to(torch.int16).view(dtype)


def edges_f32(cal) -> torch.Tensor:
    """First fp32 value of bins 1..511 under the reference's own expression (bisection over the bit patterns)."""
    k = torch.arange(1, cal._num_bins, dtype=torch.int64)
    lo, hi = torch.zeros_like(k), torch.full_like(k, 0x7F800000)
    for _ in range(31):
        mid = (lo + hi) >> 1
        at = cal._bin_index(torch.log2(mid.to(torch.int32).view(torch.float32))) >= k
        hi, lo = torch.where(at, mid, hi), torch.where(at, lo, mid)
    return hi


def run_case(out, kc, k, dtype_name, tensors, allpatterns=False):
    c = {"dtype": dtype_name, "shapes": [list(t.shape) for t in tensors], "triples": TRIPLES, "warn": []}
    if allpatterns:
        c["allpatterns"] = True
    else:
        for i, t in enumerate(tensors):
            out[f"{k}_x{i}"] = bits(t)
    amaxes = []
    for j, (anchor, upper, rho) in enumerate(TRIPLES):
        cal = NVFP4ActHeadroomCalibrator((2, 1), None, False, anchor_percentile=anchor, upper_percentile=upper, rho=rho)
        for t in tensors:
            cal.collect(t)
        if j == 0:
            if cal._hist is not None:
                out[f"{k}_hist"] = cal._hist.numpy().copy()
            out[f"{k}_rmax"] = cal._running_max.float().reshape(1).numpy().copy()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            a = cal.compute_amax()
        msgs = [str(w.message) for w in rec if "nvfp4_act_headroom" in str(w.message)]
        c["warn"].append("" if not msgs else "range" if "exceeds the FP8 scale range" in msgs[0] else "lower")
        assert a is None or (a.dtype == torch.float32 and a.dim() == 0)
        amaxes.append(float("nan") if a is None else float(a))
    out[f"{k}_amax"] = np.array(amaxes, dtype=np.float32)
    kc[k] = c


def gen_calibrator_cases(out, rng):
    kc = {}

    def normal(shape, scale=1.0):
        return torch.from_numpy(rng.standard_normal(size=shape).astype(np.float32)) * scale

    def lognormal(shape, sigma):
        mag = torch.from_numpy(np.exp(rng.standard_normal(size=shape) * sigma).astype(np.float32))
        return mag * torch.sign(normal(shape))

    # three dtypes, 2-D and 3-D
    for dn in ("bf16", "f16", "f32"):
        run_case(out, kc, f"rand2d_{dn}", dn, [normal((48, 256), 0.7).to(DT[dn])])
        run_case(out, kc, f"rand3d_{dn}", dn, [normal((3, 20, 128), 0.05).to(DT[dn])])
    # ragged last dim (zero-padded by the calibrator), three collects in a row
    run_case(out, kc, "ragged_bf16", "bf16", [normal((33, 200)).to(torch.bfloat16)])
    run_case(out, kc, "ragged_f32_small", "f32", [normal((7, 5))])
    run_case(out, kc, "three_collects_bf16", "bf16",
             [normal((16, 128), s).to(torch.bfloat16) for s in (0.3, 2.0, 0.01)])
    # whole-zero blocks, an all-zero tensor (compute_amax is None), zeros then data
    xz = normal((16, 128)).to(torch.bfloat16)
    xz[3] = 0
    xz[5, 32:80] = 0
    run_case(out, kc, "zero_blocks_bf16", "bf16", [xz])
    run_case(out, kc, "all_zero_bf16", "bf16", [torch.zeros(4, 64, dtype=torch.bfloat16)])
    run_case(out, kc, "zero_then_data_f16", "f16", [torch.zeros(4, 64, dtype=torch.float16), normal((4, 64)).to(torch.float16)])
    # log-normal activations with a few planted outlier blocks
    xl = lognormal((64, 512), 1.5)
    xl[7, 48:64] *= 3000.0
    xl[40, 0:16] *= 800.0
    xl[63, 496:512] *= 50000.0
    run_case(out, kc, "lognormal_outliers_bf16", "bf16", [xl.to(torch.bfloat16)])
    run_case(out, kc, "lognormal_wide_f32", "f32", [lognormal((32, 256), 6.0)])
    # no-headroom warnings: the rho = 2 triple meets rho * anchor <= upper on most cases above (the "lower" wording), the
    # log-normal ones exceed 28672 (the "range" wording); a distribution narrower than every rho never warns, and two levels
    # 5e10 apart always do
    run_case(out, kc, "narrow_bf16", "bf16", [(torch.ones(32, 128) * 1.5 + normal((32, 128), 1e-3)).to(torch.bfloat16)])
    xr = torch.ones(64, 64)
    xr[:32] *= 1e-6
    xr[32:] *= 5e4
    run_case(out, kc, "two_levels_f32", "f32", [xr])
    # every positive finite bf16 / f16 value as a block amax: both neighbours of every bin edge are among them
    run_case(out, kc, "all_bf16", "bf16", [all_patterns(torch.bfloat16)], allpatterns=True)
    run_case(out, kc, "all_f16", "f16", [all_patterns(torch.float16)], allpatterns=True)
    # fp32: the first value of every bin and its neighbours at -2 .. +2 ulp
    e = edges_f32(NVFP4ActHeadroomCalibrator())
    e = e[e < 0x7F800000]
    near = torch.cat([e + d for d in (-2, -1, 0, 1, 2)]).to(torch.int32).view(torch.float32)
    xe = torch.zeros(near.numel(), 16)
    xe[torch.arange(near.numel()), torch.arange(near.numel()) % 16] = near * torch.where(torch.arange(near.numel()) % 2 == 0, 1.0, -1.0)
    run_case(out, kc, "edges_f32", "f32", [xe])
    # powers of two: exact bin edges of the 80-octave / 512-bin grid wherever 6.4 * exponent is whole
    p2 = torch.zeros(100, 16)
    p2[torch.arange(100), 3] = 2.0 ** torch.arange(-50, 50).float()
    run_case(out, kc, "pow2_f32", "f32", [p2])
    p2b = torch.zeros(100, 16)
    p2b[torch.arange(100), 9] = -(2.0 ** torch.arange(-50, 50).float())
    run_case(out, kc, "pow2_bf16", "bf16", [p2b.to(torch.bfloat16)])
    return kc


def gen_flow(out, rng):
    from transformers import LlamaConfig, LlamaForCausalLM

    base = np.load(os.path.join(HERE, "export_llama.npz"))
    cfgd = json.loads(str(base["cases"]))["config"]
    orig = {k[len("orig/"):]: from_bits(base[k], torch.bfloat16) for k in base.files if k.startswith("orig/")}
    tokens = torch.from_numpy(rng.integers(0, cfgd["vocab_size"], size=(2, 2, 12)).astype(np.int64))
    out["flow_tokens"] = tokens.numpy().copy()

    def fresh():
        model = LlamaForCausalLM(LlamaConfig(architectures=["LlamaForCausalLM"], **cfgd)).to(torch.bfloat16).eval()
        assert not model.load_state_dict(orig, strict=False).unexpected_keys
        return model

    batch = [0]

    def loop(m):
        for b, t in enumerate(tokens):
            batch[0] = b
            m(t)

    names = None
    for tag, algo in (("flow", {"method": "nvfp4_act_headroom"}), ("flow_max", "max")):
        cfg = copy.deepcopy(mtq.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
        cfg["algorithm"] = algo
        model = fresh()
        seen = {}
        if tag == "flow":
            hooks = [m.register_forward_pre_hook(lambda _m, a, _n=n: seen.__setitem__((_n, batch[0]), a[0].detach()))
                     for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "lm_head" not in n]
        q = mtq.quantize(model, cfg, forward_loop=loop)
        got = {n: m.amax for n, m in q.named_modules() if n.endswith("input_quantizer") and m.is_enabled
               and getattr(m, "amax", None) is not None}
        assert got, "no calibrated input quantizer"
        names = names or sorted(got)
        assert sorted(got) == names
        for n, a in got.items():
            assert a.numel() == 1
            out[f"{tag}/{n}.amax"] = a.detach().float().reshape(1).numpy().copy()
        if tag == "flow":
            for h in hooks:
                h.remove()
            alias, owner_of = {}, {}
            for (n, b), x in seen.items():
                key = (x.data_ptr(), b)
                if key not in owner_of:
                    owner_of[key] = n
                    out[f"flow_in/{n}/{b}"] = bits(x)
                    out[f"flow_in_shape/{n}/{b}"] = np.array(x.shape, dtype=np.int64)
                elif owner_of[key] != n:
                    alias[n] = owner_of[key]
            linears = sorted({n for n, _ in seen})
    differ = sum(1 for n in names if out[f"flow/{n}.amax"][0] != out[f"flow_max/{n}.amax"][0])
    assert differ == len(names), "the headroom amax must differ from the max-calibrated one everywhere"
    return dict(config=cfgd, input_quantizers=names, linears=linears, alias=alias, n_batches=int(tokens.shape[0]))


def main():
    torch.manual_seed(20261017)
    rng = np.random.Generator(np.random.Philox(20261017))
    out = {}
    cases = {"kcases": gen_calibrator_cases(out, rng)}
    cases["flow"] = gen_flow(out, rng)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "nvfp4_act_headroom.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases['kcases'])} calibrator cases, {len(cases['flow']['input_quantizers'])} input quantizers, "
          f"{os.path.getsize(path)} bytes")
    print({k: c["warn"] for k, c in cases["kcases"].items() if any(c["warn"])})


if __name__ == "__main__":
    main()
