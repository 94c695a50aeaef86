"""moq_block_amax_log2_hist (the collect pass of NVFP4ActHeadroomCalibrator) on one MI355X: one JSON line.
Per activation size -- 131072 x 8192 bf16 (2.1 GB, the tensor of bench.py's extra.hist_abs_2048bins) and 8192 x 4096 (67 MB):
  block_hist   the kernel, event-timed after a warm-up: ms and the fraction of 8 TB/s at 2 B per element (its only traffic)
  hist_abs     moq_hist_abs, 2048 bins, on the same tensor in the same process: the yardstick (GB/s parity is the aim)
  torch        the calibrator's torch composition (block abs-max, log2, bins, bincount) on the same tensor, device log2
  equal        the kernel's counts equal the torch restatement's (searchsorted over the same table)
flow: wall-clock of nvfp4_act_headroom calibration of a synthetic Llama-3-8B decoder stack (--layers, random weights with
massive channels) against plain max calibration of the same stack and loop in the same process, and the share of the
quantizers whose amax the two algorithms set differently.
Usage (GPU box): python tools/nvfp4_act_headroom_bench.py [--layers N] [--reps R] [--no-flow]"""

import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _moa_import  # noqa: E402

moa = _moa_import.load()
ops = moa.ops
DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def activation(rows, cols):
    g = torch.Generator(device=DEV).manual_seed(7)
    chan = torch.exp(torch.randn(cols, generator=g, device=DEV))
    chan[:4] *= 50.0
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    for r in range(0, rows, 16384):
        n = min(16384, rows - r)
        x[r:r + n] = (torch.randn(n, cols, generator=g, device=DEV) * chan).to(torch.bfloat16)
    return x


def kernel_part(rows, cols, reps):
    from model_optimizer_amd import calib
    import nvfp4_act_headroom_host as ah

    x = activation(rows, cols)
    table = ops.log2_hist_thresholds(512, -40.0, 40.0, DEV)
    counts = torch.zeros(512, dtype=torch.int64, device=DEV)
    rmax = torch.zeros((), device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.block_amax_log2_hist(x, 16, table, counts, rmax, bad)
    want, want_max, _ = ah.block_hist_big(x, table)
    equal = bool(torch.equal(counts, want) and torch.equal(rmax, want_max))
    ms_k = timed(lambda: ops.block_amax_log2_hist(x, 16, table, counts, rmax, bad), reps)
    edge = float(x.float().abs().max()) if x.numel() < (1 << 28) else float(ops.reduce_amax(x))
    hc = torch.zeros(2048, dtype=torch.int64, device=DEV)
    ms_h = timed(lambda: ops.hist_abs(x, 2048, edge, counts=hc), reps)
    cal = calib.NVFP4ActHeadroomCalibrator()
    cal.use_kernel = False
    with moa.numerics.scale_math("device"):  # the logarithm on the device: the fastest form torch ops have
        ms_t = timed(lambda: cal.collect(x), max(1, reps // 5))
    gb = x.numel() * 2 / 1e9
    return {"activation_GB": round(gb, 3), "equal": equal,
            "block_hist_ms": round(ms_k, 4), "block_hist_GBs": round(gb / ms_k * 1e3, 1), "block_hist_frac_8TBs": round(gb / ms_k / 8, 4),
            "hist_abs_ms": round(ms_h, 4), "hist_abs_GBs": round(gb / ms_h * 1e3, 1), "hist_abs_frac_8TBs": round(gb / ms_h / 8, 4),
            "ratio_block_hist_over_hist_abs_GBs": round(ms_h / ms_k, 3),
            "torch_composition_ms": round(ms_t, 3), "torch_over_kernel": round(ms_t / ms_k, 1)}


def flow_part(layers, rows, seq, n_batches):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(11)
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=8, vocab_size=1024, max_position_embeddings=max(1024, seq),
                      architectures=["LlamaForCausalLM"])
    base = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    with torch.no_grad():
        hot = torch.randperm(4096, generator=torch.Generator().manual_seed(5))[:24]
        base.model.embed_tokens.weight[:, hot] *= 30.0
        for layer in base.model.layers:
            layer.input_layernorm.weight[hot] *= 8.0
            layer.post_attention_layernorm.weight[hot] *= 8.0
    base = base.to(DEV)
    batches = [torch.randint(0, 1024, (rows, seq), generator=torch.Generator().manual_seed(90 + i)).to(DEV) for i in range(n_batches)]

    def loop(m):
        with torch.no_grad():
            for b in batches:
                m(b)

    out = {"layers": layers, "tokens_per_batch": rows * seq, "batches": n_batches}
    amax = {}
    for rep in range(2):  # the first pair warms every kernel and allocation up; the second is reported
        for name, algo in (("max", "max"), ("nvfp4_act_headroom", {"method": "nvfp4_act_headroom"})):
            model = copy.deepcopy(base)
            cfgq = copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
            cfgq["algorithm"] = None
            moa.quantize(model, cfgq, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            moa.model_quant.calibrate(model, algo, loop)
            torch.cuda.synchronize()
            out[f"{name}_calibrate_s"] = round(time.perf_counter() - t0, 4)
            amax[name] = {n: float(m.amax) for n, m in model.named_modules() if n.endswith("input_quantizer") and m.amax is not None}
            del model
    out["headroom_over_max_wallclock"] = round(out["nvfp4_act_headroom_calibrate_s"] / out["max_calibrate_s"], 3)
    out["input_quantizers"] = len(amax["max"])
    out["amax_changed"] = sum(1 for n in amax["max"] if amax["max"][n] != amax["nvfp4_act_headroom"][n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-flow", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nvfp4_act_headroom_bench needs a GPU")
    res = {"metric": "nvfp4_act_headroom", "big": kernel_part(131072, 8192, args.reps), "small": kernel_part(8192, 4096, args.reps * 5)}
    if not args.no_flow:
        res["flow"] = flow_part(args.layers, 4, 1024, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
