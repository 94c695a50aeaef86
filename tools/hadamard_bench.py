"""moq_hadamard / moq_hadamard_mx_qdq (rotating quantizers) on one MI355X: one JSON line, everything in one process.
(i)   moq_hadamard bf16, event-timed after a warm-up, ms and the fraction of 8 TB/s for one read + one write:
        k_states    [8, 8, 4096, 128] (67 MB), B = 128
        act_b128    [262144, 4096] (2.1 GB), B = 128    (in-wave tier)
        act_b4096   the same tensor, B = 4096            (LDS tier)
      each beside moq_mx_fused_amax_convert E2M1 / E4M3 g16 on the same tensor: the same bytes, the yardstick;
      `with_amax`: the same launch with the running abs-max fused (per-tensor max calibration of a rotating quantizer).
(ii)  moq_hadamard_mx_qdq (NVFP4, B = 128) against the two-launch composition (moq_hadamard, moq_mx_fused_amax_convert) and
      against the torch composition (x @ H on hipBLASLt, then the same block QDQ launch), on k_states and on the activation;
      `equal`: fused and composed outputs are the same bits.
(iii) wall-clock of NVFP4_KV_ROTATE_CFG against NVFP4_KV_CFG max calibration of a synthetic Llama-3-8B decoder stack
      (--layers), same loop, same process, the second of two rounds.
Usage (GPU box): python tools/hadamard_bench.py [--layers N] [--reps R] [--no-flow]"""

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


def tensor(shape):
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    flat = x.view(-1, shape[-1])
    for r in range(0, flat.shape[0], 16384):
        n = min(16384, flat.shape[0] - r)
        flat[r:r + n] = torch.randn(n, shape[-1], generator=g, device=DEV).to(torch.bfloat16)
    return x


def rates(ms, gb):
    return {"ms": round(ms, 4), "GBs": round(gb / ms * 1e3, 1), "frac_8TBs": round(gb / ms / 8, 4)}


def transform_part(x, block, reps):
    y = torch.empty_like(x)
    gb = 2 * x.numel() * 2 / 1e9  # one read + one write
    amax = torch.zeros(1, dtype=torch.float32, device=DEV)
    g_amax = ops.reduce_amax(x).float()
    out = {"GB_moved": round(gb, 3), "block": block,
           "hadamard": rates(timed(lambda: ops.hadamard(x, block, out=y), reps), gb),
           "hadamard_with_amax": rates(timed(lambda: ops.hadamard(x, block, running_amax=amax, out=y), reps), gb),
           "mx_qdq_nvfp4_g16": rates(timed(lambda: ops.fused_amax_convert(x, 16, "E2M1", "E4M3", g_amax, out=y), reps), gb)}
    out["hadamard_over_mx_qdq_GBs"] = round(out["hadamard"]["GBs"] / out["mx_qdq_nvfp4_g16"]["GBs"], 3)
    return out


def fused_part(x, block, reps):
    import scipy.linalg

    gb = 2 * x.numel() * 2 / 1e9
    amax = ops.reduce_amax(ops.hadamard(x, block)).float()
    tmp = torch.empty_like(x)
    h = torch.from_numpy(scipy.linalg.hadamard(block)).to(torch.bfloat16).to(DEV)  # entries +-1: exact in bf16

    def composed():
        ops.hadamard(x, block, out=tmp)
        return ops.fused_amax_convert(tmp, 16, "E2M1", "E4M3", amax, out=tmp)

    def torch_composed():
        t = (x.view(-1, block) @ h) * block ** -0.5
        return ops.fused_amax_convert(t.view(x.shape), 16, "E2M1", "E4M3", amax, out=tmp)

    fused = ops.hadamard_block_quant(x, block, 16, amax, (2, 1), (4, 3))
    equal = bool(torch.equal(fused.view(torch.int16), composed().view(torch.int16)))
    ms_f = timed(lambda: ops.hadamard_block_quant(x, block, 16, amax, (2, 1), (4, 3)), reps)
    ms_c = timed(composed, reps)
    ms_t = timed(torch_composed, max(1, reps // 2))
    return {"equal": equal, "fused": rates(ms_f, gb), "two_launches_ms": round(ms_c, 4), "torch_gemm_composition_ms": round(ms_t, 4),
            "two_launches_over_fused": round(ms_c / ms_f, 3), "torch_over_fused": round(ms_t / ms_f, 3)}


def flow_part(layers, rows, seq, n_batches):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(11)
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=8, vocab_size=1024, max_position_embeddings=max(1024, seq),
                      architectures=["LlamaForCausalLM"])
    base = LlamaForCausalLM(cfg).to(torch.bfloat16).eval().to(DEV)
    batches = [torch.randint(0, 1024, (rows, seq), generator=torch.Generator().manual_seed(90 + i)).to(DEV) for i in range(n_batches)]

    def loop(m):
        with torch.no_grad():
            for b in batches:
                m(b)

    out = {"layers": layers, "tokens_per_batch": rows * seq, "batches": n_batches}
    for rep in range(2):  # the first pair warms every kernel and allocation up; the second is reported
        for name in ("NVFP4_KV_CFG", "NVFP4_KV_ROTATE_CFG"):
            model = copy.deepcopy(base)
            cfgq = {"quant_cfg": [{"quantizer_name": "*", "enable": False}] + copy.deepcopy(getattr(moa.model_quant, name)["quant_cfg"]),
                    "algorithm": None}
            moa.quantize(model, cfgq, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            moa.model_quant.calibrate(model, "max", loop)
            torch.cuda.synchronize()
            out[f"{name}_calibrate_s"] = round(time.perf_counter() - t0, 4)
            del model
    out["rotate_over_plain_wallclock"] = round(out["NVFP4_KV_ROTATE_CFG_calibrate_s"] / out["NVFP4_KV_CFG_calibrate_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-flow", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hadamard_bench needs a GPU")
    res = {"metric": "hadamard_rotate"}

    def part(name, fn, *a):
        res[name] = fn(*a)
        print(f"[hadamard_bench] {name}: {json.dumps(res[name])}", file=sys.stderr, flush=True)  # (progress; the result is the last line)

    k = tensor((8, 8, 4096, 128))
    part("k_states", transform_part, k, 128, args.reps * 5)
    part("k_states_fused", fused_part, k, 128, args.reps * 5)
    del k
    act = tensor((262144, 4096))
    part("act_b128", transform_part, act, 128, args.reps)
    part("act_b4096", transform_part, act, 4096, args.reps)
    part("act_fused", fused_part, act, 128, args.reps)
    del act
    if not args.no_flow:
        part("flow", flow_part, args.layers, 4, 1024, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
