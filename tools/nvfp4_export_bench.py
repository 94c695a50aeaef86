"""The NVFP4 checkpoint packer (moq_nvfp4_pack) on synthetic Llama-3-8B weights (224 bf16 linears, one MI355X) beside
moq_mxfp4_pack on the same tensors in the same run: one JSON line.
  nvfp4_pack   static path (block amax given), event-timed after a warm-up pass: ms, GB/s over the algorithmic bytes
               (2 B read + 4/16 B block amax read + 0.5 B + 1/16 B written per element) and the fraction of 8 TB/s
  mxfp4_pack   block 32: 2 B read + 0.5 B + 1/32 B written per element
  ratio        nvfp4 GB/s / mxfp4 GB/s (the yardstick: at least 0.85)
  nvfp4_unpack 0.5 B + 1/16 B read, 2 B written per element
  fq_vs_unpack on a 4096 x 4096 and a 14336 x 4096 weight with sweep-chosen block amax: the fraction of blocks whose
               unpack(pack(w)) equals the static fake quant of w bit for bit (the two decode with different fp32 factors)
Usage (GPU box): python tools/nvfp4_export_bench.py [--layers N] [--reps R]"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _moa_import  # noqa: E402

moa = _moa_import.load()
ops = moa.ops
DEV = "cuda:0"
LAYER = [("q", 4096, 4096), ("k", 1024, 4096), ("v", 1024, 4096), ("o", 4096, 4096), ("gate", 14336, 4096),
         ("up", 14336, 4096), ("down", 4096, 14336)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    ws = [(torch.randn(co, ci, device=DEV) * 0.02).to(torch.bfloat16) for _ in range(args.layers) for _, co, ci in LAYER]
    n_el = sum(w.numel() for w in ws)
    amax = [w.float().reshape(-1, 16).abs().amax(1) for w in ws]
    ga = [a.max().reshape(1) for a in amax]
    s2 = [g / torch.full_like(g, 2688.0) for g in ga]  # on the device already: no host round trip inside the timed loop
    packed = [ops.nvfp4_quantize(w, 16, amax=a, global_amax=g, scale_2=s) for w, a, g, s in zip(ws[:7], amax, ga, s2)]

    t_nv = timed(lambda: [ops.nvfp4_quantize(w, 16, amax=a, global_amax=g, scale_2=s)
                          for w, a, g, s in zip(ws, amax, ga, s2)], args.reps)
    t_mx = timed(lambda: [ops.mxfp4_quantize(w, 32) for w in ws], args.reps)
    t_un = timed(lambda: [ops.nvfp4_dequantize(p, sc, s, torch.bfloat16) for p, sc, s in packed], args.reps)
    n7 = sum(w.numel() for w in ws[:7])
    gb_nv = n_el * (2 + 4 / 16 + 0.5 + 1 / 16) / t_nv / 1e9
    gb_mx = n_el * (2 + 0.5 + 1 / 32) / t_mx / 1e9
    res = {"metric": "nvfp4_export", "linears": len(ws), "elements": n_el,
           "nvfp4_pack_ms": round(t_nv * 1e3, 3), "nvfp4_pack_GBs": round(gb_nv, 1), "nvfp4_pack_frac_8TBs": round(gb_nv / 8e3, 3),
           "mxfp4_pack_ms": round(t_mx * 1e3, 3), "mxfp4_pack_GBs": round(gb_mx, 1), "mxfp4_pack_frac_8TBs": round(gb_mx / 8e3, 3),
           "ratio_nvfp4_over_mxfp4": round(gb_nv / gb_mx, 3),
           "nvfp4_unpack_ms_7_linears": round(t_un * 1e3, 3),
           "nvfp4_unpack_frac_8TBs": round(n7 * (0.5 + 1 / 16 + 2) / t_un / 8e12, 3)}
    for name, co, ci in (("q", 4096, 4096), ("gate", 14336, 4096)):
        w = next(x for x in ws if tuple(x.shape) == (co, ci))
        g = w.float().abs().amax()
        best = ops.nvfp4_fp8_scale_sweep(w, g)
        fq = ops.nvfp4_static_qdq(w, best, g)
        p, sc, s = ops.nvfp4_quantize(w, 16, amax=best, global_amax=g)
        back = ops.nvfp4_dequantize(p, sc, s, torch.bfloat16)
        same = (fq.view(torch.int16).reshape(-1, 16) == back.view(torch.int16).reshape(-1, 16)).all(1)
        res[f"fq_vs_unpack_identical_blocks_{name}"] = round(same.float().mean().item(), 6)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
