"""Static NVFP4 kernels (moq_nvfp4.hip) on synthetic Llama-3-8B weights (224 bf16 linears, one MI355X): one JSON line.
  qdq    moq_nvfp4_static_qdq over every weight: seconds and fraction of 8 TB/s (2 B read + 2 B written per element and
         4 B of block amax per 16)
  sweep  moq_nvfp4_fp8_sweep over every weight: seconds; and the same search as 126 torch QDQ-and-loss passes (what the
         reference does without Triton) on one q_proj, scaled to the whole model by element count
  hess   moq_nvfp4_fp8_sweep_hessian on one down_proj (4096 x 14336) and one q_proj: ms and fraction of the 157 TF f32 peak
         (2 * 16 * 16 FLOP per block-candidate)
Usage (GPU box): python tools/nvfp4_sweep_bench.py [--layers N]"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _moa_import  # noqa: E402
import nvfp4_host as nh  # noqa: E402

moa = _moa_import.load()
ops = moa.ops
DEV = "cuda:0"
LAYER = [("q", 4096, 4096), ("k", 1024, 4096), ("v", 1024, 4096), ("o", 4096, 4096), ("gate", 14336, 4096),
         ("up", 14336, 4096), ("down", 4096, 14336)]


def timed(fn, reps=1):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def torch_sweep(w, ga):
    """126 QDQ-and-loss passes in torch (the reference's Python sweep of NVFP4MSECalibrator, one pass per candidate)."""
    a = w.reshape(-1, 16).float().abs()
    best = torch.full((a.shape[0],), float("inf"), device=w.device)
    idx = torch.zeros(a.shape[0], dtype=torch.int64, device=w.device)
    c = nh.candidates(w.device)
    for k in range(c.numel()):
        s = c[k] * ga / 6.0
        d = a - nh.fp4_round(a / s) * s
        loss = (d * d).sum(1)
        better = loss < best
        best = torch.where(better, loss, best)
        idx = torch.where(better, k, idx)
    return ga * c[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    args = ap.parse_args()
    torch.manual_seed(0)
    ws = [(torch.randn(co, ci, device=DEV) * 0.02).to(torch.bfloat16) for _ in range(args.layers) for _, co, ci in LAYER]
    n_el = sum(w.numel() for w in ws)
    amax = [w.float().reshape(-1, 16).abs().amax(1) for w in ws]
    ga = [a.max().reshape(1) for a in amax]
    outs = [torch.empty_like(w) for w in ws]

    def qdq_all():
        for w, a, g, o in zip(ws, amax, ga, outs):
            ops.nvfp4_static_qdq(w, a, g, out=o)

    t_qdq = timed(qdq_all, 3)
    t_sweep = timed(lambda: [ops.nvfp4_fp8_scale_sweep(w, g) for w, g in zip(ws, ga)], 1)
    q = ws[0]
    t_torch_q = timed(lambda: torch_sweep(q, ga[0]), 1)
    res = {"metric": "nvfp4_static", "linears": len(ws), "elements": n_el,
           "qdq_s": round(t_qdq, 5), "qdq_frac_8TBs": round(n_el * 4.25 / t_qdq / 8e12, 3),
           "sweep_s": round(t_sweep, 4), "sweep_torch_126pass_qproj_s": round(t_torch_q, 4),
           "sweep_torch_126pass_model_s_scaled": round(t_torch_q * n_el / q.numel(), 2),
           "sweep_speedup_vs_torch": round(t_torch_q * n_el / q.numel() / t_sweep, 1)}
    for name, co, ci in (("down", 4096, 14336), ("q", 4096, 4096)):
        w = next(x for x in ws if tuple(x.shape) == (co, ci))
        ncb = ci // 16
        xs = torch.randn(ncb, 64, 16, device=DEV)
        h = xs.transpose(1, 2) @ xs / 64.0
        g = w.float().abs().amax()
        t = timed(lambda: ops.nvfp4_fp8_scale_sweep_hessian(w, g, h), 3)
        res[f"hess_{name}_ms"] = round(t * 1e3, 3)
        res[f"hess_{name}_frac_157TF"] = round(2 * 16 * 16 * 126 * (w.numel() // 16) / t / 157.3e12, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
