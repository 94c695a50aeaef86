"""Generate tests/golden/nvfp4_static.npz by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference checkout and Triton):  python tests/golden/gen_nvfp4_static.py

The two FP8 scale sweeps are the reference's own Triton kernels (_fp8_scale_sweep_kernel with BLOCKS_PER_PROGRAM=16,
the autotuner bypassed, and _fp8_scale_sweep_hessian_kernel), executed by the Triton interpreter (TRITON_INTERPRET=1)
on CPU tensors; the jit functions are launched directly because the public wrappers insist on CUDA tensors.  Their
candidate scales come from the reference's compute_fp4_scales, as in nvfp4_fp8_scale_sweep_hessian.

The static QDQ kernel (static_blockwise_fp4_fake_quant_kernel) does not run in the interpreter (its libdevice call),
so its expected output is the reference's compute_fp4_scales followed by the numpy restatement of nvfp4_scalar_quant
below:  scale_safe = 1 where the scale is 0 / NaN / inf; q = fp4_round_magnitude(|x| / scale_safe) (a NaN quotient
gives 6); y = (x >= 0 ? q : -q) * scale_safe; a zero scale gives +0 for the whole block.

Arrays: for every case key k (listed in the JSON string `cases`): k_x (bits: uint16 for bf16 / f16, float32 for f32),
k_g (global amax, float32 [1]); QDQ cases k_amax (float32 [n_blocks]) and k_y (bits like k_x); sweep cases
k_best (float32 [n_blocks]); Hessian cases additionally k_h (float32 [n_cin_blocks, 16, 16]).  sum16_p / sum16_s:
float32 rows [4096, 16] and their np.sum(axis=1), the reduction the interpreter runs for the kernels' tl.sum.
"""

import json
import os
import sys

os.environ["TRITON_INTERPRET"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()

from modelopt.torch.kernels.quantization.gemm import nvfp4_fp8_sweep as sweep_mod  # noqa: E402
from modelopt.torch.kernels.quantization.gemm.fp4_kernel import compute_fp4_scales  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def bits(t: torch.Tensor) -> np.ndarray:
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()
    return t.contiguous().numpy().copy()


def fp4_round_np(r):
    return np.where(r <= 0.25, 0.0, np.where(r < 0.75, 0.5, np.where(r <= 1.25, 1.0, np.where(r < 1.75, 1.5, np.where(
        r <= 2.5, 2.0, np.where(r < 3.5, 3.0, np.where(r <= 5.0, 4.0, 6.0))))))).astype(np.float32)


def static_qdq_expected(x: torch.Tensor, amax: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    scale = compute_fp4_scales(amax, g, quantize_block_scales=True).numpy().astype(np.float32).reshape(-1, 1)
    xb = x.float().numpy().reshape(-1, 16)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        zero = scale == 0.0
        safe = np.where(zero | np.isnan(scale) | np.isinf(scale), np.float32(1.0), scale).astype(np.float32)
        m = (fp4_round_np(np.abs(xb) / safe) * safe).astype(np.float32)
        y = np.where(xb >= 0, m, -m).astype(np.float32)
        y = np.where(zero, np.float32(0.0), y).astype(np.float32)
    return torch.from_numpy(y).to(x.dtype).reshape(x.shape)


def run_sweep(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    xf = x.contiguous().view(-1)
    n_blocks = xf.numel() // 16
    cand = sweep_mod.fp8_scale_candidates("cpu").to(torch.float32)
    best = torch.empty(n_blocks, dtype=torch.float32)
    bpp = 16
    sweep_mod._fp8_scale_sweep_kernel.fn[((n_blocks + bpp - 1) // bpp,)](
        xf, cand, g.float().reshape(1), best, n_blocks, BLOCK_SIZE=16, NUM_CANDIDATES=int(cand.numel()),
        BLOCKS_PER_PROGRAM=bpp)
    return best


def run_sweep_hessian(x: torch.Tensor, g: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    xf = x.contiguous().view(-1)
    n_blocks = xf.numel() // 16
    ncb = h.shape[0]
    cout = n_blocks // ncb
    ga = g.float().reshape(())
    cand_amax = sweep_mod.fp8_scale_candidates("cpu").to(torch.float32) * ga
    cand_scale = compute_fp4_scales(cand_amax, ga, quantize_block_scales=True).to(torch.float32)
    best = torch.empty(n_blocks, dtype=torch.float32)
    rpp = sweep_mod._HESSIAN_ROWS_PER_PROGRAM
    sweep_mod._fp8_scale_sweep_hessian_kernel[((cout + rpp - 1) // rpp * ncb,)](
        xf, h.contiguous().float().view(-1), cand_scale, cand_amax, best, cout, ncb, BLOCK_SIZE=16,
        NUM_CANDIDATES=int(cand_amax.numel()), ROWS_PER_PROGRAM=rpp)
    return best


def block_amax(x: torch.Tensor) -> torch.Tensor:
    return x.float().reshape(-1, 16).abs().amax(dim=1)


def main():
    torch.manual_seed(20261016)
    out, cases = {}, {}

    def put(k, kind, x, g, **arrays):
        cases[k] = {"kind": kind, "dtype": {v: n for n, v in DT.items()}[x.dtype], "shape": list(x.shape)}
        out[f"{k}_x"] = bits(x)
        out[f"{k}_g"] = g.float().reshape(1).numpy().copy()
        for name, a in arrays.items():
            out[f"{k}_{name}"] = bits(a) if name == "y" else a.float().numpy().copy()

    # ---- (a) static QDQ: every bf16 pattern, block amax from 2^-24 to 2 x the global amax (FP8-subnormal and flushed
    # block scales, 448 saturation), plus NaN / inf / zero block amax
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).reshape(-1, 16)
    g = torch.tensor(3.0)
    u = torch.linspace(-24.0, 1.0, x.shape[0])
    amax = (g * torch.pow(2.0, u)).float()
    amax[::97] = 0.0
    amax[1::211] = float("nan")
    amax[2::307] = float("inf")
    put("qdq_all_bf16", "qdq", x, g, amax=amax, y=static_qdq_expected(x, amax, g))
    for dn, gv in (("f16", 0.75), ("f32", 1.0e-3)):
        xr = (torch.randn(128, 64) * gv).to(DT[dn])
        am = block_amax(xr) * torch.empty(xr.numel() // 16).uniform_(0.5, 1.5)
        ga = am.max()
        put(f"qdq_rand_{dn}", "qdq", xr, ga, amax=am, y=static_qdq_expected(xr, am, ga))
    xz = torch.zeros(8, 32)
    put("qdq_g0", "qdq", xz, torch.tensor(0.0), amax=torch.zeros(16), y=static_qdq_expected(xz, torch.zeros(16),
                                                                                            torch.tensor(0.0)))
    # tiny global amax (g / 6 <= 2^-24: the FP8 scale of every block flushes)
    xt = (torch.randn(4, 32) * 1e-8).float()
    at = block_amax(xt)
    put("qdq_tiny_g", "qdq", xt, at.max(), amax=at, y=static_qdq_expected(xt, at, at.max()))

    # ---- (b) plain sweep
    for dn in ("bf16", "f16", "f32"):
        w = (torch.randn(96, 128) * 0.02).to(DT[dn])
        w[3] = 0  # all-zero blocks
        w[5, :16] = w[5, :16] * 100.0  # outlier blocks near the global amax
        ga = block_amax(w).max()
        put(f"sweep_{dn}", "sweep", w, ga, best=run_sweep(w, ga))
    wz = torch.zeros(4, 32, dtype=torch.bfloat16)
    put("sweep_g0", "sweep", wz, torch.tensor(0.0), best=run_sweep(wz, torch.tensor(0.0)))
    wn = (torch.randn(8, 64) * 0.1).float()
    wn[0, 3] = float("nan")
    wn[1, 17] = float("inf")
    wn[2, 40] = float("-inf")
    gn = block_amax(wn[3:]).max()
    put("sweep_nan_inf", "sweep", wn, gn, best=run_sweep(wn, gn))
    # heavy-tailed weights: many candidates in play per block
    wh = (torch.randn(64, 64) ** 3 * 0.01).to(torch.bfloat16)
    gh = block_amax(wh).max()
    put("sweep_heavy_bf16", "sweep", wh, gh, best=run_sweep(wh, gh))

    # ---- (c) Hessian sweep: PSD (normalised X^T X of the block's input features), indefinite and non-symmetric Hessians
    for dn, kind in (("bf16", "psd"), ("f16", "indef"), ("f32", "psd"), ("bf16", "indef"), ("f32", "nonsym")):
        cout, cin = 48, 128
        w = (torch.randn(cout, cin) * 0.02).to(DT[dn])
        ncb = cin // 16
        if kind == "psd":
            xs = torch.randn(ncb, 64, 16)
            h = (xs.transpose(1, 2) @ xs) / 64.0
        elif kind == "indef":
            r = torch.randn(ncb, 16, 16)
            h = (r + r.transpose(1, 2)) * 0.5
        else:  # not symmetric: pins the orientation of dw @ H (hdw_j = sum_k dw_k H[k, j])
            xs = torch.randn(ncb, 64, 16)
            h = (xs.transpose(1, 2) @ xs) / 64.0 + torch.randn(ncb, 16, 16).triu(1) * 2.0
        ga = block_amax(w).max()
        put(f"hess_{kind}_{dn}", "hessian", w, ga, h=h, best=run_sweep_hessian(w, ga, h))

    # the 16-term order of tl.sum(axis=1) in the interpreter (np.sum over the contiguous last axis): random rows with
    # terms of mixed magnitude, so that any other order shows
    p = (torch.randn(4096, 16) * torch.pow(2.0, torch.randint(-20, 20, (4096, 16)).float())).abs().numpy()
    out["sum16_p"] = p
    out["sum16_s"] = np.sum(p, axis=1)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "nvfp4_static.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
