"""Static NVFP4 weights on the GPU: the three kernels of moq_nvfp4.hip against the reference's Triton kernels run by
the Triton interpreter (tests/golden/nvfp4_static.npz) and against the torch restatements of tests/nvfp4_host.py on
Llama-width weights (run on the same GPU with one elementwise torch kernel per rounding)."""

import pytest
import torch

import _moa_import
import nvfp4_flow
import nvfp4_host as nh

pytestmark = pytest.mark.gpu
moa = _moa_import.load()

DEV = "cuda:0"
Z, CASES = nh.fixture()


def _kind(kind):
    return [k for k, c in CASES.items() if c["kind"] == kind]


def _llama_weight(rows, cols, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(rows, cols, generator=g, device=DEV) * 0.02
    w[:, :: 97] *= 8.0  # outlier input channels, as in real checkpoints
    return w.to(dtype)


@pytest.mark.parametrize("k", _kind("qdq"))
def test_static_qdq_matches_reference(k):
    c = CASES[k]
    x = nh.case_x(Z, k, c).to(DEV)
    y = moa.ops.nvfp4_static_qdq(x, torch.from_numpy(Z[f"{k}_amax"]).to(DEV), torch.from_numpy(Z[f"{k}_g"]).to(DEV))
    want = nh.case_x({f"{k}_x": Z[f"{k}_y"]}, k, c)
    assert nh.bits_equal(y.cpu(), want), k


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
def test_static_qdq_matches_restatement_llama_width(dt):
    w = _llama_weight(1024, 4096, 7, dt)
    amax = w.float().reshape(-1, 16).abs().amax(1) * torch.rand(w.numel() // 16, device=DEV).add_(0.5)
    ga = amax.max()
    y = moa.ops.nvfp4_static_qdq(w, amax, ga)
    want = nh.static_qdq(w.cpu(), amax.cpu(), ga.cpu())
    bad = (y.cpu().float().view(torch.int32) != want.float().view(torch.int32)).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} elements differ, e.g. x={w[tuple(bad[0])].item()!r} "
                                f"amax={amax[(bad[0, 0] * w.shape[1] + bad[0, 1]) // 16].item()!r} "
                                f"got={y[tuple(bad[0])].item()!r} want={want[tuple(bad[0])].item()!r}")
    out = w.clone()
    moa.ops.nvfp4_static_qdq(out, amax, ga, out=out)  # in place
    assert nh.bits_equal(out, y)


@pytest.mark.parametrize("k", _kind("sweep"))
def test_sweep_matches_reference(k):
    c = CASES[k]
    best = moa.ops.nvfp4_fp8_scale_sweep(nh.case_x(Z, k, c).to(DEV), torch.from_numpy(Z[f"{k}_g"]).to(DEV))
    assert torch.equal(best.cpu().view(torch.int32), torch.from_numpy(Z[f"{k}_best"]).view(torch.int32)), k


@pytest.mark.parametrize("shape", [(4096, 4096), (14336, 4096)])
def test_sweep_matches_restatement_llama_width(shape):
    w = _llama_weight(*shape, seed=shape[0])
    ga = w.float().abs().amax()
    best = moa.ops.nvfp4_fp8_scale_sweep(w, ga)
    want = nh.sweep(w, ga)
    diff = (best.view(torch.int32) != want.view(torch.int32)).sum().item()
    assert diff == 0, f"{diff} of {best.numel()} block picks differ"
    # the search does more than return the max: most blocks pick a scale below it
    assert (best < w.float().reshape(-1, 16).abs().amax(1)).float().mean().item() > 0.2


@pytest.mark.parametrize("k", _kind("hessian"))
def test_sweep_hessian_matches_reference_within_stated_tolerance(k):
    """>= 99.5 % identical picks against the interpreter (its tl.dot is a BLAS call); every other pick a near tie by an
    fp64 re-score (relative gap <= 1e-5); bit-exact against the restatement of the kernel's own order."""
    c = CASES[k]
    x, g, h = nh.case_x(Z, k, c), torch.from_numpy(Z[f"{k}_g"]), torch.from_numpy(Z[f"{k}_h"])
    best = moa.ops.nvfp4_fp8_scale_sweep_hessian(x.to(DEV), g.to(DEV), h.to(DEV)).cpu()
    assert torch.equal(best, nh.sweep_hessian(x, g, h)), k
    want = torch.from_numpy(Z[f"{k}_best"])
    same = best == want
    assert same.float().mean().item() >= 0.995, k
    if not bool(same.all()):
        l_got, l_want = nh.hessian_loss64(x, g, h, best), nh.hessian_loss64(x, g, h, want)
        gap = ((l_got - l_want).abs() / torch.maximum(l_got.abs(), l_want.abs()).clamp_min(1e-300))[~same]
        assert gap.max().item() <= 1e-5, k


@pytest.mark.parametrize("rows,cin,dt", [(1000, 4096, torch.bfloat16), (64, 1024, torch.float32), (37, 48, torch.float16)])
def test_sweep_hessian_matches_restatement(rows, cin, dt):
    w = _llama_weight(rows, cin, rows + cin, dt)
    ncb = cin // 16
    gen = torch.Generator(device=DEV).manual_seed(cin)
    xs = torch.randn(ncb, 32, 16, generator=gen, device=DEV)
    h = xs.transpose(1, 2) @ xs / 32.0
    h[0] -= 0.5 * torch.eye(16, device=DEV)  # one indefinite block
    h[1] += torch.randn(16, 16, generator=gen, device=DEV).triu(1)  # one non-symmetric block: pins dw @ H, not H @ dw
    ga = w.float().abs().amax()
    best = moa.ops.nvfp4_fp8_scale_sweep_hessian(w, ga, h)
    want = nh.sweep_hessian(w, ga, h)
    diff = (best.view(torch.int32) != want.view(torch.int32)).sum().item()
    assert diff == 0, f"{diff} of {best.numel()} block picks differ"


def test_empty_and_refused_on_gpu():
    x = torch.zeros(0, 16, device=DEV, dtype=torch.bfloat16)
    assert moa.ops.nvfp4_fp8_scale_sweep(x, torch.tensor(1.0)).numel() == 0
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_fp8_scale_sweep_hessian(torch.zeros(4, 40, device=DEV), torch.tensor(1.0),
                                              torch.eye(16, device=DEV).repeat(3, 1, 1))


def _boundary_blocks(g: float, two_level: bool, n_blocks: int, seed: int) -> torch.Tensor:
    """|w| values at and one or two ulps around fl(T_j * s_k) -- the rounding thresholds of the candidate scales, where a
    wrong boundary of the kernel's table would put an element on the other side -- mixed with a few block maxima."""
    c = nh.candidates()
    gt = torch.tensor(g)
    s = nh.block_scales(c * gt, gt) if two_level else nh._div(c * gt, 6.0)
    t = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    a0 = (s[:, None] * t[None, :]).reshape(-1)  # fl(T * s), [126 * 7]
    bits = a0.view(torch.int32)
    vals = torch.cat([(bits + d).view(torch.float32) for d in (-2, -1, 0, 1, 2)])  # (int32 + Python int stays int32)
    vals = vals[(vals > 0) & (vals <= g)]
    gen = torch.Generator().manual_seed(seed)
    blocks = vals[torch.randint(0, vals.numel(), (n_blocks, 16), generator=gen)]
    # most blocks draw their values near the thresholds of ONE candidate, so that candidate is in play for the pick
    k = torch.randint(0, 126, (n_blocks,), generator=gen)
    j = torch.randint(0, 7, (n_blocks, 12), generator=gen)
    d = torch.randint(-2, 3, (n_blocks, 12), generator=gen, dtype=torch.int32)
    near = (bits.reshape(126, 7)[k[:, None], j] + d).view(torch.float32)
    blocks[:, :12] = near.clamp(max=g)
    sign = torch.where(torch.rand(n_blocks, 16, generator=gen) < 0.5, -1.0, 1.0)
    return blocks * sign


@pytest.mark.parametrize("g", [1.0, 0.0123, 3.0e-5])
def test_sweeps_on_values_at_the_rounding_boundaries(g):
    x = _boundary_blocks(g, False, 1 << 16, 1).to(DEV)
    ga = torch.tensor(g, device=DEV)
    best = moa.ops.nvfp4_fp8_scale_sweep(x, ga)
    want = nh.sweep(x, ga)
    assert torch.equal(best.view(torch.int32), want.view(torch.int32)), f"{(best != want).sum().item()} picks differ"
    assert best.unique().numel() > 20  # many different candidates win: the boundaries of many candidates are exercised
    xh = _boundary_blocks(g, True, 64 * 32, 2).to(DEV)  # 64 rows x cin 512
    gen = torch.Generator(device=DEV).manual_seed(5)
    xs = torch.randn(32, 16, 16, generator=gen, device=DEV)
    h = xs.transpose(1, 2) @ xs / 16.0 + torch.randn(32, 16, 16, generator=gen, device=DEV).triu(1)
    best = moa.ops.nvfp4_fp8_scale_sweep_hessian(xh, ga, h)
    want = nh.sweep_hessian(xh, ga, h)
    assert torch.equal(best.view(torch.int32), want.view(torch.int32)), f"{(best != want).sum().item()} picks differ"


@pytest.mark.parametrize("cfg", ["NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG", "NVFP4_W4A4_WEIGHT_LOCAL_HESSIAN_CFG"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_presets_end_to_end_on_the_gpu(cfg, dt):
    nvfp4_flow.check(moa, cfg, DEV, dt)
