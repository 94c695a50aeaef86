"""Static NVFP4 weights (E2M1 under FP8-E4M3 block scales relative to a tensor-wide amax), CPU tier.

The torch restatements of tests/nvfp4_host.py -- the checker of the three kernels on the GPU -- are first pinned bit for
bit to the reference's own Triton kernels run by the Triton interpreter (tests/golden/nvfp4_static.npz); then the ops
wrappers are run on CPU tensors with those restatements standing in for libmoquant, and the C-ABI's refusals are checked
on the real library (no kernel is launched)."""

import ctypes

import numpy as np
import pytest
import torch

import _moa_import
import hostmem_backend
import nvfp4_host as nh

moa = _moa_import.load()
from model_optimizer_amd import _lib  # noqa: E402

Z, CASES = nh.fixture()


def _kind(kind):
    return [k for k, c in CASES.items() if c["kind"] == kind]


def test_fixture_covers_the_issue_cases():
    assert len(_kind("qdq")) >= 4 and len(_kind("sweep")) >= 5 and len(_kind("hessian")) >= 4
    x = nh.case_x(Z, "qdq_all_bf16", CASES["qdq_all_bf16"])
    assert x.numel() == 65536 and len(set(x.view(torch.int16).reshape(-1).tolist())) == 65536
    assert any(c["dtype"] == d for c in CASES.values() for d in ("bf16", "f16", "f32"))


def test_sum16_is_the_interpreters_order():
    p = torch.from_numpy(Z["sum16_p"].copy())
    want = torch.from_numpy(Z["sum16_s"].copy())
    assert torch.equal(nh.sum16(p).view(torch.int32), want.view(torch.int32))
    # the recorded rows do tell orders apart: a plain left-to-right sum differs on some of them
    seq = p[:, 0].clone()
    for j in range(1, 16):
        seq = seq + p[:, j]
    assert not torch.equal(seq, want)


def test_candidates_are_the_126_e4m3_values():
    c = nh.candidates()
    assert c.numel() == 126 and bool((c[1:] > c[:-1]).all()) and c[-1].item() == 1.0 and c[0].item() == float(np.float32(2.0 ** -9 / 448))


@pytest.mark.parametrize("k", _kind("qdq"))
def test_static_qdq_restatement_matches_reference(k):
    c = CASES[k]
    x = nh.case_x(Z, k, c)
    y = nh.static_qdq(x, torch.from_numpy(Z[f"{k}_amax"]), torch.from_numpy(Z[f"{k}_g"]))
    want = nh.case_x({f"{k}_x": Z[f"{k}_y"]}, k, c)
    assert nh.bits_equal(y, want), k


@pytest.mark.parametrize("k", _kind("sweep"))
def test_sweep_restatement_matches_reference(k):
    c = CASES[k]
    best = nh.sweep(nh.case_x(Z, k, c), torch.from_numpy(Z[f"{k}_g"]))
    assert torch.equal(best.view(torch.int32), torch.from_numpy(Z[f"{k}_best"]).view(torch.int32)), k


@pytest.mark.parametrize("k", _kind("hessian"))
def test_hessian_restatement_matches_reference_within_stated_tolerance(k):
    """The interpreter's tl.dot is a BLAS call (its own summation order): >= 99.5 % identical picks, and every other
    pick a near tie (fp64 re-score, relative gap <= 1e-5)."""
    c = CASES[k]
    x, g, h = nh.case_x(Z, k, c), torch.from_numpy(Z[f"{k}_g"]), torch.from_numpy(Z[f"{k}_h"])
    best = nh.sweep_hessian(x, g, h)
    want = torch.from_numpy(Z[f"{k}_best"])
    same = best == want
    assert same.float().mean().item() >= 0.995, k
    if not bool(same.all()):
        l_got, l_want = nh.hessian_loss64(x, g, h, best), nh.hessian_loss64(x, g, h, want)
        gap = ((l_got - l_want).abs() / torch.maximum(l_got.abs(), l_want.abs()).clamp_min(1e-300))[~same]
        assert gap.max().item() <= 1e-5, k


def test_fma32_rounds_once():
    # a * b + c whose float64 sum sits exactly on a float32 midpoint only after its own rounding
    a = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    b = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    c = torch.tensor([-(2.0 ** -24)], dtype=torch.float32)
    exact = (1.0 + 2.0 ** -12) ** 2 - 2.0 ** -24  # = 1 + 2^-11 + 2^-24 - 2^-24: representable in f64
    assert nh.fma32(a, b, c).item() == float(np.float32(exact))
    # double-rounding trap: (1 + 2^-12)^2 + 2^-80 lies 2^-80 above the float32 midpoint 1 + 2^-11 + 2^-24; a fused
    # multiply-add rounds up, a float64 sum rounded again to float32 lands on the midpoint and ties to even (down)
    a = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    c = torch.tensor([2.0 ** -80], dtype=torch.float32)
    assert nh.fma32(a, a, c).item() == 1.0 + 2.0 ** -11 + 2.0 ** -23
    assert (a.double() * a.double() + c.double()).float().item() == 1.0 + 2.0 ** -11  # what the trap catches
    assert nh.fma32(-a, a, -c).item() == -(1.0 + 2.0 ** -11 + 2.0 ** -23)


def test_ops_through_the_host_backend(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    k = "qdq_rand_f16"
    x = nh.case_x(Z, k, CASES[k])
    y = moa.ops.nvfp4_static_qdq(x, torch.from_numpy(Z[f"{k}_amax"]), torch.from_numpy(Z[f"{k}_g"]))
    assert nh.bits_equal(y, nh.case_x({f"{k}_x": Z[f"{k}_y"]}, k, CASES[k]))
    k = "sweep_bf16"
    best = moa.ops.nvfp4_fp8_scale_sweep(nh.case_x(Z, k, CASES[k]), torch.from_numpy(Z[f"{k}_g"]))
    assert torch.equal(best, torch.from_numpy(Z[f"{k}_best"]))
    k = "hess_psd_f32"
    best = moa.ops.nvfp4_fp8_scale_sweep_hessian(nh.case_x(Z, k, CASES[k]), torch.from_numpy(Z[f"{k}_g"]),
                                                 torch.from_numpy(Z[f"{k}_h"]))
    assert best.shape == (CASES[k]["shape"][0] * CASES[k]["shape"][1] // 16,)


def test_ops_refusals(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    x = torch.randn(8, 48)
    g = torch.tensor(1.0)
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_fp8_scale_sweep(x, g, block_size=32)  # NVFP4 blocks are 16
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_static_qdq(x, torch.ones(12), g, block_size=32)
    with pytest.raises(moa.MoquantUnsupported):  # cin = 48 is 3 cin-blocks; a Hessian of 2 does not tile the rows
        moa.ops.nvfp4_fp8_scale_sweep_hessian(torch.randn(1, 48), g, torch.eye(16).repeat(2, 1, 1))
    with pytest.raises(ValueError):
        moa.ops.nvfp4_fp8_scale_sweep(torch.randn(3, 10), g)  # not whole blocks
    with pytest.raises(ValueError):
        moa.ops.nvfp4_static_qdq(x, torch.ones(5), g)  # amax count
    with pytest.raises(ValueError):
        moa.ops.nvfp4_fp8_scale_sweep_hessian(x, g, torch.eye(16))  # not [n, 16, 16]
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_fp8_scale_sweep(x.to(torch.float64), g)


def test_ops_refuse_cpu_tensors():
    x = torch.randn(4, 32)
    for call in (lambda: moa.ops.nvfp4_static_qdq(x, torch.ones(8), torch.tensor(1.0)),
                 lambda: moa.ops.nvfp4_fp8_scale_sweep(x, torch.tensor(1.0)),
                 lambda: moa.ops.nvfp4_fp8_scale_sweep_hessian(x, torch.tensor(1.0), torch.eye(16).repeat(2, 1, 1))):
        with pytest.raises(moa.MoquantError, match="must live on the GPU"):
            call()


def test_c_abi_refusals_without_gpu():
    lib = _lib.lib()
    P = ctypes.c_void_p(256)
    assert lib.moq_nvfp4_static_qdq(P, P, P, P, 4, 32, _lib.BF16, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_static_qdq(None, P, P, P, 4, 16, _lib.BF16, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_static_qdq(ctypes.c_void_p(258), P, P, P, 4, 16, _lib.BF16, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_fp8_sweep(P, P, P, 4, 8, _lib.F32, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_fp8_sweep(P, None, P, 4, 16, _lib.F32, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_fp8_sweep_hessian(P, P, P, P, 10, 3, 16, _lib.BF16, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert b"cin" in lib.moq_last_error()
    assert lib.moq_nvfp4_fp8_sweep_hessian(P, P, P, P, 12, 3, 32, _lib.BF16, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_fp8_sweep_hessian(P, P, P, P, 12, 0, 16, _lib.BF16, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_fp8_sweep(None, None, None, 0, 16, _lib.BF16, None) == _lib.MOQ_OK  # nothing to do


# ----------------------------------------------------------------------------------------------- the host layers
import copy  # noqa: E402
import warnings  # noqa: E402

import nvfp4_flow  # noqa: E402


@pytest.fixture
def hostmem_nvfp4(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    return fake


@pytest.mark.parametrize("cfg", ["NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG", "NVFP4_W4A4_WEIGHT_LOCAL_HESSIAN_CFG"])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_presets_end_to_end(hostmem_nvfp4, cfg, dt):
    model = nvfp4_flow.check(moa, cfg, "cpu", dt)
    # the inputs are the dynamic NVFP4 quantizers of the preset
    iq = model.layers[0].q_proj.input_quantizer
    assert iq.is_enabled and iq._block_dynamic and tuple(iq._num_bits) == (2, 1)


def test_static_nvfp4_quantizer_forward_without_calibration(hostmem_nvfp4):
    from model_optimizer_amd.tensor_quantizer import TensorQuantizer

    cfg = moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG["quant_cfg"]["*weight_quantizer"]
    q = TensorQuantizer(moa.QuantizerAttributeConfig(**cfg))
    w = torch.randn(32, 64)
    am = w.reshape(-1, 16).abs().amax(1)
    assert nh.bits_equal(q(w), nh.static_qdq(w, am, am.max()))


def test_non_nvfp4_weights_stay_at_max(hostmem_nvfp4):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    cfg = copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
    cfg["quant_cfg"]["*o_proj.weight_quantizer"] = {"num_bits": 4, "block_sizes": {-1: 16, "type": "static"}}
    moa.quantize(model, cfg, lambda m: [m(b) for b in batches])
    o = model.layers[0].o_proj
    assert not o.weight_quantizer.is_nvfp4_static
    assert torch.equal(o.weight_quantizer._amax.float().reshape(-1), o.weight.float().reshape(-1, 16).abs().amax(1))


def test_local_hessian_warning_stays_without_nvfp4(hostmem_nvfp4):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    cfg = copy.deepcopy(moa.model_quant.INT4_BLOCKWISE_WEIGHT_ONLY_CFG)
    cfg["quant_cfg"]["*weight_quantizer"] = {"num_bits": 4, "block_sizes": {-1: 16, "type": "static"}}
    cfg["algorithm"] = {"method": "local_hessian"}
    with pytest.warns(UserWarning, match="static NVFP4 quantizers only"):
        moa.quantize(model, cfg, lambda m: [m(b) for b in batches])


def test_nvfp4_refusals(hostmem_nvfp4):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    cfg = copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
    cfg["algorithm"] = {"method": "mse", "fp8_scale_sweep": True, "shared_states": {"x": ["q_proj"]}}
    with pytest.raises(moa.MoquantUnsupported):
        moa.quantize(copy.deepcopy(model), cfg, lambda m: [m(b) for b in batches])
    cfg = copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_LOCAL_HESSIAN_CFG)
    cfg["algorithm"] = {"method": "local_hessian", "shared_states": {"x": ["q_proj"]}}
    with pytest.raises(moa.MoquantUnsupported):
        moa.quantize(copy.deepcopy(model), cfg, lambda m: [m(b) for b in batches])
    cfg = copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
    cfg["quant_cfg"]["*weight_quantizer"]["block_sizes"] = {-1: 32, "type": "static", "scale_bits": (4, 3)}
    with pytest.raises(moa.MoquantUnsupported):
        moa.quantize(copy.deepcopy(model), cfg, lambda m: [m(b) for b in batches])
    odd = torch.nn.Sequential(torch.nn.Linear(40, 16, bias=False))  # cin % 16 != 0
    with pytest.raises(moa.MoquantUnsupported):
        moa.quantize(odd, copy.deepcopy(moa.model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG),
                     lambda m: m(torch.randn(4, 40)))
