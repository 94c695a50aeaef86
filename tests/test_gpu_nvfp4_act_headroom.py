"""moq_block_amax_log2_hist and the nvfp4_act_headroom flow on the GPU.

The kernel against what the reference's calibrator produced on CPU (tests/golden/nvfp4_act_headroom.npz), against the torch
restatement of tests/nvfp4_act_headroom_host.py on Llama-3-8B linear-input shapes and on the neighbours of every bin edge,
repeated launches into one buffer, NaN / Inf blocks; then the whole flow against the same flow with the calibrator forced
onto its torch composition."""

import copy
import math
import warnings

import pytest
import torch

import _moa_import
import nvfp4_act_headroom_host as ah
import nvfp4_flow

moa = _moa_import.load()
from model_optimizer_amd import calib, model_calib, model_quant  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z, CASES = ah.fixture()
K = CASES["kcases"]
FLOW = CASES["flow"]


def _table():
    return moa.ops.log2_hist_thresholds(512, -40.0, 40.0, DEV)


def _state():
    return (torch.zeros(512, dtype=torch.int64, device=DEV), torch.zeros((), dtype=torch.float32, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("k", sorted(K))
def test_kernel_matches_reference_fixture(k):
    counts, rmax, bad = _state()
    for t in ah.case_tensors(Z, k, K[k]):
        moa.ops.block_amax_log2_hist(t.to(DEV), 16, _table(), counts, rmax, bad)
    assert torch.equal(counts.cpu(), ah.case_hist(Z, k)), k
    assert torch.equal(rmax.cpu().reshape(1), torch.from_numpy(Z[f"{k}_rmax"])), k
    assert int(bad) == 0


@pytest.mark.parametrize("k", sorted(K))
def test_calibrator_matches_reference_fixture(k):
    c = K[k]
    tensors = [t.to(DEV) for t in ah.case_tensors(Z, k, c)]
    for j, (anchor, upper, rho) in enumerate(c["triples"]):
        cal = calib.NVFP4ActHeadroomCalibrator((2, 1), None, False, anchor_percentile=anchor, upper_percentile=upper, rho=rho)
        for t in tensors:
            cal.collect(t)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            a = cal.compute_amax()
        msgs = [str(w.message) for w in rec if "[nvfp4_act_headroom]" in str(w.message)]
        kind = "" if not msgs else "range" if "exceeds the FP8 scale range (28672)" in msgs[0] else "lower"
        assert kind == c["warn"][j], (k, j)
        want = Z[f"{k}_amax"][j]
        if math.isnan(float(want)):
            assert a is None
        else:
            assert a.is_cuda and a.dtype == torch.float32 and a.dim() == 0
            assert a.cpu().reshape(1).view(torch.int32).item() == torch.from_numpy(Z[f"{k}_amax"][j:j + 1].copy()).view(torch.int32).item()


def _activation(rows, cols, dtype, seed):
    """Log-normal channel scales with a few massive channels, row by row spread over 2^-12 .. 2^4, whole-zero rows."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    chan = torch.exp(torch.randn(cols, generator=g, device=DEV) * 1.2)
    chan[:6] *= 60.0
    x = torch.empty(rows, cols, dtype=dtype, device=DEV)
    step = 1 << 14
    for r in range(0, rows, step):
        n = min(step, rows - r)
        row = torch.exp2(torch.rand(n, 1, generator=g, device=DEV) * 16.0 - 12.0)
        x[r:r + n] = (torch.randn(n, cols, generator=g, device=DEV) * chan * row).to(dtype)
    x[5::1000] = 0
    return x


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [4096, 14336])
def test_kernel_matches_restatement_on_llama_shapes(cols, dtype):
    x = _activation(64 * 4096, cols, dtype, seed=cols + (1 if dtype == torch.float16 else 0))
    counts, rmax, bad = _state()
    moa.ops.block_amax_log2_hist(x, 16, _table(), counts, rmax, bad)
    want, want_max, want_bad = ah.block_hist_big(x, _table())
    assert int(counts.sum()) > 0.99 * (x.numel() // 16)
    assert torch.equal(counts, want) and torch.equal(rmax, want_max) and int(bad) == want_bad == 0
    assert int((counts > 0).sum()) > 60  # the blocks spread over many bins


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_kernel_on_the_neighbours_of_every_edge(dtype):
    x = ah.neighbours(moa.ops.log2_hist_thresholds(512, -40.0, 40.0), dtype)
    counts, rmax, bad = _state()
    moa.ops.block_amax_log2_hist(x.to(DEV), 16, _table(), counts, rmax, bad)
    want, want_max, _ = ah.block_hist(x, moa.ops.log2_hist_thresholds(512, -40.0, 40.0))
    assert torch.equal(counts.cpu(), want) and torch.equal(rmax.cpu(), want_max) and int(bad) == 0
    # and the restatement agrees with the reference's log2 expression on these values
    amax = x.float().abs().amax(1)
    amax = amax[amax > 0]
    assert torch.equal(torch.bincount(moa.ops.log2_bin_index(amax, 512, -40.0, 40.0), minlength=512), want)


def test_counts_accumulate_over_launches():
    xs = [_activation(1000 + 37 * i, 1024 + 16 * i, torch.bfloat16, seed=i) for i in range(4)]
    counts, rmax, bad = _state()
    total = torch.zeros_like(counts)
    top = torch.zeros((), device=DEV)
    for x in xs:
        moa.ops.block_amax_log2_hist(x, 16, _table(), counts, rmax, bad)
        c, m, _ = ah.block_hist(x, _table())
        total += c
        top = torch.maximum(top, m)
        assert torch.equal(counts, total) and torch.equal(rmax, top)
    # an unaligned view, a ragged last dim and a tail that is not a whole chunk
    x = _activation(33, 1000, torch.float16, seed=9)[:, 3:]
    counts, rmax, bad = _state()
    moa.ops.block_amax_log2_hist(x, 16, _table(), counts, rmax, bad)
    c, m, _ = ah.block_hist(ah.padded(x.contiguous()), _table())
    assert torch.equal(counts, c) and torch.equal(rmax, m)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_nan_and_inf_blocks_set_the_flag_and_are_not_counted(dtype):
    x = _activation(512, 2048, dtype, seed=3)
    clean = x.clone()
    clean[7, 32:48] = 0
    clean[300, 2032:2048] = 0
    want, want_max, _ = ah.block_hist(clean, _table())
    for planted, flag in (((7, 40, float("nan")),), 1), (((300, 2047, float("-inf")),), 2), \
            (((7, 33, float("inf")), (300, 2040, float("nan"))), 3):
        y = clean.clone()
        for r, c, v in planted:
            y[r, c] = v
            y[r, c - 1] = 3.0  # the rest of the poisoned block is not counted either
        counts, rmax, bad = _state()
        moa.ops.block_amax_log2_hist(y, 16, _table(), counts, rmax, bad)
        assert int(bad) == flag
        assert torch.equal(counts, want) and torch.equal(rmax, want_max)
    cal = calib.NVFP4ActHeadroomCalibrator()
    cal.collect(clean)
    y = clean.clone()
    y[0, 0] = float("nan")
    cal.collect(y)
    with pytest.raises(AssertionError, match="detected nan values in amax"):
        cal.compute_amax()


def test_refusals_on_the_device():
    counts, rmax, bad = _state()
    x = torch.randn(4, 64, device=DEV)
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.block_amax_log2_hist(x, 32, _table(), counts, rmax, bad)
    with pytest.raises(moa.MoquantError):
        moa.ops.block_amax_log2_hist(x, 16, _table().cpu(), counts, rmax, bad)
    big = torch.zeros(5000, dtype=torch.int64, device=DEV)
    with pytest.raises(moa.MoquantUnsupported, match="at most 4096"):
        moa.ops.block_amax_log2_hist(x, 16, torch.ones(4999, device=DEV), big, rmax, bad)


def test_other_grids_and_many_bins():
    x = _activation(2048, 1024, torch.bfloat16, seed=21)
    for bins, lo, hi in ((4096, -20.0, 12.0), (64, -200.0, 200.0), (1, -1.0, 1.0), (2, -3.0, 3.0)):
        t = moa.ops.log2_hist_thresholds(bins, lo, hi, DEV)
        counts = torch.zeros(bins, dtype=torch.int64, device=DEV)
        _, rmax, bad = _state()
        moa.ops.block_amax_log2_hist(x, 16, t, counts, rmax, bad)
        want, want_max, _ = ah.block_hist(x, t)
        assert torch.equal(counts, want) and torch.equal(rmax, want_max), bins


def _flow(use_kernel, model, batches, **kw):
    old = calib.NVFP4ActHeadroomCalibrator.use_kernel
    calib.NVFP4ActHeadroomCalibrator.use_kernel = use_kernel
    try:
        cfg = copy.deepcopy(model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
        cfg["algorithm"] = {"method": "nvfp4_act_headroom", **kw}
        with torch.no_grad():
            moa.quantize(model, cfg, lambda m: [m(b) for b in batches])
    finally:
        calib.NVFP4ActHeadroomCalibrator.use_kernel = old
    return ah.input_amaxes(model)


@pytest.mark.parametrize("weights", [None, {"method": "mse", "fp8_scale_sweep": True}])
def test_flow_equals_the_torch_composition(weights):
    model, batches = nvfp4_flow.make(DEV, torch.bfloat16)
    kw = {} if weights is None else {"weight_scale_algorithm": weights}
    a = _flow(True, copy.deepcopy(model), batches, **kw)
    b = _flow(False, copy.deepcopy(model), batches, **kw)
    plain = copy.deepcopy(model)
    cfg = copy.deepcopy(model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG)
    cfg["algorithm"] = "max"
    moa.quantize(plain, cfg, lambda m: [m(x) for x in batches])
    p = ah.input_amaxes(plain)
    assert len(a) == 14 and sorted(a) == sorted(b) == sorted(p)
    for n in a:
        assert torch.equal(a[n], b[n]), n
        assert not torch.equal(a[n], p[n]), n


def test_llama_flow_on_the_device():
    tokens = torch.from_numpy(Z["flow_tokens"].copy()).to(DEV)
    a = _flow(True, ah.build_llama(FLOW["config"], DEV), list(tokens))
    b = _flow(False, ah.build_llama(FLOW["config"], DEV), list(tokens))
    lw = _flow(True, ah.build_llama(FLOW["config"], DEV), list(tokens), layerwise={"enable": True})
    assert sorted(a) == sorted(FLOW["input_quantizers"])
    for n in a:
        assert torch.equal(a[n], b[n]) and torch.equal(a[n], lw[n]), n
    # against the reference's CPU run: the activations differ in the last bits between the devices, the amax is a bin
    # centre -- equal, or one of the 6.4 bins per octave away
    for n in a:
        ratio = float(a[n]) / float(Z[f"flow/{n}.amax"][0])
        assert 2 ** (-1.01 / 6.4) < ratio < 2 ** (1.01 / 6.4), (n, ratio)


def test_calibrators_restored_on_the_device():
    model, batches = nvfp4_flow.make(DEV, torch.bfloat16)
    moa.nn.replace_quant_module(model)
    model_quant.set_quantizer_by_cfg(model, model_quant.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG["quant_cfg"])
    before = {n: m._calibrator for n, m in model.named_modules() if n.endswith("input_quantizer")}
    model_calib.nvfp4_act_headroom_calibrate(model, lambda m: [m(b) for b in batches])
    assert all(before[n] is m._calibrator for n, m in model.named_modules() if n in before)
