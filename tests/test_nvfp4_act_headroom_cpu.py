"""nvfp4_act_headroom calibration, CPU tier.

First the table of bin edges (ops.log2_hist_thresholds) is checked against the reference's fp32 log2 expression; then the
torch restatement of moq_block_amax_log2_hist (tests/nvfp4_act_headroom_host.py) and the calibrator -- on its torch
composition and through the host-memory stand-in of libmoquant -- against what the reference's calibrator produced on CPU
(tests/golden/nvfp4_act_headroom.npz); then the algorithm: refusals, restored calibrators, the weight algorithms, layerwise,
the tiny-Llama flow against the reference's run, and the exported input_scale."""

import copy
import ctypes
import json
import math
import os
import warnings

import pytest
import torch

import _moa_import
import hostmem_backend
import nvfp4_act_headroom_host as ah
import nvfp4_export_host as eh
import nvfp4_flow
import nvfp4_host as nh

moa = _moa_import.load()
from model_optimizer_amd import _lib, calib, export, model_calib, model_quant  # noqa: E402
from model_optimizer_amd.tensor_quantizer import SequentialQuantizer, TensorQuantizer  # noqa: E402

Z, CASES = ah.fixture()
K = CASES["kcases"]
FLOW = CASES["flow"]
TABLE = moa.ops.log2_hist_thresholds(512, -40.0, 40.0)


def _expr(v):
    return moa.ops.log2_bin_index(v, 512, -40.0, 40.0)


# ----------------------------------------------------------------------------------------------- the table
def test_fixture_covers_the_issue_cases():
    assert {c["dtype"] for c in K.values()} == {"bf16", "f16", "f32"}
    assert {len(s) for c in K.values() for s in c["shapes"]} >= {2, 3}
    assert any(s[-1] % 16 for c in K.values() for s in c["shapes"])
    assert any(len(c["shapes"]) == 3 for c in K.values())
    assert {w for c in K.values() for w in c["warn"]} == {"", "lower", "range"}
    assert math.isnan(float(Z["all_zero_bf16_amax"][0])) and "all_zero_bf16_hist" not in Z.files
    assert any(t[1] == 100.0 for t in K["rand2d_bf16"]["triples"])
    assert os.path.getsize(os.path.join(ah.HERE, "golden", "nvfp4_act_headroom.npz")) < 640 * 1024


def test_threshold_table_is_the_log2_expression():
    assert TABLE.dtype == torch.float32 and TABLE.numel() == 511
    assert bool((TABLE[1:] > TABLE[:-1]).all()) and bool(torch.isfinite(TABLE).all()) and bool((TABLE > 0).all())
    # monotone over every positive finite bf16 and f16 value
    for dt, top in ((torch.bfloat16, 0x7F80), (torch.float16, 0x7C00)):
        v = torch.arange(1, top, dtype=torch.int32).to(torch.int16).view(dt).float()
        b = _expr(v)
        assert bool((b[1:] >= b[:-1]).all())
        assert torch.equal(b, torch.searchsorted(TABLE, v, right=True))
    # random positive fp32 patterns, and every pattern within two ulps of every edge
    g = torch.Generator().manual_seed(7)
    p = torch.randint(1, 0x7F800000, (20_000_000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert torch.equal(_expr(p), torch.searchsorted(TABLE, p, right=True))
    bits = TABLE.view(torch.int32).to(torch.int64)
    near = torch.cat([bits + d for d in (-2, -1, 0, 1, 2)]).to(torch.int32).view(torch.float32)
    want = torch.searchsorted(TABLE, near, right=True)
    assert torch.equal(_expr(near), want)
    # each edge is the FIRST value of its bin
    assert torch.equal(_expr(TABLE), torch.arange(1, 512)) and torch.equal(_expr((bits - 1).to(torch.int32).view(torch.float32)),
                                                                            torch.arange(0, 511))
    # the scalar tail of torch's vectorised log2: the same values in tensors of length 1 .. 17, and with 1 and 8 threads
    for n in range(1, 18):
        rows = near[: (near.numel() // n) * n][: 40 * n].reshape(-1, n)
        got = torch.cat([_expr(r.clone()) for r in rows])
        assert torch.equal(got, want[: got.numel()]), n
    threads = torch.get_num_threads()
    try:
        for t in (1, 8):
            torch.set_num_threads(t)
            assert torch.equal(_expr(p[:1_000_000]), torch.searchsorted(TABLE, p[:1_000_000], right=True))
    finally:
        torch.set_num_threads(threads)


def test_threshold_table_of_other_grids():
    # a grid whose low bins no fp32 value reaches and whose top lies beyond fp32: edges clamp to the smallest pattern / +inf
    t = moa.ops.log2_hist_thresholds(64, -200.0, 200.0)
    assert t.numel() == 63 and bool((t[1:] >= t[:-1]).all()) and bool(torch.isinf(t[-1]))
    g = torch.Generator().manual_seed(8)
    p = torch.randint(1, 0x7F800000, (200_000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    assert torch.equal(moa.ops.log2_bin_index(p, 64, -200.0, 200.0), torch.searchsorted(t, p, right=True))
    assert moa.ops.log2_hist_thresholds(1, -1.0, 1.0).numel() == 0


# ----------------------------------------------------------------------------------------------- fixture cases
@pytest.mark.parametrize("k", sorted(K))
def test_restatement_matches_reference(k):
    counts = torch.zeros(512, dtype=torch.int64)
    rmax = torch.zeros(())
    for t in ah.case_tensors(Z, k, K[k]):
        c, m, bad = ah.block_hist(ah.padded(t), TABLE)
        assert bad == 0
        counts += c
        rmax = torch.maximum(rmax, m)
    assert torch.equal(counts, ah.case_hist(Z, k)), k
    assert torch.equal(rmax.reshape(1), torch.from_numpy(Z[f"{k}_rmax"])), k


@pytest.fixture
def hostmem(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    eh.install(fake)
    ah.install(fake)
    return fake


def _check_case(k):
    c = K[k]
    tensors = ah.case_tensors(Z, k, c)
    for j, (anchor, upper, rho) in enumerate(c["triples"]):
        cal = calib.NVFP4ActHeadroomCalibrator((2, 1), None, False, anchor_percentile=anchor, upper_percentile=upper, rho=rho)
        for t in tensors:
            cal.collect(t)
        if j == 0:
            assert cal._running_max.dtype == torch.float32 and cal._running_max.dim() == 0
            assert torch.equal(cal._running_max.reshape(1), torch.from_numpy(Z[f"{k}_rmax"])), k
            if cal._hist is None:
                assert f"{k}_hist" not in Z.files
            else:
                assert cal._hist.dtype == torch.int64 and torch.equal(cal._hist, ah.case_hist(Z, k)), k
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            a = cal.compute_amax()
        msgs = [str(w.message) for w in rec if "[nvfp4_act_headroom]" in str(w.message)]
        kind = "" if not msgs else "range" if "exceeds the FP8 scale range (28672)" in msgs[0] else "lower"
        assert kind == c["warn"][j], (k, j, msgs)
        if msgs:
            assert "leaves no headroom at rho=" in msgs[0] and "the scale falls back to the top of the calibrated range" in msgs[0]
            assert ("Lower anchor_percentile or raise rho for more headroom." in msgs[0]) == (kind == "lower")
        want = Z[f"{k}_amax"][j]
        if math.isnan(float(want)):
            assert a is None, (k, j)
        else:
            assert a is not None and a.dtype == torch.float32 and a.dim() == 0
            assert a.reshape(1).view(torch.int32).item() == torch.from_numpy(Z[f"{k}_amax"][j:j + 1].copy()).view(torch.int32).item(), (k, j)
        cal.reset()
        assert cal._hist is None and cal._running_max is None and cal.compute_amax() is None


@pytest.mark.parametrize("k", sorted(K))
def test_calibrator_torch_composition_matches_reference(k):
    _check_case(k)


@pytest.mark.parametrize("k", sorted(K))
def test_calibrator_through_the_host_backend_matches_reference(hostmem, k):
    _check_case(k)


def test_constructor_refusals():
    C = calib.NVFP4ActHeadroomCalibrator
    for bad in (0.0, -1.0, 28672.0, 1e9):
        with pytest.raises(ValueError, match=r"rho must be in \(0, 28672.0\)"):
            C(rho=bad)
    for bad in (0.0, -5.0, 100.5):
        with pytest.raises(ValueError, match=r"anchor_percentile must be in \(0, 100\]"):
            C(anchor_percentile=bad)
        with pytest.raises(ValueError, match=r"upper_percentile must be in \(0, 100\]"):
            C(upper_percentile=bad)
    c = C(rho=28671.0, anchor_percentile=100.0, upper_percentile=100.0)
    assert "NVFP4ActHeadroomCalibrator(anchor_percentile=100.0, upper_percentile=100.0, rho=28671.0, block_size=16)" == repr(c)
    assert c.compute_amax() is None


def test_nan_and_inf_are_reported(hostmem):
    x = torch.randn(4, 64)
    for value, word in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "inf")):
        cal = calib.NVFP4ActHeadroomCalibrator()
        cal.collect(x)
        y = x.clone()
        y[2, 17] = value
        cal.collect(y)  # no host sync, no raise
        with pytest.raises(AssertionError, match=f"detected {word} values in amax. {word} in original tensor: True"):
            cal.compute_amax()
    # the torch composition raises where the reference does
    cal = calib.NVFP4ActHeadroomCalibrator()
    cal.use_kernel = False
    y = x.clone()
    y[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="detected nan values in amax"):
        cal.collect(y)


def test_torch_path_then_kernel_path_share_one_state(hostmem):
    """A calibrator that gathered through the torch composition first hands the kernel path a complete state."""
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(8, 64, generator=g) * s for s in (0.01, 1.0, 30.0)]
    want = calib.NVFP4ActHeadroomCalibrator()
    for x in xs:
        want.collect(x)
    for first_torch in (1, 2):
        cal = calib.NVFP4ActHeadroomCalibrator()
        for i, x in enumerate(xs):
            cal.use_kernel = i >= first_torch
            cal.collect(x)
        assert cal._bad is not None
        assert torch.equal(cal._hist, want._hist) and torch.equal(cal._running_max, want._running_max)
        assert torch.equal(cal.compute_amax(), want.compute_amax())
    # a NaN that arrives on the kernel path after a torch-path collect is still reported
    cal = calib.NVFP4ActHeadroomCalibrator()
    cal.use_kernel = False
    cal.collect(xs[0])
    cal.use_kernel = True
    y = xs[1].clone()
    y[3, 3] = float("nan")
    cal.collect(y)
    with pytest.raises(AssertionError, match="detected nan values in amax"):
        cal.compute_amax()


def test_ops_refusals(hostmem):
    ops = moa.ops
    counts, rm, bad = torch.zeros(512, dtype=torch.int64), torch.zeros(()), torch.zeros(1, dtype=torch.int32)
    x = torch.randn(4, 64)
    with pytest.raises(moa.MoquantUnsupported, match="blocks of 16 only"):
        ops.block_amax_log2_hist(x, 32, TABLE, counts, rm, bad)
    with pytest.raises(moa.MoquantUnsupported):
        ops.block_amax_log2_hist(x.double(), 16, TABLE, counts, rm, bad)
    with pytest.raises(moa.MoquantError):
        ops.block_amax_log2_hist(x, 16, TABLE, counts.int(), rm, bad)
    with pytest.raises(moa.MoquantError):
        ops.block_amax_log2_hist(x, 16, TABLE[:-1], counts, rm, bad)
    with pytest.raises(moa.MoquantError):
        ops.block_amax_log2_hist(x, 16, TABLE, counts, rm, bad.long())
    ops.block_amax_log2_hist(torch.zeros(0, 64), 16, TABLE, counts, rm, bad)
    assert int(counts.sum()) == 0
    # a transposed view and a ragged last dim are taken (copied / zero-padded)
    ops.block_amax_log2_hist(x.t(), 16, TABLE, counts, rm, bad)
    assert int(counts.sum()) == 64 and rm.item() == x.abs().max().item()


def test_ops_refuse_cpu_tensors():
    with pytest.raises(moa.MoquantError, match="must live on the GPU"):
        moa.ops.block_amax_log2_hist(torch.randn(4, 64), 16, TABLE, torch.zeros(512, dtype=torch.int64), torch.zeros(()),
                                     torch.zeros(1, dtype=torch.int32))


def test_c_abi_refusals_without_gpu():
    lib = _lib.lib()
    P = ctypes.c_void_p(256)
    bf = _lib.BF16
    f = lib.moq_block_amax_log2_hist
    assert f(P, 4, 64, bf, 32, P, 512, P, P, P, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert b"block size 32" in lib.moq_last_error()
    assert f(P, 4, 8, bf, 8, P, 512, P, P, P, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert f(P, 4, 40, bf, 16, P, 512, P, P, P, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert b"zero-pad" in lib.moq_last_error()
    assert f(P, 4, 64, bf, 16, P, 5000, P, P, P, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert f(ctypes.c_void_p(264), 4, 64, bf, 16, P, 512, P, P, P, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert f(None, 4, 64, bf, 16, P, 512, P, P, P, None) == _lib.MOQ_ERR_INVALID
    assert f(P, 4, 64, bf, 16, None, 512, P, P, P, None) == _lib.MOQ_ERR_INVALID
    assert f(P, 4, 64, bf, 16, P, 512, None, P, P, None) == _lib.MOQ_ERR_INVALID
    assert f(P, 4, 64, bf, 16, P, 512, P, None, P, None) == _lib.MOQ_ERR_INVALID
    assert f(P, 4, 64, bf, 16, P, 512, P, P, None, None) == _lib.MOQ_ERR_INVALID
    assert f(P, 4, 64, bf, 16, P, 0, P, P, P, None) == _lib.MOQ_ERR_INVALID
    assert f(P, -1, 64, bf, 16, P, 512, P, P, P, None) == _lib.MOQ_ERR_INVALID
    assert f(None, 0, 64, bf, 16, P, 512, P, P, P, None) == _lib.MOQ_OK  # nothing to do


# ----------------------------------------------------------------------------------------------- the algorithm
CFG = "NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG"


def _small(dtype=torch.float32):
    model, batches = nvfp4_flow.make("cpu", dtype)
    moa.nn.replace_quant_module(model)
    model_quant.set_quantizer_by_cfg(model, getattr(model_quant, CFG)["quant_cfg"])
    return model, (lambda m: [m(b) for b in batches])


def _calibrators(model):
    return {n: m._calibrator for n, m in model.named_modules() if isinstance(m, TensorQuantizer)}


def _input_amax(model):
    return {n: m.amax.clone() for n, m in model.named_modules() if n.endswith("input_quantizer") and m.amax is not None}


def _weight_state(model):
    out = {}
    for n, m in model.named_modules():
        if n.endswith("weight_quantizer"):
            out[n] = (m._amax.clone(), None if m.global_amax is None else m.global_amax.clone())
    return out


def test_sequential_input_quantizer_is_refused_and_the_model_untouched(hostmem):
    model, loop = _small()
    q0 = model.layers[1].o_proj.input_quantizer
    attrs = dict(getattr(model_quant, CFG)["quant_cfg"]["*input_quantizer"])
    model.layers[1].o_proj.input_quantizer = SequentialQuantizer(TensorQuantizer(moa.QuantizerAttributeConfig(**attrs)),
                                                                 TensorQuantizer(moa.QuantizerAttributeConfig(num_bits=(4, 3))))
    before = _calibrators(model)
    with pytest.raises(NotImplementedError, match="does not support SequentialQuantizer activation quantizers, but "
                                                  "'layers.1.o_proj.input_quantizer' is one wrapping an NVFP4 dynamic-block"):
        model_calib.nvfp4_act_headroom_calibrate(model, loop)
    after = _calibrators(model)
    assert before.keys() == after.keys() and all(before[n] is after[n] for n in before)
    assert not _input_amax(model) and q0.amax is None
    # a bad option or weight method is refused before any swap as well
    with pytest.raises(ValueError, match="rho must be in"):
        model_calib.nvfp4_act_headroom_calibrate(_small()[0], loop, rho=0.0)


def test_calibrators_are_restored(hostmem):
    model, loop = _small()
    before = _calibrators(model)
    model_calib.nvfp4_act_headroom_calibrate(model, loop)
    after = _calibrators(model)
    assert all(before[n] is after[n] for n in before)
    assert len(_input_amax(model)) == 14
    # an exception in the forward loop
    model, loop = _small()
    before = _calibrators(model)
    seen = []

    def failing(m):
        seen.extend(type(q._calibrator).__name__ for n, q in m.named_modules() if n.endswith("input_quantizer"))
        raise RuntimeError("calibration data ran out")

    with pytest.raises(RuntimeError, match="ran out"):
        model_calib.nvfp4_act_headroom_calibrate(model, failing)
    assert seen and set(seen) == {"NVFP4ActHeadroomCalibrator"}
    assert all(before[n] is _calibrators(model)[n] for n in before)


def test_input_amax_is_the_calibrators_and_not_the_max(hostmem):
    model, loop = _small()
    ref, _ = _small()
    model_calib.max_calibrate(ref, loop)
    model_calib.nvfp4_act_headroom_calibrate(model, loop)
    got, plain = _input_amax(model), _input_amax(ref)
    assert got.keys() == plain.keys() and len(got) == 14
    # what a calibrator fed by hand with the same activations gives
    acts = {}
    probe, _ = _small()
    hooks = [m.register_forward_pre_hook(lambda _m, a, _n=n: acts.setdefault(_n, []).append(a[0].detach().clone()))
             for n, m in probe.named_modules() if n.endswith("input_quantizer")]
    for q in probe.modules():
        if isinstance(q, TensorQuantizer):
            q.disable()
    loop(probe)
    for h in hooks:
        h.remove()
    for n in got:
        cal = calib.NVFP4ActHeadroomCalibrator()
        cal.use_kernel = False
        for x in acts[n]:
            cal.collect(x)
        assert torch.equal(got[n].reshape(()), cal.compute_amax()), n
        assert got[n].dtype == torch.float32 and got[n].item() != plain[n].item(), n
    # weights at max: the same state as max_calibrate alone
    ws, wr = _weight_state(model), _weight_state(ref)
    assert all(torch.equal(ws[n][0], wr[n][0]) and torch.equal(ws[n][1], wr[n][1]) for n in wr)


def test_weight_scale_algorithms(hostmem):
    runs = {}
    for name, algo in (("max", None), ("max2", {"method": "max"}), ("mse", {"method": "mse", "fp8_scale_sweep": True}),
                       ("local_hessian", {"method": "local_hessian"}), ("mse_str", "mse")):
        model, loop = _small()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model_calib.nvfp4_act_headroom_calibrate(model, loop, weight_scale_algorithm=algo)
        runs[name] = model
    base = _input_amax(runs["max"])
    for name, model in runs.items():
        got = _input_amax(model)
        assert got.keys() == base.keys() and all(torch.equal(got[n], base[n]) for n in base), name
    # mse with the FP8 sweep: the weight state of mse_calibrate alone.  (local_hessian takes its Hessians in a forward with
    # the input quantizers ON, so its weights legitimately follow the input amax.)
    alone, loop = _small()
    model_calib.mse_calibrate(alone, loop, fp8_scale_sweep=True)
    ws, wa = _weight_state(runs["mse"]), _weight_state(alone)
    assert ws.keys() == wa.keys()
    assert all(torch.equal(ws[n][0], wa[n][0]) and torch.equal(ws[n][1], wa[n][1]) for n in wa)
    assert all(m.weight_quantizer.is_nvfp4_static for m in runs["local_hessian"].layers[0].children())
    assert any(not torch.equal(_weight_state(runs["mse"])[n][0], _weight_state(runs["max"])[n][0]) for n in _weight_state(runs["max"]))
    for bad in ({"method": "awq_lite"}, {"method": "smoothquant"}, "gptq", {"method": None}):
        model, loop = _small()
        before = _calibrators(model)
        with pytest.raises(ValueError, match="weight_scale_algorithm"):
            model_calib.nvfp4_act_headroom_calibrate(model, loop, weight_scale_algorithm=bad)
        assert all(before[n] is _calibrators(model)[n] for n in before)


def test_no_matching_quantizer_warns(hostmem):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    moa.nn.replace_quant_module(model)
    model_quant.set_quantizer_by_cfg(model, model_quant.FP8_DEFAULT_CFG["quant_cfg"])
    ref = copy.deepcopy(model)
    with pytest.warns(UserWarning, match="no NVFP4 dynamic-block input quantizer matched"):
        model_calib.nvfp4_act_headroom_calibrate(model, lambda m: [m(b) for b in batches])
    model_calib.max_calibrate(ref, lambda m: [m(b) for b in batches])
    a, b = _input_amax(model), _input_amax(ref)
    assert a and all(torch.equal(a[n], b[n]) for n in b)


def test_through_quantize_and_calibrate(hostmem):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    cfg = copy.deepcopy(getattr(model_quant, CFG))
    cfg["algorithm"] = {"method": "nvfp4_act_headroom", "rho": 4096.0, "anchor_percentile": 2.0, "upper_percentile": 100.0,
                        "weight_scale_algorithm": {"method": "mse", "fp8_scale_sweep": True}}
    moa.quantize(model, cfg, lambda m: [m(b) for b in batches])
    direct, loop = _small()
    model_calib.nvfp4_act_headroom_calibrate(direct, loop, rho=4096.0, anchor_percentile=2.0, upper_percentile=100.0,
                                             weight_scale_algorithm={"method": "mse", "fp8_scale_sweep": True})
    a, b = _input_amax(model), _input_amax(direct)
    assert len(a) == 14 and all(torch.equal(a[n], b[n]) for n in b)
    with pytest.raises(ValueError, match="unknown nvfp4_act_headroom option"):
        model_quant.calibrate(_small()[0], {"method": "nvfp4_act_headroom", "percentile": 3.0}, loop)
    assert "nvfp4_act_headroom" in model_quant._AMAX_ONLY_ALGORITHMS


def _llama_quantized(algorithm, loop=None, device="cpu"):
    model = ah.build_llama(FLOW["config"], device)
    cfg = copy.deepcopy(getattr(model_quant, CFG))
    cfg["algorithm"] = algorithm
    tokens = torch.from_numpy(Z["flow_tokens"].copy()).to(device)
    with torch.no_grad():
        moa.quantize(model, cfg, loop or (lambda m: [m(t) for t in tokens]))
    return model


def _replay_loop(device="cpu"):
    cache = {}

    def x_of(name, b):
        owner = FLOW["alias"].get(name, name)
        if (owner, b) not in cache:
            shape = [int(v) for v in Z[f"flow_in_shape/{owner}/{b}"]]
            cache[(owner, b)] = ah.from_bits(Z[f"flow_in/{owner}/{b}"], torch.bfloat16).reshape(shape).to(device)
        return cache[(owner, b)]

    def loop(model):
        for b in range(FLOW["n_batches"]):
            for name in FLOW["linears"]:
                model.get_submodule(name)(x_of(name, b))

    return loop, x_of


def test_llama_flow_matches_the_reference_run(hostmem):
    want = {n: torch.from_numpy(Z[f"flow/{n}.amax"].copy()).reshape(()) for n in FLOW["input_quantizers"]}
    plain = {n: torch.from_numpy(Z[f"flow_max/{n}.amax"].copy()).reshape(()) for n in FLOW["input_quantizers"]}
    # the reference's per-linear inputs replayed: every amax, bit for bit
    loop, x_of = _replay_loop()
    got = ah.input_amaxes(_llama_quantized({"method": "nvfp4_act_headroom"}, loop))
    assert sorted(got) == sorted(want)
    for n in want:
        assert torch.equal(got[n], want[n]), n
        assert not torch.equal(got[n], plain[n]), n
    # the model's own forward: wherever it reproduces the stored activations (the first linears always do)
    seen = {}
    model = ah.build_llama(FLOW["config"])
    tokens = torch.from_numpy(Z["flow_tokens"].copy())
    batch = [0]
    hooks = [m.register_forward_pre_hook(lambda _m, a, _n=n: seen.__setitem__((_n, batch[0]), a[0].detach().clone()))
             for n, m in model.named_modules() if n in FLOW["linears"]]

    def own_loop(m):
        for b, t in enumerate(tokens):
            batch[0] = b
            m(t)

    cfg = copy.deepcopy(getattr(model_quant, CFG))
    cfg["algorithm"] = {"method": "nvfp4_act_headroom"}
    with torch.no_grad():
        moa.quantize(model, cfg, own_loop)
    got = ah.input_amaxes(model)
    same = [n for n in FLOW["linears"] if all(eh.bits_equal(seen[(n, b)], x_of(n, b)) for b in range(FLOW["n_batches"]))]
    assert "model.layers.0.self_attn.q_proj" in same
    for n in same:
        assert torch.equal(got[f"{n}.input_quantizer"], want[f"{n}.input_quantizer"]), n


def test_layerwise_gives_the_whole_model_amax(hostmem):
    whole = ah.input_amaxes(_llama_quantized({"method": "nvfp4_act_headroom"}))
    by_layer = ah.input_amaxes(_llama_quantized({"method": "nvfp4_act_headroom", "layerwise": {"enable": True}}))
    assert sorted(whole) == sorted(by_layer) and len(whole) == 14
    for n in whole:
        assert torch.equal(whole[n], by_layer[n]), n


def test_exported_input_scale_is_the_headroom_amax(hostmem, tmp_path):
    from safetensors import safe_open

    loop, _ = _replay_loop()
    model = _llama_quantized({"method": "nvfp4_act_headroom", "weight_scale_algorithm": {"method": "mse", "fp8_scale_sweep": True}},
                             loop)
    amax = ah.input_amaxes(model)
    plain = {n: torch.from_numpy(Z[f"flow_max/{n}.amax"].copy()).reshape(()) for n in FLOW["input_quantizers"]}
    export.export_hf_checkpoint(model, export_dir=str(tmp_path))
    with safe_open(os.path.join(tmp_path, "model.safetensors"), "pt") as f:
        state = {k: f.get_tensor(k) for k in f.keys()}
    groups = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"))
    checked = 0
    for n in FLOW["linears"]:
        parent, _, leaf = n.rpartition(".")
        sibs = next((g for g in groups if leaf in g), (leaf,))
        unified = torch.stack([amax[f"{parent}.{s}.input_quantizer"] for s in sibs]).max()  # the exporter's rule for fused siblings
        got = state[f"{n}.input_scale"]
        assert got.dtype == torch.float32
        assert got.reshape(()).item() == (unified / torch.tensor(2688.0)).item(), n
        assert got.reshape(()).item() != (plain[f"{n}.input_quantizer"] / torch.tensor(2688.0)).item(), n
        checked += 1
    assert checked == 14
    assert json.load(open(os.path.join(tmp_path, "hf_quant_config.json")))["quantization"]["quant_algo"] == "NVFP4"
