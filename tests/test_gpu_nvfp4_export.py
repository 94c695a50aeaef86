"""Static NVFP4 checkpoint export on the GPU: moq_nvfp4_pack / moq_nvfp4_unpack against every case the reference's
NVFP4QTensor wrote on CPU (tests/golden/export_llama_nvfp4.npz), against the torch restatements of
tests/nvfp4_export_host.py on Llama-size weights (run on the same GPU, one elementwise torch kernel per rounding), and the
exporter against the reference's checkpoint of the tiny Llama and against the same flow run on CPU through the stand-in.

unpack(export) is NOT compared with the model's fake-quantized weight: the two decode with different fp32 factors
(1 / (448 / (g / 6)) against g / 2688); tools/nvfp4_export_bench.py measures how often they agree."""

import copy

import pytest
import torch

import _moa_import
import hostmem_backend
import nvfp4_export_host as eh
import nvfp4_flow
import nvfp4_host as nh

pytestmark = pytest.mark.gpu
moa = _moa_import.load()
from model_optimizer_amd import export, qtensor  # noqa: E402

DEV = "cuda:0"
Z, CASES = eh.fixture()
K = CASES["kcases"]


def _llama_weight(rows, cols, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(rows, cols, generator=g, device=DEV) * 0.02
    w[:, :: 97] *= 8.0  # outlier input channels, as in real checkpoints
    return w.to(dtype)


@pytest.mark.parametrize("k", sorted(K))
def test_kernels_match_reference(k):
    c = K[k]
    x = eh.case_x(Z, k, c).to(DEV)
    packed, scale, s2 = moa.ops.nvfp4_quantize(x, 16, **eh.case_inputs(Z, k, c, DEV))
    assert torch.equal(s2.cpu().reshape(1), torch.from_numpy(Z[f"{k}_s2"])), k
    assert torch.equal(scale.cpu().view(torch.uint8).reshape(-1), torch.from_numpy(Z[f"{k}_scale"]).reshape(-1)), k
    want = torch.from_numpy(Z[f"{k}_packed"])
    bad = (packed.cpu() != want).nonzero()
    assert bad.shape[0] == 0, f"{k}: {bad.shape[0]} packed bytes differ, first at {bad[0].tolist()}"
    if c.get("deq"):
        y = moa.ops.nvfp4_dequantize(packed, scale, s2, x.dtype)
        assert eh.bits_equal(y.cpu(), eh.from_bits(Z[f"{k}_deq"], x.dtype).reshape(x.shape)), k
    # the scale bytes handed back in: the same nibbles
    again, _, _ = moa.ops.nvfp4_quantize(x, 16, scale=scale, scale_2=s2)
    assert torch.equal(again, packed), k


@pytest.mark.parametrize("shape", [(4096, 4096), (14336, 4096)])
def test_pack_matches_restatement_llama_size(shape):
    w = _llama_weight(*shape, seed=11)
    g = w.float().abs().amax()
    best = moa.ops.nvfp4_fp8_scale_sweep(w, g)
    packed, scale, s2 = moa.ops.nvfp4_quantize(w, 16, amax=best, global_amax=g)
    wp, wsb, ws2 = eh.pack(w, amax=best, global_amax=g)
    assert torch.equal(s2, ws2) and torch.equal(scale.view(torch.uint8).reshape(-1), wsb)
    bad = (packed != wp).sum().item()
    assert bad == 0, f"{bad} of {packed.numel()} packed bytes differ"
    assert scale.view(torch.uint8).unique().numel() > 20
    y = moa.ops.nvfp4_dequantize(packed, scale, s2, torch.bfloat16)
    assert eh.bits_equal(y, eh.unpack(wp, wsb, ws2, torch.bfloat16))
    # dynamic path on the same weight
    pd, sd, s2d = moa.ops.nvfp4_quantize(w, 16)
    wpd, wsd, ws2d = eh.pack(w)
    assert torch.equal(s2d, ws2d) and torch.equal(sd.view(torch.uint8).reshape(-1), wsd) and torch.equal(pd, wpd)


@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
def test_pack_matches_restatement_other_dtypes(dt):
    w = _llama_weight(1024, 4096, 5, dt)
    amax = w.float().reshape(-1, 16).abs().amax(1) * nh.candidates(DEV)[torch.randint(60, 126, (w.numel() // 16,), device=DEV)]
    g = w.float().abs().amax()
    packed, scale, s2 = moa.ops.nvfp4_quantize(w, 16, amax=amax, global_amax=g)
    wp, wsb, ws2 = eh.pack(w, amax=amax, global_amax=g)
    assert torch.equal(scale.view(torch.uint8).reshape(-1), wsb) and torch.equal(packed, wp)
    assert eh.bits_equal(moa.ops.nvfp4_dequantize(packed, scale, s2, dt), eh.unpack(wp, wsb, ws2, dt))


@pytest.mark.parametrize("g", [1.0, 0.0123, 3.0e-5, 700.0])
def test_pack_on_quotients_at_the_rounding_bounds(g):
    """f32 x = bound * d moved by -2..2 ulp for every divisor d = float(scale byte) * scale_2 a candidate block amax
    gives under g: a quotient rounded on the wrong side of a bound changes a nibble."""
    gt = torch.tensor(g)
    c = nh.candidates()
    amax_c = gt * c
    d = eh.static_scales(amax_c, gt).view(torch.float8_e4m3fn).float() * eh.scale_2_of(gt)
    t = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    a0 = (d[:, None] * t[None, :]).reshape(126, 7)
    vals = torch.stack([(a0.view(torch.int32) + s).view(torch.float32) for s in (-2, -1, 0, 1, 2)], dim=2).reshape(126, 35)
    x = torch.cat([vals, -vals, torch.zeros(126, 10)], dim=1).reshape(126 * 5, 16).to(DEV)
    amax = amax_c.repeat_interleave(5).to(DEV)
    packed, scale, _ = moa.ops.nvfp4_quantize(x, 16, amax=amax, global_amax=gt.to(DEV))
    wp, wsb, _ = eh.pack(x, amax=amax, global_amax=gt.to(DEV))
    assert torch.equal(scale.view(torch.uint8).reshape(-1), wsb)
    assert torch.equal(packed, wp), f"{(packed != wp).sum().item()} bytes differ"
    assert set((wp.reshape(-1) & 7).tolist()) == set(range(8))


def test_empty_and_refused_on_gpu():
    x = torch.zeros(0, 16, device=DEV, dtype=torch.bfloat16)
    p, s, _ = moa.ops.nvfp4_quantize(x, 16, amax=torch.zeros(0, device=DEV), global_amax=torch.tensor(1.0))
    assert p.numel() == 0 and s.numel() == 0
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_quantize(torch.zeros(4, 40, device=DEV))
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_quantize(torch.zeros(4, 64, device=DEV), 32)


def _fixture_model():
    model, orig = eh.build_llama(CASES, DEV)
    return eh.set_fixture_state(moa, model, Z, CASES, DEV), orig


def test_export_from_reference_state_is_byte_identical(tmp_path):
    import json
    import os

    from safetensors import safe_open

    model, orig = _fixture_model()
    state = export.export_state_dict(model, torch.bfloat16, lambda: model(torch.ones([1, 2], dtype=torch.long, device=DEV)))
    eh.compare_state(state, Z, CASES, orig)
    assert state["model.layers.0.self_attn.q_proj.weight"].is_cuda
    cfg = export.hf_quant_config(model)
    assert cfg["quantization"] == CASES["hf_quant_config"]["quantization"]
    conv, want = export.convert_hf_quant_config_format(cfg), dict(CASES["quantization_config"])
    conv.pop("producer"), want.pop("producer")
    assert conv == want
    export.save_checkpoint(state, str(tmp_path), cfg)
    with safe_open(os.path.join(tmp_path, "model.safetensors"), "pt") as f:
        eh.compare_state({k: f.get_tensor(k) for k in f.keys()}, Z, CASES, orig)
    assert json.load(open(os.path.join(tmp_path, "hf_quant_config.json")))["quantization"]["quant_algo"] == "NVFP4"


def _quantize_and_export(device, cfg_name, monkeypatch=None):
    if monkeypatch is not None:
        fake = hostmem_backend.install(monkeypatch, moa)
        nh.install(fake)
        eh.install(fake)
    model, batches = nvfp4_flow.make(device, torch.bfloat16)
    moa.quantize(model, copy.deepcopy(getattr(moa.model_quant, cfg_name)), lambda m: [m(b) for b in batches])
    state = export.export_state_dict(model, torch.bfloat16, lambda: model(batches[0][:2]))
    return model, {k: v.detach().cpu() for k, v in state.items()}


def test_quantize_then_export_equals_the_cpu_flow(monkeypatch):
    """NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG end to end on the device, then the export: the weight side never sees a GEMM, so
    weight / weight_scale / weight_scale_2 equal the same flow on CPU (through the stand-in) byte for byte; input_scale
    depends on activations and follows the two-bf16-ulp rule of test_gpu_export._compare_exported."""
    _, got = _quantize_and_export(DEV, "NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG")
    with monkeypatch.context() as mp:
        _, want = _quantize_and_export("cpu", "NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG", mp)
    assert set(got) == set(want)
    n_packed = 0
    ulp = torch.finfo(torch.bfloat16).eps
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if k.endswith("input_scale"):
            assert ((g.float() - w.float()).abs() <= 2 * ulp * w.float().abs() + 1e-30).all(), f"{k}: {g.item()} vs {w.item()}"
        else:
            assert eh.bits_equal(g, w), k
            n_packed += k.endswith(".weight")
    assert n_packed == 14
    assert got["layers.0.q_proj.weight"].dtype == torch.uint8 and got["layers.0.q_proj.weight_scale"].dtype == torch.float8_e4m3fn


def test_local_hessian_export_structure():
    model, state = _quantize_and_export(DEV, "NVFP4_W4A4_WEIGHT_LOCAL_HESSIAN_CFG")
    for li in range(2):
        for n in nvfp4_flow.LINEARS:
            p = f"layers.{li}.{n}."
            w = getattr(model.layers[li], n).weight
            packed, scale, s2 = state[p + "weight"], state[p + "weight_scale"], state[p + "weight_scale_2"]
            assert packed.dtype == torch.uint8 and tuple(packed.shape) == (w.shape[0], w.shape[1] // 2)
            assert scale.dtype == torch.float8_e4m3fn and tuple(scale.shape) == (w.shape[0], w.shape[1] // 16)
            assert s2.dtype == torch.float32 and s2.dim() == 0 and s2.item() > 0
            assert state[p + "input_scale"].dtype == torch.float32 and state[p + "input_scale"].dim() == 0
            assert p + "pre_quant_scale" not in state
            qt = qtensor.NVFP4QTensor(w.shape, w.dtype, packed.to(DEV))
            y = qt.dequantize(scale=scale.to(DEV), double_scale=s2.to(DEV), block_sizes={-1: 16})
            assert eh.bits_equal(y.cpu(), eh.unpack(packed, scale.view(torch.uint8), s2, torch.bfloat16)), p
    assert export.hf_quant_config(model)["quantization"]["quant_algo"] == "NVFP4"
