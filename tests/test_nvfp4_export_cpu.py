"""Static NVFP4 checkpoint export (packed E2M1 under E4M3 block scales), CPU tier.

The torch restatements of tests/nvfp4_export_host.py -- the checker of moq_nvfp4_pack / moq_nvfp4_unpack on the GPU -- are
first pinned bit for bit to what the reference's NVFP4QTensor wrote on CPU (tests/golden/export_llama_nvfp4.npz); then
ops, NVFP4QTensor and the exporter are run on CPU tensors with those restatements standing in for libmoquant, against the
reference's exported checkpoint of the tiny Llama; the C-ABI's refusals are checked on the real library (no launch)."""

import ctypes
import json
import os

import pytest
import torch

import _moa_import
import hostmem_backend
import nvfp4_export_host as eh
import nvfp4_host as nh

moa = _moa_import.load()
from model_optimizer_amd import _lib, export, qtensor  # noqa: E402

Z, CASES = eh.fixture()
K = CASES["kcases"]


def test_fixture_covers_the_issue_cases():
    assert sum(1 for c in K.values() if c.get("allbf16")) >= 3
    assert {c["dtype"] for c in K.values()} == {"bf16", "f16", "f32"}
    assert {c["kind"] for c in K.values()} == {"static", "dynamic"}
    assert sum(1 for k in K if k.startswith("bounds_")) >= 3
    assert int((Z["clamp448_f32_scale"] == 0x7E).sum()) > 0  # the clamp at 448
    assert int((Z["clamp_min_bf16_scale"] == 0x01).sum()) > 0  # the clamp at 2^-9
    assert 0x08 in set((Z["neg_to_zero_f32_packed"].reshape(-1) & 0xF).tolist())  # a negative value rounded to zero
    assert os.path.getsize(os.path.join(os.path.dirname(eh.__file__), "golden", "export_llama_nvfp4.npz")) < (1 << 20)


@pytest.mark.parametrize("k", sorted(K))
def test_pack_restatement_matches_reference(k):
    c = K[k]
    x = eh.case_x(Z, k, c)
    packed, sb, s2 = eh.pack(x, **eh.case_inputs(Z, k, c))
    assert torch.equal(s2.reshape(1), torch.from_numpy(Z[f"{k}_s2"])), k
    assert torch.equal(sb, torch.from_numpy(Z[f"{k}_scale"]).reshape(-1)), k
    bad = (packed != torch.from_numpy(Z[f"{k}_packed"])).sum().item()
    assert bad == 0, f"{k}: {bad} packed bytes differ"
    if c.get("deq"):
        y = eh.unpack(packed, sb, s2, eh.DT[c["dtype"]])
        assert eh.bits_equal(y, eh.from_bits(Z[f"{k}_deq"], eh.DT[c["dtype"]]).reshape(c["shape"])), k


def test_boundary_cases_reach_both_sides_of_every_bound():
    """The bounds_* cases hold quotients on and beside each of the seven rounding bounds: all eight codes appear, and a
    restatement with a reciprocal multiplication instead of the division does NOT reproduce them."""
    codes, wrong = set(), 0
    for k in (k for k in K if k.startswith("bounds_")):
        x = eh.case_x(Z, k, K[k])
        want = torch.from_numpy(Z[f"{k}_packed"])
        codes |= set((want.reshape(-1) & 7).tolist())
        d = (torch.from_numpy(Z[f"{k}_scale"]).view(torch.float8_e4m3fn).float() * torch.from_numpy(Z[f"{k}_s2"])).reshape(-1, 1)
        nib = eh.e2m1_codes(x.reshape(-1, 16) * (1.0 / d)).reshape(-1, 2)
        wrong += ((nib[:, 1] << 4 | nib[:, 0]).reshape(want.shape) != want).sum().item()
    assert codes == set(range(8)) and wrong > 0


@pytest.fixture
def hostmem(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    eh.install(fake)
    return fake


@pytest.mark.parametrize("k", ["rand_bf16", "rand_f16_dyn", "zeros_bf16", "bounds_f32_1", "all_bf16_1"])
def test_ops_through_the_host_backend(hostmem, k):
    c = K[k]
    x = eh.case_x(Z, k, c)
    packed, scale, s2 = moa.ops.nvfp4_quantize(x, 16, **eh.case_inputs(Z, k, c))
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (*x.shape[:-1], x.shape[-1] // 2)
    assert scale.dtype == torch.float8_e4m3fn and tuple(scale.shape) == (*x.shape[:-1], x.shape[-1] // 16)
    assert s2.dtype == torch.float32 and s2.dim() == 0
    assert torch.equal(packed, torch.from_numpy(Z[f"{k}_packed"]))
    assert torch.equal(scale.view(torch.uint8), torch.from_numpy(Z[f"{k}_scale"]).reshape(scale.shape))
    assert torch.equal(s2.reshape(1), torch.from_numpy(Z[f"{k}_s2"]))
    if c.get("deq"):
        y = moa.ops.nvfp4_dequantize(packed, scale, s2, x.dtype)
        assert eh.bits_equal(y, eh.from_bits(Z[f"{k}_deq"], x.dtype).reshape(x.shape))
    # the scale bytes given: the same nibbles
    again, sc2, _ = moa.ops.nvfp4_quantize(x, 16, scale=scale, scale_2=s2)
    assert torch.equal(again, packed) and sc2.data_ptr() == scale.data_ptr()


def _static_quantizer(amax, g, block=16, **extra):
    from model_optimizer_amd.tensor_quantizer import TensorQuantizer

    q = TensorQuantizer(moa.QuantizerAttributeConfig(num_bits=(2, 1), block_sizes={-1: block, "type": "static",
                                                                                  "scale_bits": (4, 3), **extra}))
    q.amax = amax.reshape(-1, 1)
    q.promote_static_block()
    q.global_amax = g
    return q


def test_nvfp4_qtensor_surface(hostmem):
    T = qtensor.NVFP4QTensor
    k = "rand_bf16"
    x = eh.case_x(Z, k, K[k])
    wq = _static_quantizer(torch.from_numpy(Z[f"{k}_amax"].copy()), torch.from_numpy(Z[f"{k}_g"].copy()).reshape(()))
    s2 = T.get_weights_scaling_factor_2_from_quantizer(wq)
    assert torch.equal(s2.reshape(1), torch.from_numpy(Z[f"{k}_s2"]))
    scale, s2b = T.get_weights_scaling_factor_from_quantizer(wq, x)
    assert torch.equal(scale.view(torch.uint8).reshape(-1), torch.from_numpy(Z[f"{k}_scale"]).reshape(-1)) and torch.equal(s2, s2b)
    qt, scale_q, _ = T.quantize(x, 16, scale, s2)
    assert torch.equal(qt._quantized_data, torch.from_numpy(Z[f"{k}_packed"])) and qt.metadata["shape"] == x.shape
    y = qt.dequantize(scale=scale_q, double_scale=s2, block_sizes={-1: 16})
    assert eh.bits_equal(y, eh.from_bits(Z[f"{k}_deq"], x.dtype).reshape(x.shape))
    assert qt.dequantize(dtype=torch.float32, scale=scale_q, double_scale=s2, block_sizes={-1: 16}).dtype == torch.float32
    qt1, sc1, s21 = T.quantize_from_quantizer(wq, x)
    assert torch.equal(qt1._quantized_data, qt._quantized_data) and torch.equal(sc1.view(torch.uint8), scale.view(torch.uint8))
    # dynamic: scales from the tensor
    kd = "rand_f32_dyn"
    xd = eh.case_x(Z, kd, K[kd])
    qd, sd, s2d = T.quantize(xd, 16)
    assert torch.equal(qd._quantized_data, torch.from_numpy(Z[f"{kd}_packed"]))
    assert torch.equal(T.get_weights_scaling_factor_2(xd).reshape(1), torch.from_numpy(Z[f"{kd}_s2"]))
    sd2, _ = T.get_weights_scaling_factor(xd, 16, s2d)
    assert torch.equal(sd2.view(torch.uint8), sd.view(torch.uint8))
    # activations: amax / (6 * 448); a disabled quantizer has none
    iq = moa.tensor_quantizer.TensorQuantizer(moa.QuantizerAttributeConfig(
        num_bits=(2, 1), axis=None, block_sizes={-1: 16, "type": "dynamic", "scale_bits": (4, 3)}))
    assert T.get_activation_scaling_factor(iq) is None
    iq.amax = torch.tensor(2.75)
    assert T.get_activation_scaling_factor(iq).item() == (torch.tensor(2.75) / torch.tensor(2688.0)).item()
    iq.disable()
    assert T.get_activation_scaling_factor(iq) is None
    # refused, not ignored
    for call in (lambda: T.quantize(x, 16, keep_high_precision=True), lambda: T.quantize(x, 16, try_tensorrt=True),
                 lambda: qt.dequantize(fast=True, scale=scale_q, double_scale=s2, block_sizes={-1: 16}),
                 lambda: T.get_weights_scaling_factor(x, 16, keep_high_precision=True),
                 lambda: T.quantize(x, 32),
                 lambda: T.get_weights_scaling_factor_2_from_quantizer(
                     _static_quantizer(torch.ones(4), torch.tensor(1.0), four_over_six=True))):
        with pytest.raises(moa.MoquantUnsupported):
            call()


def test_ops_refusals(hostmem):
    x = torch.randn(8, 48)
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_quantize(x, 32)
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_quantize(torch.randn(4, 40))  # cin % 16
    with pytest.raises(ValueError):
        moa.ops.nvfp4_quantize(x, 16, amax=torch.ones(5), global_amax=torch.tensor(1.0))
    with pytest.raises(ValueError):
        moa.ops.nvfp4_quantize(x, 16, amax=torch.ones(24))
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_quantize(x.double(), 16)
    with pytest.raises(moa.MoquantUnsupported):
        moa.ops.nvfp4_dequantize(torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(2, 1).to(torch.float8_e4m3fn),
                                 torch.tensor(1.0), torch.float32, block_size=32)
    with pytest.raises(moa.MoquantError):
        moa.ops.nvfp4_dequantize(torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(2, 2).to(torch.float8_e4m3fn),
                                 torch.tensor(1.0), torch.float32)


def test_ops_refuse_cpu_tensors():
    with pytest.raises(moa.MoquantError, match="must live on the GPU"):
        moa.ops.nvfp4_quantize(torch.randn(4, 32))
    with pytest.raises(moa.MoquantError, match="must live on the GPU"):
        moa.ops.nvfp4_dequantize(torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(2, 1).to(torch.float8_e4m3fn),
                                 torch.tensor(1.0), torch.float32)


def test_c_abi_refusals_without_gpu():
    lib = _lib.lib()
    P = ctypes.c_void_p(256)
    bf = _lib.BF16
    assert lib.moq_nvfp4_pack(P, P, P, P, P, P, 0, 4, 32, bf, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert b"block size" in lib.moq_last_error()
    assert lib.moq_nvfp4_pack(None, P, P, P, P, P, 0, 4, 16, bf, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_pack(P, P, None, P, P, P, 0, 4, 16, bf, None) == _lib.MOQ_ERR_INVALID  # static without a global amax
    assert lib.moq_nvfp4_pack(P, None, None, None, P, P, 0, 4, 16, bf, None) == _lib.MOQ_ERR_INVALID  # no scale_2
    assert lib.moq_nvfp4_pack(ctypes.c_void_p(264), P, P, P, P, P, 0, 4, 16, bf, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_pack(P, P, P, P, ctypes.c_void_p(258), P, 0, 4, 16, bf, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_pack(P, P, P, P, P, P, 0, -1, 16, bf, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_pack(None, None, None, None, None, None, 0, 0, 16, bf, None) == _lib.MOQ_OK  # nothing to do
    assert lib.moq_nvfp4_unpack(P, P, P, P, 4, 8, bf, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_unpack(P, None, P, P, 4, 16, bf, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_nvfp4_unpack(P, P, P, ctypes.c_void_p(264), 4, 16, bf, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert lib.moq_nvfp4_unpack(None, None, None, None, 0, 16, bf, None) == _lib.MOQ_OK


# ----------------------------------------------------------------------------------------------- the exporter
def _fixture_model():
    model, orig = eh.build_llama(CASES)
    return eh.set_fixture_state(moa, model, Z, CASES), orig


def _probe(model):
    return lambda: model(torch.ones([1, 2], dtype=torch.long))


def test_export_from_reference_state_is_byte_identical(hostmem, tmp_path):
    model, orig = _fixture_model()
    q = model.model.layers[0].self_attn.q_proj
    assert export.get_quantization_format(q) == export.QUANTIZATION_NVFP4 == "nvfp4"
    state = export.export_state_dict(model, torch.bfloat16, _probe(model))
    eh.compare_state(state, Z, CASES, orig)
    assert "model.layers.0.mlp.down_proj.pre_quant_scale" not in state
    # both JSON configs (the producer names the library that wrote the file)
    cfg = export.hf_quant_config(model)
    assert cfg["quantization"] == CASES["hf_quant_config"]["quantization"]
    conv = export.convert_hf_quant_config_format(cfg)
    want = dict(CASES["quantization_config"])
    assert conv.pop("producer") == cfg["producer"] and want.pop("producer")
    assert conv == want
    # the directory on disk: float8 block scales survive safetensors
    from safetensors import safe_open

    export.save_checkpoint(state, str(tmp_path), cfg)
    with safe_open(os.path.join(tmp_path, "model.safetensors"), "pt") as f:
        assert set(f.keys()) == set(CASES["dtypes"])
        back = {k: f.get_tensor(k) for k in f.keys()}
    eh.compare_state(back, Z, CASES, orig)
    assert back["model.layers.0.self_attn.q_proj.weight_scale"].dtype == torch.float8_e4m3fn
    assert json.load(open(os.path.join(tmp_path, "hf_quant_config.json")))["quantization"]["quant_algo"] == "NVFP4"


def test_export_hf_checkpoint_writes_both_configs(hostmem, tmp_path):
    from safetensors import safe_open

    model, orig = _fixture_model()
    export.export_hf_checkpoint(model, export_dir=str(tmp_path))
    with safe_open(os.path.join(tmp_path, "model.safetensors"), "pt") as f:
        eh.compare_state({k: f.get_tensor(k) for k in f.keys()}, Z, CASES, orig)
    qc = json.load(open(os.path.join(tmp_path, "config.json")))["quantization_config"]
    want = dict(CASES["quantization_config"])
    qc.pop("producer"), want.pop("producer")
    assert qc == want
    assert json.load(open(os.path.join(tmp_path, "hf_quant_config.json")))["quantization"] == CASES["hf_quant_config"]["quantization"]


def test_sharded_export_is_the_same_dict(hostmem):
    model, orig = _fixture_model()
    state = export.export_state_dict(model, torch.bfloat16, _probe(model), shard_weights=False)
    assert state.sharded is False
    eh.compare_state(state, Z, CASES, orig)


def test_fused_siblings_with_unequal_global_amax_are_unified(hostmem):
    model, _ = _fixture_model()
    attn, mlp = model.model.layers[1].self_attn, model.model.layers[1].mlp
    g = attn.q_proj.weight_quantizer.global_amax.clone()
    attn.k_proj.weight_quantizer.global_amax = g * 0.5
    attn.v_proj.weight_quantizer.global_amax = g * 1.75
    mlp.up_proj.weight_quantizer.global_amax = mlp.gate_proj.weight_quantizer.global_amax * 3.0
    attn.k_proj.input_quantizer.amax = torch.tensor(9.0)
    state = export.export_state_dict(model, torch.bfloat16, _probe(model))
    for n in ("q_proj", "k_proj", "v_proj"):
        m = getattr(attn, n)
        assert torch.equal(m.weight_quantizer.global_amax, g * 1.75), n
        p = f"model.layers.1.self_attn.{n}."
        assert state[p + "weight_scale_2"].item() == eh.scale_2_of(g * 1.75).item()
        assert state[p + "input_scale"].item() == (torch.tensor(9.0) / torch.tensor(2688.0)).item()
        packed, sb, _ = eh.pack(m.weight.detach(), amax=m.weight_quantizer._amax, global_amax=g * 1.75)
        assert torch.equal(state[p + "weight"], packed) and torch.equal(state[p + "weight_scale"].view(torch.uint8).reshape(-1), sb)
    assert torch.equal(mlp.gate_proj.weight_quantizer.global_amax, mlp.up_proj.weight_quantizer.global_amax)
    # a linear on its own keeps its global amax
    o = f"model.layers.1.self_attn.o_proj.weight_scale_2"
    assert state[o].item() == eh.scale_2_of(attn.o_proj.weight_quantizer.global_amax).item()


def test_weight_only_static_nvfp4(hostmem):
    model, orig = _fixture_model()
    for m in model.modules():
        if hasattr(m, "input_quantizer"):
            m.input_quantizer.disable()
    assert export.get_quantization_format(model.model.layers[0].mlp.down_proj) == "w4a16_nvfp4"
    state = export.export_state_dict(model, torch.bfloat16, _probe(model))
    assert not any(k.endswith("input_scale") for k in state)
    k = "model.layers.0.mlp.down_proj.weight"
    assert eh.bits_equal(state[k], eh.expected_tensor(Z, CASES, orig, k))
    cfg = export.hf_quant_config(model)
    assert cfg["quantization"]["quant_algo"] == "W4A16_NVFP4" and cfg["quantization"]["group_size"] == 16
    grp = export.convert_hf_quant_config_format(cfg)["config_groups"]["group_0"]
    assert "input_activations" not in grp and grp["weights"] == {"dynamic": False, "num_bits": 4, "type": "float", "group_size": 16}


def test_export_refusals(hostmem):
    mq = moa.model_quant

    def linear(cfg):
        m = torch.nn.Sequential(torch.nn.Linear(128, 64, bias=False))
        moa.nn.replace_quant_module(m)
        mq.set_quantizer_by_cfg(m, cfg)
        return m[0]

    with pytest.raises(NotImplementedError, match="dynamic NVFP4 blocks"):
        export.get_quantization_format(linear(mq.NVFP4_DEFAULT_CFG["quant_cfg"]))
    static = mq.NVFP4_W4A4_WEIGHT_MSE_FP8_SWEEP_CFG["quant_cfg"]
    m = linear(static)
    assert export.get_quantization_format(m) == "nvfp4"
    with pytest.raises(ValueError, match="no calibrated"):
        export.export_quantized_weight(m, torch.float32)
    m.input_quantizer.pre_quant_scale = torch.ones(128)
    with pytest.raises(NotImplementedError, match="nvfp4_awq"):
        export.get_quantization_format(m)
    cfg46 = {"*weight_quantizer": {"num_bits": (2, 1), "block_sizes": {-1: 16, "type": "static", "scale_bits": (4, 3),
                                                                       "four_over_six": True}},
             "*input_quantizer": static["*input_quantizer"]}
    try:
        m46 = linear(cfg46)
    except Exception:  # noqa: BLE001 -- a config layer that refuses the key earlier is a refusal too
        m46 = None
    if m46 is not None:
        with pytest.raises(NotImplementedError, match="four-over-six"):
            export.get_quantization_format(m46)
    # fused experts with NVFP4 quantizers stay outside
    wq = linear(static).weight_quantizer
    with pytest.raises(NotImplementedError, match="fused experts"):
        export.get_quantization_format(export._ExpertProjection(None, wq, linear(static).input_quantizer))
