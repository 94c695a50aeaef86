"""Rotation (Hadamard) quantizers without a GPU: the arithmetic definition against mathematics, block-size selection, the
forward order of a rotating TensorQuantizer against a literal transcription of the reference's forward, every refusal,
the printed form, the presets, and the host flows on the host-memory stand-in against what the REFERENCE produced on CPU
(tests/golden/hadamard_rotate.npz, tests/golden/gen_hadamard_rotate.py)."""

import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import scipy.linalg
import torch

import _moa_import
import hadamard_host as hh
import hostmem_backend
import nvfp4_act_headroom_host as ah
import nvfp4_flow
from conftest import GOLDEN, assert_bits_equal, from_bits

moa = _moa_import.load()
from model_optimizer_amd import _lib, export, model_calib, model_quant, ops, sparsity  # noqa: E402
from model_optimizer_amd.tensor_quantizer import QuantizerAttributeConfig as Cfg  # noqa: E402
from model_optimizer_amd.tensor_quantizer import RotateConfig  # noqa: E402
from model_optimizer_amd.tensor_quantizer import TensorQuantizer as TQ  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
Z = np.load(os.path.join(GOLDEN, "hadamard_rotate.npz"))
CASES = json.loads(str(Z["cases"]))


@pytest.fixture
def hostmem(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    hh.install(fake)
    return fake


# ----------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("block", [2, 4, 8, 16, 128, 512, 2048, 16384])
def test_restatement_against_mathematics(block):
    """f32 inputs, 37 rows, magnitudes 2^-30 .. 2^10, against scipy.linalg.hadamard in float64 (for B = 16384 through the
    Sylvester identity H_16384 = H_8 (x) H_2048: the 2 GB matrix itself is not built).  Bound, every element:
        |y - exact| <= 1.01 * (log2 B + 2) * 2^-24 * B^-0.5 * sum_i |x_i|     (sum over the block)
    -- a depth-log2(B) tree of fp32 adds (each intermediate is bounded by the partial sum of |x|, each add contributes a
    relative 2^-24), plus the rounding of `scale`, plus the product."""
    g = torch.Generator().manual_seed(block)
    x = torch.randn(37, block, generator=g) * torch.exp2(torch.randint(-30, 11, (37, block), generator=g).float())
    y = hh.fwht(x, block).double().numpy()
    xd = x.double().numpy()
    if block <= 2048:
        exact = xd @ scipy.linalg.hadamard(block).astype(np.float64).T
    else:
        outer, inner = scipy.linalg.hadamard(block // 2048).astype(np.float64), scipy.linalg.hadamard(2048).astype(np.float64)
        exact = np.einsum("ab,rbk->rak", outer, xd.reshape(37, -1, 2048) @ inner.T).reshape(37, block)
    exact = exact * block ** -0.5
    bound = 1.01 * (math.log2(block) + 2) * 2.0 ** -24 * block ** -0.5 * np.abs(xd).sum(axis=1, keepdims=True)
    err = np.abs(y - exact)
    assert err.shape == (37, block) and bool((err <= bound).all()), f"B={block}: worst {float((err / bound).max()):.3f} of the bound"


def test_block_size_selection_and_errors():
    for cols, want in ((1536, 512), (896, 128), (14336, 2048), (24, 8), (128, 128), (16384, 16384)):
        assert ops.hadamard_block_size(cols) == want
    with pytest.raises(RuntimeError, match="dimension 7 has no power-of-2 divisor >= 2"):
        ops.hadamard_block_size(7)
    with pytest.raises(ValueError, match="block_size must be power of 2, got 12"):
        ops.hadamard_block_size(96, 12)
    with pytest.raises(RuntimeError, match=r"inputs.shape\[-1\]=96 is not divisible by block_size=64"):
        ops.hadamard_block_size(96, 64)
    for bad in (True, 0, -4, 2.0):
        with pytest.raises(ValueError):
            ops.hadamard_block_size(64, bad)
        with pytest.raises(ValueError, match="block_size must be a positive int"):
            Cfg(rotate={"enable": True, "block_size": bad})
    with pytest.raises(moa.MoquantUnsupported, match="16384"):
        ops.hadamard_block_size(65536)
    assert ops.hadamard_block_size(65536, 128) == 128
    with pytest.raises(ValueError, match="mode"):
        Cfg(rotate={"enable": True, "mode": "back"})
    with pytest.raises(ValueError, match="unknown rotate option"):
        Cfg(rotate={"enable": True, "sign_vector": 1})


def test_config_normalises_to_a_rotate_config():
    assert Cfg().rotate == RotateConfig() and not TQ(Cfg()).rotate_is_enabled
    assert Cfg(rotate=True).rotate == RotateConfig(enable=True)
    q = TQ(Cfg(rotate={"enable": True, "mode": "rotate_back", "rotate_fp32": True, "block_size": 32}))
    assert q.rotate_is_enabled and q.rotate_back_is_enabled and q.rotate_is_fp32 and q.rotate_block_size == 32
    q.disable_rotate()
    q.disable_rotate()  # idempotent
    assert not (q.rotate_is_enabled or q.rotate_back_is_enabled or q.rotate_is_fp32) and q.rotate_block_size is None
    off = TQ(Cfg(rotate={"enable": False, "mode": "rotate_back", "rotate_fp32": True, "block_size": 8}))
    assert not (off.rotate_is_enabled or off.rotate_back_is_enabled or off.rotate_is_fp32) and off.rotate_block_size is None


def test_entries_check_arguments_before_any_launch():
    """The C-ABI entries on the real library, no GPU: every refusal comes back before a HIP call (tests/test_abi_cpu.py)."""
    lib = _lib.lib()
    P = ctypes.c_void_p(16)
    bf16, e2m1, e4m3, e8m0 = _lib.BF16, _lib.MX_TYPES["E2M1"], _lib.MX_TYPES["E4M3"], _lib.MX_TYPES["E8M0"]
    assert lib.moq_hadamard(None, None, 0, 64, 64, 0.125, bf16, None, None) == _lib.MOQ_OK               # empty
    assert lib.moq_hadamard(None, P, 4, 64, 64, 0.125, bf16, None, None) == _lib.MOQ_ERR_INVALID         # null input
    assert lib.moq_hadamard(P, P, 4, 96, 64, 0.125, bf16, None, None) == _lib.MOQ_ERR_INVALID            # 64 does not divide 96
    assert b"not divisible" in lib.moq_last_error()
    assert lib.moq_hadamard(P, P, 4, 96, 12, 0.3, bf16, None, None) == _lib.MOQ_ERR_INVALID              # not a power of two
    assert lib.moq_hadamard(P, P, 4, 96, 1, 1.0, bf16, None, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_hadamard(P, P, 4, 64, 64, 0.125, 7, None, None) == _lib.MOQ_ERR_INVALID               # dtype code
    assert lib.moq_hadamard(P, P, 1, 32768, 32768, 0.0055, bf16, None, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert b"16384" in lib.moq_last_error()
    q = lib.moq_hadamard_mx_qdq
    assert q(None, None, 0, 128, 128, 0.088, 16, bf16, e2m1, e4m3, None, 0, None) == _lib.MOQ_OK
    assert q(P, P, 4, 1024, 1024, 0.03125, 16, bf16, e2m1, e4m3, None, 0, None) == _lib.MOQ_ERR_UNSUPPORTED   # LDS tier
    assert b"compose" in lib.moq_last_error()
    assert q(P, P, 4, 512, 512, 0.044, 16, _lib.F32, e2m1, e4m3, None, 0, None) == _lib.MOQ_ERR_UNSUPPORTED  # f32 edge is 256
    assert q(P, P, 4, 16, 16, 0.25, 32, bf16, e2m1, e8m0, None, 0, None) == _lib.MOQ_ERR_UNSUPPORTED         # block > rot_block
    assert q(P, P, 4, 128, 128, 0.088, 24, bf16, e2m1, e8m0, None, 0, None) == _lib.MOQ_ERR_UNSUPPORTED      # odd QDQ block
    assert q(ctypes.c_void_p(18), P, 4, 128, 128, 0.088, 16, bf16, e2m1, e4m3, None, 0, None) == _lib.MOQ_ERR_UNSUPPORTED
    assert q(P, P, 4, 128, 128, 0.088, 32, bf16, e2m1, e8m0, P, 0, None) == _lib.MOQ_ERR_UNSUPPORTED         # E8M0 + global amax
    assert q(P, P, 4, 128, 128, 0.088, 16, bf16, 99, e4m3, None, 0, None) == _lib.MOQ_ERR_INVALID            # element format
    assert q(P, P, 4, 96, 64, 0.125, 16, bf16, e2m1, e4m3, None, 0, None) == _lib.MOQ_ERR_INVALID
    x = torch.randn(4, 128)
    for call in (lambda: ops.hadamard(x), lambda: ops.hadamard_block_quant(x, None, 16, None, (2, 1), (4, 3))):
        with pytest.raises(moa.MoquantError, match="must live on the GPU"):
            call()


def test_ops_check_arguments_on_the_host(hostmem, monkeypatch):
    x = torch.randn(4, 96).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="not divisible"):
        ops.hadamard(x, 64)
    with pytest.raises(moa.MoquantError, match="running_amax"):
        ops.hadamard(x, 32, running_amax=torch.zeros(2))
    with pytest.raises(moa.MoquantError, match="out must be"):
        ops.hadamard(x, 32, out=torch.empty(4, 96))
    with pytest.raises(NotImplementedError):
        ops.hadamard_block_quant(x, 32, 16, None, (7, 7), (4, 3))
    assert hh.same_bits(ops.hadamard(x), hh.fwht(x, 32))
    # the composition where the entry has no fused kernel: same result as the launches in a row
    amax = hh.fwht(x, 32).abs().amax().float()
    for back in (False, True):
        want = ops.dynamic_block_quant(hh.fwht(x, 32), 16, amax, (2, 1), (4, 3))
        want = hh.fwht(want, 32) if back else want
        for fused in (True, False):
            monkeypatch.setattr(ops, "_HADAMARD_QDQ_FUSED", fused)
            assert hh.same_bits(ops.hadamard_block_quant(x, 32, 16, amax, (2, 1), (4, 3), rotate_back=back), want)


# ----------------------------------------------------------------------------------------------- forward order
def _reference_forward(q, inputs):
    """tensor_quantizer.py:1142-1219, line for line, on this package's quantizer state (the rotation is the restatement)."""
    rot = lambda t: hh.fwht(t.contiguous(), ops.hadamard_block_size(t.shape[-1], q.rotate_block_size))  # noqa: E731
    if q.pre_quant_scale is not None:
        inputs = inputs * q.pre_quant_scale
    if q.rotate_back_is_enabled and q._if_quant and not q.fake_quant:
        raise ValueError("rotate_back mode is only supported with fake_quant=True.")
    if q.rotate_is_enabled:
        inputs = rot(inputs)
    if q._disabled:
        if q.rotate_back_is_enabled:
            inputs = rot(inputs)
        return inputs
    if q.block_sizes is not None and q._fake_quant:
        q._block_sizes_to_axis(inputs)
    if q.is_static_block_quant:
        q._setup_for_blockquant(inputs)
        inputs = q._process_for_blockquant(inputs)
    outputs = inputs
    if q._if_calib and not q._dynamic:
        q.collect(inputs)
    if q._if_quant:
        outputs = q._fake_quantize(inputs.contiguous())
    if q.is_static_block_quant:
        outputs = q._reset_to_original_shape(outputs)
    if q.rotate_back_is_enabled and isinstance(outputs, torch.Tensor):
        outputs = rot(outputs)
    return outputs


def _pair(**kw):
    return TQ(Cfg(**copy.deepcopy(kw))), TQ(Cfg(**copy.deepcopy(kw)))


@pytest.mark.parametrize("dn", sorted(DT))
def test_forward_order_and_shortcuts(hostmem, dn):
    x = (torch.randn(4, 96) * 3).to(DT[dn])
    # a disabled rotating quantizer (the preset's q_bmm_quantizer) rotates: it does not hand back
    for rot, twice in ((True, False), ({"enable": True, "mode": "rotate_back"}, True)):
        a, b = _pair(rotate=rot, enable=False)
        assert not a.hands_back()
        y = a(x)
        assert_bits_equal(y, _reference_forward(b, x), "disabled")
        assert_bits_equal(y, hh.fwht(hh.fwht(x, 32), 32) if twice else hh.fwht(x, 32), "disabled, by hand")
    assert TQ(Cfg(enable=False)).hands_back()
    # pre_quant_scale, then the rotation
    a, b = _pair(num_bits=8, axis=None, rotate={"enable": True, "block_size": 8})
    pqs = (torch.rand(96) + 0.5).to(DT[dn])
    for q in (a, b):
        q.pre_quant_scale = pqs
    assert_bits_equal(a(x), _reference_forward(b, x), "pre_quant_scale + rotate")
    # calibration mode returns the rotated tensor (mode rotate) or the transform applied twice (rotate_back), and the
    # per-tensor amax is that of the tensor rotated ONCE
    for fmt in ({"num_bits": 8, "axis": None}, {"num_bits": (4, 3), "axis": None}, {"num_bits": 8, "axis": 0},
                {"num_bits": (2, 1), "block_sizes": {-1: 16, "type": "dynamic", "scale_bits": (4, 3)}},
                {"num_bits": 4, "block_sizes": {-1: 16, "type": "static"}}):
        for rot in (True, {"enable": True, "mode": "rotate_back", "block_size": 16}):
            a, b = _pair(**fmt, rotate=rot)
            for q in (a, b):
                q.enable_calib()
                q.disable_quant()
            for t in (x, x * 0.5):  # (a second call keeps accumulating: the collect_per_tensor_fast shortcut must not take it)
                ya, yb = a(t), _reference_forward(b, t)
                assert_bits_equal(ya, yb, f"calibration return {fmt} {rot}")
            once = hh.fwht(x, 16 if isinstance(rot, dict) else 32)
            assert_bits_equal(ya, hh.fwht(once * 0.5, 16) if isinstance(rot, dict) else once * 0.5, "calibration return, by hand")
            for q in (a, b):
                q.load_calib_amax()
                q.disable_calib()
                q.enable_quant()
            assert_bits_equal(a._amax.float(), b._amax.float(), f"amax {fmt} {rot}")
            if fmt.get("axis", 1) is None and "block_sizes" not in fmt or fmt["num_bits"] == (2, 1):
                assert_bits_equal(a._amax.float().reshape(()), once.abs().amax().float(), "amax is of the rotated tensor")
            assert_bits_equal(a(x), _reference_forward(b, x), f"quantized forward {fmt} {rot}")
    # static INT4 blocks on a rotated weight, amax from the input itself (the awq_scale_qdq / fused group paths must yield)
    a, b = _pair(num_bits=4, block_sizes={-1: 16, "type": "static"}, rotate=True)
    assert_bits_equal(a(x), _reference_forward(b, x), "static INT4 blocks")
    a, b = _pair(num_bits=4, block_sizes={-1: 16, "type": "static"}, rotate=True)
    for q in (a, b):
        q.pre_quant_scale = pqs
    assert_bits_equal(a(x), _reference_forward(b, x), "static INT4 blocks behind a pre_quant_scale")
    # rotate_back without fake quant
    a = TQ(Cfg(num_bits=8, axis=None, rotate={"enable": True, "mode": "rotate_back"}))
    a.__dict__["_fake_quant"] = False
    with pytest.raises(ValueError, match="rotate_back mode is only supported with fake_quant=True"):
        a(x)


def test_weight_statistics_shortcuts_yield_to_rotation(hostmem):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    moa.nn.replace_quant_module(model)
    cfg = {"quant_cfg": {"*weight_quantizer": {"num_bits": 8, "axis": None, "rotate": {"enable": True, "block_size": 16}},
                         "*input_quantizer": {"enable": False}}, "algorithm": "max"}
    model_quant.set_quantizer_by_cfg(model, cfg["quant_cfg"])
    model_calib.max_calibrate(model, lambda m: [m(b) for b in batches])
    n = 0
    for name, m in model.named_modules():
        if moa.nn.is_quantized_linear(m):
            wq = m.weight_quantizer
            assert wq._weight_stats_done is None and not wq.weight_already_counted(m.weight)
            assert_bits_equal(wq._amax.float().reshape(()), hh.fwht(m.weight.detach(), 16).abs().amax().float(), name)
            n += 1
    assert n >= 2


def test_fold_weight_bakes_the_rotation_in_once(hostmem):
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    moa.nn.replace_quant_module(model)
    rot = {"enable": True, "mode": "rotate_back", "block_size": 16}
    model_quant.set_quantizer_by_cfg(model, {"*weight_quantizer": {"num_bits": (4, 3), "axis": None, "rotate": rot},
                                             "*input_quantizer": {"enable": False}})
    model_calib.max_calibrate(model, lambda m: [m(b) for b in batches])
    lins = [m for m in model.modules() if moa.nn.is_quantized_linear(m)]
    want = [m.weight_quantizer(m.weight.detach().float().contiguous()).to(m.weight.dtype) for m in lins]
    y = model(batches[0])
    model_quant.fold_weight(model)
    for m, w in zip(lins, want):
        assert_bits_equal(m.weight.detach(), w, "folded weight == the quantizer's forward")
        assert not m.weight_quantizer.rotate_is_enabled and not m.weight_quantizer.is_enabled
        assert_bits_equal(m.weight_quantizer(m.weight.detach()), m.weight.detach(), "a second forward does not rotate again")
    assert_bits_equal(model(batches[0]), y, "the folded model computes what the quantized model computed")


# ----------------------------------------------------------------------------------------------- refusals
def _rotating_model():
    model, batches = nvfp4_flow.make("cpu", torch.float32)
    moa.nn.replace_quant_module(model)
    model_quant.set_quantizer_by_cfg(model, {"*weight_quantizer": {"num_bits": 8, "axis": 0, "rotate": True},
                                             "*input_quantizer": {"num_bits": 8, "axis": None}})
    return model, (lambda m: [m(b) for b in batches])


@pytest.mark.parametrize("algorithm", ["mse", "local_hessian", "smoothquant", "awq_lite", "awq_clip", "awq_full", "gptq",
                                       "nvfp4_act_headroom"])
def test_algorithms_other_than_max_refuse_rotating_quantizers(hostmem, algorithm):
    model, loop = _rotating_model()
    with pytest.raises(moa.MoquantUnsupported, match=r"weight_quantizer: rotate is enabled"):
        model_quant.calibrate(model, algorithm, loop)
    direct = {"mse": model_calib.mse_calibrate, "local_hessian": model_calib.local_hessian_calibrate,
              "smoothquant": model_calib.smoothquant, "gptq": model_calib.gptq,
              "nvfp4_act_headroom": model_calib.nvfp4_act_headroom_calibrate}.get(algorithm)
    if direct is None:
        direct = lambda m, f: model_calib.awq(m, f, algorithm=algorithm)  # noqa: E731
    with pytest.raises(moa.MoquantUnsupported, match="rotate is enabled"):
        direct(model, loop)
    own = {"awq_lite": model_calib.awq_lite, "awq_clip": model_calib.awq_clip}.get(algorithm)  # public entries of their own
    if own is not None:
        with pytest.raises(moa.MoquantUnsupported, match="rotate is enabled"):
            own(model, loop)


def test_other_refusals(hostmem, tmp_path):
    model, loop = _rotating_model()
    for mode in ("sparse_magnitude", "sparsegpt"):
        with pytest.raises(moa.MoquantUnsupported, match="rotate is enabled"):
            sparsity.sparsify(model, mode, loop)
    model_quant.calibrate(model, "max", loop)  # max is the algorithm that does go through the rotation
    with pytest.raises(moa.MoquantUnsupported, match="checkpoint export does not take rotating quantizers"):
        export.export_state_dict(model, torch.float32)
    with pytest.raises(moa.MoquantUnsupported, match="checkpoint export"):
        export.export_hf_checkpoint(model, torch.float32, str(tmp_path))
    q = TQ(Cfg(num_bits=8))
    with pytest.raises(moa.MoquantUnsupported, match="set_from_attribute_config"):
        q.update_attributes({"rotate": True})
    q.set_from_attribute_config(Cfg(num_bits=8, rotate=True))  # the full-config path takes it
    assert q.rotate_is_enabled
    from model_optimizer_amd import modelopt_algorithms as seam

    class _Ref:  # the seam reads a reference quantizer's __dict__
        def __init__(self):
            self._fake_quant, self._rotate = True, {"enable": True}

    with pytest.raises(seam.CannotAdopt, match="rotation"):
        seam._twin(_Ref(), {})


def test_set_quantizer_by_cfg_context_restores_the_rotation(hostmem):
    model, _ = _rotating_model()
    wq = next(m.weight_quantizer for m in model.modules() if moa.nn.is_quantized_linear(m))
    with model_quant.set_quantizer_by_cfg_context(model, {"*weight_quantizer": {"num_bits": 4, "axis": 0}}):
        assert not wq.rotate_is_enabled
    assert wq.rotate_is_enabled and wq.num_bits == 8


# ----------------------------------------------------------------------------------------------- printed form, presets
def test_extra_repr_suffixes():
    assert repr(TQ(Cfg(rotate=True, enable=False))) == "TensorQuantizer(disabled rotated)"
    assert repr(TQ(Cfg(num_bits=(4, 3), axis=None, rotate=True))) == \
        "TensorQuantizer((4, 3) bit fake per-tensor amax=dynamic rotated calibrator=MaxCalibrator quant)"
    full = TQ(Cfg(num_bits=8, axis=None, rotate={"enable": True, "mode": "rotate_back", "rotate_fp32": True, "block_size": 16}))
    assert " amax=dynamic rotated (rotate_back) (fp32) (block=16) calibrator=" in repr(full)
    assert "rotated" not in repr(TQ(Cfg(num_bits=8))) and "block=" not in repr(TQ(Cfg(rotate={"enable": False, "block_size": 8})))
    for k, c in CASES["qcases"].items():  # the reference's own lines, quantizer by quantizer
        q = TQ(Cfg(**_fmt(c["format"]), rotate=_ROTATES[c["rotate"]]))
        q.amax = from_bits(Z[f"{k}_amax"], torch.float32)
        assert q.extra_repr() == c["repr"].replace("StaticBlockScaleQuantizer", "TensorQuantizer"), k


def _plain(v):
    """JSON form of a config: tuples as lists, integer keys as strings; `effective_bits` (the cost annotation of the
    reference's auto_quantize search: no quantizer attribute) dropped."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items() if k != "effective_bits"}
    return [_plain(x) for x in v] if isinstance(v, (list, tuple)) else v


def test_presets_are_the_references():
    for name in ("NVFP4_KV_CFG", "NVFP4_KV_ROTATE_CFG"):
        assert _plain(getattr(model_quant, name)) == _plain(CASES["presets"][name]), name
    entries = {e["quantizer_name"]: e for e in model_quant.NVFP4_KV_ROTATE_CFG["quant_cfg"]}
    assert entries["*q_bmm_quantizer"]["enable"] is False and entries["*q_bmm_quantizer"]["cfg"] == {"rotate": True}
    assert entries["*k_bmm_quantizer"]["cfg"]["rotate"] is True and "rotate" not in entries["*v_bmm_quantizer"]["cfg"]
    assert model_quant.NVFP4_KV_ROTATE_CFG["algorithm"] == "max"


# ----------------------------------------------------------------------------------------------- the reference's runs
_ROTATES = {"rot": True, "back": {"enable": True, "mode": "rotate_back"}, "fp32": {"enable": True, "rotate_fp32": True},
            "b8": {"enable": True, "block_size": 8}}


def _fmt(name):
    return copy.deepcopy({"int8": {"num_bits": 8, "axis": None}, "fp8": {"num_bits": (4, 3), "axis": None},
                          "int8_pc": {"num_bits": 8, "axis": 0}, "fp8_pc": {"num_bits": (4, 3), "axis": 0},
                          "int4_g16": {"num_bits": 4, "block_sizes": {-1: 16, "type": "static"}}}[name])


def quantizer_case(k, device="cpu"):
    """Fixture (a), case k, through this package's TensorQuantizer: calibration-mode return, amax, quantized forward."""
    c = CASES["qcases"][k]
    dt = DT[c["dtype"]]
    x = from_bits(Z[f"{k}_x"], dt).to(device)
    q = TQ(Cfg(**_fmt(c["format"]), rotate=copy.deepcopy(_ROTATES[c["rotate"]])))
    q.enable_calib()
    q.disable_quant()
    assert_bits_equal(q(x), from_bits(Z[f"{k}_cal"], dt), f"{k}: calibration-mode return")
    q.load_calib_amax()
    q.enable_quant()
    q.disable_calib()
    assert list(q._amax.shape) == c["amax_shape"], k
    assert_bits_equal(q._amax.float().cpu(), from_bits(Z[f"{k}_amax"], torch.float32), f"{k}: amax")
    assert_bits_equal(q(x), from_bits(Z[f"{k}_y"], dt), f"{k}: quantized forward")


def test_fixture_covers_the_issue_cases():
    assert len(CASES["qcases"]) == 5 * 4 * 3
    assert {c["format"] for c in CASES["qcases"].values()} == {"int8", "fp8", "int8_pc", "fp8_pc", "int4_g16"}
    assert all(Z[f"{k}_x"].size <= 4 * 96 for k in CASES["qcases"])
    # rotate_fp32 gives the bits of rotate for 16-bit tensors (documented: the arithmetic is always fp32)
    for k in CASES["qcases"]:
        if "_fp32_" in k:
            assert np.array_equal(Z[f"{k}_y"], Z[k.replace("_fp32_", "_rot_") + "_y"]), k


@pytest.mark.parametrize("k", sorted(CASES["qcases"]))
def test_quantizer_matches_the_reference(hostmem, k):
    quantizer_case(k)


def llama_fp8(device="cpu"):
    """Fixture (b) through moa.quantize: (model, {quantizer name: amax}, logits of the first batch)."""
    L = CASES["llama"]
    model = ah.build_llama(L["config"], device)
    base = np.load(os.path.join(GOLDEN, "export_llama.npz"))
    tokens = [torch.from_numpy(base[f"tokens{i}"].copy()).to(device) for i in range(L["n_batches"])]
    entries = copy.deepcopy(CASES["llama_fp8_entries"])
    for e in entries:
        if "num_bits" in (e.get("cfg") or {}):
            e["cfg"]["num_bits"] = tuple(e["cfg"]["num_bits"])
    cfg = {"quant_cfg": model_quant.normalize_quant_cfg_list(copy.deepcopy(model_quant.FP8_DEFAULT_CFG["quant_cfg"])) + entries,
           "algorithm": "max"}
    with torch.no_grad():
        moa.quantize(model, cfg, lambda m: [m(t) for t in tokens])
        logits = model(tokens[0]).logits
    got = {n: m._amax.detach().float().reshape(-1).cpu() for n, m in model.named_modules()
           if isinstance(m, TQ) and getattr(m, "_amax", None) is not None}
    return model, got, logits


def check_llama_fp8(got, logits, model):
    L = CASES["llama"]
    assert sorted(got) == sorted(L["fp8_amax"])
    assert sorted(n for n, m in model.named_modules() if isinstance(m, TQ) and m.rotate_is_enabled) == L["fp8_rotating"]
    first = "model.layers.0.self_attn.q_proj.input_quantizer"
    for n in L["fp8_amax"]:
        want = torch.from_numpy(Z[f"llama_fp8/{n}"].copy())
        if n.endswith("weight_quantizer") or n == first:
            assert_bits_equal(got[n], want, n)  # the abs-max of a rotated weight / of the first linear's input: exact
        else:  # statistics behind bf16 GEMMs: the tolerance tests/test_gpu_host.py uses for them (2e-2 relative)
            err = float(((got[n] - want).abs() / want.abs().clamp_min(1e-12)).max())
            assert err <= 2e-2, f"{n}: rel err {err:.3e}"
    want = from_bits(Z["llama_fp8_logits"], torch.bfloat16).float().reshape(-1)
    diff = float((logits.float().cpu().reshape(-1) - want).abs().max())
    print(f"logits: max abs diff {diff:.4g}, max |logit| {float(want.abs().max()):.4g}")
    return diff, float(want.abs().max())


def test_llama_fp8_rotate_back_flow_matches_the_reference(hostmem):
    model, got, logits = llama_fp8()
    diff, scale = check_llama_fp8(got, logits, model)
    # Same host, same GEMMs, same quantizer arithmetic: the two models differ only through input amax values that moved by a
    # bf16 ulp behind a GEMM (above), i.e. through FP8 rounding of a few activations.  One E4M3 step of an activation is a
    # relative 2^-4; two decoder layers and the head each average it over >= 256 terms, which leaves a few percent of the
    # logit scale: 0.05 of the largest stored |logit| (on the GPU, where the GEMMs differ too: test_gpu_hadamard_rotate).
    assert diff <= 0.05 * scale


def llama_kv(device="cpu"):
    """Fixture (c): calibration only under NVFP4_KV_ROTATE_CFG behind a disable-all entry."""
    L = CASES["llama"]
    model = ah.build_llama(L["config"], device)
    base = np.load(os.path.join(GOLDEN, "export_llama.npz"))
    tokens = [torch.from_numpy(base[f"tokens{i}"].copy()).to(device) for i in range(L["n_batches"])]
    cfg = {"quant_cfg": [{"quantizer_name": "*", "enable": False}] + copy.deepcopy(model_quant.NVFP4_KV_ROTATE_CFG["quant_cfg"]),
           "algorithm": "max"}
    with torch.no_grad():
        moa.quantize(model, cfg, lambda m: [m(t) for t in tokens])
    return model, tokens


def check_llama_kv(model):
    L = CASES["llama"]
    got = {n: m._amax.detach().float().reshape(-1).cpu() for n, m in model.named_modules()
           if isinstance(m, TQ) and n.endswith("bmm_quantizer") and getattr(m, "_amax", None) is not None}
    assert sorted(got) == sorted(L["kv_amax"])
    for n in L["kv_amax"]:
        want = torch.from_numpy(Z[f"llama_kv/{n}"].copy())
        err = float(((got[n] - want).abs() / want.abs().clamp_min(1e-12)).max())
        assert err <= 2e-2, f"{n}: rel err {err:.3e}"  # (behind the k / v projections' bf16 GEMMs, as above)
    q = model.get_submodule("model.layers.0.self_attn.q_bmm_quantizer")
    assert q.rotate_is_enabled and not q.is_enabled and getattr(q, "_amax", None) is None


def test_llama_nvfp4_kv_rotate_calibration_matches_the_reference(hostmem):
    model, _ = llama_kv()
    check_llama_kv(model)
