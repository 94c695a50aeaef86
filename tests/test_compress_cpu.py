"""compress(): real-quantized weights, CPU tier.

The torch restatements of tests/compress_host.py -- the checker of moq_int8_pack / moq_int8_unpack on the GPU -- are first
pinned bit for bit to what the reference's INT8QTensor computed on CPU (tests/golden/compress.npz); then quantize + compress
run on CPU tensors with the host-memory stand-in of libmoquant, against what the reference's own quantize + compress left in
the tiny Llama for every preset of the fixture: packed bytes, scale buffers, wrapper metadata and the logits of the compressed
model."""

import pytest
import torch

import _moa_import
import compress_host as ch
import hostmem_backend
import nvfp4_export_host as eh
import nvfp4_host as nh

moa = _moa_import.load()
from model_optimizer_amd import qtensor  # noqa: E402
from model_optimizer_amd.nn import QuantLinear, RealQuantLinear  # noqa: E402
from model_optimizer_amd.tensor_quantizer import QuantizerAttributeConfig, TensorQuantizer  # noqa: E402

Z, CASES = ch.fixture()
IC = CASES["icases"]
PRESETS = sorted(CASES["presets"])


@pytest.fixture
def hostmem(monkeypatch):
    fake = hostmem_backend.install(monkeypatch, moa)
    nh.install(fake)
    eh.install(fake)
    ch.install(fake)
    return fake


_LIVE = []


def _live_arrays():
    """The model part of the fixture as the reference generates it on THIS host, or None without a reference here.  The
    logits (and INT4-AWQ's scales) come out of bf16 CPU GEMMs, which are not the same function on every host (see
    conftest.HOST_FORWARD_FIXTURES): where the reference itself does not reproduce the committed arrays, the comparison is
    made with its live run of the same generator."""
    if not _LIVE:
        import sys

        import numpy as np

        sys.path.insert(0, ch.GOLDEN)
        import ref_shim

        _LIVE.append(None)
        if ref_shim.reference_available():
            import gen_compress

            out = {}
            gen_compress.gen_models(out, np.random.Generator(np.random.Philox(20261019)))
            if any(not np.array_equal(out[k], Z[k]) for k in out):
                _LIVE[0] = out
    return _LIVE[0]


def pinned_or_live(check):
    try:
        return check(Z)
    except AssertionError:
        live = _live_arrays()
        if live is None:
            raise
        return check({**Z, **live})


def test_fixture_covers_the_issue_cases():
    assert set(PRESETS) == {"INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "INT4_AWQ_CFG", "FP8_DEFAULT_CFG", "INT8_DEFAULT_CFG",
                            "MXFP4_DEFAULT_CFG", "NVFP4_DEFAULT_CFG"} and not CASES["dropped"]
    assert {c["dtype"] for c in IC.values()} == {"bf16", "f16", "f32"}
    assert {(c["axis"], c["block"], c["given"]) for c in IC.values()} == {(None, None, False), (0, None, False),
                                                                          (None, 32, False), (0, None, True)}
    assert {tuple(c["shape"]) for c in IC.values()} >= {(7, 48), (1, 16)}
    q = Z["i_bf16_7x48_given_q"].view("int8").reshape(-1)
    assert q[:6].tolist() == [127, -128, 127, -128, 127, -128]  # beyond +-127.5: saturated
    assert Z["i_bf16_7x48_pt_q"].view("int8").reshape(-1)[:6].tolist() == [0, 0, 2, -2, 2, -2]  # ties at .5 go to even


def _int8_case(k):
    c = IC[k]
    dt = ch.DT[c["dtype"]]
    x = ch.from_bits(Z[f"{k}_x"], dt).reshape(c["shape"])
    given = ch.from_bits(Z[f"{k}_scales_in"], dt).reshape(c["scales_shape"]) if c["given"] else None
    return c, dt, x, given


@pytest.mark.parametrize("k", sorted(IC))
def test_int8_restatement_matches_reference(k):
    c, dt, x, given = _int8_case(k)
    sc = ch.from_bits(Z[f"{k}_scales"], dt).reshape(c["scales_shape"])
    xp = torch.nn.functional.pad(x, (0, c["q_shape"][-1] - x.shape[-1]))
    mode, axis_size, inner = ch.layout(c["q_shape"], c["scales_shape"])
    q = ch.int8_pack(xp, sc, mode, axis_size, inner)
    assert torch.equal(q, ch.from_bits(Z[f"{k}_q"], torch.int8).reshape(-1)), k
    y = ch.int8_unpack(q, sc, dt, mode, axis_size, inner).reshape(c["q_shape"])[:, : x.shape[-1]]
    assert ch.bits_equal(y, ch.from_bits(Z[f"{k}_deq"], dt).reshape(c["shape"])), k


@pytest.mark.parametrize("k", sorted(IC))
def test_int8_qtensor_through_the_host_backend(hostmem, k):
    c, dt, x, given = _int8_case(k)
    qt, sc = qtensor.INT8QTensor.quantize(x, scales=given, axis=c["axis"],
                                          block_sizes=None if c["block"] is None else {-1: c["block"]})
    assert qt._quantized_data.dtype == torch.int8 and list(qt._quantized_data.shape) == c["q_shape"]
    assert list(sc.shape) == c["scales_shape"] and ch.bits_equal(sc, ch.from_bits(Z[f"{k}_scales"], dt).reshape(sc.shape)), k
    assert torch.equal(qt._quantized_data, ch.from_bits(Z[f"{k}_q"], torch.int8).reshape(c["q_shape"])), k
    y = qt.dequantize(scale=sc, block_sizes=None if c["block"] is None else {-1: c["block"]})
    assert ch.bits_equal(y, ch.from_bits(Z[f"{k}_deq"], dt).reshape(c["shape"])), k


@pytest.mark.parametrize("preset", PRESETS)
def test_compress_matches_the_reference(hostmem, preset):
    model, was = ch.quantize_and_compress(moa, Z, CASES, preset)
    assert not was and moa.is_real_quantized(model)
    got = ch.logits_of(model, Z)

    def check(z):
        ch.compare_packed(model, z, CASES, preset)
        assert ch.bits_equal(got, ch.from_bits(z[f"{preset}/logits"], torch.bfloat16).reshape(got.shape)), \
            f"{preset}: logits of the compressed model differ from the reference's"

    pinned_or_live(check)
    # a second compress changes nothing
    before = {k: v.clone() for k, v in model.state_dict().items()}
    moa.compress(model, {"compress": {"default": True}, "quant_gemm": False})
    after = model.state_dict()
    assert list(after) == list(before) and all(ch.bits_equal(after[k], before[k]) for k in before)
    assert ch.bits_equal(ch.logits_of(model, Z), got)


@pytest.mark.parametrize("preset", [p for p in PRESETS if "mlp_compressed" in CASES["presets"][p]])
def test_pattern_leaves_the_mlp_linears_fake_quantized(hostmem, preset):
    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset, pattern={"*mlp*": False, "default": True})
    packed = [n for n, m in model.named_modules() if isinstance(getattr(m, "weight", None), qtensor.QTensorWrapper)]
    assert packed == CASES["presets"][preset]["mlp_compressed"]
    for n, m in model.named_modules():
        if isinstance(m, RealQuantLinear) and "mlp" in n:
            assert m.weight_quantizer.fake_quant and m.weight.dtype == torch.bfloat16 and not m.is_compressed
    got = ch.logits_of(model, Z)

    def check(z):
        assert ch.bits_equal(got, ch.from_bits(z[f"{preset}/mlp/logits"], torch.bfloat16).reshape(got.shape)), preset

    pinned_or_live(check)


@pytest.mark.parametrize("preset", ["INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "NVFP4_DEFAULT_CFG", "INT8_DEFAULT_CFG"])
def test_state_dict_round_trip(hostmem, preset):
    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset)
    want = ch.logits_of(model, Z)
    state = model.state_dict()
    n0 = next(iter(CASES["presets"][preset]["linears"]))
    assert state[f"{n0}.weight"].dtype in (torch.uint8, torch.int8) and f"{n0}.weight_quantizer._scale" in state
    other, _ = ch.quantize_and_compress(moa, Z, CASES, preset, model=ch.build_llama(CASES, seed=7))
    assert not ch.bits_equal(ch.logits_of(other, Z), want)
    other.load_state_dict(state)
    assert isinstance(other.get_submodule(n0).weight, qtensor.QTensorWrapper)
    assert ch.bits_equal(ch.logits_of(other, Z), want)
    # a loader that REPLACES the parameter by a plain tensor of the packed shape keeps the wrapper and its metadata
    lin = other.get_submodule(n0)
    lin._parameters["weight"] = state[f"{n0}.weight"].clone()
    assert isinstance(lin.weight, qtensor.QTensorWrapper) and lin.weight.metadata["shape"] == model.get_submodule(n0).weight.metadata["shape"]
    assert ch.bits_equal(ch.logits_of(other, Z), want)


def test_fold_weight_leaves_compressed_linears_alone(hostmem):
    model, _ = ch.quantize_and_compress(moa, Z, CASES, "INT8_DEFAULT_CFG", pattern={"*mlp*": False, "default": True})
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    moa.fold_weight(model)
    for n, m in model.named_modules():
        if isinstance(m, RealQuantLinear):
            if m.is_compressed:
                assert m.weight_quantizer.is_enabled and torch.equal(m.weight.data, before[f"{n}.weight"])
            else:
                assert not m.weight_quantizer.is_enabled


def test_export_of_a_compressed_model_raises(hostmem, tmp_path):
    from model_optimizer_amd import export

    model, _ = ch.quantize_and_compress(moa, Z, CASES, "FP8_DEFAULT_CFG")
    with pytest.raises(NotImplementedError, match="compress"):
        export.export_hf_checkpoint(model, export_dir=str(tmp_path))
    with pytest.raises(NotImplementedError, match="compress"):
        export.export_state_dict(model, torch.bfloat16)


def _real(cfg: dict):
    return TensorQuantizer(QuantizerAttributeConfig(fake_quant=False, **cfg))


def test_fake_quant_false_is_accepted_everywhere():
    q = _real({"num_bits": 8, "axis": 0})
    assert not q.fake_quant and q._is_real_quantize_support()
    q2 = TensorQuantizer(QuantizerAttributeConfig(num_bits=8, axis=0))
    q2.update_attributes({"fake_quant": False})
    assert not q2.fake_quant
    q2.set_from_attribute_config(QuantizerAttributeConfig(num_bits=(4, 3), fake_quant=False))
    assert not q2.fake_quant and q2._is_real_quantize_support()
    assert not _real({"num_bits": 4})._is_real_quantize_support()  # INT4 needs blocks


def test_unsupported_real_formats_raise_by_name(hostmem):
    w = torch.randn(8, 64).to(torch.bfloat16)
    nf4 = _real({"num_bits": 4, "block_sizes": {-1: 32, "scale_bits": 8, "scale_block_sizes": {-1: 16}}})
    with pytest.raises(moa.MoquantUnsupported, match="NF4"):
        nf4(w)
    fos = _real({"num_bits": (2, 1), "block_sizes": {-1: 16, "type": "dynamic", "scale_bits": (4, 3), "four_over_six": True}})
    with pytest.raises(NotImplementedError, match="Four-Over-Six"):
        fos(w)
    rot = _real({"num_bits": 4, "block_sizes": {-1: 32}, "rotate": True})
    with pytest.raises(moa.MoquantUnsupported, match="rotating"):
        rot(w)
    back = _real({"num_bits": 4, "block_sizes": {-1: 32}, "rotate": {"enable": True, "mode": "rotate_back"}})
    with pytest.raises(ValueError, match="rotate_back mode is only supported with fake_quant=True"):
        back(w)
    plain = _real({"num_bits": 4, "block_sizes": {-1: 32}})
    packed = plain(w)
    assert isinstance(packed, qtensor.INT4QTensor) and plain._dequantize and plain._scale.shape == (16, 1)
    with pytest.raises(ValueError, match="_dequantize is True"):
        plain(w)  # a quantizer that has packed its weight only dequantizes
    y = plain(qtensor.QTensorWrapper(packed))
    assert y.shape == w.shape and y.dtype == w.dtype


def test_compress_config_forms(hostmem):
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32, bias=True)).to(torch.bfloat16)
    moa.quantize(lin, moa.model_quant.INT8_DEFAULT_CFG, forward_loop=lambda m: m(torch.randn(4, 64).to(torch.bfloat16)))
    assert type(lin[0]) is QuantLinear and not moa.is_real_quantized(lin)
    with pytest.raises(ValueError, match="expected a boolean"):
        moa.compress(lin, {"*": "yes"})
    moa.compress(lin, {"0*": False, "default": True})  # the later, specific pattern overrides the default
    assert type(lin[0]) is RealQuantLinear and not lin[0].is_compressed and lin[0].weight_quantizer.fake_quant
    moa.compress(lin)
    assert lin[0].is_compressed and lin[0].weight.dtype == torch.int8 and lin[0].weight.dim() == 2
    assert lin[0].weight.get_state()["quantized_data.dtype"] == torch.int8


@pytest.mark.parametrize("preset", ["INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "NVFP4_DEFAULT_CFG", "FP8_DEFAULT_CFG"])
def test_quant_gemm_dispatch(hostmem, preset):
    """quant_gemm=True hands calls of at most WQ_LINEAR_MAX_TOKENS tokens of the two 4-bit formats to ops.wq_linear (here its
    float64 stand-in), everything else to the unpack route; a calibrating input quantizer keeps the unpack route."""
    from model_optimizer_amd import nn as mnn

    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset, quant_gemm=True)
    prompt = torch.from_numpy(Z["batch"][:1, :5])
    long = torch.from_numpy(Z["batch"][:2]).repeat(1, 3)[:, : mnn.WQ_LINEAR_MAX_TOKENS // 2 + 1]  # 2 x 17 = 34 tokens
    fused_fmt = preset != "FP8_DEFAULT_CFG"

    def run(tokens):
        mnn.ROUTE_CALLS.update(wq_linear=0, unpack=0)
        with torch.no_grad():
            out = model(tokens).logits
        return out, dict(mnn.ROUTE_CALLS)

    fused, calls = run(prompt)
    assert calls == ({"wq_linear": 14, "unpack": 0} if fused_fmt else {"wq_linear": 0, "unpack": 14})
    assert run(long)[1] == {"wq_linear": 0, "unpack": 14}
    if preset == "INT4_BLOCKWISE_WEIGHT_ONLY_CFG":  # an enabled input quantizer that is calibrating: this linear unpacks
        iq = model.get_submodule("model.layers.0.self_attn.q_proj").input_quantizer
        iq.enable(), iq.disable_quant(), iq.enable_calib()
        assert run(prompt)[1] == {"wq_linear": 13, "unpack": 1}
        iq.disable_calib(), iq.disable()
    for m in model.modules():
        if isinstance(m, RealQuantLinear):
            m._use_real_quant_gemm = False
    plain, calls = run(prompt)
    assert calls == {"wq_linear": 0, "unpack": 14}
    span = (plain.float().max() - plain.float().min()).item()
    assert (fused.float() - plain.float()).abs().max().item() <= 2e-2 * span
