"""compress() on the GPU: moq_int8_pack / moq_int8_unpack against the reference's INT8QTensor (tests/golden/compress.npz) and the
torch restatements of tests/compress_host.py; quantize + compress of the tiny Llama against what the reference packed; and the
fused small-batch linear on packed weights (moq_wq_linear) against the unpack route.

What depends on the model's own GEMMs cannot equal the CPU fixture bit for bit: activations come out of different GEMMs on
the two devices (tests/test_gpu_export.py), so INT4-AWQ's packed bytes and every logit differ in the last bits.  What is
asserted instead:
  * the weight-determined presets (all but INT4-AWQ): packed bytes, scale buffers and metadata byte for byte;
  * INT4-AWQ: every dequantized weight within TWO quantization steps of the fixture's.  The smoothing scale s comes out of
    activation means that differ by a few bf16 ulps (relative r <= 2^-6 with room), so W * s moves by at most 7 r < 0.11 step
    plus its own rounding, a nibble by at most one step, and the group's scale by r, i.e. 8 r < 0.13 step at the largest nibble;
  * every preset: the weight each compressed linear dequantizes to equals, bit for bit, the restatement applied to the bytes
    it holds, and the logits are within 2e-2 of the fixture logits' span (the bound tests/test_gpu_reference_live.py uses
    for the same model across GEMM implementations)."""

import pytest
import torch
import torch.nn.functional as F

import _moa_import
import compress_host as ch

pytestmark = pytest.mark.gpu
moa = _moa_import.load()
from model_optimizer_amd import nn as mnn, numerics, ops, qtensor  # noqa: E402

DEV = "cuda:0"
Z, CASES = ch.fixture()
IC = CASES["icases"]
WEIGHT_DETERMINED = [p for p in sorted(CASES["presets"]) if p != "INT4_AWQ_CFG"]


# ----------------------------------------------------------------------------------------------- INT8 pack / unpack
@pytest.mark.parametrize("k", sorted(IC))
def test_int8_kernels_match_reference_and_restatement(k):
    c = IC[k]
    dt = ch.DT[c["dtype"]]
    x = ch.from_bits(Z[f"{k}_x"], dt).reshape(c["shape"]).to(DEV)
    given = ch.from_bits(Z[f"{k}_scales_in"], dt).reshape(c["scales_shape"]).to(DEV) if c["given"] else None
    bs = None if c["block"] is None else {-1: c["block"]}
    assert numerics.on_host()
    qt, sc = qtensor.INT8QTensor.quantize(x, scales=given, axis=c["axis"], block_sizes=bs)
    assert ch.bits_equal(sc, ch.from_bits(Z[f"{k}_scales"], dt).reshape(sc.shape)), k
    want_q = ch.from_bits(Z[f"{k}_q"], torch.int8).reshape(c["q_shape"])
    assert torch.equal(qt._quantized_data.cpu(), want_q), k
    y = qt.dequantize(scale=sc, block_sizes=bs)
    assert ch.bits_equal(y, ch.from_bits(Z[f"{k}_deq"], dt).reshape(c["shape"])), k
    # the restatement on the same device
    mode, axis_size, inner = ch.layout(c["q_shape"], c["scales_shape"])
    xp = F.pad(x, (0, c["q_shape"][-1] - x.shape[-1]))
    assert torch.equal(ch.int8_pack(xp, sc, mode, axis_size, inner), qt._quantized_data.reshape(-1)), k


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("layout,shape", [(lay, sh) for lay in ("pt", "ax0", "b32") for sh in ((7, 48), (1, 16))]
                         + [("ax1of3", (3, 5, 64)), ("pt", (3, 5, 7))])
def test_int8_c_abi_against_restatement(dn, layout, shape):
    """Every layout x dtype through ops (the C-ABI), odd sizes included: a 7 x 48 row tail, the smallest 1 x 16 packet, the
    middle axis of a [outer, axis, inner] view, and an element count that 4 does not divide."""
    dt = ch.DT[dn]
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.randn(shape, generator=g, device=DEV) * 3).to(dt)
    x.view(-1)[:4] = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0], device=DEV, dtype=dt)
    if layout == "pt":
        sc = (x.float().nan_to_num(0, 0, 0).abs().amax() / 127).to(dt).reshape(())
    elif layout == "ax0":
        sc = (x.float().nan_to_num(0, 0, 0).abs().amax(dim=1, keepdim=True) / 127).to(dt)
    elif layout == "ax1of3":
        sc = (x.float().nan_to_num(0, 0, 0).abs().amax(dim=(0, 2), keepdim=True) / 127).to(dt)
    else:
        if shape[-1] % 32:
            x = F.pad(x, (0, 32 - shape[-1] % 32))
        sc = (x.float().nan_to_num(0, 0, 0).abs().reshape(x.shape[0], -1, 32).amax(dim=-1) / 127).to(dt)
    sc = torch.where(sc == 0, torch.ones_like(sc), sc)
    mode, axis_size, inner = ch.layout(tuple(x.shape), tuple(sc.shape))
    q = ops.int8_quantize(x, sc)
    assert torch.equal(q.reshape(-1), ch.int8_pack(x, sc, mode, axis_size, inner))
    y = ops.int8_dequantize(q, sc, dt)
    assert ch.bits_equal(y.reshape(-1), ch.int8_unpack(q, sc, dt, mode, axis_size, inner))


# ----------------------------------------------------------------------------------------------- whole-model flows
def _restated_weight(m):
    """The weight the reference's formulas give from the bytes and scales this compressed linear holds."""
    w, wq = m.weight, m.weight_quantizer
    cls, (n, k), dt = w.metadata["qtensor_class"].__name__, w.metadata["shape"], w.metadata["dtype"]
    if cls == "INT4QTensor":
        return ch.int4_unpack(w.data, wq._scale, wq.block_sizes[-1])
    if cls == "NVFP4QTensor":
        return ch.nvfp4_unpack(w.data, wq._scale.view(torch.uint8), wq._double_scale, dt)
    if cls == "INT8QTensor":
        return (w.data.to(dt) * wq._scale.to(dt)).reshape(n, k)
    if cls == "FP8QTensor":
        return (w.data.view(torch.float8_e4m3fn).to(dt) * wq._scale.to(dt)).reshape(n, k)
    return None


@pytest.mark.parametrize("preset", sorted(CASES["presets"]))
def test_compress_flow_on_the_device(preset):
    assert numerics.on_host()
    model, was = ch.quantize_and_compress(moa, Z, CASES, preset, device=DEV, quant_gemm=False)
    assert not was and moa.is_real_quantized(model)
    if preset in WEIGHT_DETERMINED:
        ch.compare_packed(model, Z, CASES, preset)
    else:
        same = total = 0
        for n, rec in CASES["presets"][preset]["linears"].items():
            m = model.get_submodule(n)
            ref_bytes = torch.from_numpy(Z[f"{preset}/{n}.weight"].copy()).to(DEV)
            ref_scale = ch.from_bits(Z[f"{preset}/{n}._scale"], torch.bfloat16).reshape(rec["scales"]["_scale"]["shape"]).to(DEV)
            ref_w = ch.int4_unpack(ref_bytes, ref_scale, 128).float()
            got_w = m.weight_quantizer(m.weight).float()
            step = (1.0 / ref_scale.float()).reshape(-1, 1).expand(-1, 128).reshape(ref_w.shape)
            worst = ((got_w - ref_w).abs() / step).max().item()
            assert worst <= 2.0, f"{preset} {n}: a dequantized weight is {worst:.2f} steps from the reference's"
            same += int((m.weight.data == ref_bytes).sum())
            total += ref_bytes.numel()
        print(f"{preset}: {same / total:.4f} of the packed bytes equal the reference's CPU run")
    seen = 0
    for n, rec in CASES["presets"][preset]["linears"].items():
        m = model.get_submodule(n)
        w, wq = m.weight, m.weight_quantizer
        assert isinstance(w, qtensor.QTensorWrapper) and w.is_cuda and list(w.data.shape) == rec["packed_shape"]
        # parameter bytes: numel / 2 (4-bit) or numel (8-bit) of the original weight, plus the scale buffers
        numel = rec["shape"][0] * rec["shape"][1]
        four_bit = rec["qtensor_class"] in ("INT4QTensor", "NVFP4QTensor", "MXFP4QTensor")
        assert w.data.numel() * w.data.element_size() == (numel // 2 if four_bit else numel), n
        scale_bytes = sum(getattr(wq, k).numel() * getattr(wq, k).element_size() for k in rec["scales"])
        want_scale_bytes = sum(int(torch.Size(s["shape"]).numel()) * torch.tensor([], dtype=ch.TD[s["dtype"]]).element_size()
                               for s in rec["scales"].values())
        assert scale_bytes == want_scale_bytes and scale_bytes < numel // 4, n
        want = _restated_weight(m)
        if want is not None:
            assert ch.bits_equal(wq(w), want), f"{preset} {n}: the dequantized weight differs from the restatement"
            seen += 1
    assert seen or preset == "MXFP4_DEFAULT_CFG"
    mnn.ROUTE_CALLS.update(wq_linear=0, unpack=0)
    logits = ch.logits_of(model, Z, DEV)
    assert torch.isfinite(logits.float()).all() and mnn.ROUTE_CALLS["wq_linear"] == 0 and mnn.ROUTE_CALLS["unpack"] == 14
    assert ch.bits_equal(ch.logits_of(model, Z, DEV), logits)
    _assert_logits_near_fixture(logits, f"{preset}/logits")
    # a second compress changes nothing
    before = {k: v.clone() for k, v in model.state_dict().items()}
    moa.compress(model, {"compress": {"default": True}, "quant_gemm": False})
    after = model.state_dict()
    assert list(after) == list(before) and all(ch.bits_equal(after[k], before[k]) for k in before)
    assert ch.bits_equal(ch.logits_of(model, Z, DEV), logits)


def _assert_logits_near_fixture(logits, key):
    ref = ch.from_bits(Z[key], torch.bfloat16).reshape(logits.shape).float()
    span = (ref.max() - ref.min()).item()
    worst = (logits.float().cpu() - ref).abs().max().item()
    print(f"{key}: max |logits - reference CPU logits| = {worst:.4g} (span {span:.4g})")
    assert worst <= 2e-2 * span, f"{key}: {worst:.4g} against 2e-2 x span {span:.4g}"


@pytest.mark.parametrize("preset", [p for p in sorted(CASES["presets"]) if "mlp_compressed" in CASES["presets"][p]])
def test_pattern_variant_on_the_device(preset):
    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset, device=DEV, pattern={"*mlp*": False, "default": True})
    packed = [n for n, m in model.named_modules() if isinstance(getattr(m, "weight", None), qtensor.QTensorWrapper)]
    assert packed == CASES["presets"][preset]["mlp_compressed"]
    for n, m in model.named_modules():
        if isinstance(m, mnn.RealQuantLinear) and "mlp" in n:
            assert m.weight_quantizer.fake_quant and m.weight.dtype == torch.bfloat16 and not m.is_compressed
    _assert_logits_near_fixture(ch.logits_of(model, Z, DEV), f"{preset}/mlp/logits")


@pytest.mark.parametrize("preset", ["INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "NVFP4_DEFAULT_CFG", "INT8_DEFAULT_CFG"])
def test_state_dict_round_trip_on_the_device(preset):
    """Same device, same GEMMs: loading the packed state into a model compressed from OTHER weights reproduces the logits bit
    for bit; so does a loader that replaces the parameter by a plain tensor of the packed shape."""
    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset, device=DEV)
    want = ch.logits_of(model, Z, DEV)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    n0 = next(iter(CASES["presets"][preset]["linears"]))
    assert state[f"{n0}.weight"].is_cuda and state[f"{n0}.weight"].dtype in (torch.uint8, torch.int8)
    other, _ = ch.quantize_and_compress(moa, Z, CASES, preset, device=DEV, model=ch.build_llama(CASES, DEV, seed=7))
    assert not ch.bits_equal(ch.logits_of(other, Z, DEV), want)
    other.load_state_dict(state)
    lin = other.get_submodule(n0)
    assert isinstance(lin.weight, qtensor.QTensorWrapper) and lin.weight.is_cuda
    assert ch.bits_equal(ch.logits_of(other, Z, DEV), want)
    lin._parameters["weight"] = state[f"{n0}.weight"].clone()
    assert isinstance(lin.weight, qtensor.QTensorWrapper) and lin.weight.metadata["shape"] == model.get_submodule(n0).weight.metadata["shape"]
    assert ch.bits_equal(ch.logits_of(other, Z, DEV), want)


def test_forward_unpacks_when_the_kernel_refuses():
    """An input whose storage is not 16-byte aligned is refused by moq_wq_linear (negative status): the linear takes the
    unpack route instead of raising, and computes what it computes for the aligned copy."""
    model, _ = ch.quantize_and_compress(moa, Z, CASES, "INT4_BLOCKWISE_WEIGHT_ONLY_CFG", device=DEV, quant_gemm=True)
    lin = model.get_submodule("model.layers.0.self_attn.q_proj")
    buf = torch.randn(3 * 256 + 1, device=DEV).to(torch.bfloat16)
    x_off = buf[1:].view(3, 256)
    assert x_off.data_ptr() % 16 and x_off.is_contiguous()
    mnn.ROUTE_CALLS.update(wq_linear=0, unpack=0)
    with torch.no_grad():
        y_off = lin(x_off)
        assert mnn.ROUTE_CALLS == {"wq_linear": 0, "unpack": 1}
        y = lin(x_off.clone())
        assert mnn.ROUTE_CALLS == {"wq_linear": 1, "unpack": 1}
        lin._use_real_quant_gemm = False
        assert ch.bits_equal(lin(x_off.clone()), y_off)
    span = (y.float().max() - y.float().min()).item()
    assert (y.float() - y_off.float()).abs().max().item() <= 2e-2 * span


# ----------------------------------------------------------------------------------------------- fused kernel
def _int4_case(n, k, g, dt, seed, exact):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    packed = torch.randint(0, 256, (n, k // 2), generator=gen, device=DEV, dtype=torch.uint8)
    if exact:  # scale 1 or 2: decoded values are integers or halves in [-8, 7]
        scales = torch.randint(1, 3, (n * k // g, 1), generator=gen, device=DEV).to(dt)
    else:
        scales = (7.0 / (torch.rand(n * k // g, 1, generator=gen, device=DEV) * 0.2 + 0.01)).to(dt)
    w_hat = ops.int4_dequantize(packed.reshape(-1), scales.reshape(-1), g).reshape(n, k)
    return dict(packed=packed, scales=scales, scale_2=None, group=g, fmt=ops.WQ_INT4), w_hat


def _nvfp4_case(n, k, dt, seed, exact):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    packed = torch.randint(0, 256, (n, k // 2), generator=gen, device=DEV, dtype=torch.uint8)
    packed[0, :4] = torch.tensor([0x88, 0x08, 0x80, 0x00], device=DEV, dtype=torch.uint8)  # -0 nibbles beside +0
    if exact:  # scale byte 1.0, scale_2 1: decoded values are the E2M1 values themselves
        sb = torch.full((n, k // 16), 0x38, device=DEV, dtype=torch.uint8)
        s2 = torch.ones((), device=DEV)
    else:
        sb = torch.randint(0x18, 0x60, (n, k // 16), generator=gen, device=DEV, dtype=torch.uint8)
        s2 = torch.tensor(0.0173, device=DEV)
    sb[n // 2] = 0  # a row of all-zero block scales: every weight of the row is (+-)0
    scales = sb.view(torch.float8_e4m3fn)
    w_hat = ops.nvfp4_dequantize(packed, scales, s2, dt, 16).reshape(n, k)
    return dict(packed=packed, scales=scales, scale_2=s2, group=16, fmt=ops.WQ_NVFP4), w_hat


def _sparse_x(t, k, dt, seed, asymmetric=False):
    """At most four entries of +-1 per token.  asymmetric: token i + 1 is token i with ONE k moved, so an operand k order that
    differs between the two MFMA sides shows up as a wrong difference between neighbouring tokens."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.zeros(t, k)
    for i in range(t):
        if asymmetric and i:
            x[i] = x[i - 1]
            on = x[i].nonzero().reshape(-1)
            off = (x[i] == 0).nonzero().reshape(-1)
            src, dst = on[torch.randint(len(on), (1,), generator=gen)], off[torch.randint(len(off), (1,), generator=gen)]
            x[i, dst], x[i, src] = x[i, src], 0.0
        else:
            idx = torch.randperm(k, generator=gen)[:4]
            x[i, idx] = torch.where(torch.rand(4, generator=gen) < 0.5, -1.0, 1.0)
    return x.to(dt).to(DEV)


FUSED_SHAPES = ([("int4", n, k, 128) for n in (8, 72) for k in (128, 640)] + [("int4", 72, 64, 32)]
                + [("nvfp4", n, k, 16) for n in (8, 72) for k in (32, 416)])


def _case(fmt, n, k, g, dt, seed, exact):
    return _int4_case(n, k, g, dt, seed, exact) if fmt == "int4" else _nvfp4_case(n, k, dt, seed, exact)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("fmt,n,k,g", FUSED_SHAPES)
def test_fused_linear_exact(fmt, n, k, g, dn):
    """Sums of at most four decoded weights that are multiples of 0.5 with |w| <= 8: every partial sum, the bias sum and the
    result are exactly representable, so the kernel must equal F.linear on the unpacked weight whatever its summation order."""
    dt = ch.DT[dn]
    kw, w_hat = _case(fmt, n, k, g, dt, 11, exact=True)
    assert float(w_hat.float().abs().max()) <= 8 and torch.equal(w_hat.float() * 2, (w_hat.float() * 2).round())
    bias = (torch.randint(-8, 9, (n,), device=DEV).float() / 2).to(dt)
    for t, asym, b in ((1, False, None), (5, True, bias), (32, True, None), (32, False, bias)):
        x = _sparse_x(t, k, dt, 3 + t, asymmetric=asym)
        want = F.linear(x.float(), w_hat.float(), None if b is None else b.float()).to(dt)
        got = ops.wq_linear(x, bias=b, **kw)
        assert ch.bits_equal(got, want), f"{fmt} N={n} K={k} T={t} asym={asym} bias={b is not None}"
        assert ch.bits_equal(ops.wq_linear(x, bias=b, **kw), got)  # run to run
    with pytest.raises(moa.MoquantUnsupported):
        ops.wq_linear(_sparse_x(33, k, dt, 1), bias=None, **kw)


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("fmt,n,k,g", FUSED_SHAPES)
def test_fused_linear_random_within_the_derived_bound(fmt, n, k, g, dn):
    """|y - exact| <= 1.01 (u |exact| + (K + 1) 2^-24 sum_k |x w|): one output rounding (u = 2^-8 bf16, 2^-11 f16) plus an
    fp32 accumulation chain of length K, against the float64 product of the UNPACKED weights."""
    dt, u = ch.DT[dn], (2.0 ** -8 if dn == "bf16" else 2.0 ** -11)
    kw, w_hat = _case(fmt, n, k, g, dt, 23, exact=False)
    gen = torch.Generator(device=DEV).manual_seed(29)
    bias = torch.randn(n, generator=gen, device=DEV).to(dt)
    for t, b in ((1, bias), (5, None), (32, bias)):
        x = torch.randn(t, k, generator=gen, device=DEV).to(dt)
        exact = x.double() @ w_hat.double().T + (0 if b is None else b.double())
        mass = x.double().abs() @ w_hat.double().abs().T + (0 if b is None else b.double().abs())
        got = ops.wq_linear(x, bias=b, **kw)
        err = (got.double() - exact).abs()
        bound = 1.01 * (u * exact.abs() + (k + 1) * 2.0 ** -24 * mass)
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{fmt} {dn} N={n} K={k} T={t}: max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"{fmt} N={n} K={k} T={t}: {worst:.3f} of the bound"
        assert ch.bits_equal(ops.wq_linear(x, bias=b, **kw), got)


def test_fused_linear_refuses_what_it_does_not_read():
    kw, _ = _int4_case(8, 128, 128, torch.bfloat16, 1, True)
    x = torch.zeros(2, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(moa.MoquantUnsupported):  # groups that 32 does not divide
        ops.wq_linear(x, bias=None, **{**kw, "group": 16, "scales": kw["scales"].repeat(8, 1)})
    with pytest.raises((moa.MoquantUnsupported, moa.MoquantError)):  # K % 32
        ops.wq_linear(x[:, :48].contiguous(), kw["packed"][:, :24].contiguous(), kw["scales"], None, None, 48, ops.WQ_INT4)


@pytest.mark.parametrize("preset", ["INT4_BLOCKWISE_WEIGHT_ONLY_CFG", "INT4_AWQ_CFG", "NVFP4_DEFAULT_CFG", "FP8_DEFAULT_CFG"])
def test_compressed_llama_takes_the_kernel(preset):
    """A 1 x 5 prompt through the compressed tiny Llama with quant_gemm on and off.  Each fused linear is within the kernel's
    bound of the unpack route on the SAME input (checked per layer with a hook); the logits of the two routes then differ by the
    few bf16 roundings that propagate, far inside the span of the logits."""
    model, _ = ch.quantize_and_compress(moa, Z, CASES, preset, device=DEV, quant_gemm=True)
    prompt = torch.from_numpy(Z["batch"][:1, :5]).to(DEV)
    worst = [0.0]

    def per_layer(m, args, out):
        if isinstance(m, mnn.RealQuantLinear) and m.is_compressed and m._fused_operands(5, out.dtype) is not None:
            x = m.input_quantizer(args[0])
            w_hat = m.weight_quantizer(m.weight)
            exact = x.double() @ w_hat.double().T
            mass = x.double().abs() @ w_hat.double().abs().T
            bound = 1.01 * (2.0 ** -8 * exact.abs() + (x.shape[-1] + 1) * 2.0 ** -24 * mass)
            worst[0] = max(worst[0], ((out.double() - exact).abs() / bound.clamp_min(1e-300)).max().item())

    hooks = [m.register_forward_hook(per_layer) for m in model.modules() if isinstance(m, mnn.RealQuantLinear)]
    mnn.ROUTE_CALLS.update(wq_linear=0, unpack=0)
    with torch.no_grad():
        fused = model(prompt).logits
    calls = dict(mnn.ROUTE_CALLS)
    for hk in hooks:
        hk.remove()
    for m in model.modules():
        if isinstance(m, mnn.RealQuantLinear):
            m._use_real_quant_gemm = False
    mnn.ROUTE_CALLS.update(wq_linear=0, unpack=0)
    with torch.no_grad():
        plain = model(prompt).logits
    assert mnn.ROUTE_CALLS == {"wq_linear": 0, "unpack": 14}
    if preset == "FP8_DEFAULT_CFG":
        assert calls == {"wq_linear": 0, "unpack": 14} and ch.bits_equal(fused, plain)
        return
    assert calls == {"wq_linear": 14, "unpack": 0}, calls
    print(f"{preset}: worst per-layer err / bound {worst[0]:.3f}")
    assert 0 < worst[0] <= 1.0
    span = (plain.float().max() - plain.float().min()).item()
    assert (fused.float() - plain.float()).abs().max().item() <= 2e-2 * span  # (the bound of tests/test_gpu_reference_live.py)
