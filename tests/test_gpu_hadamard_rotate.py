"""moq_hadamard and moq_hadamard_mx_qdq on the GPU, against the torch restatement of tests/hadamard_host.py.

Everything is compared by bits (NaN positions equal): the arithmetic of the transform is fixed by include/moquant.h, so
there is no tolerance to choose.  Shapes are the smallest that reach every path: strides inside a packet (B <= 8), one
case per cross-lane distance up to the in-wave tier's edge (B = 512, f32: 256), the LDS tier with one and two wave
bits and with packet bits (B = 1024, 4096, 16384), partial last chunks, several blocks per row, unaligned and strided
views, in place, empty tensors, and non-finite / subnormal data."""

import ctypes

import pytest
import torch

import _moa_import
import hadamard_host as hh

moa = _moa_import.load()
from model_optimizer_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
_ID = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def _data(shape, dtype, seed=0):
    """Magnitudes over 2^-12 .. 2^4 with random signs: sums that round in every stage, nothing overflows f16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-12, 5, shape, generator=g).float())
    return x.to(dtype).to(DEV)


def _check(x, block=None, **kw):
    b = ops.hadamard_block_size(x.shape[-1], block)
    want = hh.fwht(x.contiguous(), b)
    got = ops.hadamard(x, block, **kw)
    assert got.shape == x.shape and got.dtype == x.dtype and got.is_contiguous()
    assert hh.same_bits(got, want), f"B={b} shape={tuple(x.shape)} {x.dtype}: " \
        f"{int((got.float() != want.float()).sum())} of {x.numel()} elements differ"
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("block", [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 16384])
def test_every_block_size(dtype, block):
    # rows 1 and 3; three blocks per row where that stays small.  f32 crosses into the LDS tier at B = 512
    _check(_data((1, block), dtype, block))
    _check(_data((3, 3 * block if block <= 1024 else block), dtype, block + 1), block)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_indexing_shapes(dtype):
    _check(_data((67, 384), dtype, 1), 128)            # three blocks per row, 3.14 chunks of 8192, partial last chunk
    _check(_data((5, 16384 * 2), dtype, 2), 16384)     # two-chunk tiles, several of them
    assert ops.hadamard_block_size(1536) == 512
    _check(_data((5, 1536), dtype, 3))                 # B = None: largest power-of-two divisor
    _check(_data((3, 7, 2), dtype, 4))                 # B = 2, n = 42: a partial 16-byte packet at the end
    x = _data((2, 3, 17, 128), dtype, 5).transpose(1, 2)
    assert not x.is_contiguous()
    _check(x)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("block", [8, 128, 2048])
def test_unaligned_view_takes_the_generic_kernel(dtype, block):
    base = _data((3 * block + 1,), dtype, 6)
    x = base[1:].reshape(3, block)                     # contiguous, storage offset of one element: not 16-byte aligned
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    _check(x)
    amax = torch.zeros(1, dtype=torch.float32, device=DEV)
    got = _check(x, running_amax=amax)
    assert torch.equal(amax.view(torch.int32), got.abs().amax().float().reshape(1).view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("block", [64, 4096])
def test_in_place_and_empty(dtype, block):
    x = _data((5, block), dtype, 7)
    want = hh.fwht(x, block)
    y = ops.hadamard(x, block, out=x)
    assert y.data_ptr() == x.data_ptr() and hh.same_bits(x, want)
    e = ops.hadamard(torch.empty(0, block, dtype=dtype, device=DEV))
    assert e.shape == (0, block)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("block", [8, 256, 2048])
def test_non_finite_zero_and_subnormal(dtype, block):
    x = _data((6, block), dtype, 8)
    x[0, 1] = float("nan")
    x[1, 0] = float("inf")
    x[1, block - 1] = float("-inf")                    # inf - inf somewhere in the butterflies: NaN by the additions
    x[2, 3] = float("inf")
    x[3] = 0.0
    x[3, 1::2] = -0.0
    x[4] = -0.0
    tiny = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -149}[dtype]
    x[5] = (torch.arange(block, device=DEV) % 100 + 1).to(torch.float32).mul(tiny).to(dtype)  # subnormals of the dtype
    if dtype != torch.float32:
        assert bool((x[5].float().abs() < torch.finfo(dtype).tiny).all()) and bool((x[5] != 0).all())
    got = _check(x)
    assert torch.isnan(got[0]).all() and torch.isnan(got[1]).any() and not torch.isnan(got[3:]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("block", [128, 1024])
def test_running_amax(dtype, block):
    x1, x2 = _data((40, 3 * block), dtype, 9), _data((7, block), dtype, 10) * 4
    amax = torch.zeros(1, dtype=torch.float32, device=DEV)
    y1 = ops.hadamard(x1, block, running_amax=amax)
    assert hh.same_bits(y1, hh.fwht(x1, block))
    assert torch.equal(amax.view(torch.int32), ops.hadamard(x1, block).abs().amax().float().reshape(1).view(torch.int32))
    y2 = ops.hadamard(x2, block, running_amax=amax)    # accumulates over launches
    both = torch.maximum(y1.abs().amax(), y2.abs().amax()).float().reshape(1)
    assert torch.equal(amax.view(torch.int32), both.view(torch.int32))
    big = torch.full((1,), 3.0e38, dtype=torch.float32, device=DEV)
    ops.hadamard(x1, block, running_amax=big)          # a larger value already there is kept
    assert float(big) == float(torch.tensor(3.0e38, dtype=torch.float32))
    x1[3, 5] = float("nan")                            # the NaN rule of moq_amax: a NaN output makes the running max NaN
    ops.hadamard(x1, block, running_amax=amax)
    assert bool(torch.isnan(amax).all())


# ----------------------------------------------------------------------------------------------- fused with the block QDQ
FORMATS = {"nvfp4": (16, (2, 1), (4, 3), True), "mxfp4": (32, (2, 1), (8, 0), False), "mxfp8": (32, (4, 3), (8, 0), False)}


def _composed(x, rot, block, amax, num_bits, scale_bits, back):
    y = ops.hadamard(x, rot)
    y = ops.dynamic_block_quant(y, block, amax, num_bits, scale_bits)
    return ops.hadamard(y, rot) if back else y


def _fused_rc(x, rot, block, num_bits, scale_bits, amax, back):
    y = torch.empty_like(x)
    f, sf = (_lib.MX_TYPES[ops._MX_FORMAT_MAP[b]] for b in (num_bits, scale_bits))
    ga = None if amax is None or scale_bits == (8, 0) else amax.float().reshape(1)
    rc = _lib.lib().moq_hadamard_mx_qdq(ops._p(x), ops._p(y), x.numel() // x.shape[-1], x.shape[-1], rot,
                                        ops._hadamard_scale(rot), block, ops._dt(x), f, sf, ops._p(ga), int(back), None)
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("rot", [16, 64, 128, 256, 512])
def test_fused_equals_the_standalone_launches(dtype, fmt, rot):
    block, num_bits, scale_bits, needs_amax = FORMATS[fmt]
    x = _data((2, 3, 19, rot), dtype, rot)
    x[0, 0, 1] = 0.0                                                   # an all-zero rotation block
    x[1, 2, 5] = x[1, 2, 5] * 2.0 ** -24                               # a block far below ...
    x[1, 1, 3] = x[1, 1, 3] * 2.0 ** 6                                 # ... and one far above the rest: amax 2^30 apart
    in_wave = rot <= (256 if dtype == torch.float32 else 512)
    for back in (False, True):
        amax = hh.fwht(x, rot).abs().amax().float() if needs_amax else None
        want = _composed(x, rot, block, amax, num_bits, scale_bits, back)
        rc, y = _fused_rc(x, rot, block, num_bits, scale_bits, amax, back)
        if in_wave and rot % block == 0:
            assert rc == _lib.MOQ_OK, (rc, _lib.lib().moq_last_error())
            assert hh.same_bits(y, want), f"{fmt} rot={rot} back={back} {dtype}"
        else:
            assert rc == _lib.MOQ_ERR_UNSUPPORTED
        got = ops.hadamard_block_quant(x, rot, block, amax, num_bits, scale_bits, rotate_back=back)
        assert hh.same_bits(got, want), f"ops {fmt} rot={rot} back={back} {dtype}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID.get)
def test_fused_entry_refuses_what_ops_composes(dtype):
    for rot, block, num_bits, scale_bits in ((1024, 16, (2, 1), (4, 3)), (16, 32, (2, 1), (8, 0))):
        x = _data((3, 5, max(rot, 32)), dtype, rot + block)
        amax = hh.fwht(x, rot).abs().amax().float()
        rc, _ = _fused_rc(x, rot, block, num_bits, scale_bits, amax, False)
        assert rc == _lib.MOQ_ERR_UNSUPPORTED
        for back in (False, True):
            got = ops.hadamard_block_quant(x, rot, block, amax, num_bits, scale_bits, rotate_back=back)
            assert hh.same_bits(got, _composed(x, rot, block, amax, num_bits, scale_bits, back))


def test_the_transform_is_a_rotation():
    """Q and K both rotated, nothing quantized: the attention output is that of the unrotated tensors within the tolerance
    of the reference's test_kv_rotate (tests/gpu/torch/quantization/test_hadamard.py:101: atol=0.05 -- the reference's own
    figure, read there; rotating K alone must NOT pass it, :111)."""
    q, k, v = (torch.randn(2, 4, 33, 128, generator=torch.Generator().manual_seed(s)).to(torch.bfloat16).to(DEV)
               for s in (1, 2, 3))

    def attend(q_, k_):
        return torch.nn.functional.scaled_dot_product_attention(q_, k_, v)

    ref = attend(q, k)
    assert torch.allclose(ref, attend(ops.hadamard(q), ops.hadamard(k)), atol=0.05)
    assert not torch.allclose(ref, attend(q, ops.hadamard(k)), atol=0.05)


def test_entries_check_arguments_before_any_launch():
    lib = _lib.lib()
    P = ctypes.c_void_p(16)
    assert lib.moq_hadamard(P, P, 4, 96, 64, 0.125, _lib.BF16, None, None) == _lib.MOQ_ERR_INVALID
    assert lib.moq_hadamard(P, P, 1, 32768, 32768, 0.1, _lib.BF16, None, None) == _lib.MOQ_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------- host flows on the GPU
import copy  # noqa: E402

import test_hadamard_rotate_cpu as host  # noqa: E402  (the fixture walkers, shared with the CPU tier)
from conftest import assert_bits_equal  # noqa: E402
from model_optimizer_amd import model_calib, model_quant  # noqa: E402
from model_optimizer_amd.tensor_quantizer import QuantizerAttributeConfig as Cfg  # noqa: E402
from model_optimizer_amd.tensor_quantizer import TensorQuantizer as TQ  # noqa: E402


@pytest.mark.parametrize("k", sorted(host.CASES["qcases"]))
def test_quantizer_matches_the_reference_through_the_c_abi(k):
    host.quantizer_case(k, DEV)


def test_llama_fp8_rotate_back_flow_matches_the_reference():
    model, got, logits = host.llama_fp8(DEV)
    diff, scale = host.check_llama_fp8(got, logits, model)
    assert diff <= 0.05 * scale  # (the bound and its reasoning: the CPU tier's test of the same name)


def test_llama_nvfp4_kv_rotate_flow(monkeypatch):
    model, tokens = host.llama_kv(DEV)
    host.check_llama_kv(model)
    # quantized forward: the K states go through ONE fused launch each; forcing the composition gives the same bits
    with torch.no_grad():
        fused = model(tokens[0]).logits
    real = ops.hadamard_block_quant
    calls = []

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "hadamard_block_quant", counted)
    monkeypatch.setattr(ops, "_HADAMARD_QDQ_FUSED", False)
    with torch.no_grad():
        unfused = model(tokens[0]).logits
    assert len(calls) == 2  # one K quantizer per decoder layer
    assert_bits_equal(fused, unfused, "fused entry vs composition")
    assert bool(torch.isfinite(fused).all())


class _Counting:
    """The library handle with a count of the entries called through it."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("moq_") or name == "moq_last_error":
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)

        return call


def test_fast_paths_are_one_launch(monkeypatch):
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    x = _data((2, 4, 33, 128), torch.bfloat16, 11)
    q = TQ(Cfg(**copy.deepcopy(model_quant.NVFP4_KV_ROTATE_CFG["quant_cfg"][1]["cfg"])))
    q.enable_calib()
    q.disable_quant()
    for t in (x, x * 0.5):
        counting.calls.clear()
        y = q(t)
        assert counting.calls == ["moq_hadamard"], counting.calls  # rotation + running abs-max of the calibrator
        assert hh.same_bits(y, hh.fwht(t, 128))
    q.load_calib_amax()
    q.disable_calib()
    q.enable_quant()
    assert_bits_equal(q._amax.float().reshape(()), hh.fwht(x, 128).abs().amax().float(), "amax of the rotated tensor")
    counting.calls.clear()
    y = q(x)
    assert counting.calls == ["moq_hadamard_mx_qdq"], counting.calls
    assert hh.same_bits(y, ops.dynamic_block_quant(hh.fwht(x, 128), 16, q.amax, (2, 1), (4, 3)))


def test_fold_weight_on_a_rotating_weight_quantizer():
    lin = torch.nn.Linear(384, 64, bias=False, dtype=torch.bfloat16, device=DEV)
    model = torch.nn.Sequential(lin)
    moa.nn.replace_quant_module(model)
    rot = {"enable": True, "mode": "rotate_back", "block_size": 128}
    model_quant.set_quantizer_by_cfg(model, {"*weight_quantizer": {"num_bits": (4, 3), "axis": None, "rotate": rot},
                                             "*input_quantizer": {"enable": False}})
    x = _data((5, 384), torch.bfloat16, 12)
    with torch.no_grad():
        model_calib.max_calibrate(model, lambda m: m(x))
        wq = model[0].weight_quantizer
        assert_bits_equal(wq._amax.float().reshape(()), hh.fwht(model[0].weight.detach(), 128).abs().amax().float(), "weight amax")
        # (the fold shows the quantizer the fp32 weight, quant_module.py:148, so it is this -- not the bf16 forward's weight)
        want = wq(model[0].weight.detach().float().contiguous()).to(torch.bfloat16)
        model_quant.fold_weight(model)
        assert_bits_equal(model[0].weight.detach(), want, "folded weight == the quantizer's forward")
        assert not wq.rotate_is_enabled and not wq.is_enabled
        assert_bits_equal(wq(model[0].weight.detach()), model[0].weight.detach(), "a second forward does not rotate again")
        assert_bits_equal(model(x), torch.nn.functional.linear(x, want), "the folded model uses the stored weight as it is")
