"""Real-quantised tensors of the path -- mirrors of modelopt.torch.quantization.qtensor.{INT4QTensor, FP8QTensor,
MXFP4QTensor, INT8QTensor} (qtensor/int4_tensor.py:39-130, fp8_tensor.py:40-151, mxfp4_tensor.py:37-144,
int8_tensor.py:35-124) and of QTensorWrapper / pack_real_quantize_weight (qtensor/base_qtensor.py:96-238): same classmethod
`quantize(...) -> (qtensor, scales)` and `dequantize(dtype, scale=..., block_sizes=...)` surface, every pass over
tensor data is one HIP kernel (block amax, pack, unpack).  GPU tensors only."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib, numerics, ops
from ._lib import MoquantUnsupported


class BaseQuantizedTensor:
    """qtensor/base_qtensor.py: original shape / dtype + the packed data."""

    def __init__(self, original_shape, original_dtype, quantized_data):
        self.metadata = {"shape": torch.Size(original_shape), "dtype": original_dtype}
        self._quantized_data = quantized_data


def _div448(amax: torch.Tensor) -> torch.Tensor:
    return _div_const(amax, 448.0)


def _div_const(amax: torch.Tensor, c: float) -> torch.Tensor:
    """amax / c (c = 448.0, 127.0).  torch's GPU `tensor / python_float` multiplies by the reciprocal, which is one ulp off the CPU result
    for some inputs (tensor / tensor divides on both devices).  numerics "host" (default): the TRUE division = the
    reference's CPU run, whatever the device; "device": torch's own kernel on the tensor's device = the reference's run
    there (numerics.py; tools/ops_fuzz.py compares that mode with the reference on the GPU)."""
    if numerics.on_host() or not amax.is_cuda:
        return amax / torch.full((), c, dtype=amax.dtype, device=amax.device)
    return amax / c


def _pad_last(x: torch.Tensor, block: int) -> torch.Tensor:
    pad = (-x.shape[-1]) % block
    return F.pad(x, (0, pad), "constant", 0) if pad else x


class INT4QTensor(BaseQuantizedTensor):
    @classmethod
    def quantize(cls, input: torch.Tensor, block_size: int, rounding: int = _lib.ROUND_HALF_AWAY):
        """int4_tensor.py:39-87: flat view padded to a block multiple, scales = 7 / block amax (input dtype),
        byte = ((q_even + 8) << 4) | (q_odd + 8).  Rounding follows the reference's CUDA kernel (the path taken
        for GPU tensors there): clamp, then round-half-away of v + 8 (tensor_quant_gpu.cu:322-333); ROUND_HALF_EVEN is
        its eager twin (:69-84), what the reference's CPU run computes."""
        assert input.shape[-1] % 2 == 0, "Input tensor must have even number on last dimension."
        flat = _pad_last(input.reshape(-1), block_size).contiguous()
        amax = ops.reduce_amax(flat.view(-1, block_size), axis=(1,))  # input dtype, [n/g, 1]
        scales = (7.0 / amax).view(-1, 1)
        packed = ops.int4_quantize(flat, scales.reshape(-1), block_size, rounding=rounding)
        packed = packed.reshape(*input.shape[:-1], -1)
        return cls(input.shape, input.dtype, packed), scales

    def dequantize(self, dtype: torch.dtype = None, **kwarg):
        """int4_tensor.py:89-130 (CUDA branch): (nibble - 8) / scale in the scale dtype."""
        dtype = dtype or self.metadata["dtype"]
        scales, block = kwarg["scale"], kwarg["block_sizes"][-1]
        out = ops.int4_dequantize(self._quantized_data.reshape(-1), scales.to(self._quantized_data.device).reshape(-1),
                                  block)
        n = math.prod(self.metadata["shape"])
        return out.view(-1)[:n].view(self.metadata["shape"]).to(dtype)


class FP8QTensor(BaseQuantizedTensor):
    @classmethod
    def quantize(cls, input: torch.Tensor, scales: torch.Tensor = None, axis=None, block_sizes: dict | None = None):
        """fp8_tensor.py:40-112.  Supported layouts: per-tensor, one kept axis whose scales run along the flattened
        leading dims (per-channel rows), 1-D blocks along the last dim, and blocks on both axes of a 2-D tensor
        (the FP8 2-D blockwise weight format); other N-D block grids raise."""
        x = input
        if block_sizes:
            dims = {(d if d >= 0 else input.dim() + d): b for d, b in block_sizes.items() if isinstance(d, int)}
            if input.dim() == 2 and set(dims) == {0, 1}:
                # blocks on both axes (fp8_tensor.py:62-100): pad, tile amax, one scale per br x bc tile
                x = ops.reduce_block_padding(input, dims).contiguous()
                br, bc = dims[0], dims[1]
                if scales is None:
                    scales = _div448(ops.reduce_block_amax(x, dims))
                else:
                    scales = scales.reshape(x.shape[0] // br, x.shape[1] // bc)
                q = ops.fp8_quantize_tile(x, scales, br, bc)
                if q.shape != input.shape:
                    q = q[tuple(slice(0, d) for d in input.shape)]
                return cls(input.shape, input.dtype, q), scales
            if list(dims) != [input.dim() - 1]:
                raise MoquantUnsupported("FP8QTensor: blocks along the last dim, or on both axes of a 2-D tensor "
                                         "(reference N-D blocks: fp8_tensor.py:77-100)")
            block = dims[input.dim() - 1]
            x = _pad_last(input, block).contiguous()
            if scales is None:
                amax = ops.reduce_amax(x.view(-1, block), axis=(1,))
                scales = _div448(amax).reshape(*x.shape[:-1], x.shape[-1] // block)
            else:
                scales = scales.reshape(*x.shape[:-1], x.shape[-1] // block)
        elif scales is None:
            if axis is None:
                scales = _div448(ops.reduce_amax(x))
            else:
                ax = [axis] if isinstance(axis, int) else list(axis)
                reduce_axis = [i for i in range(x.dim()) if i not in ax and (i - x.dim()) not in ax]
                scales = _div448(ops.reduce_amax(x, axis=reduce_axis))
        q = ops.fp8_quantize(x, scales)
        if q.shape != input.shape:
            q = q[tuple(slice(0, d) for d in input.shape)]
        return cls(input.shape, input.dtype, q), scales

    def dequantize(self, dtype: torch.dtype = None, **kwarg):
        """fp8_tensor.py:114-151."""
        dtype = dtype or self.metadata["dtype"]
        assert "scale" in kwarg, "Require scale for FP8 dequantization."
        scales, block_sizes = kwarg["scale"], kwarg.get("block_sizes")
        q = self._quantized_data
        dims = {(d if d >= 0 else q.dim() + d): b for d, b in (block_sizes or {}).items() if isinstance(d, int)}
        if q.dim() == 2 and set(dims) == {0, 1}:
            qp = ops.reduce_block_padding(q.view(torch.uint8), dims).contiguous()
            out = ops.fp8_dequantize_tile(qp, scales, dtype, dims[0], dims[1])
            return out[tuple(slice(0, d) for d in self.metadata["shape"])]
        if block_sizes:
            block = block_sizes.get(-1) or block_sizes.get(q.dim() - 1)
            q = _pad_last(q.view(torch.uint8), block).contiguous()
        out = ops.fp8_dequantize(q, scales, dtype)
        return out[tuple(slice(0, d) for d in self.metadata["shape"])]


class MXFP4QTensor(BaseQuantizedTensor):
    E2M1_max = 6.0

    @classmethod
    def quantize(cls, input: torch.Tensor, block_size: int | None):
        """mxfp4_tensor.py:37-81."""
        block_size = block_size or 32
        packed, e8m0 = ops.mxfp4_quantize(input, block_size)
        return cls(input.shape, input.dtype, packed), e8m0

    def dequantize(self, dtype: torch.dtype = None, **kwarg):
        """mxfp4_tensor.py:83-144."""
        dtype = dtype or self.metadata["dtype"]
        return ops.mxfp4_dequantize(self._quantized_data, kwarg["scale"], dtype, kwarg["block_sizes"][-1])


class MXFP8QTensor(BaseQuantizedTensor):
    """E4M3 elements with one E8M0 scale byte per 32 elements of the last dim (qtensor/mxfp8_tensor.py:26-268).

    Two passes over the tensor, both existing kernels: the per-block abs-max (row reduction of the (-1, 32) view,
    `moq_amax_axis`) and the tile pack with a 1 x 32 tile (`moq_fp8_pack_tile`, fp32 scales: the quotient is not
    rounded to the tensor dtype, as torch promotes `weight * scale_factor` to fp32).  The scale bytes in between are the
    reference's own formula on the [..., K / 32] amax tensor.  Dividing by 2^(e-127) here is the reference's
    multiplication by 2^(127-e): both are exact up to the same final rounding (fp32 denormals are preserved on gfx950).
    """

    E4M3_MAX = 448.0
    BLOCK_SIZE = 32
    SCALE_DTYPE = torch.uint8

    @classmethod
    def _compute_e8m0_exponent(cls, amax: torch.Tensor) -> torch.Tensor:
        """mxfp8_tensor.py:43-68: ceil(log2(amax / 448)) in fp32, -127 for blocks without a positive amax."""
        descale = amax.float() / cls.E4M3_MAX
        log2_descale = torch.where(descale > 0, torch.log2(descale), torch.tensor(-127.0, device=descale.device))
        return torch.clamp(torch.ceil(log2_descale), min=-127, max=127)

    @classmethod
    def get_weights_scaling_factor(cls, weight: torch.Tensor) -> torch.Tensor:
        """mxfp8_tensor.py:70-97: uint8 biased exponents [..., K / 32]."""
        assert weight.dim() >= 2, f"Weight must be at least 2D, got {weight.dim()}D"
        assert weight.shape[-1] % cls.BLOCK_SIZE == 0, (
            f"Weight inner dimension ({weight.shape[-1]}) must be divisible by MXFP8 block size ({cls.BLOCK_SIZE})")
        amax = ops.reduce_block_amax(weight, {-1: cls.BLOCK_SIZE})
        return (cls._compute_e8m0_exponent(amax) + 127).to(cls.SCALE_DTYPE)

    @classmethod
    def get_weights_scaling_factor_from_quantizer(cls, weight: torch.Tensor, weight_quantizer) -> torch.Tensor:
        """mxfp8_tensor.py:99-147."""
        assert weight_quantizer.block_sizes[-1] == cls.BLOCK_SIZE, (
            f"MXFP8 requires block size {cls.BLOCK_SIZE}, got {weight_quantizer.block_sizes[-1]}")
        expected = (*weight.shape[:-1], weight.shape[-1] // cls.BLOCK_SIZE)
        scale = getattr(weight_quantizer, "_scale", None)
        if scale is not None:
            assert scale.dtype == cls.SCALE_DTYPE, f"MXFP8 scale must be {cls.SCALE_DTYPE} (E8M0 format), got {scale.dtype}"
            assert tuple(scale.shape) == expected, f"Scale shape {scale.shape} does not match expected shape {expected}"
            return scale
        return cls.get_weights_scaling_factor(weight)

    @classmethod
    def quantize_with_scale(cls, weight: torch.Tensor, weights_scaling_factor: torch.Tensor) -> torch.Tensor:
        """mxfp8_tensor.py:149-197: float8_e4m3fn tensor of the weight's shape."""
        assert weights_scaling_factor.dtype == cls.SCALE_DTYPE, (
            f"weights_scaling_factor must be {cls.SCALE_DTYPE} (E8M0 format), got {weights_scaling_factor.dtype}")
        k = weight.shape[-1]
        assert k % cls.BLOCK_SIZE == 0, f"Weight inner dimension ({k}) must be divisible by MXFP8 block size ({cls.BLOCK_SIZE})"
        descale = torch.exp2(weights_scaling_factor.float() - 127)
        q = ops.fp8_quantize_tile(weight.detach().reshape(-1, k), descale.reshape(-1, k // cls.BLOCK_SIZE), 1, cls.BLOCK_SIZE)
        return q.view(weight.shape)

    @classmethod
    def quantize(cls, input: torch.Tensor, weights_scaling_factor: torch.Tensor | None = None):
        """mxfp8_tensor.py:199-233: ragged last dims are zero-padded to a whole block and cropped afterwards."""
        shape, dtype = input.shape, input.dtype
        x = ops.reduce_block_padding(input, {-1: cls.BLOCK_SIZE})
        if weights_scaling_factor is None:
            amax = ops.reduce_block_amax(x, {-1: cls.BLOCK_SIZE})
            weights_scaling_factor = (cls._compute_e8m0_exponent(amax) + 127).to(cls.SCALE_DTYPE)
        q = cls.quantize_with_scale(x, weights_scaling_factor)[..., : shape[-1]]
        return cls(shape, dtype, q), weights_scaling_factor

    def dequantize(self, dtype: torch.dtype = None, **kwarg):
        """mxfp8_tensor.py:235-268: e4m3 value * 2^(e - 127), computed in fp32, cast to `dtype`."""
        assert "scale" in kwarg, "dequantize requires 'scale' in kwargs"
        dtype = dtype or self.metadata["dtype"]
        shape = self.metadata["shape"]
        q = ops.reduce_block_padding(self._quantized_data.view(torch.uint8), {-1: self.BLOCK_SIZE})
        k = q.shape[-1]
        descale = torch.exp2(kwarg["scale"].float() - 127)
        # the product of an e4m3 value and a power of two is exact in fp32, so rounding it once to `dtype` is the
        # reference's fp32 product followed by .to(dtype)
        out = ops.fp8_dequantize_tile(q.reshape(-1, k).view(torch.float8_e4m3fn), descale.reshape(-1, k // self.BLOCK_SIZE),
                                      torch.float32, 1, self.BLOCK_SIZE)
        return out.view(*q.shape)[..., : shape[-1]].to(dtype)


class NVFP4QTensor(BaseQuantizedTensor):
    """E2M1 elements in blocks of 16, one E4M3 scale per block, one fp32 scale per tensor (qtensor/nvfp4_tensor.py:49-407).

    quantize and dequantize are one kernel each (`moq_nvfp4_pack`: scale bytes and nibbles in one pass, with the block amax
    given -- static quantizers -- or taken from the block; `moq_nvfp4_unpack`).  The scalar `amax / (6 * 448)` runs where
    numerics.mode() puts it; the committed fixtures pin "host", the reference's CPU run.  Not carried over, and refused
    rather than ignored: `keep_high_precision`, `try_tensorrt`, the Triton `fast` dequantize and four-over-six block scales
    (`fp8_max_for_normalization` = 256)."""

    E2M1_MAX = 6.0
    E4M3_MAX = 448.0
    BLOCK_SIZE = 16

    @staticmethod
    def _refuse_four_over_six(quantizer) -> None:
        bs = getattr(quantizer, "block_sizes", None) or {}
        if bs.get("four_over_six", False):
            raise MoquantUnsupported("NVFP4QTensor: four-over-six block scales (fp8_max_for_normalization = 256) are "
                                     "outside this path")

    @staticmethod
    def _refuse(keep_high_precision=False, try_tensorrt=False, fast=False) -> None:
        for flag, name in ((keep_high_precision, "keep_high_precision"), (try_tensorrt, "try_tensorrt"), (fast, "fast")):
            if flag:
                raise MoquantUnsupported(f"NVFP4QTensor: {name}=True is outside this path")

    @classmethod
    def _get_static_global_amax(cls, weight_quantizer):
        g = getattr(weight_quantizer, "global_amax", None)
        return g if g is not None else getattr(weight_quantizer, "_global_amax", None)

    @classmethod
    def _is_static_quantizer(cls, weight_quantizer) -> bool:
        return cls._get_static_global_amax(weight_quantizer) is not None

    @classmethod
    def get_weights_scaling_factor_2_from_quantizer(cls, weight_quantizer) -> torch.Tensor:
        """nvfp4_tensor.py:87-108: global_amax (static) or _amax (dynamic) / (6 * 448), fp32."""
        cls._refuse_four_over_six(weight_quantizer)
        g = cls._get_static_global_amax(weight_quantizer)
        if g is None:
            assert hasattr(weight_quantizer, "_amax"), "Weight quantizer does not have attribute amax"
            g = weight_quantizer._amax
        return numerics.div_scalar(g, cls.E2M1_MAX * cls.E4M3_MAX)

    @classmethod
    def get_weights_scaling_factor_2(cls, input: torch.Tensor) -> torch.Tensor:
        """nvfp4_tensor.py:204-207."""
        return numerics.div_scalar(ops.reduce_amax(input), cls.E2M1_MAX * cls.E4M3_MAX)

    @classmethod
    def get_weights_scaling_factor_from_quantizer(cls, weight_quantizer, weight: torch.Tensor,
                                                  weights_scaling_factor_2: torch.Tensor | None = None,
                                                  keep_high_precision: bool = False):
        """nvfp4_tensor.py:110-166: (float8_e4m3fn [..., cin / 16], scale_2).  The scale bytes come out of the packer, so
        this costs a pack whose nibbles are dropped; export_quantized_weight calls `quantize_from_quantizer` instead."""
        cls._refuse(keep_high_precision=keep_high_precision)
        _, scale, scale_2 = cls._pack_from_quantizer(weight_quantizer, weight, weights_scaling_factor_2)
        return scale, scale_2

    @classmethod
    def _pack_from_quantizer(cls, weight_quantizer, weight, weights_scaling_factor_2=None):
        cls._refuse_four_over_six(weight_quantizer)
        block = weight_quantizer.block_sizes[-1]
        if weights_scaling_factor_2 is None:
            weights_scaling_factor_2 = cls.get_weights_scaling_factor_2_from_quantizer(weight_quantizer)
        if cls._is_static_quantizer(weight_quantizer):
            return ops.nvfp4_quantize(weight, block, amax=weight_quantizer._amax,
                                      global_amax=cls._get_static_global_amax(weight_quantizer),
                                      scale_2=weights_scaling_factor_2)
        return ops.nvfp4_quantize(weight, block, scale_2=weights_scaling_factor_2)

    @classmethod
    def quantize_from_quantizer(cls, weight_quantizer, weight: torch.Tensor):
        """get_weights_scaling_factor_from_quantizer followed by quantize with both scales (what the reference's exporter
        does in two steps, export/quant_utils.py:300-303, :913-933), as ONE pass over the weight:
        (NVFP4QTensor, scale, scale_2)."""
        packed, scale, scale_2 = cls._pack_from_quantizer(weight_quantizer, weight)
        return cls(weight.shape, weight.dtype, packed), scale, scale_2

    @classmethod
    def get_weights_scaling_factor(cls, input: torch.Tensor, block_size: int,
                                   weights_scaling_factor_2: torch.Tensor | None = None, keep_high_precision: bool = False):
        """nvfp4_tensor.py:168-202 (dynamic: the block amax is the block's abs-max)."""
        cls._refuse(keep_high_precision=keep_high_precision)
        assert block_size != 0, "Block size is zero. Cannot return per_block amax for given input."
        _, scale, scale_2 = ops.nvfp4_quantize(input, block_size, scale_2=weights_scaling_factor_2)
        return scale, scale_2

    @classmethod
    def get_activation_scaling_factor(cls, quantizer):
        """nvfp4_tensor.py:209-227: amax.float() / (maxbound * 448)."""
        if not quantizer.is_enabled:
            return None
        amax = quantizer.export_amax()
        if amax is None:
            return None
        scale = numerics.div_scalar(amax, quantizer.maxbound * cls.E4M3_MAX)
        assert torch.all(scale > 0), f" activation scaling factor {scale} not positive."
        return scale

    @classmethod
    def quantize(cls, input: torch.Tensor, block_size: int, weights_scaling_factor: torch.Tensor | None = None,
                 weights_scaling_factor_2: torch.Tensor | None = None, keep_high_precision: bool = False,
                 try_tensorrt: bool = False):
        """nvfp4_tensor.py:253-342: (NVFP4QTensor, scale, scale_2); a ragged last dim is zero-padded to a whole block."""
        cls._refuse(keep_high_precision=keep_high_precision, try_tensorrt=try_tensorrt)
        x = ops.reduce_block_padding(input, {-1: block_size}) if input.shape[-1] % block_size else input
        packed, scale, scale_2 = ops.nvfp4_quantize(x, block_size, scale=weights_scaling_factor,
                                                    scale_2=weights_scaling_factor_2)
        return cls(input.shape, input.dtype, packed), scale, scale_2

    def dequantize(self, dtype: torch.dtype = None, fast: bool = False, **kwarg):
        """nvfp4_tensor.py:344-407, the non-fast branch: kwarg scale=, double_scale=, block_sizes=."""
        self._refuse(fast=fast)
        dtype = dtype or self.metadata["dtype"]
        scale = kwarg["scale"]
        if scale.dtype != torch.float8_e4m3fn:
            raise MoquantUnsupported(f"NVFP4QTensor.dequantize: block scales must be float8_e4m3fn (got {scale.dtype})")
        out = ops.nvfp4_dequantize(self._quantized_data, scale, kwarg["double_scale"], dtype, kwarg["block_sizes"][-1])
        shape = self.metadata["shape"]
        return out[..., : shape[-1]].reshape(shape)


class INT8QTensor(BaseQuantizedTensor):
    """int8 elements under scales of the storage dtype (qtensor/int8_tensor.py:28-124): per-tensor, one kept axis, or blocks
    along the last dim.  One pass each way (`moq_int8_pack` / `moq_int8_unpack`); the arithmetic is the reference's, in
    the storage dtype: scales = amax / 127 in the input dtype, the quotient rounded to it before the round-half-even."""

    @staticmethod
    def _last_block(input: torch.Tensor, block_sizes: dict) -> int:
        dims = {(d if d >= 0 else input.dim() + d): b for d, b in block_sizes.items() if isinstance(d, int)}
        if list(dims) != [input.dim() - 1]:
            raise MoquantUnsupported("INT8QTensor: blocks along the last dim only (reference N-D blocks: int8_tensor.py:68-85)")
        return dims[input.dim() - 1]

    @classmethod
    def quantize(cls, input: torch.Tensor, scales: torch.Tensor | None = None, axis=None, block_sizes: dict | None = None):
        """int8_tensor.py:35-90: (INT8QTensor, scales).  With blocks the data keeps the zero padding of a ragged last dim
        (the reference pads only when it computes the scales itself); dequantize crops it."""
        x = input
        if block_sizes:
            block = cls._last_block(input, block_sizes)
            if scales is None:
                x = _pad_last(input, block).contiguous()
                scales = _div_const(ops.reduce_block_amax(x, {-1: block}), 127.0)
            assert x.shape[-1] % block == 0, f"Tensor dimension {x.dim() - 1}, {x.shape[-1]} is not divisible by {block}."
            expected = (*x.shape[:-1], x.shape[-1] // block)
            assert tuple(scales.shape) == expected, f"Mismatch in expected scale shape: {scales.shape} vs {expected}"
        elif scales is None:
            if axis is None:
                scales = _div_const(ops.reduce_amax(x), 127.0)
            else:
                ax = [axis] if isinstance(axis, int) else list(axis)
                reduce_axis = [i for i in range(x.dim()) if i not in ax and (i - x.dim()) not in ax]
                scales = _div_const(ops.reduce_amax(x, axis=reduce_axis), 127.0)
        return cls(input.shape, input.dtype, ops.int8_quantize(x, scales)), scales

    def dequantize(self, dtype: torch.dtype = None, **kwarg):
        """int8_tensor.py:92-124."""
        dtype = dtype or self.metadata["dtype"]
        assert "scale" in kwarg, "Require scale for INT8 dequantization."
        scales, block_sizes = kwarg["scale"], kwarg.get("block_sizes")
        q = self._quantized_data
        if block_sizes:
            block = self._last_block(q, block_sizes)
            assert q.shape[-1] % block == 0, f"Dimension {q.shape[-1]} is not divisible by {block}."
            expected = (*q.shape[:-1], q.shape[-1] // block)
            assert tuple(scales.shape) == expected, f"Scales shape {scales.shape} must match expected {expected}."
        out = ops.int8_dequantize(q, scales, dtype)
        return out[tuple(slice(0, d) for d in self.metadata["shape"])]


class QTensorWrapper(torch.nn.Parameter):
    """A packed weight as an nn.Parameter (the interface of qtensor/base_qtensor.py:96-145): `.data` is the packed storage,
    `metadata` the original shape and dtype and the QTensor class that reads it.  Built from a QTensor, or from packed storage
    plus the metadata of the wrapper it replaces."""

    _META_KEYS = ("qtensor_class", "shape", "dtype")

    def __new__(cls, qtensor, metadata: dict | None = None):
        storage = qtensor
        if isinstance(qtensor, BaseQuantizedTensor):
            storage = qtensor._quantized_data
            if metadata is None:
                metadata = {**qtensor.metadata, "qtensor_class": type(qtensor)}
        missing = [k for k in cls._META_KEYS if k not in (metadata or {})]
        assert not missing, f"metadata: {metadata} lacks {missing}"
        wrapper = super().__new__(cls, storage, requires_grad=False)
        wrapper.metadata = metadata
        return wrapper

    def _qtensor_as(self, dtype):
        meta = self.metadata
        return meta["qtensor_class"](meta["shape"], dtype, self.data)

    def dim(self):
        """The rank of the ORIGINAL weight (what module code asks a weight for), not of the packed storage."""
        return len(self.metadata["shape"])

    def to(self, *args, **kwargs):
        """Moves the packed bytes; a dtype only changes what the weight dequantizes to."""
        device, dtype = torch._C._nn._parse_to(*args, **kwargs)[:2]
        if device is not None:
            self.data = self.data.to(device)
        return QTensorWrapper(self._qtensor_as(dtype or self.metadata["dtype"]))

    def get_qtensor(self):
        return self._qtensor_as(self.metadata["dtype"])

    def get_state(self):
        return {"metadata": self.metadata, "quantized_data.shape": self.data.shape, "quantized_data.dtype": self.data.dtype}


def dynamically_update_state_methods(module):
    """load_state_dict for a module whose weight may be a QTensorWrapper (the role of base_qtensor.py:172-202): nn.Module would
    refuse the packed tensor for its shape and dtype, so packed entries are taken out of the incoming dict first -- copied into
    the wrapper, or wrapped where the parameter is still on the meta device -- the module's own loader sees the rest, and the
    entries are put back for whoever reads the dict afterwards."""
    inherited = module._load_from_state_dict

    def load_packed_first(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        packed = {}
        for name, held in list(self._parameters.items()):
            key = prefix + name
            if not isinstance(held, QTensorWrapper) or key not in state_dict:
                continue
            packed[key] = state_dict.pop(key)
            if held.is_meta:
                self._parameters[name] = QTensorWrapper(packed[key], metadata=held.metadata)
            else:
                with torch.no_grad():
                    held.data.copy_(packed[key])
        inherited(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        missing_keys[:] = [k for k in missing_keys if k not in packed]  # (loaded above, not missing)
        state_dict.update(packed)

    module._load_from_state_dict = load_packed_first.__get__(module, type(module))


def _packs_its_weight(m) -> bool:
    w, wq = getattr(m, "weight", None), getattr(m, "weight_quantizer", None)
    if w is None or wq is None or w.is_meta:  # nothing to pack, or nothing materialised yet
        return False
    return bool(wq.is_enabled and not wq._fake_quant and w.element_size() > 1)  # (one-byte storage is packed already)


def pack_real_quantize_weight(module, force_quantize: bool = False):
    """Replace the weight of every submodule whose weight quantizer is enabled and in real-quantize mode by its packed form
    (the role of base_qtensor.py:205-238).  A quantizer chain packs with its first member, as in the reference; with
    `force_quantize` a quantizer that had already packed once packs again."""
    from .tensor_quantizer import SequentialQuantizer

    with SequentialQuantizer.convert_to_single_quantizer(module), torch.no_grad():
        for m in [m for m in module.modules() if m is not module and _packs_its_weight(m)]:
            if force_quantize:
                m.weight_quantizer._dequantize = False
            m.weight = QTensorWrapper(m.weight_quantizer(m.weight))


torch.serialization.add_safe_globals([QTensorWrapper, INT4QTensor, FP8QTensor, MXFP4QTensor, MXFP8QTensor, NVFP4QTensor,
                                      INT8QTensor])
