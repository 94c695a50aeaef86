"""QuantLinear -- mirror of the reference's _QuantLinear (nn/modules/quant_linear.py:38-53,
quant_module.py:227-278): an nn.Linear with input / weight / output TensorQuantizers -- and RealQuantLinear (:196-330), the
same module once mtq.compress has packed its weight."""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .tensor_quantizer import QuantizerAttributeConfig, TensorQuantizer


class QuantLinear(nn.Linear):
    """forward = output_quantizer(F.linear(input_quantizer(x), weight_quantizer(W), b))."""

    default_quant_desc_input = QuantizerAttributeConfig(num_bits=8, axis=None)
    default_quant_desc_weight = QuantizerAttributeConfig(num_bits=8, axis=0)

    def _setup(self):
        # (input, output, weight: the reference's registration order -- the order of named_modules(), hence of the lines of
        # print_quant_summary and of the quantizer buffers in state_dict())
        self.input_quantizer = TensorQuantizer(self.default_quant_desc_input)
        self.output_quantizer = TensorQuantizer(QuantizerAttributeConfig(enable=False))
        self.weight_quantizer = TensorQuantizer(self.default_quant_desc_weight)

    @classmethod
    def convert(cls, linear: nn.Linear) -> "QuantLinear":
        """In-place class swap (the reference's DynamicModule conversion keeps parameters in place)."""
        linear.__class__ = cls
        linear._setup()
        return linear

    def forward(self, input):
        x = self.input_quantizer(input)
        wq, oq, w = self.weight_quantizer, self.output_quantizer, self.weight
        if not (type(wq) is TensorQuantizer and wq.weight_already_counted(w)):
            w = wq(w)
        y = F.linear(x, w, self.bias)
        return y if type(oq) is TensorQuantizer and oq.hands_back() else oq(y)


# Which calls of a compressed linear RealQuantLinear hands to the fused kernel on packed weights (ops.wq_linear); every other call
# unpacks the weight and runs F.linear.  From the table of profiles/r11_compress.md (both routes timed alternately in one run,
# weights never cache-resident, T = 1, 8, 16, 32): on every measured shape with K <= 4096 (4096 x 4096, 14336 x 4096,
# 1024 x 4096, 4096 x 2048) the kernel wins at every T for both formats (1.36-2.3x, spreads under 6 %); on 4096 x 14336 its 128
# workgroups walk K in too long a chain: INT4 is ahead by more than the spread only up to T = 8 (1.00-1.02x), NVFP4 loses at
# every T (0.77x).  The issue's single threshold over its three shapes would be INT4 8 / NVFP4 0; this rule keeps the kernel
# where it measured faster: up to WQ_LINEAR_MAX_TOKENS tokens where K <= WQ_LINEAR_SHORT_K, above that K the per-format limit
# the long shape measured (0 = never).  K between 4096 and 14336 is unmeasured and treated like 14336.
WQ_LINEAR_MAX_TOKENS = 32
WQ_LINEAR_SHORT_K = 4096
WQ_LINEAR_LONG_K_MAX_TOKENS = {"int4": 8, "nvfp4": 0}
ROUTE_CALLS = {"wq_linear": 0, "unpack": 0}  # forwards of compressed linears by route (tests, tools/compress_bench.py)


class _RealQuantParameterDict(dict):
    """The `_parameters` table of a RealQuantLinear (quant_linear.py:247-286): a plain tensor assigned to `weight` -- loaders
    that replace parameters instead of copying into them -- is re-wrapped when it has the packed shape, and packed by the
    weight quantizer when it is a high-precision weight."""

    def __init__(self, weight_quantizer, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.weight_quantizer = weight_quantizer

    def __setitem__(self, key, value):
        from .qtensor import QTensorWrapper

        if key == "weight" and value is not None and not isinstance(value, QTensorWrapper):
            existing, wq = self.get("weight"), self.weight_quantizer
            if isinstance(existing, QTensorWrapper) and not existing.is_meta and existing.shape == value.shape:
                super().__setitem__(key, QTensorWrapper(value.data, metadata=existing.metadata))
                return
            if (isinstance(wq, TensorQuantizer) and wq.is_enabled and not wq._fake_quant and value.element_size() > 1
                    and not value.is_meta):
                with torch.no_grad():
                    value = QTensorWrapper(wq(value))
        super().__setitem__(key, value)


class RealQuantLinear(QuantLinear):
    """A QuantLinear whose weight may be a QTensorWrapper: forward = F.linear(input_quantizer(x), weight_quantizer(W), b), the
    weight quantizer dequantizing the packed weight through the unpack kernels."""

    list_of_scale_tensors = ["_scale", "_double_scale", "_scale_zeros"]

    @classmethod
    def convert(cls, linear: QuantLinear) -> "RealQuantLinear":
        from .qtensor import dynamically_update_state_methods

        linear.__class__ = cls
        linear._parameters = _RealQuantParameterDict(linear.weight_quantizer, linear._parameters)
        dynamically_update_state_methods(linear)
        return linear

    @property
    def is_compressed(self) -> bool:
        from .qtensor import QTensorWrapper

        return isinstance(self._parameters.get("weight"), QTensorWrapper)

    def _fused_operands(self, tokens: int, dtype):
        """(packed, scales, scale_2, group, fmt) when this call may take ops.wq_linear, else None: `quant_gemm` on, one of the
        two 4-bit formats in a layout the kernel reads, a token count inside the measured limits above, input quantizer not calibrating."""
        from . import ops
        from .qtensor import INT4QTensor, NVFP4QTensor

        wq, iq, w = self.weight_quantizer, self.input_quantizer, self.weight
        if (not getattr(self, "_use_real_quant_gemm", False) or tokens > WQ_LINEAR_MAX_TOKENS or tokens == 0
                or type(wq) is not TensorQuantizer or dtype not in (torch.bfloat16, torch.float16)
                or (iq.is_enabled and iq._if_calib)):
            return None
        meta = w.metadata
        if len(meta["shape"]) != 2 or meta["dtype"] != dtype or w.data.dim() != 2 or not ops._is_gpu(w):
            return None
        n, k = meta["shape"]
        scale, bs = getattr(wq, "_scale", None), wq.block_sizes or {}
        g = bs.get(-1) or bs.get(1)
        if k % 32 or scale is None or not g or tuple(w.data.shape) != (n, k // 2):
            return None
        long_k = k > WQ_LINEAR_SHORT_K
        if meta["qtensor_class"] is INT4QTensor and g % 32 == 0 and k % g == 0 and scale.dtype == dtype:
            if long_k and tokens > WQ_LINEAR_LONG_K_MAX_TOKENS["int4"]:
                return None
            return w.data, scale, None, g, ops.WQ_INT4
        if (meta["qtensor_class"] is NVFP4QTensor and g == 16 and scale.dtype == torch.float8_e4m3fn
                and getattr(wq, "_double_scale", None) is not None and wq._double_scale.numel() == 1):
            if long_k and tokens > WQ_LINEAR_LONG_K_MAX_TOKENS["nvfp4"]:
                return None
            return w.data, scale, wq._double_scale, 16, ops.WQ_NVFP4
        return None

    def forward(self, input):
        if not self.is_compressed:  # (left fake-quantized by the compress pattern)
            return super().forward(input)
        x = self.input_quantizer(input)  # pre-quant scale and input QDQ: the same on both routes
        fused = self._fused_operands(x.numel() // max(x.shape[-1], 1), x.dtype)
        if fused is not None and (self.bias is None or self.bias.dtype == x.dtype):
            from . import ops

            from ._lib import MoquantUnsupported

            packed, scale, scale_2, g, fmt = fused
            try:
                y = ops.wq_linear(x, packed, scale, scale_2, self.bias, g, fmt)
                ROUTE_CALLS["wq_linear"] += 1
            except MoquantUnsupported:  # the kernel's own refusal (an x or weight that is not 16-byte aligned): unpack
                fused = None
        else:
            fused = None
        if fused is None:
            y = F.linear(x, self.weight_quantizer(self.weight), self.bias)
            ROUTE_CALLS["unpack"] += 1
        oq = self.output_quantizer
        return y if type(oq) is TensorQuantizer and oq.hands_back() else oq(y)


class QuantLayerNorm(nn.LayerNorm):
    """nn.LayerNorm with an input (and output) quantizer -- the reference registers nn.LayerNorm with QuantInputBase
    (nn/modules/quant_layernorm.py:28, quant_module.py:192-240), so the `*input_quantizer` entries of the presets also
    fake-quantize what goes INTO every LayerNorm of OPT / GPT-style models.  RMSNorm classes of the Llama family are
    model code, not nn.LayerNorm, and stay untouched on both sides."""

    def _setup(self):
        self.input_quantizer = TensorQuantizer(QuantLinear.default_quant_desc_input)
        self.output_quantizer = TensorQuantizer(QuantizerAttributeConfig(enable=False))

    @classmethod
    def convert(cls, norm: nn.LayerNorm) -> "QuantLayerNorm":
        norm.__class__ = cls
        norm._setup()
        return norm

    def forward(self, input):
        return self.output_quantizer(super().forward(self.input_quantizer(input)))


def is_quantized_linear(m) -> bool:
    return isinstance(m, QuantLinear)


def replace_quant_module(model: nn.Module) -> nn.Module:
    """nn.Linear -> QuantLinear everywhere (conversion.py:214 replace_quant_module for the Linear entry); attention
    modules of a Hugging Face model get their KV-cache quantizers (plugins/huggingface.py:371-415, run by the
    reference from the same place through its on-the-fly plugin registry); fused 3-D expert containers get per-expert
    weight quantizers (:1697-1730)."""
    from .hf_attention import register_hf_attentions_on_the_fly
    from .hf_experts import register_fused_experts_on_the_fly

    register_hf_attentions_on_the_fly(model)
    register_fused_experts_on_the_fly(model)
    for mod in list(model.modules()):
        # nn.Linear itself, and FalconLinear (an nn.Linear subclass computing input @ W.T + b), which the reference
        # registers explicitly (plugins/huggingface.py:1417-1420, :1574-1590); other subclasses are left alone
        if type(mod) is nn.Linear or (type(mod).__name__ == "FalconLinear" and isinstance(mod, nn.Linear)):
            QuantLinear.convert(mod)
        elif type(mod) is nn.LayerNorm:
            QuantLayerNorm.convert(mod)
        elif type(mod).__name__ == "Conv1D" and type(mod).__module__.startswith("transformers."):
            # transformers' Conv1D (GPT-2) is a linear layer with a transposed [in, out] weight and addmm: the weight
            # is transposed once and the module becomes a quantized nn.Linear (plugins/huggingface.py:559-571)
            with torch.no_grad():
                mod.weight = nn.Parameter(mod.weight.T.contiguous())
            mod.out_features, mod.in_features = mod.weight.shape
            QuantLinear.convert(mod)
    return model
