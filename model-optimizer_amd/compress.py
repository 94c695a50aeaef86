"""mtq.compress -- real-quantize the weights of a quantized model (quantization/compress.py:53-133, :196-227).

A calibrated, fake-quantized model becomes one whose linear weights stay PACKED in memory (INT4 nibbles, E2M1 under FP8 block
scales, FP8, INT8, MXFP4 / MXFP8): every quantized linear is class-swapped to RealQuantLinear, `fake_quant` is set on the matching
weight quantizers, and pack_real_quantize_weight replaces each weight by a QTensorWrapper.  The forward dequantizes through the
unpack kernels.  Not carried over: the mode / state framework (compress_restore, modelopt_state), Megatron and FSDP variants."""

from __future__ import annotations

import fnmatch
import warnings

from torch import nn

from .model_quant import set_quantizer_attributes_partial
from .nn import QuantLinear, RealQuantLinear
from .qtensor import QTensorWrapper, pack_real_quantize_weight

__all__ = ["compress", "is_real_quantized"]


def _normalize(config):
    """None, a {pattern: bool} dict, or {"compress": {...}, "quant_gemm": bool} (config.py: CompressConfig)."""
    if config is None:
        return {"default": True}, True
    if not isinstance(config, dict):
        raise ValueError(f"Invalid compression configuration: {config!r}, expected a dict or None.")
    if "compress" in config and isinstance(config["compress"], dict):
        unknown = set(config) - {"compress", "quant_gemm"}
        if unknown:
            raise ValueError(f"Invalid compression configuration: unknown key(s) {sorted(unknown)}")
        return dict(config["compress"]), bool(config.get("quant_gemm", True))
    return dict(config), True


def compress(model: nn.Module, config=None) -> nn.Module:
    """Compress the weights of every layer with an enabled weight quantizer of a supported format, in place.

    config: {pattern: bool} over module names, "default" for everything else; patterns other than "default" are applied in
    order, so later ones override earlier ones ({"*mlp*": False, "default": True} leaves the mlp linears fake-quantized)."""
    patterns, quant_gemm = _normalize(config)
    for value in patterns.values():
        if not isinstance(value, bool):
            raise ValueError(f"Invalid compression configuration: {value}, expected a boolean as value.")
    for module in model.modules():
        if isinstance(module, QuantLinear) and not isinstance(module, RealQuantLinear):
            RealQuantLinear.convert(module)
    if "default" in patterns:
        set_quantizer_attributes_partial(model, "*weight_quantizer*", {"fake_quant": not patterns["default"]})
    for pattern, to_compress in patterns.items():
        if pattern == "default":
            continue
        set_quantizer_attributes_partial(model, lambda name, _p=pattern: fnmatch.fnmatch(name, _p) and "weight_quantizer" in name,
                                         {"fake_quant": not to_compress})
    pack_real_quantize_weight(model)
    if any(isinstance(getattr(m, "weight", None), QTensorWrapper) for m in model.modules()):
        warnings.warn("Real quantization has been applied to the model. Converting it back to its original state and checkpoint "
                      "export of the compressed model are not available.")
    for module in model.modules():
        if isinstance(module, RealQuantLinear):
            module._use_real_quant_gemm = quant_gemm
    return model


def is_real_quantized(model: nn.Module) -> bool:
    return any(isinstance(m, RealQuantLinear) for m in model.modules())
