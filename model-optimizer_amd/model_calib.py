"""Calibration algorithms of the path -- mirrors of quantization/model_calib.py on our kernels:
max_calibrate (:310-498), smoothquant (:1273-1359), awq_clip (:1724-1940) and their helpers; awq_lite (:1394-1721) lives in
awq_search.py and is re-exported at the bottom of this file.

Host-side orchestration is the reference's; the passes over tensor data are HIP kernels:
  weights            -> ONE multi-tensor launch per pass for all linears that share a format
  activations        -> fused column statistics (sum |x| + abs-max in one read)
  AWQ search weights -> fused (W * s) -> group amax -> INT-k QDQ
  cross-rank sync    -> one bucketed collective per reduce op (distributed.py)
"""

from __future__ import annotations

import math
import time
import warnings

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from . import distributed as mdist
from . import numerics
from . import ops
from .multi_tensor import SegmentTable
from .hf_experts import is_quant_fused_experts
from .nn import QuantLinear, is_quantized_linear
from ._lib import MoquantUnsupported
from .tensor_quantizer import SequentialQuantizer, TensorQuantizer


def _quantizers(model):
    return [m for m in model.modules() if isinstance(m, TensorQuantizer)]


def _dist_on() -> bool:
    return mdist.active()


def enable_stats_collection(model: nn.Module, distributed_sync: bool = False):
    """model_calib.py:1128-1141.  Every enabled quantizer stops quantizing while statistics are collected -- the
    dynamic ones too (their `enable_calib` is a no-op), so that the static quantizers downstream of them calibrate on
    clean activations; a quantizer without a calibrator is switched off altogether (:1140-1141).

    distributed_sync (data-parallel calibration): histogram calibrators take the bin width of rank 0's first batch
    (one broadcast at their first collect), so that the ranks' counts can be summed exactly at the end."""
    for q in _quantizers(model):
        if not q.is_enabled:
            continue
        if q._use_constant_amax or q._constant_amax is not None:
            q.disable_quant()  # nothing to calibrate; no quantization error into the other quantizers' statistics (:1132-1136)
            continue
        if q._calibrator is not None:
            q.disable_quant()
            q.enable_calib()
            if hasattr(q._calibrator, "share_range_across_ranks"):
                q._calibrator.share_range_across_ranks(distributed_sync and _dist_on())
        else:
            q.disable()


def finish_stats_collection(model: nn.Module, method: str | None = None, distributed_sync: bool = False, **kwargs):
    """model_calib.py:1144-1167: load_calib_amax on every calibrated quantizer, back to quant mode.

    distributed_sync: the raw histograms of all histogram calibrators are SUM-reduced in one bucket before their
    amax is computed (the reference leaves every rank with its own histogram, calib/histogram.py:158-163); running
    maxima need nothing here -- their amax is MAX-reduced afterwards (sync_amax_bucketed)."""
    from . import calib as _calib

    if _calib.DeferredAmax.current is not None:
        _calib.DeferredAmax.current.flush()  # nobody reads a calibrator before the requests noted for it are answered
    qs = [q for q in _quantizers(model) if q.is_enabled]
    live = [q for q in qs if not (q._use_constant_amax or q._constant_amax is not None)]  # the others were never calibrating
    if distributed_sync and _dist_on():
        mdist.sync_calibrators_bucketed([q._calibrator for q in live if q._calibrator is not None and not q._dynamic
                                         and hasattr(q._calibrator, "share_range_across_ranks")])
    # histogram calibrators: every threshold search is QUEUED first (device kernels, calib.HistogramCalibrator.begin_amax)
    # and read afterwards, so a model's searches overlap and the host does not wait once per quantizer
    tickets = {}
    if method:
        for q in live:
            if q._calibrator is not None and not q._dynamic and hasattr(q._calibrator, "begin_amax"):
                tickets[id(q)] = q._calibrator.begin_amax(method, **kwargs)
    from .calib import MaxCalibrator

    plain_max = [q._calibrator for q in live if type(q._calibrator) is MaxCalibrator and not q._dynamic] if not method else []
    max_verified = bool(plain_max) and MaxCalibrator.verify_finite(plain_max)  # one host read for the NaN / inf asserts
    for q in qs:
        if q._use_constant_amax or q._constant_amax is not None:
            q.enable_quant()  # (:1150-1153)
            continue
        if q._calibrator is not None and not q._dynamic:
            if id(q) in tickets:
                amax = q._calibrator.finish_amax(tickets.pop(id(q)))
            elif max_verified and type(q._calibrator) is MaxCalibrator:
                amax = q._calibrator.compute_amax(verified=True)
            else:
                amax = q._calibrator.compute_amax(**({"method": method, **kwargs} if method else {}))
            if amax is not None:  # quantizers that saw no data keep whatever amax they had (:1155-1161)
                q.replace_amax(amax)  # (buffer shape of the reference for N-D block grids, like load_calib_amax)
        if q.bias_calibrator is not None and q.bias_type == "static":
            q.load_calib_bias()  # the affine offset of the KV-cache presets (:1163-1164)
        q.enable_quant()  # dynamic quantizers come back on here (:1166)
        q.disable_calib()


def _foreign_weight_pairs(m) -> list:
    """(weight, quantizer) pairs of a quantized module of ANOTHER package that enumerates its own weights -- the reference's
    `QuantModule.iter_weights_for_calibration` (nn/modules/quant_module.py:123-129; the per-expert slices of its fused MoE
    containers, plugins/huggingface.py:1085-1101).  Under the algorithm seam such a module keeps its class for the call while
    its quantizers are this package's (modelopt_algorithms.Adoption); the reference calibrates those weights from the tensors
    themselves, whatever the routing of the calibration batches did (model_calib.py:348-352), and so does this."""
    it = getattr(m, "iter_weights_for_calibration", None)
    if not callable(it) or is_quantized_linear(m) or is_quant_fused_experts(m):
        return []
    return [(w, q) for w, q in it() if isinstance(q, (TensorQuantizer, SequentialQuantizer))]


def refuse_rotation(model: nn.Module, what: str):
    """Raise for the first quantizer of `model` whose rotation is on: `what` (a calibration algorithm other than max, a
    sparsity search, the checkpoint export) works on the tensors with kernels of its own, past TensorQuantizer.forward, and
    would drop the rotation without a word."""
    for name, mod in model.named_modules():
        if isinstance(mod, TensorQuantizer) and mod.rotate_is_enabled:
            raise MoquantUnsupported(f"{what} does not take rotating quantizers ({name}: rotate is enabled); only max "
                                     "calibration, quantized forwards and fold_weight go through the rotation")


def weight_only_quantize(model: nn.Module, shard: bool = False):
    """model_calib.py:187-199: pass every weight through its quantizer (collects weight statistics).

    Fast path: all enabled per-tensor 'max' weight quantizers of one dtype are calibrated by ONE
    multi-tensor abs-max launch instead of one reduction per layer.

    shard (data-parallel replicas): the (weight, quantizer) list is dealt round-robin over the ranks
    (distributed.shard_list) and every rank calibrates only its share -- independent units, no data-path collective;
    the values reach the other ranks with the amax MAX-reduction that follows (a rank without a value joins with the
    identity, distributed.sync_amax_bucketed).  Only valid when that reduction runs (max_calibrate does both)."""
    pairs = [(m.weight, m.weight_quantizer) for m in model.modules()
             if is_quantized_linear(m) and m.weight_quantizer.is_enabled]
    for m in model.modules():  # fused MoE expert containers: one (slice, quantizer) pair per expert and projection
        if is_quant_fused_experts(m):
            pairs += [(w, q) for w, q in m.iter_weights_for_calibration() if q.is_enabled]
        else:
            pairs += [(w, q) for w, q in _foreign_weight_pairs(m) if q.is_enabled]
    if shard and _dist_on():
        pairs = mdist.shard_list(pairs)
    batched = []
    for w, wq in pairs:
        per_tensor_max = (isinstance(wq, TensorQuantizer) and wq._if_calib and wq.axis is None and wq.block_sizes is None
                          and type(wq._calibrator).__name__ == "MaxCalibrator" and w.is_cuda
                          and w.is_contiguous() and wq.pre_quant_scale is None and wq.bias is None
                          and not wq.rotate_is_enabled)  # (the statistics are those of the ROTATED weight: its own forward)
        if per_tensor_max:
            batched.append((w, wq))
        else:
            wq(w)
            if isinstance(wq, TensorQuantizer) and wq._if_calib:
                wq.mark_weight_stats_done(w)
    by_key = {}
    for w, wq in batched:
        by_key.setdefault((w.dtype, w.device), []).append((w, wq))
    for group in by_key.values():
        tab = SegmentTable([w.detach() for w, _ in group], outputs=[w.detach() for w, _ in group])
        amax = tab.calibrate_amax()
        held = amax.clone()  # ONE copy; every fresh calibrator keeps a one-element view of it (was a clone launch per weight)
        for i, (w, wq) in enumerate(group):
            cal = wq._calibrator
            if cal._buf is None:
                cal._buf = held[i:i + 1]
                cal._shape, cal._dtype = (), w.dtype
            else:
                torch.maximum(cal._buf, amax[i:i + 1], out=cal._buf)
            wq.mark_weight_stats_done(w)


_MAX_CALIBRATE_DEPTH = [0]


def _deferred_stats_plan(model: nn.Module, forward_loop, defer_stats):
    """(device, decoder layers) when the per-tensor running maxima of this calibration may be answered layer by layer
    (calib.DeferredAmax), else None.  Automatic (defer_stats=None) for Hugging Face decoder stacks on a GPU -- the flush
    points are their decoder layers' ends, and between a linear's forward and the end of its layer such a model leaves the
    linear's input alone (a write is caught at the flush); defer_stats=True asks for it on any model that has a decoder
    stack layerwise.get_decoder_layers finds; False never defers."""
    from . import calib as _calib

    if defer_stats is False or forward_loop is None or _calib.DeferredAmax.current is not None or not isinstance(model, nn.Module):
        return None
    dev = next((p.device for p in model.parameters()), None)
    if dev is None or dev.type != "cuda":
        return None
    from . import layerwise
    from .hf_attention import _is_supported_hf_model

    layers = layerwise.get_decoder_layers(model)
    if layers is None or (defer_stats is None and not _is_supported_hf_model(model)):
        return None
    return dev, list(layers)


@torch.no_grad()
def max_calibrate(model: nn.Module, forward_loop=None, distributed_sync: bool = True, shard_weights: bool | None = None,
                  sync_expert_weight_amax: bool = False, defer_stats: bool | None = None):
    """model_calib.py:310-498 (DP part): collect abs-max statistics for weights and activations, load them,
    then MAX-reduce every amax across the data-parallel group in ONE bucket; each rank's forward_loop sees its own
    share of the calibration batches.

    shard_weights: deal the weight statistics over the ranks (weight_only_quantize(shard=True)); the values reach the
    other ranks with the MAX bucket.  Only correct when every rank holds the SAME weights (data-parallel replicas):
    under tensor parallelism / FSDP the ranks hold different shards and each must calibrate all of its own -- so the
    default (None) shards only after `distributed.declare_data_parallel()`, and never without `distributed_sync`.
    Tensor-parallel callers pass distributed_sync=False and synchronise by `distributed.sync_amax_tensor_parallel`.

    sync_expert_weight_amax: blocks of separate expert modules share one weight amax per projection as well (the input
    amax is always shared, hf_moe.layer_sync_moe_local_experts_amax; model_calib.py:365-368).

    defer_stats: ONE statistics launch per decoder layer instead of one per quantizer call (calib.DeferredAmax;
    _deferred_stats_plan says when).  Same amax, bit for bit: a maximum does not care in which launch it was taken.

    MAX_CALIBRATE_STATS (phase clock, device drained at the phase boundaries) is filled by the OUTERMOST call only: nested
    calls -- per linear inside awq(), per layer in layerwise / gptq, per starved expert in hf_moe -- neither wipe it nor
    add host syncs to the product path."""
    sync = distributed_sync and _dist_on()
    outer = _MAX_CALIBRATE_DEPTH[0] == 0
    stats = MAX_CALIBRATE_STATS if outer else {}
    stats.clear()
    dev0 = next((p.device for p in model.parameters()), None)

    def lap(name, t=[None]):
        if not outer:
            return
        if dev0 is not None and dev0.type == "cuda":
            torch.cuda.synchronize(dev0)
        now = time.perf_counter()
        if t[0] is not None:
            stats[name] = round(now - t[0], 4)
        t[0] = now

    _MAX_CALIBRATE_DEPTH[0] += 1
    try:
        lap(None)
        enable_stats_collection(model, distributed_sync=sync)
        lap("enable_s")
        weight_only_quantize(model, shard=sync and mdist.resolve_shard(shard_weights))
        lap("weights_s")
        if forward_loop is not None:
            plan = _deferred_stats_plan(model, forward_loop, defer_stats)
            if plan is None:
                forward_loop(model)
            else:
                from . import calib as _calib

                # (defer_stats=None: nobody vouched for the model -- the first pass through the layers only watches, see
                # DeferredAmax.probation; defer_stats=True: deferred from the first request, a write is an error)
                batch = _calib.DeferredAmax(plan[0], probation=defer_stats is None, flush_points=len(plan[1]))
                hooks = [layer.register_forward_hook(lambda *_a, _b=batch, _k=id(layer): _b.flush(key=_k)) for layer in plan[1]]
                _calib.DeferredAmax.current = batch
                try:
                    forward_loop(model)
                    batch.flush()  # (requests from outside the decoder stack: the head, a vision tower, ...)
                finally:
                    _calib.DeferredAmax.current = None
                    batch.entries.clear()
                    for h in hooks:
                        h.remove()
                stats["deferred_stats"] = dict(batch.stats)
        lap("forward_loop_s")
        finish_stats_collection(model)
        from . import hf_moe

        hf_moe.layer_sync_moe_local_experts_amax(
            model, sync_weight_amax=sync_expert_weight_amax,
            calibrate_missing=lambda q, w: max_calibrate(q, lambda m: m(w), distributed_sync=False))
        lap("finish_s")
    finally:
        _MAX_CALIBRATE_DEPTH[0] -= 1
    if sync:
        dev = next((p.device for p in model.parameters()), None)
        # the data-parallel group when one was declared (the reference reduces over its DP group, :390-407), else the
        # world; the dealt weight statistics reach the other replicas through this same reduction
        group = mdist.replica_group() if mdist.replicas_declared() else None
        mdist.sync_amax_bucketed(_quantizers(model), group=group, device=dev)
    promote_static_block_weight_quantizers(model)


@torch.no_grad()
def histogram_calibrate(model: nn.Module, forward_loop, method: str = "percentile", distributed_sync: bool = True,
                        **kwargs):
    """The classic histogram flow -- enable_stats_collection, forward, finish_stats_collection(method=...) as users of
    the reference write it by hand (model_calib.py:1128-1167 with calib/histogram.py) -- for models whose quantizers
    were configured with `calibrator: "histogram"`; max calibrators in the same model are loaded as usual.

    Data parallel: every rank feeds its share of the batches; histogram calibrators bin with rank 0's first-batch
    width and their int64 counts are SUM-reduced in one bucket before the threshold search, so every rank computes the
    amax of the WHOLE calibration set -- equal to a single-rank run over all batches when rank 0 holds the first
    batch.  Contract: every rank reaches every histogram-calibrated quantizer (dense models)."""
    sync = distributed_sync and _dist_on()
    enable_stats_collection(model, distributed_sync=sync)
    weight_only_quantize(model, shard=False)
    forward_loop(model)
    hist, rest = nn.ModuleList(), nn.ModuleList()
    for q in _quantizers(model):
        (hist if hasattr(q._calibrator, "share_range_across_ranks") else rest).append(q)
    finish_stats_collection(hist, method, distributed_sync=sync, **kwargs)
    finish_stats_collection(rest)
    if sync:
        dev = next((p.device for p in model.parameters()), None)
        mdist.sync_amax_bucketed(list(rest), device=dev)
    promote_static_block_weight_quantizers(model)


def promote_static_block_weight_quantizers(model: nn.Module) -> int:
    """utils/core_utils.py:1077-1150, INT branch: once their amax is final, enabled static-block INT weight
    quantizers of quantized linears keep `_amax` in fp32 (the reference swaps their class to
    StaticBlockScaleQuantizer).  Later amax writes (MSE refinement, AWQ re-calibration) are then not rounded to
    the weight dtype."""
    n = 0
    nvfp4 = {}
    for name, m in model.named_modules():
        if not is_quantized_linear(m):
            continue
        wq = m.weight_quantizer
        if isinstance(wq, SequentialQuantizer):
            continue
        if wq.is_enabled and wq.is_nvfp4_static and wq.amax is not None:
            nvfp4[name] = wq
            if not getattr(wq, "_is_static_block_scale_quantizer", False):
                wq.promote_static_block()
                n += 1
            continue
        if (wq.is_enabled and wq.is_static_block_quant and wq.amax is not None and isinstance(wq._num_bits, int)
                and not getattr(wq, "_is_static_block_scale_quantizer", False)):
            wq.promote_static_block()
            n += 1
    _set_nvfp4_global_amax(nvfp4)
    return n


# the linears that read one input and are fused at deployment share one NVFP4 global amax (utils/shared_input.py:58-62,
# core_utils.py:1095-1150): siblings under one parent module
NVFP4_SHARED_SIBLINGS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"), ("w1", "w3"))


def _set_nvfp4_global_amax(quantizers: dict) -> None:
    """global_amax = max of the per-block amax (StaticBlockScaleQuantizer.from_tensor_quantizer, :1531-1546), the max over
    the group for fusible siblings."""
    groups: dict = {}
    for name, wq in quantizers.items():
        parent, _, leaf = name.rpartition(".")
        key = next(((parent, i) for i, g in enumerate(NVFP4_SHARED_SIBLINGS) if leaf in g), name)
        groups.setdefault(key, []).append(wq)
    for members in groups.values():
        g = torch.stack([wq._amax.float().max().to(members[0]._amax.device) for wq in members]).max()
        for wq in members:
            wq.global_amax = g


def _nvfp4_sweep_weights(model: nn.Module, hessian_for=None) -> int:
    """The FP8 scale sweep of every static NVFP4 weight quantizer (_make_weight_mse_calibrator with fp8_scale_sweep,
    model_calib.py:670-730): NVFP4MSECalibrator over the weight's blocks, one kernel per weight; every other weight keeps
    its max-calibrated amax.  hessian_for(quantizer) -> normalised per-block Hessian [cin // 16, 16, 16] or None."""
    from .calib import NVFP4MSECalibrator

    n = 0
    for m in model.modules():
        if not is_quantized_linear(m):
            continue
        wq = m.weight_quantizer
        if (not isinstance(wq, TensorQuantizer) or not wq.is_enabled or not wq.is_nvfp4_static
                or getattr(wq, "_amax", None) is None or wq.global_amax is None):
            continue
        w = m.weight
        wq._setup_for_blockquant(w)
        blocks = wq._process_for_blockquant(w.detach())
        h = hessian_for(wq) if hessian_for is not None else None
        cal = NVFP4MSECalibrator(amax=wq._amax.clone().detach(), global_amax=wq.global_amax, axis=wq._axis, hessian=h)
        cal.collect(blocks)
        wq.amax = cal.compute_amax()
        cal.reset()
        n += 1
    return n


# ------------------------------------------------------------------------------------------------ mse
def _mse_quant_func(x, amax, quantizer):
    """model_calib.py:639-662: QDQ `x` with a trial amax through the quantizer itself."""
    had = hasattr(quantizer, "_amax")
    original = quantizer._amax.clone() if had else None
    quantizer._amax = amax
    state = (quantizer._if_quant, quantizer._if_calib)
    quantizer._if_quant, quantizer._if_calib = True, False
    try:
        if hasattr(quantizer, "_original_shape"):
            x = quantizer._reset_to_original_shape(x)
        xq = quantizer(x)
        if hasattr(quantizer, "_block_reshape_size"):
            xq = quantizer._process_for_blockquant(xq)
    finally:
        quantizer._if_quant, quantizer._if_calib = state
        if had:
            quantizer._amax = original
        else:
            delattr(quantizer, "_amax")
    return xq


@torch.no_grad()
def mse_calibrate(model: nn.Module, forward_loop=None, distributed_sync: bool = True, step_size: float = 0.1,
                  start_multiplier: float = 0.25, stop_multiplier: float = 4.0, fp8_scale_sweep: bool = False,
                  shared_states=None):
    """model_calib.py:732-826 (multiplier search, fp8_scale_sweep=False): max calibration first, then every
    eligible weight quantizer's amax is refined by the MSE sweep -- here one fused kernel per weight."""
    refuse_rotation(model, "mse_calibrate")
    if shared_states:
        # shared quantizer state other than the default sibling groups (model_calib.py:770-826) is outside this path
        raise MoquantUnsupported("mse_calibrate: shared_states are outside this path")
    max_calibrate(model, forward_loop, distributed_sync)
    if fp8_scale_sweep:
        # only static NVFP4 weights are searched (the FP8 scale sweep); every other weight stays at max (:695-718)
        _nvfp4_sweep_weights(model)
        return
    _mse_calibrate_weights(model, step_size, start_multiplier, stop_multiplier)


def _mse_calibrate_weights(model: nn.Module, step_size: float, start_multiplier: float, stop_multiplier: float,
                           error_func_for=None):
    """_mse_calibrate_weights (model_calib.py:780-826): the weight search of mse_calibrate / local_hessian_calibrate.
    `error_func_for(weight_quantizer)` -> error function or None (plain squared error: the fused one-kernel sweep)."""
    from functools import partial

    from .calib import MseCalibrator

    # every QuantModule's (weight, quantizer) pairs (quant_module.py:123-129): the linears, and a fused MoE expert container's
    # slice per expert and projection (huggingface.py:1084-1100)
    pairs = []
    for m in model.modules():
        if is_quantized_linear(m):
            pairs.append((m.weight, m.weight_quantizer))
        elif is_quant_fused_experts(m):
            pairs += list(m.iter_weights_for_calibration())
        else:
            pairs += _foreign_weight_pairs(m)
    for weight, wq in pairs:
        if (not isinstance(wq, TensorQuantizer) or not wq.is_enabled or wq._dynamic or wq._block_dynamic
                or wq._calibrator is None or getattr(wq, "_amax", None) is None):
            continue  # _make_weight_mse_calibrator's eligibility test (model_calib.py:681-689)
        nb = wq._num_bits
        fused = (nb, wq._unsigned, wq._narrow_range) if isinstance(nb, int) or tuple(nb) == (4, 3) else None
        error_func = error_func_for(wq) if error_func_for is not None else None
        cal = MseCalibrator(amax=wq._amax.clone().detach(), axis=wq._calibrator._axis, step_size=step_size,
                            start_multiplier=start_multiplier, stop_multiplier=stop_multiplier,
                            quant_func=partial(_mse_quant_func, quantizer=wq), error_func=error_func,
                            fused_format=fused if error_func is None else None)
        wq._calibrator = cal
        wq.disable_quant()
        wq.enable_calib()
        wq(weight)
        wq.load_calib_amax(strict=False)
        wq.enable_quant()
        wq.disable_calib()
        cal.reset()


# ------------------------------------------------------------------------------------------------ local Hessian
class _LocalHessianAccumulator:
    """sum X^T X of one linear's input, kept per block of `block_size` input features (model_calib.py:829-899): the
    metric (W - Wq)^T H (W - Wq) of a block of the weight approximates that block's share of the output error.  One
    accumulator serves every linear that reads the same tensor; Cin that the block does not divide has none (plain MSE)."""

    def __init__(self, cout: int, cin: int, block_size: int):
        self.cout, self.cin, self.block_size = cout, cin, block_size
        self.n_blocks = cin // block_size
        self.is_enabled = cin % block_size == 0
        self.hessian_per_block = None  # fp32 [n_blocks, bs, bs], allocated by the first batch
        self.num_samples = 0
        self._mean = None

    @torch.no_grad()
    def accumulate(self, activation: torch.Tensor):
        if not self.is_enabled:
            return
        tokens = activation.reshape(-1, self.cin).float()          # fp32 like the reference (no 16-bit products)
        blocks = tokens.t().reshape(self.n_blocks, self.block_size, -1)  # [n_blocks, bs, tokens]
        gram = torch.bmm(blocks, blocks.transpose(1, 2))
        if self.hessian_per_block is None:
            self.hessian_per_block = gram
        else:
            self.hessian_per_block += gram
        self.num_samples += tokens.shape[0]

    def normalized_hessian(self):
        """H / samples, cached (the raw sum may be released once the error functions exist)."""
        if self._mean is None and self.hessian_per_block is not None and self.num_samples > 0:
            self._mean = self.hessian_per_block / self.num_samples
        return self._mean

    def build_error_func(self, cout: int, keep_buffer: bool = False):
        """error(x, xq): every element gets its Hessian block's weighted error dw^T H dw, so that a sum over the quantizer's
        reduce axes ranks the candidates by it; None without samples."""
        h = self.normalized_hessian()
        if h is None:
            return None
        if not keep_buffer:
            self.hessian_per_block = None
        bs = self.block_size

        def weighted_error(x: torch.Tensor, xq: torch.Tensor) -> torch.Tensor:
            diff = (x - xq).reshape(cout, -1, bs)
            per_block = torch.einsum("cnb,nbd,cnd->cn", diff, h, diff)
            return per_block.reshape(-1, 1).expand(-1, bs).reshape(x.shape)

        return weighted_error


@torch.no_grad()
def local_hessian_calibrate(model: nn.Module, forward_loop=None, distributed_sync: bool = True, step_size: float = 0.1,
                            start_multiplier: float = 0.25, stop_multiplier: float = 4.0, fp8_scale_sweep: bool = True,
                            block_size: int = 16, debug: bool = False, shared_states=None):
    """model_calib.local_hessian_calibrate (model_calib.py:1005-1127): the amax search of mse_calibrate with the
    Hessian-weighted error (W - Wq)^T H (W - Wq), H = per-block sum X^T X of the linear's input taken in a forward with
    the weight quantizers off.  Phases as in the reference: max calibration; Hessians; weight search.
    `fp8_scale_sweep` (the reference's default True) selects its FP8-scale sweep, which exists for static NVFP4
    quantizers only -- every other quantizer is then left at its max-calibrated amax, as in the reference
    (_make_weight_mse_calibrator, :695-718); pass False for the multiplier search over the quantizers of this path.
    The Hessians are not combined across ranks (the reference warns the same)."""
    refuse_rotation(model, "local_hessian_calibrate")
    if forward_loop is None:
        warnings.warn("forward_loop must be provided for local_hessian; skipping local_hessian")
        return
    if shared_states:
        raise MoquantUnsupported("local_hessian_calibrate: shared_states are outside this path")
    max_calibrate(model, forward_loop, distributed_sync)
    linears = [(n, m) for n, m in model.named_modules() if is_quantized_linear(m) and isinstance(m.weight_quantizer, TensorQuantizer)
               and m.weight_quantizer.is_enabled and m.weight.dim() == 2]
    accumulators: dict = {}
    followers: set = set()
    shared = {"input": None, "acc": None}
    for n, m in linears:
        cin = m.weight.shape[1]
        if cin % block_size:
            warnings.warn(f"local_hessian: {n} input features ({cin}) not divisible by block_size ({block_size}); "
                          "falling back to plain MSE for these weights.")
        qb = (m.weight_quantizer.block_sizes or {}).get(-1)
        if qb is not None and qb != block_size:
            warnings.warn(f"local_hessian: block_size ({block_size}) != quantizer scale block ({qb}) for {n}; Hessian "
                          "weighting will not align with the scale blocks.")

    def hook(mod, args):
        if not args:
            return
        x = args[0]
        x = x.to_local() if hasattr(x, "to_local") else x
        wq = mod.weight_quantizer
        acc = accumulators.get(id(wq))
        if acc is None:
            # q / k / v and gate / up read one tensor: the per-block Hessian depends on the input and the block size only
            if shared["input"] is x and shared["acc"].cin == mod.weight.shape[1]:
                accumulators[id(wq)] = shared["acc"]
                followers.add(id(wq))
                return
            acc = accumulators[id(wq)] = _LocalHessianAccumulator(mod.weight.shape[0], mod.weight.shape[1], block_size)
        elif id(wq) in followers:
            if not (shared["input"] is x and shared["acc"] is acc):
                raise RuntimeError("local_hessian: a linear that shared its input with another one in an earlier batch got "
                                   "a different tensor now")
            return  # (this batch is already in the shared accumulator)
        acc.accumulate(x)
        shared["input"], shared["acc"] = x, acc

    handles = [m.register_forward_pre_hook(hook) for _, m in linears]
    qs = [m.weight_quantizer for _, m in linears]
    saved = [q._disabled for q in qs]
    for q in qs:
        q._disabled = True
    try:
        forward_loop(model)
    finally:
        for q, d in zip(qs, saved):
            q._disabled = d
        for h in handles:
            h.remove()
        shared["input"] = shared["acc"] = None
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        warnings.warn("local_hessian: Hessian is not synced across ranks; refined weight amaxes may diverge under "
                      "tensor/data parallelism. Treat local_hessian as single-rank for now.")
    if fp8_scale_sweep:
        if not any(m.weight_quantizer.is_nvfp4_static for _, m in linears):
            warnings.warn("local_hessian: fp8_scale_sweep=True searches static NVFP4 quantizers only (none in this "
                          "model): every weight keeps its max-calibrated amax; pass fp8_scale_sweep=False for the "
                          "multiplier search.")
            accumulators.clear()
            return
        # the Hessian-weighted FP8 scale sweep of the static NVFP4 weights (a linear without samples or with cin % 16
        # takes the plain sweep); every other weight stays at max
        hess = {qid: (acc.normalized_hessian() if acc.is_enabled else None) for qid, acc in accumulators.items()}
        _nvfp4_sweep_weights(model, hessian_for=lambda q: hess.get(id(q)))
        if debug:
            model._local_hessian_accumulators = accumulators
        else:
            accumulators.clear()
        return
    cout_of = {id(m.weight_quantizer): m.weight.shape[0] for _, m in linears}
    funcs = {qid: acc.build_error_func(cout_of[qid], keep_buffer=debug) for qid, acc in accumulators.items()}
    _mse_calibrate_weights(model, step_size, start_multiplier, stop_multiplier, error_func_for=lambda q: funcs.get(id(q)))
    funcs.clear()
    if debug:
        model._local_hessian_accumulators = accumulators
    else:
        accumulators.clear()


# ---------------------------------------------------------------------------------------- nvfp4_act_headroom
def _is_nvfp4_dynamic_activation_quantizer(q) -> bool:
    """An enabled NVFP4 quantizer with dynamic blocks (E2M1 under E4M3 block scales): its calibrated per-tensor `_amax` is the
    global scale, the quantizer itself is not `_dynamic` (model_calib.py:501-517)."""
    if not isinstance(q, TensorQuantizer) or q._disabled or q._dynamic:
        return False
    bs, nb = q.block_sizes, q.num_bits
    return (bs is not None and bs.get("type", None) == "dynamic" and not isinstance(nb, int) and tuple(nb) == (2, 1)
            and tuple(bs.get("scale_bits", None) or ()) == (4, 3))


def _swap_in_nvfp4_act_headroom_calibrators(model: nn.Module, **options) -> list:
    """(quantizer, its own calibrator) for every NVFP4 dynamic-block `*input_quantizer`, each now holding a fresh
    calib.NVFP4ActHeadroomCalibrator (model_calib.py:529-564).  Refusals come first: a refused model is left as it was."""
    from .calib import NVFP4ActHeadroomCalibrator

    named = [(n, m) for n, m in model.named_modules() if n.endswith("input_quantizer")]
    for n, m in named:
        if isinstance(m, SequentialQuantizer) and any(_is_nvfp4_dynamic_activation_quantizer(q) for q in m.modules()):
            raise NotImplementedError(
                f"nvfp4_act_headroom does not support SequentialQuantizer activation quantizers, but {n!r} is one "
                f"wrapping an NVFP4 dynamic-block quantizer. Use a single activation quantizer config for these modules, "
                f"or calibrate with 'max'.")
    fresh = [(m, NVFP4ActHeadroomCalibrator(m.num_bits, None, m._unsigned, block_size=m.block_sizes.get(-1, 16), **options))
             for _, m in named if _is_nvfp4_dynamic_activation_quantizer(m)]  # (a bad option raises before any swap)
    swapped = []
    for q, cal in fresh:
        swapped.append((q, q._calibrator))
        q._calibrator = cal
    return swapped


@torch.no_grad()
def nvfp4_act_headroom_calibrate(model: nn.Module, forward_loop=None, *, anchor_percentile: float = 1.0,
                                 upper_percentile: float = 99.99, rho: float = 16384.0, weight_scale_algorithm=None):
    """model_calib.nvfp4_act_headroom_calibrate (model_calib.py:567-636): the global scale of every NVFP4 dynamic-block
    input quantizer from the distribution of its per-block amaxes, amax = max(rho * anchor, upper)
    (calib.NVFP4ActHeadroomCalibrator), which leaves headroom above the calibration data where plain max leaves none.

    The weights are a separate matter: `weight_scale_algorithm` is {"method": "max"} (the default, also for None), "mse"
    or "local_hessian" with that algorithm's own options.  Each of them begins with max calibration, whose ONE forward
    loop fills the swapped-in calibrators through the quantizers' plain `collect` (they are block quantizers with a
    calibrator of their own class: neither the per-tensor fast path nor calib.DeferredAmax takes them); what follows
    touches weights only.  The quantizers get their own calibrators back whatever happens.

    Data parallel: every rank's amax comes from its own batches and the amaxes are MAX-reduced with all the others
    (max_calibrate); the histograms are not pooled (the reference's note, :605-608)."""
    refuse_rotation(model, "nvfp4_act_headroom_calibrate")
    algo = weight_scale_algorithm or {"method": "max"}
    algo = {"method": algo} if isinstance(algo, str) else dict(algo)
    method = algo.pop("method", None)
    funcs = {"max": max_calibrate, "mse": mse_calibrate, "local_hessian": local_hessian_calibrate}
    if method not in funcs:
        raise ValueError(f"nvfp4_act_headroom: weight_scale_algorithm method {method!r} is not one of 'max', 'mse', "
                         f"'local_hessian'")
    swapped = _swap_in_nvfp4_act_headroom_calibrators(model, anchor_percentile=anchor_percentile,
                                                      upper_percentile=upper_percentile, rho=rho)
    if not swapped:
        warnings.warn("nvfp4_act_headroom: no NVFP4 dynamic-block input quantizer matched, so this is equivalent to plain "
                      "max calibration. Check that the recipe enables NVFP4 activation quantizers.")
    try:
        funcs[method](model, forward_loop, **algo)
    finally:
        for q, own in swapped:
            q._calibrator = own


# ------------------------------------------------------------------------------------------------ smoothquant
@torch.no_grad()
def apply_pre_quant_scale_and_smooth(linear: QuantLinear, pre_quant_scale: torch.Tensor, fold_later: list | None = None):
    """model_calib.py:1226-1270: input quantizer gets s (in W.dtype), W <- (W * (1/s)_fp32).to(dtype),
    weight amax recalibrated, input amax <- max(amax_for_smoothing * s).

    fold_later: a list that takes (linear, 1/s) INSTEAD of the weight being folded and re-calibrated here -- the caller folds
    all of them in one launch that also bakes the weight quantizer in (smoothquant(fold_weights=True))."""
    assert linear.input_quantizer.pre_quant_scale is None, "pre_quant_scale should be None first!"
    assert torch.all(pre_quant_scale > 0), "pre_quant_scale should be positive"
    pre_quant_scale = pre_quant_scale.to(torch.float32)
    linear.input_quantizer._enable_pre_quant_scale = True
    linear.input_quantizer.pre_quant_scale = pre_quant_scale.to(linear.weight.dtype)
    inv_scale = 1.0 / pre_quant_scale
    if fold_later is not None:
        fold_later.append((linear, inv_scale))
    else:
        ops.scale_cols(linear.weight.data, inv_scale, out=linear.weight.data)  # fp32 multiply, one rounding
        linear.weight_quantizer.reset_amax()
        max_calibrate(linear, lambda lin: lin.weight_quantizer(lin.weight), distributed_sync=False)
    if linear.input_quantizer.amax is not None:
        dev, dt = linear.weight.device, linear.weight.dtype
        a = linear.input_quantizer._amax_for_smoothing.to(device=dev, dtype=dt)
        linear.input_quantizer.amax = (a * pre_quant_scale.to(dev)).amax().to(dt)


_MX_ELEMENT_FORMATS = {(2, 1): "E2M1", (4, 3): "E4M3", (5, 2): "E5M2", (3, 2): "E3M2", (2, 3): "E2M3", 8: "INT8"}


def _fold_rides_in_mx(m) -> tuple | None:
    """(block, element format) when this linear's fold W <- dt(W / s) can ride inside its MX weight quantizer's fake
    quantization (ops: moq_mt_fold_mx_fused): a dynamic-block E8M0 quantizer along the last axis of a dense 2-D GPU weight --
    nothing to re-calibrate after the fold (block scales come from every input), so fold + QDQ is one read and one write."""
    wq, w = m.weight_quantizer, m.weight
    if not isinstance(wq, TensorQuantizer) or not wq.is_enabled or not wq.is_mx_format or wq.pre_quant_scale is not None:
        return None
    nb = tuple(wq._num_bits) if isinstance(wq._num_bits, (list, tuple)) else wq._num_bits
    fmt = _MX_ELEMENT_FORMATS.get(nb)
    if fmt is None or not set(wq._block_sizes) <= {-1, w.dim() - 1, "type", "scale_bits"}:
        return None
    g = wq._block_sizes.get(-1, None) or wq._block_sizes.get(w.dim() - 1, None)
    vec = 4 if w.dtype == torch.float32 else 8
    if (not g or w.dim() != 2 or not ops._is_gpu(w) or not w.is_contiguous() or w.data_ptr() % 16 or w.shape[-1] % g
            or w.dtype not in (torch.float32, torch.float16, torch.bfloat16) or g % vec or (g // vec) not in (1, 2, 4, 8)):
        return None
    return int(g), fmt


def _broadcast_smoothed(linears, group):
    """Data-parallel SmoothQuant with the fold dealt over the ranks: linear i was smoothed on rank i % world only; the
    folded weight, the pre-quant scale and the re-calibrated amaxes reach the other ranks from there (whole weights
    in place, the small vectors in one bucket per owner)."""
    world, me = dist.get_world_size(group), dist.get_rank(group)
    payload, owners = [], []
    for i, m in enumerate(linears):
        r = i % world
        iq, wq = m.input_quantizer, m.weight_quantizer
        if r != me:  # buffers of the right shape to receive into
            iq._enable_pre_quant_scale = True
            iq.pre_quant_scale = torch.empty(m.weight.shape[1], dtype=m.weight.dtype, device=m.weight.device)
        for t in (m.weight.data, iq._pre_quant_scale, getattr(wq, "_amax", None), getattr(iq, "_amax", None)):
            if t is not None:
                payload.append(t)
                owners.append(r)
    mdist.broadcast_from_owners(payload, group=group, owners=owners)


@torch.no_grad()
def smoothquant(model: nn.Module, forward_loop, alpha: float = 1.0, formats: str = "int8",
                shard_weights: bool | None = None, fold_weights: bool = False):
    """model_calib.py:1273-1359.

    shard_weights (data-parallel replicas; None follows distributed.declare_data_parallel): the weight side of the
    smoothing -- |W| column abs-max, the fold W <- W / s, the re-calibration of the folded weight: three passes over
    every weight -- is dealt over the ranks and the results are broadcast from their owners.  The per-channel
    activation amax is MAX-reduced before (max_calibrate), so every rank would compute the same scales.

    formats = "int8" (default): the reference's behaviour -- only linears whose input AND weight quantizers are INT8
              are smoothed, every other one is skipped with a warning (:1344-1346).
    formats = "all": the per-channel scale math (:1309-1335) and the fold (:1226-1270) do not depend on the number
              format, so any linear with an enabled input quantizer is smoothed -- BASELINE configs[4]: SmoothQuant
              scaling composed with MXFP4 (g = 32, E8M0 block scales).  Per-tensor formats get the reference's
              post-smoothing input amax max(act_amax * s); dynamic-block (MX) quantizers, which recompute their block
              scales from every input, keep no amax at all.  The scales and folded weights are bit-identical to the
              reference's INT8 run on the same model (tests/test_host_flows_cpu.py: sq_mxfp4 fixture).

    fold_weights = True: the call ends like `smoothquant(...); model_quant.fold_weight(model)` -- every weight quantizer baked
              into its weight and switched off (mtq.fold_weight, model_quant.py:728-736) -- and the result is that sequence's
              bit for bit; but a linear whose weight quantizer is a dynamic MX block format (configs[4]: MXFP4 g32) is neither
              folded nor re-calibrated on the way: its smoothing fold rides INSIDE the MX quantize-dequantize, all such
              linears in ONE launch at one read + one write per element (multi_tensor.fold_mx_fused) instead of the fold's read
              + write, the re-calibration's read and the QDQ's read + write."""
    refuse_rotation(model, "smoothquant")
    assert forward_loop is not None, "forward_loop must be provided for smoothquant"
    if formats not in ("int8", "all"):
        raise ValueError(f"smoothquant: formats must be 'int8' or 'all', got {formats!r}")
    for m in model.modules():
        if is_quantized_linear(m) and m.input_quantizer.is_enabled and m.input_quantizer.axis is None:
            m.input_quantizer.axis = -1
    max_calibrate(model, forward_loop, shard_weights=shard_weights)
    shard = mdist.resolve_shard(shard_weights)
    world, me = (dist.get_world_size(mdist.replica_group()), dist.get_rank(mdist.replica_group())) if shard else (1, 0)
    smoothed = 0
    dealt = []
    fold_later = []  # (linear, 1 / s) whose fold rides inside the MX QDQ (fold_weights=True)
    for name, m in model.named_modules():
        if not is_quantized_linear(m):
            continue
        iq, wq = m.input_quantizer, m.weight_quantizer
        if not hasattr(iq, "_amax"):
            warnings.warn(f"{name} is not calibrated, skip smoothing")
            continue
        if formats == "int8" and (iq.num_bits != 8 or wq.num_bits != 8):
            warnings.warn(f"Only int8 smoothing is supported, skip {name}")
            continue
        if iq.axis != -1:
            warnings.warn(f"Only per-channel smoothing is supported, skip {name}")
            continue
        act_amax = iq._amax.float().reshape(-1)  # the buffer: `amax` reads None on MX inputs (formats="all")
        dealt.append(m)
        if shard and (len(dealt) - 1) % world != me:
            # another rank smooths this linear; the state every rank sets without touching the weight
            iq.reset_amax()
            iq.axis = None
            if not iq._block_dynamic:
                iq._amax_for_smoothing = act_amax.cpu()
                iq.amax = act_amax.amax().to(dtype=m.weight.dtype, device=m.weight.device)
            smoothed += 1
            continue
        # |W|.amax(dim=0) stays in the WEIGHT dtype and so does its power (model_calib.py:1311, :1319): for a 16-bit
        # model weight_scale^(1 - alpha) is rounded to 16 bits before the fp32 division
        weight_scale = ops.reduce_amax(m.weight, axis=(0,)).reshape(-1)
        scale_a = weight_scale.pow(1 - alpha) / act_amax.pow(alpha)
        iq.reset_amax()
        iq.axis = None
        if not iq._block_dynamic:
            iq._amax_for_smoothing = act_amax.cpu()
            iq.amax = act_amax.amax().to(dtype=m.weight.dtype, device=m.weight.device)
        epsilon = 1.0 / (1 << 31)
        if scale_a.min() <= epsilon:
            scale_a[act_amax <= epsilon] = 1
        scale_a = scale_a.clamp(min=1e-4, max=1e4)
        rides = fold_weights and not shard and _fold_rides_in_mx(m) is not None
        apply_pre_quant_scale_and_smooth(m, scale_a, fold_later=fold_later if rides else None)
        smoothed += 1
    if shard and dealt:
        _broadcast_smoothed(dealt, mdist.replica_group())
    if fold_weights:
        groups = {}
        for m, inv_scale in fold_later:
            groups.setdefault((_fold_rides_in_mx(m), m.weight.dtype, m.weight.device), []).append((m, inv_scale))
        for ((block, fmt), _, _), pairs in groups.items():
            ws = [m.weight.data for m, _ in pairs]
            SegmentTable(ws, outputs=ws).fold_mx_fused([s for _, s in pairs], block, fmt)
        for m, _ in fold_later:
            m.weight_quantizer.disable()  # baked in; fold_weight below leaves it alone and drops what it holds
        from .model_quant import fold_weight

        fold_weight(model, shard_weights=shard_weights)
    return smoothed


# ------------------------------------------------------------------------------------------------ AWQ (the lite search: awq_search.py)
def get_scale(x_max, w_max, alpha):
    """model_calib.py:1474-1487 (no tensor parallel group here).

    The [Cin] vector math (pow, divide, clamp, normalise) runs where numerics.mode() puts it.  "host" (default): IEEE fp32
    on the host whatever device the statistics live on -- the GPU math library's pow and torch's reciprocal-multiply for
    `tensor / scalar` differ from the host's in the last bit, which would make the folded weights, and with them every byte
    of the exported checkpoint, depend on the device the search ran on; the result equals the reference's CPU run.
    "device": the same expression on the statistics' device -- the reference's run on THAT device bit for bit, no round
    trip.  The result goes back to x_max's device."""
    dev = x_max.device
    x, w = numerics.vec(x_max), numerics.vec(w_max)
    w = w.to(x.device)
    scales = (x.pow(alpha) / (w.pow(1 - alpha) + torch.finfo(torch.float32).tiny)).clamp(min=1e-4, max=1e4).view(-1)
    return (scales / (scales.max() * scales.min()).sqrt()).view(-1).to(dev)


# wall-clock of the last max_calibrate call by phase (the device is drained at the phase boundaries)
MAX_CALIBRATE_STATS: dict = {}
_NO_INSTANCE_FORWARD = object()


def _restore_forward(m, previous):
    """Undo `m.forward = patched`: put back the INSTANCE attribute the module had before (an accelerate hook, a user's patch) or
    remove the instance attribute, so that the class's own forward is looked up again -- assigning the bound method read before the
    patch would pin the module to the class it had during the search (under the algorithm seam that class is handed back to the
    reference afterwards; the reference's `unpatch_forward_method` does the same: utils/network.py)."""
    if previous is _NO_INSTANCE_FORWARD:
        m.__dict__.pop("forward", None)
    else:
        m.forward = previous


# ------------------------------------------------------------------------------------------------ AWQ clip
class AWQClipHelper:
    """Per-linear state of awq_clip (model_calib.py:1746-1785): the max-calibrated block amax, one block-loss
    table for all clip ratios (device fp32 [K, nblk, Cout], the layout the kernel writes) and the result."""

    def __init__(self, module: QuantLinear, min_clip_ratio: float, shrink_step: float):
        wq = module.weight_quantizer
        self.num_tokens = 0
        self.block_size = wq.block_sizes.get(-1, None) or wq.block_sizes.get(module.weight.dim() - 1)
        wq.reset_amax()  # cache the original amax (:1751-1756)
        enable_stats_collection(wq)
        wq(module.weight)
        finish_stats_collection(wq)
        self.w_amax = wq.amax.clone()
        co, ci = module.weight.shape
        # same float keys as :1759-1761
        self.clip_ratios = [round(float(k), 2) for k in torch.arange(min_clip_ratio, 1.0, shrink_step)] + [1.0]
        self.nblk = math.ceil(ci / self.block_size)
        self.shrinks = torch.tensor(self.clip_ratios, dtype=torch.float32, device=module.weight.device)
        self.loss_buf = torch.zeros(len(self.clip_ratios), self.nblk, co, dtype=torch.float32,
                                    device=module.weight.device)
        self.best_clip_val = None
        self.best_loss = None
        self.is_input_quantized = module.input_quantizer.is_enabled
        wq.disable()

    @property
    def loss(self):
        """{clip ratio: fp32 [Cout, nblk]} -- the reference's per-shrink dict view of the loss table."""
        return {k: self.loss_buf[i].t() for i, k in enumerate(self.clip_ratios)}

    def update_best_params(self):
        """model_calib.py:1788-1798: first strictly smaller loss wins; clip value = w_amax * shrink in
        w_amax's dtype."""
        self.best_loss = torch.ones_like(self.w_amax) * float("inf")
        self.best_clip_val = torch.zeros_like(self.w_amax)
        for shrink, loss in self.loss.items():
            loss = loss.reshape(self.w_amax.shape)
            indices = loss < self.best_loss
            self.best_loss = torch.where(indices, loss.to(self.best_loss.dtype), self.best_loss)
            self.best_clip_val = torch.where(indices, self.w_amax * shrink, self.best_clip_val)


@torch.no_grad()
def awq_clip(model: nn.Module, forward_loop, max_co_batch_size: int = 1024, max_tokens_per_batch: int = 64,
             min_clip_ratio: float = 0.5, shrink_step: float = 0.05, debug: bool = False, **kwargs):
    """AWQ-clip (model_calib.py:1724-1940) for static-block INT weight quantizers: per weight block, the clip
    ratio of the block amax that minimises the block's output error on (sub-sampled) calibration tokens.
    `max_co_batch_size` bounds the reference's broadcast temporaries and has no effect here: the search is one
    kernel pass over the weight per forward call (ops.awq_clip_loss)."""
    refuse_rotation(model, "awq_clip")
    assert forward_loop is not None, "forward_loop must be provided for awq_clip"
    mods = [(n, m) for n, m in model.named_modules()
            if is_quantized_linear(m) and m.weight_quantizer.is_enabled and m.weight_quantizer.block_sizes is not None]
    for name, m in mods:
        wq = m.weight_quantizer
        if not wq.is_static_block_quant or not isinstance(wq._num_bits, int) or wq._unsigned or wq._narrow_range:
            raise ValueError(f"awq_clip: {name}: only signed static-block INT weight quantizers are on this path "
                             "(the per-tensor NVFP4 branch, model_calib.py:1804-1813, is outside it)")
    helpers = {m: AWQClipHelper(m, min_clip_ratio, shrink_step) for _, m in mods}

    def patched_forward(self, input):
        h = helpers[self]
        iq = self.input_quantizer
        if h.is_input_quantized:  # :1873-1876: calibrate the input quantizer on this batch, then bypass it
            iq.enable()
            max_calibrate(iq, lambda q: q(input), distributed_sync=False)
            iq.disable()
        x = iq(input)  # applies pre_quant_scale (awq_full: the AWQ-lite scale) even though disabled
        x2 = x.reshape(-1, x.shape[-1])
        if x2.shape[0] > 0:
            step = max(1, x2.shape[0] // max_tokens_per_batch)  # inputs[0::step] (:1820)
            h.num_tokens += -(-x2.shape[0] // step)
            ops.awq_clip_loss(x2, self.weight, h.w_amax, h.shrinks, h.block_size, self.weight_quantizer.num_bits,
                              h.loss_buf, token_step=step)
        return F.linear(x, self.weight, self.bias)  # _forward_no_awq with the weight quantizer disabled (:1893)

    originals = {}
    for _, m in mods:
        originals[m] = m.__dict__.get("forward", _NO_INSTANCE_FORWARD)
        m.forward = patched_forward.__get__(m, type(m))
    try:
        enable_stats_collection(model)  # input / KV quantizers collect during the same pass (:1910-1913)
        forward_loop(model)
        finish_stats_collection(model)
        if dist.is_available() and dist.is_initialized():
            # DP: the reference all-reduces every block-loss tensor inside the search loop (:1861-1863); linear
            # in the loss, so ONE bucketed SUM + divide at the end is the same value
            mdist.all_reduce_bucket([h.loss_buf for h in helpers.values()], dist.ReduceOp.SUM, average=True)
            mdist.sync_amax_bucketed([q for q in _quantizers(model) if q.is_enabled])
    finally:
        for m, f in originals.items():
            _restore_forward(m, f)
    for _, m in mods:
        h = helpers[m]
        if h.num_tokens > 0:  # postprocess (:1921-1929)
            h.update_best_params()
            m.weight_quantizer.amax = h.best_clip_val
            m.weight_quantizer.enable()
            if h.is_input_quantized:
                m.input_quantizer.enable()
        if debug:
            m.awq_clip = h
    return helpers


@torch.no_grad()
def awq(model: nn.Module, forward_loop=None, algorithm: str = "awq_lite", **kwargs):
    """model_calib.py:1362-1391: awq_lite, awq_clip or both (awq_full)."""
    refuse_rotation(model, "awq")
    out = {}
    with SequentialQuantizer.convert_to_single_quantizer(model):  # search on the first (INT4) stage only (:1378)
        if algorithm in ("awq_full", "awq_lite"):
            lite_kw = {k: v for k, v in kwargs.items() if k in ("alpha_step", "search", "tie_margin", "tie_check", "layer_local", "store_activations")}
            out["awq_lite"] = awq_lite(model, forward_loop, **lite_kw)
        if algorithm in ("awq_full", "awq_clip"):
            clip_kw = {k: v for k, v in kwargs.items()
                       if k in ("max_co_batch_size", "max_tokens_per_batch", "min_clip_ratio", "shrink_step", "debug")}
            out["awq_clip"] = awq_clip(model, forward_loop, **clip_kw)
    for m in model.modules():  # every stage of a sequential weight quantizer is re-calibrated on the final weight (:1385-1391)
        if is_quantized_linear(m) and isinstance(m.weight_quantizer, SequentialQuantizer):
            max_calibrate(m, lambda linear: linear.weight_quantizer(linear.weight), distributed_sync=False)
    return out


def gptq(model: nn.Module, forward_loop, perc_damp: float = 0.01, block_size: int = 128, fused: bool = False, **kwargs):
    """model_calib.gptq (model_calib.py:2192-2271): the implementation lives in gptq.py."""
    from . import gptq as _gptq

    return _gptq.gptq(model, forward_loop, perc_damp=perc_damp, block_size=block_size, fused=fused, **kwargs)


# AWQ-lite lives in awq_search.py; these are its names that code outside reads from here -- the same objects, not copies.
# The import stands LAST on purpose: awq_search imports this module at its top and reads get_scale, max_calibrate and the
# rest as attributes at call time, so everything above must exist before it loads (the package imports model_calib first).
from .awq_search import (AWQ_LITE_STATS, GRAM_PLANES_SLACK, GRAM_SCORE_PLANES, GRAM_TIE_MARGIN, GRAM_TIE_NOISE,  # noqa: E402, F401
                         TIE_CHECK_MAX_ROUNDS, TIE_HEADROOM, TIE_SPREAD_FACTOR, AWQLiteHelper, _WeightCacheBudget, awq_lite,
                         gram_score_planes, host_math_threads, tie_margin_check)
