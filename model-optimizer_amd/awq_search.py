"""AWQ-lite (the reference's quantization/model_calib.py:1394-1721): the per-linear helper, the Gram and error-GEMM
scoring engines, the tie check of the re-scoring margin, the layer-local walk and the flow itself (`_AWQLiteRun`,
`awq_lite`).  model_calib re-exports the public names; what this module takes from model_calib (get_scale, max_calibrate,
the stats collection, _restore_forward) it reads through the module at call time, so a rebinding there reaches the search.
"""

from __future__ import annotations

import contextlib
import math
import time
import warnings

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import nn

from . import distributed as mdist
from . import model_calib
from . import numerics
from . import ops
from .nn import QuantLinear, is_quantized_linear
from .tensor_quantizer import TensorQuantizer


def _dist_initialized() -> bool:
    """A process group exists -- a world of one included, unlike model_calib._dist_on(): the flow's collectives have always
    run whenever there is a group, and the ranks' sequences must stay what they were."""
    return dist.is_available() and dist.is_initialized()


@contextlib.contextmanager
def host_math_threads(n: int = 1):
    """The [Cin]-sized host math of the AWQ search (get_scale and friends: ~30 small CPU tensor ops per candidate) on
    ONE thread.  torch parallelises some of these ops (sqrt, reductions) over its OpenMP pool even for a few thousand
    elements; on hosts where the visible CPUs exceed what the process may use (the GPU boxes show 256 CPUs under a
    16-CPU quota) every such fork/join stalls for milliseconds -- measured 1.35 s vs 0.25 s for the 2464 scale vectors
    of Llama-3-8B in the build container, 1.3-1.6 s of the flow on the GPU box.  Elementwise results do not depend on
    the thread count."""
    before = torch.get_num_threads()
    try:
        torch.set_num_threads(n)
        yield
    finally:
        torch.set_num_threads(before)


class _WeightCacheBudget:
    """HBM budget for keeping the 11 search weights QDQ(W * s_alpha) of every linear resident between
    calibration batches (the reference re-quantizes them on every forward, model_calib.py:1552-1554).  288 GB of
    HBM3E hold all of Llama-3-8B's candidates (11 x 14 GB); larger models cache what fits and recompute the rest."""

    host_bytes = 0  # budget on a non-GPU device (the CPU test tier's stand-in backend sets it)

    def __init__(self, device):
        self.left = int(self.host_bytes)
        if device.type == "cuda":
            # what the flow can still get: the driver's free memory PLUS what torch's caching allocator holds without using
            # (a process that has run anything large before sits on such blocks -- and a harness may park the flow's memory
            # there on purpose, tools/awq_bench.py: counting the driver's share alone sent that run into a second pass)
            free, _ = torch.cuda.mem_get_info(device)
            cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
            self.left = int((free + max(cached, 0)) * 0.6)

    def reserve(self, nbytes: int) -> bool:
        if nbytes <= self.left:
            self.left -= nbytes
            return True
        return False

    def release(self, nbytes: int):
        self.left += nbytes


def _awq_searched(m) -> bool:
    """awq_lite's own rule (model_calib.py:1563-1567): EVERY quantized linear whose weight quantizer is enabled -- whatever
    its format: a per-layer override that puts FP8 or INT8 on part of an INT4-AWQ model is smoothed and searched too."""
    return is_quantized_linear(m) and m.weight_quantizer.is_enabled


def _awq_fused_format(wq, weight) -> bool:
    """INT-k static blocks along the last axis only: the format the fused search kernels (scale + per-group QDQ, weight scale,
    Gram scores) are written for.  Everything else takes the GENERIC route: the same search with the scaled weight passed
    through the quantizer itself (dynamic amax of its own layout) and the error-GEMM engine."""
    if not (isinstance(wq, TensorQuantizer) and wq.is_static_block_quant and isinstance(wq._num_bits, int)):
        return False
    axes = {(k % weight.dim()) for k in wq._block_sizes if isinstance(k, int)}
    return axes == {weight.dim() - 1}


def _awq_block_size(wq, weight):
    """_get_awq_quantizer_block_size (model_calib.py:1943-1952): None without block sizes (whole rows)."""
    if wq.block_sizes is None:
        return None
    if -1 in wq.block_sizes:
        return wq.block_sizes[-1]
    if 1 in wq.block_sizes:
        return wq.block_sizes[1]
    raise ValueError("AWQ requires block quantization along -1 axis")


def _awq_weight_scale_generic(weight: torch.Tensor, block) -> torch.Tensor:
    """get_weight_scale (model_calib.py:1453-1469) for the layouts moq_awq_weight_scale does not take (whole rows, blocks that
    are no power-of-two number of packets): every |w| over the abs-max of its block (+ tiny) in the weight dtype, the mean over
    the output rows (torch: fp32 accumulation, one rounding to the dtype), widened to fp32."""
    rows, cin = weight.shape
    w = weight.detach()
    if block and cin % block:
        w = F.pad(w, (0, block - cin % block), "constant", 0)
    groups = w.contiguous().view(-1, block) if block else w.contiguous()
    top = ops.reduce_amax(groups, axis=1, keepdims=True).to(w.dtype)
    share = (groups.abs() / (top + torch.finfo(w.dtype).tiny)).view(rows, -1)[:, :cin]
    return share.mean(0).to(torch.float32)


class AWQLiteHelper:
    """Per-linear state of awq_lite (model_calib.py:1416-1451)."""

    def __init__(self, module: QuantLinear, alpha_step: float):
        wq = module.weight_quantizer
        self.fused = _awq_fused_format(wq, module.weight)
        if not self.fused:
            self._init_generic(module, alpha_step)
            return
        self.block_size = wq.block_sizes.get(-1, None) or wq.block_sizes.get(module.weight.dim() - 1)
        # Cin that is not a block multiple: the reference zero-pads the last block (get_weight_scale, :1453-1469; the
        # static block quantizer, tensor_quantizer.py:975-1043).  The kernels take whole blocks, so such a linear works on
        # a zero-padded copy of its weight and cuts the padding off again: zeros change neither a block's abs-max nor
        # any quantized value.
        self.cin = module.weight.shape[1]
        self.dtype = module.weight.dtype  # 1 / s is rounded to it where the forward uses it (prepare_scales)
        self.pad = (-self.cin) % self.block_size
        if numerics.on_host():
            self.weight_scale = ops.awq_weight_scale(self._padded(module.weight), self.block_size)[:self.cin].contiguous()
        else:
            # numerics "device" = the reference's run on this device: like the activation mean (patched_forward), this statistic
            # is a 16-bit-rounded MEAN -- over Cout of |w| / (group amax + tiny) -- whose last bit depends on the summation
            # order at full width; torch's own expression (get_weight_scale, :1453-1469), a handful of passes over the weight,
            # once per linear
            self.weight_scale = _awq_weight_scale_generic(module.weight, self.block_size).contiguous()
        self._init_state(module, alpha_step)

    def _init_generic(self, module, alpha_step):
        self.block_size = _awq_block_size(module.weight_quantizer, module.weight)
        self.cin = module.weight.shape[1]
        self.dtype = module.weight.dtype
        self.pad = 0
        self.weight_scale = _awq_weight_scale_generic(module.weight, self.block_size)
        self._init_state(module, alpha_step)

    def _init_state(self, module, alpha_step):
        self.act_sum = torch.zeros(module.weight.shape[1], dtype=torch.float32, device=module.weight.device)
        self.act_scale = None
        self.num_cache_steps = 0
        self.num_search_steps = 0
        self.num_tokens = 0
        self.alphas = [k.item() for k in torch.arange(0, 1.0 + alpha_step, alpha_step)]  # same float32 keys as :1431
        # one device buffer for all per-alpha losses; loss[alpha] is a 1-element view the kernels accumulate into
        self.loss_buf = torch.zeros(len(self.alphas), dtype=torch.float32, device=module.weight.device)
        self.loss = {a: self.loss_buf[i:i + 1] for i, a in enumerate(self.alphas)}
        self.best_alpha = None
        self.best_scale = None
        self.is_enabled = True  # False: NaN in a scale on some rank, or no tokens anywhere (:1605-1629)
        self.is_input_quantized = False  # set by awq_lite's setup (:1432)
        self.setup_disabled = False  # an input quantizer with a channel axis other than the last one (:1441-1443)
        # search-pass caches (alpha -> tensors); scales depend on alpha only once act_scale is final
        self._inv_scale = None
        self._scale_dt = None
        self._w_hat = None
        self._cache_w = False
        self._s_host = self._s_dev = self._r_dev = None  # prepare_scales
        # Gram-matrix search: G = sum_b X_b^T X_b / T_b (fp32 [Cin, Cin]), accumulated in the cache pass
        self.gram = None
        self.use_gram = False
        self.gram_owner = None  # the helper whose Gram matrix this one aliases (same input tensor)
        self.gram_stage = None  # ops.GramStage: several calibration batches per Gram launch
        self.gram_stage_denied = False
        self.num_gram_steps = 0  # batches that reached the Gram accumulation (own or aliased)
        self.gram_symmetrized = False
        self.gram_bytes = 0  # what this helper holds of the HBM budget for its Gram matrix
        # tie-aware re-evaluation (search="auto"): candidates whose Gram loss lies within the margin of the best one
        # are re-scored by the exact-rounding error-GEMM engine; `gram_loss` keeps the Gram scores for inspection
        self.scored_here = False  # this rank evaluated the Gram scores (data parallel: one rank per Gram matrix)
        self.loss_synced = False  # loss_buf is already summed over the ranks (pick_contenders)
        self.tokens_all_ranks = None  # num_tokens summed over the ranks (None: never summed, num_tokens stands)
        self.search_steps_all_ranks = 0  # num_search_steps summed over the ranks: 0 = no rank searched this linear
        self.exact_steps_all_ranks = 0  # num_exact_steps of the last exact pass, summed over the ranks
        self.gram_loss = None
        self.contenders = None  # indices into `alphas`, ascending, of every re-scored candidate; None: the Gram scores decide
        self.exact_buf = None  # fp32 [len(contenders)]: their exact scores
        self.num_exact_steps = 0
        self.pending = None  # candidates the NEXT exact pass scores (indices, ascending); exact_pass_buf accumulates them
        self.exact_pass_buf = None
        self.exact_scores = {}  # candidate index -> exact score (host floats, summed over the ranks)
        self.margin_used = None  # relative Gram margin the contender set was cut at (widened by the tie check)
        self.tie_need = None  # TIE_SPREAD_FACTOR * S + gap_w of the last check, relative (None: not re-scored)
        self.tie_rounds = 0  # how often the margin of this linear was widened
        self.stored = []  # store_activations: (input [T, Cin], out_actual [T, Cout]) of every cache-pass batch
        self.act_owner = None  # the helper whose act_sum this one aliases (same input tensor in the cache pass)

    def _padded(self, w: torch.Tensor, value: float = 0.0) -> torch.Tensor:
        return F.pad(w, (0, self.pad), "constant", value) if self.pad else w

    def prepare_scales(self, act_host: torch.Tensor, weight_host: torch.Tensor, dtype: torch.dtype):
        """All candidate scale vectors of this linear at once, on the HOST (get_scale), uploaded in ONE copy: s_alpha
        (fp32) and the input-side 1 / s_alpha as the forward uses it (rounded to the model dtype).  Done for every linear
        before the first scoring kernel is queued: a device -> host round trip per candidate inside the scoring loop
        would drain the stream 2464 times for Llama-3-8B (measured: +6 s on 18 s)."""
        self.upload_scales(self.host_scales(act_host, weight_host, dtype))

    def host_scales(self, act_host: torch.Tensor, weight_host: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The host half of prepare_scales: [2 A, Cin] fp32 = all s_alpha, then all (1 / s_alpha) rounded to `dtype`.
        Pure CPU tensor math on this linear's own vectors."""
        s = torch.stack([model_calib.get_scale(act_host, weight_host, a) for a in self.alphas])  # [A, Cin] fp32
        return torch.cat([s, (1.0 / s).to(dtype).float()])

    def upload_scales(self, both: torch.Tensor):
        n = len(self.alphas)
        self._s_host = both[:n]
        up = both.to(self.act_scale.device)
        self._s_dev, self._r_dev = up[:n], up[n:]

    def scale(self, alpha):
        """get_scale(act_scale, weight_scale, alpha) on the statistics' device (computed on the host, see prepare_scales)."""
        if self._s_dev is None:
            self.prepare_scales(numerics.vec(self.act_scale), numerics.vec(self.weight_scale), self.dtype)
        return self._s_dev[self.alphas.index(alpha)]

    def search_operands(self, module, subset=None):
        """(inv_s [A, Cin] fp32 = (1/s_alpha) rounded to the weight dtype, w_hat [A, Cout, Cin] = QDQ(W * s_alpha))
        for all candidates (or the `subset` of candidate indices -- fixed for the life of the caches).  Scales depend
        on alpha only (act_scale is final in the search pass) and are computed once; w_hat stays resident when the
        budget allows, otherwise it is rebuilt per batch."""
        dt = module.weight.dtype
        if self._inv_scale is None:
            alphas = self.alphas if subset is None else [self.alphas[i] for i in subset]
            scales = [self.scale(a) for a in alphas]
            idx = torch.tensor([self.alphas.index(a) for a in alphas], device=self._r_dev.device)
            self._inv_scale = self._r_dev.index_select(0, idx).contiguous()
            self._scale_dt = [s.to(dt) for s in scales]
        w_hat = self._w_hat
        if w_hat is None:
            w_hat = torch.empty(len(self._scale_dt), *module.weight.shape, dtype=dt, device=module.weight.device)
            if not self.fused:
                # the scaled weight through the quantizer itself, which holds no amax during the search and takes that of
                # its input in its own layout (per tensor, per channel, 2-D blocks, ...): the weight quantizer with
                # pre_quant_scale = s of the patched forward (:1548-1554)
                for i, s in enumerate(self._scale_dt):
                    w_hat[i].copy_(module.weight_quantizer(ops.scale_cols(module.weight.detach(), s.float())))
            elif self.pad:  # whole blocks for the kernel (zero weight columns, unit scales), the padding cut off again
                w_pad = self._padded(module.weight)
                for i, s in enumerate(self._scale_dt):
                    y = ops.awq_scale_qdq(w_pad, self._padded(s, 1.0), self.block_size, module.weight_quantizer.num_bits)
                    w_hat[i].copy_(y[:, :self.cin])
            else:
                for i, s in enumerate(self._scale_dt):
                    ops.awq_scale_qdq(module.weight, s, self.block_size, module.weight_quantizer.num_bits, out=w_hat[i])
            if self._cache_w:
                self._w_hat = w_hat
        return self._inv_scale, w_hat

    def release(self, budget=None):
        """Drop the search operands; with `budget`, a resident w_hat hands back what it was charged there."""
        if budget is not None and self._cache_w and self._w_hat is not None:
            budget.release(self._w_hat.numel() * self._w_hat.element_size())
        self._inv_scale = self._scale_dt = self._w_hat = None


def _gram_losses(h: AWQLiteHelper, module: QuantLinear):
    """All per-alpha losses of one linear from its Gram matrix, without touching the activations again.

    The reference's loss (model_calib.py:1489-1495, :1552-1556) is sum_b mean_{t,n} (out_alpha - out_actual)^2 with
    out_alpha = (x * 1/s) @ QDQ(W * s)^T and out_actual = x @ W^T, i.e. out_alpha - out_actual = x @ E^T with the
    fp32 error weight E = QDQ(W * s) * (1/s) - W.  Hence  sum_b ||X_b E^T||_F^2 / (T_b N) = trace(E G E^T) / N  with
    G = sum_b X_b^T X_b / T_b: the 11 GEMMs over every calibration token become 11 Cout x Cin x Cin contractions that
    do not depend on the number of tokens (Llama-3-8B, 512 x 512 tokens: 4.4e16 -> 0.6e16 FLOP including the Gram
    accumulation).  What it leaves out is the reference's rounding of x/s, out_alpha and out_actual to the model
    dtype -- a noise floor ~1e-3 below the INT4 error energy (fp32 models agree to 4e-7, bf16 within 1e-2 on the
    reference fixtures, same best alpha; tests/test_gpu_host.py, tests/test_gpu_awq_search.py)."""
    w = module.weight
    dt = w.dtype
    n_out = w.shape[0]
    bits = module.weight_quantizer.num_bits
    # 16-bit models: the Cout x Cin x Cin contraction runs on the matrix cores in split precision (three bf16
    # products summed in the fp32 accumulators, ~1e-5 relative) with the <., E> product fused; fp32 models run the same
    # contraction on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 products; agreement with the reference to
    # ~1e-6 is asserted for them).  The library GEMM is left for widths the kernels do not take and for CPU tensors.
    mfma = dt in (torch.bfloat16, torch.float16) and w.shape[1] % 8 == 0 and w.shape[1] % h.block_size == 0
    wf = None if mfma else w.float()
    f32_mfma = (not mfma and dt == torch.float32 and w.is_cuda and w.shape[1] % 8 == 0 and w.shape[0] % 4 == 0
                and h.gram.is_contiguous())
    planes = gram_score_planes(dt)
    gram_op = ops.gram_operand(h.gram, planes) if mfma else None
    for i, alpha in enumerate(h.alphas):
        s = h.scale(alpha)
        r = h._r_dev[i]  # (1 / s) rounded to the model dtype: input_quantizer.pre_quant_scale as the forward uses it (:1551)
        if mfma:
            # E and its split-precision MFMA operand from ONE read of W, then <E G, E> on the matrix cores
            err, a_op = ops.awq_err_weight(w, s.to(dt), r, h.block_size, bits, planes)
            ops.awq_quadform(err, gram_op, h.loss_buf[i:i + 1], 1.0 / n_out, a_operand=a_op)
        else:
            w_hat = ops.awq_scale_qdq(w, s.to(dt), h.block_size, bits)  # QDQ((W * s).to(dtype)), one kernel
            err = w_hat.float().mul_(r).sub_(wf)
            if f32_mfma:  # <E G, E> on the fp32 matrix cores (G is symmetric: the NT kernel's G^T is G)
                ops.awq_quadform(err, h.gram, h.loss_buf[i:i + 1], 1.0 / n_out)
            else:
                h.loss_buf[i] += (torch.matmul(err, h.gram) * err).sum() / n_out


# Relative margin inside which two candidates' Gram scores do not decide the search (search="auto").  The Gram loss
# differs from the reference-structured loss by d(alpha) = loss_gemm - loss_gram: the energy of the roundings of x/s,
# `out` and `out_actual` to the model dtype.  Two candidates can only swap places if d differs between them by more than
# their score gap.  Measured on the full-size synthetic Llama-3-8B run, every candidate scored by BOTH engines (224
# linears x 11 candidates, 64 x 4096 tokens; profiles/r02_awq_tie_margin.md): d is a smooth function of the loss -- over
# all 12 320 candidate pairs |d_i - d_j| is at most 6 % of the score gap for gaps above 1e-3 (1.3 % above 5e-3), so
# distant candidates never swap -- plus a zero-mean part (cross term error x rounding) that decides only pairs closer
# than ~1e-5 (the largest gap any pair was overturned at: 6.4e-6).  The margins are 100x that for bf16 and, with the
# 8x finer rounding, 30x for f16; fp32 models agree with the reference to 4e-7 (tests/test_gpu_host.py).  The zero-mean
# part shrinks with the number of outputs in the loss: GRAM_TIE_NOISE / sqrt(tokens * Cout) is added (~8 sigma; 1.6e-5
# at full size, 2e-3 for 200-token test shapes).
GRAM_TIE_MARGIN = {torch.bfloat16: 1e-3, torch.float16: 2e-4, torch.float32: 2e-5}
GRAM_TIE_NOISE = 0.5
# what the last awq_lite call did: wall-clock per stage, passes over the calibration data, re-scoring counts (tools,
# bench.py `extra`); overwritten by every call
AWQ_LITE_STATS: dict = {}
# bf16 planes of the Gram scoring contraction <E G, E> (ops.gram_operand): 3 = split precision in both factors.  bf16
# models screen with ONE plane (E and G rounded to bf16, a third of the contraction and of the operand memory): on the
# full-size run (profiles/r02_awq_tie_margin.md, "scoring planes") the one-plane scores differ from the three-plane ones
# by at most 2.9e-4 relative, by at most 2.7e-4 between any two candidates of a linear and 6e-5 between candidates within
# 5e-3 of the best; GRAM_PLANES_SLACK widens the re-scoring margin by the larger figure.  Same 224 / 224 alphas, same
# 106 re-scored candidates.  f16 models (margin 2e-4) keep the three planes.
GRAM_SCORE_PLANES = {torch.bfloat16: 1, torch.float16: 3}
GRAM_PLANES_SLACK = 3e-4
# The margin checks itself (search="auto", tie_check=True).  For every re-scored candidate i both scores are known, hence
# d_i = (exact_i - gram_i) / best_gram; S = max d - min d over the re-scored set measures how far the two engines disagree
# about THIS linear's candidates.  A candidate k left out (Gram gap > margin) could still beat the exact winner w only if
# d_w - d_k exceeds its Gram distance to w, i.e. margin - gap_w at least.  The unscored d_k is not known; it is taken to
# lie within TIE_SPREAD_FACTOR x S of the scored ones (d varies smoothly with alpha; the factor covers the extrapolation
# past the scored set).  So a linear is settled when  margin >= TIE_SPREAD_FACTOR * S + gap_w ; otherwise its margin is
# widened to twice that requirement, the newly admitted candidates are re-scored in a further pass, and the check repeats
# (at most TIE_CHECK_MAX_ROUNDS times, then every candidate of the linear is scored).  Full-size measurements
# (profiles/r03_awq_tie_check.md): the synthetic outlier stack shows S <= 4.6e-5 against a 1.3e-3 margin (requirement /
# margin 0.07 whatever the factor); a random-init HF Llama-3-8B, whose 11 candidates lie within 0.1-0.9 % of each other,
# shows S up to 8e-4 among its contenders and a largest overturned Gram gap of 1.1e-4: factor 1.5 settles every linear
# at once with requirement / margin up to 0.98 -- at the edge -- factor 2 widens 5 of 224 linears, same alphas.  Round 3
# shipped 1.5 because a widening cost one more PASS over the calibration data; since round 4 the exact pass of a decoder
# stack is a replay of stored activations (layer_local), a widening re-scores a handful of candidates of that one linear,
# and the default is the safer 2.0.
TIE_SPREAD_FACTOR = 2.0
# ... and with room to spare (round 6).  Rounds 4 and 5 settled the random-init HF model with requirement / margin 0.984 on
# its tightest linear: inside the rule, by 2 %, on the only adversarial input measured.  A linear now counts as settled only
# when the requirement is at most TIE_HEADROOM of its margin; one that passes by less is widened like one that fails.  The
# reported `max_need_over_margin` of a run is therefore <= 0.7 by construction, and what the extra widenings cost is a few
# more candidates re-scored from stored activations (measured on the stored full-size tables, tests/test_awq_tie_check_cpu.py).
TIE_HEADROOM = 0.7
TIE_CHECK_MAX_ROUNDS = 3


def tie_margin_check(gram, exact_scores: dict, margin: float, rounds: int):
    """One round of the margin's self-check for one linear (see TIE_SPREAD_FACTOR).  gram: the Gram scores of all
    candidates; exact_scores: {candidate index: exact score} of the re-scored ones; margin: the relative Gram margin
    they were admitted with; rounds: how often it was widened already.  Returns (need, new margin, new candidates):
    need = TIE_SPREAD_FACTOR * S + gap_w (None when it cannot be formed); new candidates = [] when the linear is
    settled (need <= TIE_HEADROOM * margin, or every candidate is scored)."""
    scored = sorted(exact_scores)
    best = min(gram)
    if len(scored) >= len(gram) or not math.isfinite(best) or best <= 0.0:
        return None, margin, []
    e = [exact_scores[i] for i in scored]
    if not all(math.isfinite(v) for v in e):  # NaN / inf somewhere: score everything
        return None, float("inf"), [i for i in range(len(gram)) if i not in exact_scores]
    d = [(exact_scores[i] - gram[i]) / best for i in scored]
    spread = max(d) - min(d)
    w = scored[min(range(len(e)), key=e.__getitem__)]
    need = TIE_SPREAD_FACTOR * spread + (gram[w] - best) / best
    if need <= TIE_HEADROOM * margin:
        return need, margin, []
    margin = float("inf") if rounds + 1 >= TIE_CHECK_MAX_ROUNDS else max(2.0 * need, 2.0 * margin)
    new = [i for i, v in enumerate(gram) if i not in exact_scores and v <= best * (1.0 + margin)]
    while not new and math.isfinite(margin):
        # nothing lies inside the widened margin: the requirement is then judged against THAT margin (settled with room), or
        # the margin grows until it admits a candidate / covers the requirement
        if need <= TIE_HEADROOM * margin:
            return need, margin, []
        margin *= 2.0
        new = [i for i, v in enumerate(gram) if i not in exact_scores and v <= best * (1.0 + margin)]
    return need, margin, new


def gram_score_planes(dtype) -> int:
    """bf16 planes of the screening contraction for this model dtype (GRAM_SCORE_PLANES; a study that wants another
    precision edits that table from its own script -- the product path reads no environment knob here)."""
    return GRAM_SCORE_PLANES.get(dtype, 3)


def _drained_clock(dev):
    if dev is not None and dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter()


def _layer_local_plan(model: nn.Module, explicit: bool = False):
    """The decoder layers awq_lite may walk one at a time, or None.  Conditions: a decoder stack exists (layerwise.
    get_decoder_layers) and -- unless the caller asked for it explicitly -- the model is a Hugging Face PreTrainedModel whose
    stack is made of *DecoderLayer modules (the contract "layer N+1's first argument is layer N's output" is theirs; any
    nn.ModuleList of equal children would otherwise qualify); every searched linear lives inside the stack; no OTHER
    quantizer is enabled (KV-cache / input quantizers outside the search add their noise in the reference's search pass,
    which a single pass cannot reproduce)."""
    from . import layerwise
    from .hf_attention import _is_supported_hf_model

    layers = layerwise.get_decoder_layers(model)
    if layers is None:
        return None
    if not explicit and not (_is_supported_hf_model(model) and type(layers[0]).__name__.endswith("DecoderLayer")):
        return None
    mods = [m for m in model.modules() if _awq_searched(m)]
    inside = {id(m) for lyr in layers for m in lyr.modules()}
    if not mods or any(id(m) not in inside for m in mods):
        return None
    if not all(_awq_fused_format(m.weight_quantizer, m.weight) for m in mods):
        return None  # a linear in another format (generic route of the search): the whole-model flow
    searched = {id(q) for m in mods for q in (m.weight_quantizer, m.input_quantizer)}
    if any(q.is_enabled and id(q) not in searched for q in model_calib._quantizers(model)):
        return None
    return layers


@torch.no_grad()
def _awq_lite_layer_local(model: nn.Module, forward_loop, layers, **kw):
    """awq_lite one decoder layer at a time (see awq_lite, `layer_local`).  The model's own forward runs up to the first
    decoder layer once per batch (embeddings, rotary tables: `layerwise._capture_inputs`); from there every layer is
    called on the previous layer's outputs with the captured arguments.  KV-cache objects among those arguments are
    dropped (a layer replayed outside its model must not append to a cache another call owns)."""
    from . import layerwise

    dev = next(model.parameters()).device
    total = {"search": kw.get("search", "auto"), "passes": 0, "replayed_passes": 0, "layer_local": True, "stages_s": {},
             "linears": 0, "rescored_linears": 0, "rescored_candidates": 0, "layers": len(layers),
             "tie_check": {"enabled": bool(kw.get("tie_check", True)), "spread_factor": TIE_SPREAD_FACTOR,
                           "checked_linears": 0, "widened_linears": 0, "max_need_over_margin": 0.0, "max_need": 0.0}}

    t0 = _drained_clock(dev)
    inputs = layerwise._capture_inputs(model, layers[0], forward_loop)

    without_cache = layerwise.without_cache

    reached = torch.tensor([float(len(inputs) > 0)], device=dev)
    if model_calib._dist_on():  # data parallel: the same flow on every rank (a rank whose shard is empty walks the layers with no batches)
        dist.all_reduce(reached, op=dist.ReduceOp.MAX)
    if reached.item() == 0:
        return None  # forward_loop does not drive the decoder stack (e.g. it calls the linears directly)
    inputs = [(args, without_cache(kwargs)) for args, kwargs in inputs]
    total["stages_s"]["embed"] = round(_drained_clock(dev) - t0, 4)
    helpers = {}
    most_passes = 0
    for idx, layer in enumerate(layers):
        nxt, calls, is_last = [], {"n": 0}, idx + 1 == len(layers)

        def layer_loop(m, _in=inputs, _nxt=nxt, _calls=calls, _last=is_last):
            first = _calls["n"] == 0  # the cache pass: the layer still has its original weights and the searched linears
            _calls["n"] += 1          # return out_actual -- its outputs are the un-quantized inputs of the next layer
            for args, kwargs in _in:
                out = m(*args, **kwargs)
                if first and not _last:
                    _nxt.append(((layerwise._first_tensor(out).detach(), *args[1:]), kwargs))

        helpers.update(awq_lite(layer, layer_loop, layer_local=False, store_activations=True, **kw))
        inner = AWQ_LITE_STATS
        for k, v in (inner.get("stages_s") or {}).items():
            total["stages_s"][k] = round(total["stages_s"].get(k, 0.0) + v, 4)
        most_passes = max(most_passes, inner.get("passes", 0))
        total["replayed_passes"] += inner.get("replayed_passes", 0)
        for k in ("linears", "rescored_linears", "rescored_candidates"):
            total[k] += inner.get(k, 0)
        tc, ic = total["tie_check"], inner.get("tie_check") or {}
        for k in ("checked_linears", "widened_linears"):
            tc[k] += ic.get(k, 0)
        for k in ("max_need_over_margin", "max_need"):
            tc[k] = max(tc[k], ic.get(k, 0.0))
        inputs = nxt
    total["passes"] = most_passes  # forwards through every layer: 1 when every layer's exact pass was a replay
    AWQ_LITE_STATS.clear()
    AWQ_LITE_STATS.update(total)
    return helpers


def _forward_binder(run, module):
    """The forward awq_lite puts on a searched linear for the length of the call."""
    def patched_forward(input):
        return run.forward(module, input)
    return patched_forward


class _AWQLiteRun:
    """One awq_lite call over `model` (the whole model, or one decoder layer of the layer-local walk): the per-linear
    helpers, the HBM budget, the state of the passes and the stage clock, with one method per phase -- awq_lite() below
    reads as the flow.

    mode       "cache" / "search": the pass the patched forwards are in
    gram_pass  the pass the Gram matrices are accumulated in ("cache"; "search" with other quantizers enabled, whose
               noise only the search pass sees; None once they are scored)
    store      False / "inputs" / "full": what the cache pass keeps for a replayed search pass (store_activations)
    do_gemm    the search pass scores ALL candidates of the linears without a Gram matrix (its first time round)
    do_exact   the search pass re-scores the pending near-ties of the Gram-scored linears"""

    def __init__(self, model, forward_loop, alpha_step, search, tie_margin, tie_check, store_activations):
        self.model, self.forward_loop, self.alpha_step, self.search = model, forward_loop, alpha_step, search
        self.tie_margin, self.tie_check, self.store_activations = tie_margin, tie_check, store_activations
        self.stats = AWQ_LITE_STATS
        self.stats.clear()
        self.stats.update({"search": search, "passes": 0, "stages_s": {}})
        self.mods = [(n, m) for n, m in model.named_modules() if _awq_searched(m)]
        self.dev = self.mods[0][1].weight.device if self.mods else None
        self.clock = None  # when the running stage began
        self.helpers, self.originals = {}, {}
        self.budget = None  # _WeightCacheBudget (a model without searched linears never asks it)
        self.others, self.others_holder = [], None  # the enabled quantizers outside the search
        self.mode, self.gram_pass = "cache", "cache"
        self.do_gemm, self.do_exact = True, False
        self.store, self.store_cap = False, None
        self.stored_bytes, self.store_last, self.store_seen = 0, None, {}
        # the last input tensor that reached a Gram matrix / an act_sum, and the helper that took it (shared inputs)
        self.gram_input = self.gram_owner = self.act_input = self.act_owner = None

    def stage(self, name):
        """Wall-clock of the flow's stages (tools / bench `extra`): the device is drained only here, at points where the
        host waits for statistics anyway."""
        now = _drained_clock(self.dev)
        if name is not None and self.clock is not None:
            self.stats["stages_s"][name] = round(self.stats["stages_s"].get(name, 0.0) + now - self.clock, 4)
        self.clock = now

    # ------------------------------------------------------------------------------------------------ setup
    def setup(self):
        # the stages cover the WHOLE call (setup = helpers, weight scales, Gram buffers; teardown = the bookkeeping after the
        # fold), so that  sum(stages_s) == wall-clock of awq_lite  by construction
        self.stage(None)
        self.helpers = {m: AWQLiteHelper(m, self.alpha_step) for _, m in self.mods}
        self.stage("weight_scales")  # (helper construction: one moq_awq_weight_scale launch and four small buffers per linear)
        self.bypass_input_quantizers()
        if self.store_activations not in (True, False, "auto", "inputs"):
            raise ValueError("awq_lite: store_activations must be True, False, 'inputs' or 'auto', "
                             f"got {self.store_activations!r}")
        self.store = {True: "full", False: False, "inputs": "inputs"}.get(self.store_activations,
                                                                          "inputs" if self.search == "auto" else False)
        if self.mods:
            self.reserve_gram_buffers()
        self.stage("gram_buffers")  # (device-memory query of the budget + one zeroed [Cin, Cin] fp32 matrix per Gram-scored linear)
        searched = {id(q) for _, m in self.mods for q in (m.weight_quantizer, m.input_quantizer)}
        self.others = [q for q in model_calib._quantizers(self.model) if id(q) not in searched and q.is_enabled]
        self.others_holder = nn.ModuleList(self.others)
        # With other quantizers active (FP8 KV cache, ...) the reference's search pass sees THEIR quantization noise in
        # the activations; the Gram matrices are then accumulated in a second pass instead of the cache pass.
        self.gram_pass = "search" if self.others else "cache"
        if self.others:
            self.store = False  # the search pass must SEE the other quantizers' noise: nothing of the cache pass is reusable
        if self.store and self.store_activations == "auto" and self.mods:
            # nobody asked for the store: in the whole-model flow the kept inputs of EVERY searched linear and batch share the HBM
            # with the forward's own peak activations, which the budget (a fraction of what was free at setup) does not see --
            # the automatic store stops at half of what the budget has left (30 % of the memory that was available, Gram matrices
            # taken off first) and the search pass is then a real forward, where an explicit store_activations=True / "inputs" may
            # take all of it
            self.store_cap = self.budget.left // 2
        for _, m in self.mods:
            self.originals[m] = m.__dict__.get("forward", model_calib._NO_INSTANCE_FORWARD)
            m.forward = _forward_binder(self, m)

    def bypass_input_quantizers(self):
        for _, m in self.mods:
            # quantized inputs (W4A8 AWQ; setup, :1436-1444): the input quantizer is bypassed for the whole search -- the
            # losses are taken on UNquantized activations -- and max-calibrated per input channel in the cache pass; the
            # per-tensor amax it ends up with is that of the smoothed activation, max_c(amax_c * pre_quant_scale_c)
            h, iq = self.helpers[m], m.input_quantizer
            h.is_input_quantized = iq.is_enabled
            if h.is_input_quantized:
                iq.disable()
                if iq.axis not in (None, -1):
                    h.is_enabled = False
                    h.setup_disabled = True
                else:
                    iq.axis = -1

    def reserve_gram_buffers(self):
        self.budget = _WeightCacheBudget(self.dev)
        for _, m in self.mods:
            h = self.helpers[m]
            cin = m.weight.shape[1]
            # ragged rows (Cin not a multiple of the block: zero-padded, AWQLiteHelper) stay on the error-GEMM engine
            gram_ok = h.fused and cin % 4 == 0 and cin % h.block_size == 0
            fits = self.search != "gemm" and gram_ok and self.budget.reserve(4 * cin * cin)
            if fits or (self.search == "gram" and gram_ok):
                h.gram = torch.zeros(cin, cin, dtype=torch.float32, device=m.weight.device)
                h.gram_bytes = 4 * cin * cin if fits else 0
                h.use_gram = True
            else:
                h._cache_w = self.budget.reserve(len(h.alphas) * m.weight.numel() * m.weight.element_size())

    # ------------------------------------------------------------------------------------------------ the patched forward
    def forward(self, m, input):
        h = self.helpers[m]
        out_actual = F.linear(input, m.weight, m.bias)
        if input.numel() == 0 or h.setup_disabled:
            return out_actual
        x2 = input.reshape(-1, input.shape[-1])
        if self.mode == "cache":
            self.accumulate_act(h, input, x2)
            h.num_cache_steps += 1
            h.num_tokens += x2.shape[0]
            if h.is_input_quantized:  # :1534-1538: running per-channel amax of the raw input
                iq = m.input_quantizer
                iq.enable()
                model_calib.max_calibrate(iq, lambda q: q(input), distributed_sync=False)
                iq.disable()
        if self.mode == self.gram_pass and h.gram is not None and h.is_enabled:
            self.accumulate_gram(h, input, x2)
        if self.mode == "cache" and self.store and h.is_enabled:
            self.store_batch(h, input, x2, out_actual)
        if self.mode == "cache" or not h.is_enabled:
            return out_actual
        out2 = out_actual.reshape(-1, out_actual.shape[-1])
        if h.use_gram:
            # scores came from the Gram matrix; only near-ties are re-scored with the reference's arithmetic
            if self.do_exact and h.pending:
                self.error_gemms(m, h, x2, out2, h.pending, h.exact_pass_buf)
                h.num_exact_steps += 1
        elif self.do_gemm:
            self.error_gemms(m, h, x2, out2, None, h.loss_buf)
            h.num_search_steps += 1
        return out_actual

    def accumulate_act(self, h, input, x2):
        # act_scale += mean_tokens |x| in the activation dtype (get_act_scale, :1471-1472), one kernel pass.  Linears
        # fed by the SAME tensor object (q / k / v, gate / up) have the same statistic: the first one of a batch
        # accumulates it, the others alias its buffer (the rule of the Gram matrices below, same check: identity of the
        # tensor object, which is kept alive in between) -- three reads of a 33 MB activation less per decoder layer
        # and batch, bit-identical values
        owner = self.act_owner if self.act_input is input else None
        if owner is not None and owner.act_sum.shape == h.act_sum.shape and h.act_owner in (None, owner):
            if h.act_owner is None:
                h.act_owner = owner
                h.act_sum = owner.act_sum
            return
        if h.act_owner is not None:
            raise RuntimeError("awq_lite: a linear that shared its input with another one in an earlier batch got a "
                               "different tensor now")
        if numerics.on_host():
            ops.col_abs_mean_accum(x2, h.act_sum)
        else:
            # numerics "device" = the reference's run ON THIS DEVICE, and this statistic is the one place where that
            # needs torch's own kernel: both sides sum |x| in fp32 and round the mean to the activation dtype, but
            # in different orders, and a channel whose mean sits on a 16-bit rounding boundary lands on either side
            # (Llama-3-8B width on the MI355X: 23 of 56 scale / amax vectors one step apart, profiles/r06_dropin.md;
            # the one-pass kernel is the default mode's, where the result must not depend on the device).  Three
            # passes over a 33 MB activation instead of one, next to the layer's GEMMs.
            h.act_sum.add_(x2.abs().mean(0).to(torch.float32))
        self.act_input, self.act_owner = input, h

    def accumulate_gram(self, h, input, x2):
        h.num_gram_steps += 1
        # Linears fed by the SAME tensor (q / k / v of an attention block, gate / up of an MLP) have the same
        # Gram matrix: the first one accumulates it, the others alias it.  Identity of the tensor object is the
        # test (a reference to the last input is kept, so its address cannot be reused in between).
        owner = self.gram_owner if self.gram_input is input else None
        if owner is not None and owner.gram is not None and owner.gram.shape == h.gram.shape \
                and h.gram_owner in (None, owner):
            if h.gram_owner is None:
                h.gram_owner = owner
                h.gram = owner.gram  # the own buffer is released
                self.budget.release(h.gram_bytes)
                h.gram_bytes = 0
            return
        if h.gram_owner is not None:
            raise RuntimeError("awq_lite (Gram search): a linear that shared its input with another one in an "
                               "earlier batch got a different tensor now; use search='gemm' for this model")
        if x2.dtype in (torch.bfloat16, torch.float16):
            # G += X^T X / T_b on the matrix cores; several batches per launch when the staging buffer fits
            if h.gram_stage is None and not h.gram_stage_denied:
                if self.budget.reserve(ops.GramStage.nbytes(x2.shape[1], x2.shape[0])):
                    h.gram_stage = ops.GramStage(h.gram, x2.shape[0], x2.dtype)
                else:
                    h.gram_stage_denied = True
            if h.gram_stage is not None:
                h.gram_stage.add(x2)
            else:
                ops.hessian_accum(h.gram, x2, 1.0, 1.0 / x2.shape[0], upper_only=True)
        else:
            xf = x2.float()
            h.gram.addmm_(xf.t(), xf, alpha=1.0 / x2.shape[0])
        self.gram_input, self.gram_owner = input, h

    def error_gemms(self, m, h, x2, out2, subset, loss_buf):
        """loss_buf[j] += mean((linear(x / s_a, QDQ(W s_a)) - out_actual)^2) for the candidates `subset` (None: all)
        with the reference's roundings (x/s, the output and out_actual in the model dtype)."""
        inv_s, w_hat = h.search_operands(m, subset)
        if ops.mfma_gemm_supported(x2, m.weight):
            # all candidates in two launches: xs[a] = x * (1/s_a) (one read of x), then the batched MFMA
            # contraction with the (out - out_actual)^2 mean fused -- `out` never reaches HBM
            xs = ops.scale_cols_multi(x2, inv_s)
            ops.awq_err_gemm_multi(xs, w_hat, out2, m.bias, loss_buf)
        else:  # widths the kernels do not take: library GEMM, the reference's own arithmetic
            for j in range(inv_s.shape[0]):
                out = F.linear(ops.scale_cols(x2, inv_s[j]), w_hat[j], m.bias)
                loss_buf[j] += (out - out2).float().pow(2).mean()

    # ------------------------------------------------------------------------------------------------ the activation store
    def store_batch(self, h, input, x2, out_actual):
        """store_activations: keep this batch's input and out_actual of this linear for the replayed exact pass.  The
        tensors exist anyway -- the store only keeps them alive -- and are charged to the HBM budget (an input shared by
        q / k / v or gate / up once)."""
        if self.store == "inputs" and input.is_inference():
            # (forward_loop under torch.inference_mode(): no version counter says whether the tensor is still what the cache
            # pass read when the replay gets to it -- nothing is stored, the search pass is a real forward)
            self.drop_stores("inference tensors carry no version counter")
            return
        if self.store_cap is not None and self.stored_bytes + x2.numel() * x2.element_size() > self.store_cap:
            self.drop_stores("the automatic store reached its cap (half of what the HBM budget had left)")
            return
        if self.store == "inputs":
            # the input only, charged once per distinct tensor object (kept alive in `store_seen`, so an id cannot be
            # reused); out_actual is recomputed by the replay from the linear's own weight
            nbytes = 0 if self.store_seen.get(id(input)) is input else x2.numel() * x2.element_size()
            if x2.data_ptr() != input.data_ptr():  # a strided input: the flattened copy is this linear's own
                nbytes = x2.numel() * x2.element_size()
            if not self.budget.reserve(nbytes):
                self.drop_stores()
                return
            self.store_seen[id(input)] = input
            self.stored_bytes += nbytes
            h.stored.append((x2, None, input, input._version))
            return
        nbytes = out_actual.numel() * out_actual.element_size()
        if self.store_last is not input:
            nbytes += x2.numel() * x2.element_size()
        if not self.budget.reserve(nbytes):
            self.drop_stores()  # does not fit: the exact pass will be a real one
            return
        self.store_last = input
        self.stored_bytes += nbytes
        h.stored.append((x2, out_actual.reshape(-1, out_actual.shape[-1]), None, None))

    def drop_stores(self, why="no room in the HBM budget"):
        self.stats.setdefault("store_dropped", why)  # (the first reason: why this call's search pass is a real forward)
        for hh in self.helpers.values():
            hh.stored = []
        self.budget.release(self.stored_bytes)
        self.stored_bytes, self.store, self.store_last = 0, False, None
        self.store_seen = {}

    def stores_intact(self) -> bool:
        """"inputs" mode: every kept input still holds what the cache pass read (no in-place write since)."""
        return all(src is None or src._version == ver for hh in self.helpers.values() for _, _, src, ver in hh.stored)

    def replay_search_pass(self):
        """The search pass from the stored activations, linear by linear: every candidate this pass has to score of a
        linear (its near-ties, or all of them for a linear without a Gram matrix) over all stored batches, then the
        next linear -- one linear's search weights are alive at a time."""
        for _, m in self.mods:
            h = self.helpers[m]
            if not h.is_enabled or h.act_scale is None or not h.stored:
                continue
            if h.use_gram:
                if not (self.do_exact and h.pending):
                    continue
                subset, buf = h.pending, h.exact_pass_buf
            elif self.do_gemm:
                subset, buf = None, h.loss_buf
            else:
                continue
            keep, h._cache_w = h._cache_w, True  # resident for this linear's batches, released right after
            for x2, out2, _, _ in h.stored:
                if out2 is None:  # "inputs": out_actual from the un-folded weight, as the patched forward computes it
                    out2 = F.linear(x2, m.weight, m.bias)
                self.error_gemms(m, h, x2, out2, subset, buf)
                if h.use_gram:
                    h.num_exact_steps += 1
                else:
                    h.num_search_steps += 1
            h.release()  # (never charged to the budget: `_cache_w` was forced for the length of this loop)
            h._cache_w = keep

    def search_pass(self):
        if self.store == "inputs" and not self.stores_intact():
            self.drop_stores("a stored input was written in place after the cache pass")
        if self.store:
            self.replay_search_pass()
            self.stats["replayed_passes"] = self.stats.get("replayed_passes", 0) + 1
        else:
            self.forward_loop(self.model)
            self.stats["passes"] += 1
        self.stage("search_pass")

    # ------------------------------------------------------------------------------------------------ cache pass, statistics
    def cache_pass(self):
        # every OTHER enabled quantizer (KV-cache bmm quantizers, linears outside the search, ...) collects its amax
        # during the cache pass and quantizes during the search pass, as in the reference (:1574-1586); dynamic ones
        # are switched to pass-through for the cache pass
        model_calib.enable_stats_collection(self.others_holder)
        self.stage("setup")
        self.forward_loop(self.model)
        self.stats["passes"] += 1
        self.act_input = self.act_owner = None  # (the last batch's input need not stay alive)
        if self.store == "inputs":
            self.stats["stored_input_bytes"] = self.stored_bytes
        self.stage("cache_pass")

    def finish_gram_pass(self):
        self.gram_input = self.gram_owner = self.act_input = self.act_owner = None
        for h in self.helpers.values():
            if h.gram_stage is not None:
                h.gram_stage.flush()
                h.gram_stage = None

    def statistics(self):
        model_calib.finish_stats_collection(self.others_holder)
        if self.others and _dist_initialized():
            mdist.sync_amax_bucketed([q for q in self.others if not q._dynamic], device=self.dev)
        if _dist_initialized():
            # the per-channel input amax of W4A8 linears is synchronised like any other amax (:1581-1586, :396-398)
            chan = [m.input_quantizer for _, m in self.mods if self.helpers[m].is_input_quantized]
            if chan:
                mdist.sync_amax_bucketed(chan, device=self.dev)
        if self.gram_pass == "cache":
            self.finish_gram_pass()
        self.act_scales()
        if self.mods:
            self.sync_act_scales()
            self.scale_tables()
        self.stage("scales")

    def act_scales(self):
        cached = [h for h in self.helpers.values() if h.num_cache_steps]
        if cached and not numerics.on_host():
            # act_scale = act_sum / steps (:1601) as torch evaluates `tensor / int` on the statistics' device
            for h in cached:
                h.act_scale = h.act_sum.detach().float() / h.num_cache_steps
        elif cached:
            # act_scale = act_sum / steps (:1601) as IEEE division on the host (see get_scale) -- for ALL linears in one
            # device -> host copy and one upload instead of a stream drain per linear
            flat = torch.cat([h.act_sum.detach().float().reshape(-1) for h in cached]).cpu()
            with host_math_threads():
                steps = torch.cat([torch.full((h.act_sum.numel(),), float(h.num_cache_steps)) for h in cached])
                flat = (flat / steps).to(cached[0].act_sum.device)
            off = 0
            for h in cached:
                h.act_scale = flat[off:off + h.act_sum.numel()]
                off += h.act_sum.numel()

    def sync_act_scales(self):
        # DP: act_scale average + the any-NaN vote for ALL linears in ONE bucket (reference: one all_reduce and
        # one object gather per linear, :1588-1619); ranks whose shard never reached a linear join with zeros
        hs = [self.helpers[m] for _, m in self.mods]
        synced, enabled = mdist.sync_awq_act_scales([h.act_scale for h in hs], [h.weight_scale for h in hs],
                                                    [m.weight.shape[1] for _, m in self.mods], self.dev)
        for h, a, ok in zip(hs, synced, enabled):
            h.is_enabled = ok
            h.act_scale = a if ok else None
            if not ok:
                h.gram = None
                h.use_gram = False

    def scale_tables(self):
        # every candidate scale vector of every linear: ONE device -> host copy of all statistics, the [Cin]-sized
        # math on the host (get_scale), one upload per linear -- all before the first scoring kernel is queued
        live = [(m, self.helpers[m]) for _, m in self.mods if self.helpers[m].act_scale is not None]
        if live and not numerics.on_host():
            for m, h in live:  # the same tables from device tensors (numerics "device": no copy, no host math)
                h.prepare_scales(h.act_scale, h.weight_scale, m.weight.dtype)
        elif live:
            flat = torch.cat([t.detach().float().reshape(-1) for _, h in live for t in (h.act_scale, h.weight_scale)]).cpu()
            jobs, off = [], 0
            for m, h in live:
                c = h.act_scale.numel()
                jobs.append((h, flat[off:off + c], flat[off + c:off + 2 * c], m.weight.dtype))
                off += 2 * c
            # 11 pow / divide / normalise chains per linear on [Cin] vectors, one thread (see host_math_threads)
            with host_math_threads():
                tables = [j[0].host_scales(j[1], j[2], j[3]) for j in jobs]
            for (h, _, _, _), both in zip(jobs, tables):
                h.upload_scales(both)

    # ------------------------------------------------------------------------------------------------ scoring
    def scoring(self):
        if self.gram_pass == "cache":
            self.gram_losses()
            self.do_exact = self.pick_contenders()
        self.stage("gram_scores")
        need_gemm = any(not h.use_gram and h.act_scale is not None for h in self.helpers.values())
        need_gram = self.gram_pass == "search" and any(h.gram is not None for h in self.helpers.values())
        if need_gemm or need_gram or self.do_exact:
            self.mode = "search"
            # search pass: error GEMMs (all candidates of the linears without a Gram matrix, the near-ties of the
            # others), and the Gram matrices when they had to wait for quantized inputs -- replayed from the stored
            # activations when the call keeps them (store_activations), a second forward otherwise
            if need_gram and self.store:  # (Gram matrices from the search pass need the real forward)
                self.drop_stores("the Gram matrices come from the search pass")
            self.search_pass()
            self.do_gemm = False
            if need_gram:
                self.finish_gram_pass()
                self.gram_losses()
                self.gram_pass = None
                self.do_exact = self.pick_contenders()
                self.stage("gram_scores")
            elif self.do_exact:
                self.do_exact = self.collect_exact()
            while self.do_exact:
                # the near-ties of linears whose Gram matrix came from the search pass; candidates admitted by the
                # margin's self-check (tie_check)
                self.search_pass()
                self.do_exact = self.collect_exact()
        self.sync_late_losses()

    def sync_late_losses(self):
        late = [h for h in self.helpers.values() if not h.loss_synced]
        for h in late:
            h.search_steps_all_ranks = h.num_search_steps
        if _dist_initialized() and self.mods:
            # every rank must pick the same alpha -- and take the same "was it searched at all" decision: SUM the
            # per-alpha losses and the search-step counters in one bucket (Gram-scored linears were summed when the
            # near-ties were picked, their exact scores after every exact pass: collect_exact)
            steps = torch.tensor([float(h.num_search_steps) for h in late], device=self.dev)
            mdist.all_reduce_bucket([h.loss_buf for h in late] + [steps], dist.ReduceOp.SUM)
            for h, n in zip(late, steps.tolist()):
                h.search_steps_all_ranks = int(n)

    def shard_gram_scoring(self):
        """Data parallel: instead of every rank scoring every linear on its LOCAL Gram matrix (the scores are linear in
        it and get summed), the distinct Gram matrices are dealt over the ranks -- balanced by the scoring work they
        carry -- each is SUM-reduced to its rank over RCCL (a real exchange: sum of Cin^2 fp32 over the model, 33 GB for
        Llama-3-8B, a few hundred ms over xGMI) and only that rank scores the linears that read it; the other ranks
        contribute zeros to the score bucket.  The scoring (11 quadratic forms per linear, a third of the single-GPU
        search) then scales with the number of GPUs like the accumulation does.  Returns {owner helper: rank} or None
        when the ranks do not see the same sharing structure (then every rank scores locally, as before)."""
        if not model_calib._dist_on():
            return None
        hs = [self.helpers[m] for _, m in self.mods]
        index = {id(h): i for i, h in enumerate(hs)}
        sig = [None if (h.gram is None or h.act_scale is None or not h.is_enabled)
               else (index[id(h.gram_owner or h)], tuple(h.gram.shape), str(h.gram.dtype)) for h in hs]
        gathered = [None] * dist.get_world_size()
        dist.all_gather_object(gathered, sig)
        if any(g != sig for g in gathered):
            return None
        cost, owners = {}, []
        for (_, m), h, s_ in zip(self.mods, hs, sig):
            if s_ is None:
                continue
            o = hs[s_[0]]
            if id(o) not in cost:
                cost[id(o)] = 0
                owners.append(o)
            cost[id(o)] += m.weight.shape[0] * m.weight.shape[1] * m.weight.shape[1]
        load = [0] * dist.get_world_size()
        placement = {}
        for o in sorted(owners, key=lambda o: -cost[id(o)]):  # largest first onto the least loaded rank
            r = min(range(len(load)), key=load.__getitem__)
            placement[id(o)] = r
            load[r] += cost[id(o)]
        for o in owners:  # same order on every rank
            mdist.reduce_chunked(o.gram, placement[id(o)], dist.ReduceOp.SUM)  # <= 1 GiB per call
        return placement

    def gram_losses(self):
        """Gram-matrix linears: all alpha losses from the Gram matrix (the loss is linear in it).  Single process: the
        local matrix.  Data parallel: the reduced matrix on the rank it was dealt to (shard_gram_scoring), or -- when
        the ranks disagree on the sharing structure -- every rank's local matrix, summed later in the score bucket."""
        placement = self.shard_gram_scoring()
        me = dist.get_rank() if placement is not None else 0
        for _, m in self.mods:
            h = self.helpers[m]
            if h.gram is not None and h.act_scale is not None:
                own = h.gram_owner or h
                h.num_search_steps = h.num_gram_steps
                if placement is None or placement.get(id(own)) == me:
                    if m.weight.dtype != torch.float32 and not own.gram_symmetrized:
                        ops.symmetrize(h.gram)  # the MFMA accumulation kept the upper tiles only; once per matrix
                        own.gram_symmetrized = True
                    _gram_losses(h, m)
                    h.scored_here = True
                self.budget.release(h.gram_bytes)  # an owner's matrix really goes when its last alias has been scored
                h.gram_bytes = 0
                h.gram = None  # release Cin^2 floats as soon as the last linear using them is done

    def pick_contenders(self) -> bool:
        """After the Gram scores are known: which candidates of which linears need the exact engine.  The decision is
        taken on the scores summed over the data-parallel group, so every rank re-scores the same candidates."""
        scored = [(m, self.helpers[m]) for _, m in self.mods if self.helpers[m].use_gram and self.helpers[m].is_enabled
                  and self.helpers[m].act_scale is not None]
        if not scored:
            return False
        if _dist_initialized():
            steps = torch.tensor([float(h.num_search_steps) for _, h in scored] + [float(h.num_tokens) for _, h in scored],
                                 device=scored[0][0].weight.device)
            mdist.all_reduce_bucket([h.loss_buf for _, h in scored] + [steps], dist.ReduceOp.SUM)
            counts = steps.tolist()
            for (_, h), n, t in zip(scored, counts[:len(scored)], counts[len(scored):]):
                h.search_steps_all_ranks = int(n)
                h.tokens_all_ranks = int(t)
                h.loss_synced = True
        if self.search != "auto":
            return False
        table = torch.stack([h.loss_buf for _, h in scored]).cpu()  # one host sync for all linears
        any_tie = False
        for (m, h), row in zip(scored, table.tolist()):
            h.gram_loss = list(row)
            margin = self.tie_margin
            if margin is None:
                tokens = h.num_tokens if h.tokens_all_ranks is None else h.tokens_all_ranks
                outputs = max(1, tokens * m.weight.shape[0])
                margin = GRAM_TIE_MARGIN.get(m.weight.dtype, 5e-3) + GRAM_TIE_NOISE / math.sqrt(outputs)
                if gram_score_planes(m.weight.dtype) < 3 and m.weight.dtype != torch.float32:
                    margin += GRAM_PLANES_SLACK
            best = min(row)  # a NaN score never compares smaller: such a linear keeps the plain first-minimum rule
            if not math.isfinite(best):
                continue
            h.margin_used = margin
            close = [i for i, v in enumerate(row) if v <= best * (1.0 + margin)]
            if len(close) > 1:
                self.queue_exact(m, h, close)
                any_tie = True
        return any_tie

    def queue_exact(self, m, h, indices):
        """The next exact pass scores these candidates of this linear."""
        h.pending = list(indices)
        h.exact_pass_buf = torch.zeros(len(indices), dtype=torch.float32, device=m.weight.device)
        h.num_exact_steps = 0
        h.release(self.budget)
        # (a replayed pass keeps one linear's search weights alive at a time: nothing to reserve per linear)
        h._cache_w = (not self.store) and self.budget.reserve(len(indices) * m.weight.numel() * m.weight.element_size())

    def collect_exact(self) -> bool:
        """After an exact pass: the scores of the pending candidates (summed over the data-parallel group, so every
        rank takes the same decisions) move to `exact_scores`; with tie_check every re-scored linear's margin is
        verified against the measured disagreement of the two engines and widened if it was too small.  Returns whether
        another exact pass is needed."""
        todo = [(m, self.helpers[m]) for _, m in self.mods if self.helpers[m].pending]
        if not todo:
            return False
        dev = todo[0][0].weight.device
        steps = torch.tensor([float(h.num_exact_steps) for _, h in todo], device=dev)
        if _dist_initialized():
            mdist.all_reduce_bucket([h.exact_pass_buf for _, h in todo] + [steps], dist.ReduceOp.SUM)
        flat = torch.cat([h.exact_pass_buf for _, h in todo] + [steps]).cpu().tolist()  # one host sync
        counts = flat[len(flat) - len(todo):]
        off, again = 0, False
        for (m, h), n_steps in zip(todo, counts):
            vals = flat[off:off + len(h.pending)]
            off += len(h.pending)
            pend, h.pending, h.exact_pass_buf = h.pending, None, None
            h.release(self.budget)
            h._cache_w = False
            h.exact_steps_all_ranks = int(n_steps)
            if n_steps <= 0:
                continue  # the second pass never reached this linear: the Gram scores stand
            h.exact_scores.update(zip(pend, vals))
            if not self.tie_check or self.tie_margin is not None and not math.isfinite(self.tie_margin):
                continue
            new = self.check_margin(h)
            if new:
                self.queue_exact(m, h, new)
                again = True
        return again

    def check_margin(self, h):
        """The self-check of the re-scoring margin (tie_margin_check): candidates to add, or [] when settled."""
        need, margin, new = tie_margin_check(h.gram_loss, h.exact_scores, h.margin_used, h.tie_rounds)
        # (None: nothing left to weigh -- every candidate of the linear has its exact score, or the scores are not finite)
        h.tie_need = need
        if new:
            h.tie_rounds += 1
        h.margin_used = margin  # (also when it grew without admitting anybody: that is the margin the linear is settled at)
        return new

    # ------------------------------------------------------------------------------------------------ restore, fold, report
    def restore(self):
        for m, f in self.originals.items():
            model_calib._restore_forward(m, f)
        for h in self.helpers.values():
            h.release()
            h.gram = None
            h.stored = []
        self.store_seen = {}

    def restore_input_quantizer(self, m, h):
        """:1642-1653 / :1707-1714: the per-channel amax is kept (on the host) for the smoothing step and collapses to
        the per-tensor amax the quantizer is exported with; a dynamic input quantizer is just re-enabled."""
        iq = m.input_quantizer
        if not h.is_input_quantized:
            return
        if iq.amax is not None:
            act_amax = iq.amax
            iq._amax_for_smoothing = act_amax.cpu()
            iq.reset_amax()
            iq.axis = None
            iq.amax = act_amax.amax()
        iq.enable()

    def finish_fold(self, m, h, pre_quant_scale):
        """The tail of both fold branches: the weight quantizer is max-calibrated on the weight as it is now, the input side
        gets `pre_quant_scale` in the weight dtype (None: the neutral one, all ones -- made after the recalibration, where
        the flow has always launched it) and the bypassed input quantizer comes back."""
        m.weight_quantizer.reset_amax()
        model_calib.max_calibrate(m, lambda lin: lin.weight_quantizer(lin.weight), distributed_sync=False)
        m.input_quantizer._enable_pre_quant_scale = True
        if pre_quant_scale is None:
            pre_quant_scale = torch.ones(m.weight.shape[1], dtype=m.weight.dtype, device=m.weight.device)
        m.input_quantizer.pre_quant_scale = pre_quant_scale.to(m.weight.dtype)
        self.restore_input_quantizer(m, h)

    def pick_best_alpha(self, h):
        if h.exact_scores:
            # near-ties: the exact scores replace the Gram scores of the re-scored candidates and decide among them
            # (ascending alpha, first minimum: the reference's dict order, :1637)
            h.contenders = sorted(h.exact_scores)
            exact = [h.exact_scores[i] for i in h.contenders]
            h.exact_buf = torch.tensor(exact, dtype=torch.float32, device=h.loss_buf.device)
            h.loss_buf[torch.tensor(h.contenders, device=h.loss_buf.device)] = h.exact_buf
            losses = {a: float(v) for a, v in h.loss.items()}
            h.best_alpha = h.alphas[h.contenders[min(range(len(exact)), key=exact.__getitem__)]]
        else:
            losses = {a: float(v) for a, v in h.loss.items()}
            h.best_alpha = min(losses, key=losses.get)  # first minimal alpha (:1637)
        h.best_scale = h.scale(h.best_alpha)

    def fold(self):
        for name, m in self.mods:
            h = self.helpers[m]
            if h.is_enabled and h.search_steps_all_ranks == 0:
                h.is_enabled = False  # :1665-1672
                warnings.warn("awq_lite: Calling `forward_loop(model)` the second time did not forward data through the "
                              f"{name}. Please provide a valid `forward_loop` function that can be used to forward data "
                              "through the model many times.")
            if not h.is_enabled:
                # :1674-1700: uncalibrated / NaN / never searched -> max-calibrated weights and a neutral pre_quant_scale,
                # so that every linear of the model exports in the same format
                warnings.warn(f"awq_lite: Forcing pre_quant_scale=1 for {name} because the expert was not properly "
                              "exercised during calibration. This may degrade accuracy; consider increasing calibration "
                              "size or using a more diverse dataset.")
                m.awq_lite = h
                self.finish_fold(m, h, None)
                continue
            self.pick_best_alpha(h)
            m.awq_lite = h
            # postprocess (:1636-1659) -> apply_pre_quant_scale_and_smooth(module, 1 / best_scale) (:1226-1252): the input
            # gets 1/s in the weight dtype; the weight is multiplied (fp32, one rounding) by 1 / (1/s) -- the fp32 double
            # reciprocal, which is not always s itself -- and recalibrated
            best_idx = h.alphas.index(h.best_alpha)
            pqs_host = 1.0 / h._s_host[best_idx]  # where every scale vector was formed (get_scale: host IEEE fp32, or the device)
            both = torch.stack([pqs_host, 1.0 / pqs_host]).to(m.weight.device)
            pre_quant_scale = both[0]
            ops.scale_cols(m.weight.data, both[1], out=m.weight.data)
            self.finish_fold(m, h, pre_quant_scale)
            iq = m.input_quantizer
            if h.is_input_quantized and iq.amax is not None:
                # :1257-1265: amax of the smoothed activation, the product taken in the weight dtype
                smooth = iq._amax_for_smoothing.to(device=m.weight.device, dtype=m.weight.dtype)
                iq.amax = (smooth * pre_quant_scale.to(m.weight.device)).amax().to(m.weight.dtype)
        self.stage("fold")

    def report(self):
        resc = [h for h in self.helpers.values() if h.contenders is not None]
        checked = [h for h in resc if h.tie_need is not None and h.margin_used and math.isfinite(h.margin_used)]
        self.stats.update({"linears": len(self.mods), "rescored_linears": len(resc),
                           "rescored_candidates": sum(len(h.contenders) for h in resc),
                           "tie_check": {"enabled": bool(self.tie_check), "spread_factor": TIE_SPREAD_FACTOR,
                                         "checked_linears": len(checked),
                                         "widened_linears": sum(1 for h in resc if h.tie_rounds),
                                         "max_need_over_margin": round(max((h.tie_need / h.margin_used for h in checked),
                                                                           default=0.0), 4),
                                         "max_need": max((h.tie_need for h in checked), default=0.0)}})
        self.stage("teardown")
        return self.helpers


@torch.no_grad()
def awq_lite(model: nn.Module, forward_loop, alpha_step: float = 0.1, search: str = "auto",
             tie_margin: float | None = None, tie_check: bool = True, layer_local: bool | None = None,
             store_activations: bool | str = "auto"):
    """AWQ-lite (model_calib.py:1394-1721) over every quantized linear whose weight quantizer is enabled (:1563-1567).
    INT-k static blocks along the last axis (INT4_AWQ_CFG, the first stage of W4A8_AWQ_BETA_CFG) take the fused kernels and
    the engines below; a linear in any other format (a per-layer override: per-tensor FP8, per-channel INT8, 2-D blocks, ...)
    takes the GENERIC route -- weight scale over its own blocks or whole rows, every candidate's scaled weight through the
    quantizer itself with the amax of its own layout, scored by the error-GEMM engine (AWQLiteHelper.fused).

    search = "gemm": the reference's structure -- two passes of forward_loop (cache: act scales; search: for every
             alpha the patched forward's GEMM, here one batched MFMA error-GEMM launch per linear and batch);
    search = "gram": ONE pass of forward_loop that also accumulates every linear's Gram matrix on the matrix cores
             (ops.hessian_accum); all alpha losses then come from trace(E G E^T) (see _gram_losses);
    search = "auto" (default): the Gram scores screen the candidates of every linear whose Gram matrix fits the HBM
             budget ("gemm" for the rest); candidates whose score lies within `tie_margin` (relative; default
             GRAM_TIE_MARGIN of the weight dtype) of the linear's best one are re-scored in a further pass by the
             error-GEMM engine -- the reference's arithmetic with all its roundings -- and the best alpha is the
             first minimum of THOSE scores, so that the selection equals search="gemm" (model_calib.py:1489-1495,
             :1548-1556, :1637).  Linears with a clear winner cost nothing extra; when no linear has a near-tie the
             extra pass is skipped.  tie_check (default on): the margin verifies itself against the measured
             disagreement of the two engines on the re-scored candidates and widens per linear when it was too
             small (TIE_SPREAD_FACTOR); AWQ_LITE_STATS["tie_check"] reports the largest requirement / margin ratio.

    store_activations: True -- the cache pass keeps every searched linear's input and `out_actual` of every batch (references,
             counted against the HBM budget); the exact pass then REPLAYS them linear by linear instead of running
             forward_loop again -- no second forward, no second library GEMM for out_actual.  Only a call whose
             activations fit can do that (one decoder layer: 36 GB for Llama-3-8B at 64 x 4096 tokens); when a
             reservation fails the stores are dropped and the pass is a real one.
             "inputs" -- only the INPUTS are kept, each distinct tensor object once (q / k / v and gate / up share theirs; a
             model fed the same tensors layer after layer shares them across layers); the replay recomputes `out_actual`
             with the linear's own un-folded weight, and only for the linears that have candidates to re-score.  A stored
             tensor that was written in place afterwards (its version counter moved) sends the pass back to a real forward.
             "auto" (default) = "inputs" for search="auto" when no other quantizer is enabled (their noise belongs to a real
             search pass), else off; an automatic store stops at half of what the HBM budget has left (the forward's own peak is
             not in that budget) and the pass is then a real one.  False = always a second forward.
    layer_local (None = for search="auto" on Hugging Face decoder stacks): the model is walked ONE DECODER LAYER AT A TIME
             (layerwise.py's contract: layer N+1's input is layer N's output): the layer's batches run through it once --
             statistics, Gram matrices, stored activations and the inputs of the next layer all come from that one
             run -- its linears are scored, their near-ties re-scored from the stores, the layer is folded, the next one
             follows.  One pass over the calibration data in total (`passes == 1`), same statistics as the whole-model
             flow (every layer sees the un-quantized output of its predecessor, as in the reference's cache pass)."""
    model_calib.refuse_rotation(model, "awq_lite")
    if forward_loop is None:  # (:1412-1414)
        warnings.warn("forward_loop must be provided for awq_lite; skipping awq_lite")
        return None
    if search not in ("auto", "gram", "gemm"):
        raise ValueError(f"awq_lite: unknown search mode {search!r}")
    if layer_local is None or layer_local:
        plan = _layer_local_plan(model, explicit=bool(layer_local)) if search == "auto" or layer_local else None
        if plan is not None:
            done = _awq_lite_layer_local(model, forward_loop, plan, alpha_step=alpha_step, search=search,
                                         tie_margin=tie_margin, tie_check=tie_check)
            if done is not None:
                return done
            plan = None  # the forward loop never called the first decoder layer (it feeds the linears itself): whole-model flow
        elif layer_local:
            raise ValueError("awq_lite(layer_local=True): the model has no decoder stack that holds every searched linear, "
                             "or other quantizers are enabled (their noise belongs to the search pass)")
    run = _AWQLiteRun(model, forward_loop, alpha_step, search, tie_margin, tie_check, store_activations)
    run.setup()  # helpers and weight scales, the HBM budget and Gram buffers, the store mode, the patched forwards
    try:
        run.cache_pass()  # forward_loop once: activation statistics, Gram matrices, stored activations
        run.statistics()  # amax syncs, act_scale, every candidate's scale vector
        run.scoring()  # Gram scores, the contenders, search / replay / exact passes, the late loss all-reduce
    finally:
        run.restore()  # the forwards go back, helpers / Gram matrices / stores are released
    run.fold()  # per linear: best alpha into weight and pre_quant_scale, or the neutral scale of a disabled one
    return run.report()
