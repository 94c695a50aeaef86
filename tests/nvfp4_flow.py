"""TEST INFRASTRUCTURE: the static-NVFP4 calibration flows checked step by step against the bit-pinned restatements of
tests/nvfp4_host.py (shared by tests/test_nvfp4_static_cpu.py and tests/test_gpu_nvfp4_static.py)."""

import copy

import torch

import nvfp4_host as nh


class Block(torch.nn.Module):
    """An attention-plus-MLP block with the projection names the fusible-sibling groups key on."""

    def __init__(self, d=64, f=96):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (torch.nn.Linear(d, d, bias=False) for _ in range(3))
        self.o_proj = torch.nn.Linear(d, d, bias=False)
        self.gate_proj, self.up_proj = torch.nn.Linear(d, f, bias=False), torch.nn.Linear(d, f, bias=False)
        self.down_proj = torch.nn.Linear(f, d, bias=False)

    def forward(self, x):
        a = self.o_proj(self.q_proj(x) * torch.sigmoid(self.k_proj(x)) + self.v_proj(x))
        return self.down_proj(torch.nn.functional.silu(self.gate_proj(a)) * self.up_proj(a))


class Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = torch.nn.ModuleList([Block(), Block()])

    def forward(self, x):
        for b in self.layers:
            x = b(x)
        return x


LINEARS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
GROUPS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"), ("o_proj",), ("down_proj",))


def make(device, dtype, seed=3):
    torch.manual_seed(seed)
    m = Model()
    for p in m.parameters():
        p.data.mul_(3.0)
        p.data[:, ::7] *= 4.0  # outlier input channels: block amax far below the global one
    batches = [torch.randn(8, 64) for _ in range(3)]
    return m.to(device=device, dtype=dtype), [b.to(device=device, dtype=dtype) for b in batches]


def check(moa, cfg_name, device, dtype):
    """Quantize with the preset, then check every weight quantizer: global amax = max of its sibling group's block amax,
    block amax = the sweep's pick, output = the static QDQ of the weight."""
    model, batches = make(device, dtype)
    ref_model = copy.deepcopy(model)
    cfg = copy.deepcopy(getattr(moa.model_quant, cfg_name))
    hess = None
    if "HESSIAN" in cfg_name:
        # the per-block Hessians the flow accumulated (the accumulator is pinned to the reference's run by
        # tests/test_local_hessian_cpu.py); the inputs of later linears depend on the quantized inputs before them
        cfg["algorithm"]["debug"] = True
    moa.quantize(model, cfg, lambda m: [m(b) for b in batches])
    hess = "HESSIAN" in cfg_name or None
    for li, (layer, ref_layer) in enumerate(zip(model.layers, ref_model.layers)):
        for group in GROUPS:
            block_max = [getattr(ref_layer, n).weight.float().reshape(-1, 16).abs().amax(1) for n in group]
            g = torch.stack([a.max() for a in block_max]).max()
            for n in group:
                wq = getattr(layer, n).weight_quantizer
                assert wq.is_nvfp4_static and wq.has_quantized_block_scale, n
                assert wq.global_amax is not None and wq.global_amax.dtype == torch.float32
                assert torch.equal(wq.global_amax.reshape(()), g), f"layer {li} {n}: global amax"
                w = getattr(ref_layer, n).weight
                if hess is None:
                    want = nh.sweep(w, g)
                else:
                    h = model._local_hessian_accumulators[id(wq)].normalized_hessian()
                    want = nh.sweep_hessian(w, g, h)
                got = wq._amax.float().reshape(-1)
                assert torch.equal(got, want), f"layer {li} {n}: {(got != want).sum().item()} block amax differ"
                wq_out = wq(w)
                assert nh.bits_equal(wq_out, nh.static_qdq(w, want, g)), f"layer {li} {n}: static QDQ"
                # the search moved some blocks away from their max
                assert bool((want != block_max[group.index(n)]).any())
    return model
