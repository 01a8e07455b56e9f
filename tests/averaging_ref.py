"""Reference for the averaged-weights tests ("Averaged weights"): torch's own optimizers on the CPU.  ``kind="asgd"`` is
``torch.optim.ASGD``; an exponential moving average beside SGD / Adam / AdamW is ``Tensor.lerp_`` after ``torch.optim.*.step()``, started
as a copy (what ``torch.optim.swa_utils.AveragedModel`` does on its first update)."""
import torch

#: the shapes of tests/test_gpu_optimizer.py plus the ones where the averaging kernel can newly go wrong: chunk boundaries at 65536
#: elements (one element short of / past a chunk), sizes that are no multiple of the 4-element vector, one element, two dimensions
SHAPES = [(5,), (70001,), (33, 17), (200, 300), (64, 3, 3, 8), (1,), (131073,), (65536,), (65537,)]
BOUND = 2e-6            # of max(1, |ref|max): the bound of tests/test_gpu_optimizer.py


def groups(ps):
    """the three groups of tests/test_gpu_optimizer.py"""
    return [{"params": ps[:2], "lr": 1e-2, "weight_decay": 0.0}, {"params": ps[2:4], "lr": 3e-3, "weight_decay": 0.05},
            {"params": ps[4:], "lr": 1e-3, "weight_decay": 0.0}]


def make_params(seed=7):
    """CPU leaves: SHAPES, then a channels_last (64, 8, 3, 3) filter, then a 4099-element leaf (the device twin of the last one is a view at
    storage offset 1: ``device_twins``)"""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    ps.append(torch.randn(64, 8, 3, 3, generator=g).contiguous(memory_format=torch.channels_last))
    ps.append(torch.randn(4099, generator=g))
    return [p.requires_grad_() for p in ps], g


def device_twins(ref):
    """the same leaves on the GPU: the filter carries a bf16 copy (``_sat_bf16_shadow``), the last leaf is a view at storage offset 1, so
    its data is only 4-byte aligned while its freshly allocated average is 16-byte aligned"""
    dev = [p.detach().clone().cuda().requires_grad_() for p in ref[:-1]]
    base = torch.empty(ref[-1].numel() + 1, device="cuda")
    base[1:].copy_(ref[-1].detach())
    dev.append(base[1:].requires_grad_())
    assert dev[-1].data_ptr() % 16 == 4 and dev[-1].is_leaf
    f = dev[-2]
    assert f.is_contiguous(memory_format=torch.channels_last) and not f.is_contiguous()
    f._sat_bf16_shadow = f.detach().to(torch.bfloat16)
    f._sat_shadow_version = f._version
    return dev


def torch_optimizer(kind, params, **kw):
    if kind == "asgd":
        return torch.optim.ASGD(params, lr=1e-2, lambd=kw.get("lambd", 1e-4), alpha=kw.get("alpha", 0.75), t0=kw.get("t0", 1e6))
    if kind == "sgd":
        return torch.optim.SGD(params, lr=1e-2, momentum=0.9, nesterov=True)
    if kind == "adam":
        return torch.optim.Adam(params, lr=1e-2, betas=(0.8, 0.95))
    return torch.optim.AdamW(params, lr=1e-2, betas=(0.8, 0.95))


def clip(params, how):
    """Lightning's clipping before the step; returns the norm when clipping by norm"""
    if how and how[0] == "norm":
        return torch.nn.utils.clip_grad_norm_(params, how[1])
    if how:
        torch.nn.utils.clip_grad_value_(params, how[1])
    return None


class Ema:
    """``ema = ema + (p - ema) * c`` after every step, c = 1 on the first one (a copy), 1 - decay afterwards"""

    def __init__(self, params, decay):
        self.params, self.decay, self.avg, self.steps = list(params), decay, None, 0

    @torch.no_grad()
    def update(self):
        self.steps += 1
        if self.avg is None:
            self.avg = [p.detach().clone() for p in self.params]
        else:
            for a, p in zip(self.avg, self.params):
                a.lerp_(p.detach(), 1.0 - self.decay)


def within(dev_t, ref_t, what):
    err = float((dev_t.detach().cpu() - ref_t.detach()).abs().max())
    bound = BOUND * max(1.0, float(ref_t.detach().abs().max()))
    print("%s: max|d| = %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err, bound)
