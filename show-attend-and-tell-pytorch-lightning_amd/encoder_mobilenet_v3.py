"""MobileNetV3-Small encoder (model.py:38-39: ``get_encoder`` keeps ``m.features`` of torchvision's model, i.e. everything but the avgpool
and the classifier).  Same conventions as ``encoder_mobilenet.py``: the children hold parameters under torchvision's state-dict keys (``1.0.0.weight``
the stem convolution, ``1.<i>.block.<j>.*`` the inverted residuals with the squeeze-and-excitation layers at ``1.<i>.block.<j>.fc1`` / ``fc2``,
``1.12.*`` the last 1x1, ``2.*`` the optional projection); the layers run in ``libsat_hip.so`` on NHWC activations (fp32, or bf16 storage with
fp32 statistics / SE vectors / parameter gradients / master weights).

The network (Howard et al. 2019 table 2; torchvision 0.10 ``_mobilenet_v3_conf("mobilenet_v3_small")``): stem 3x3 stride 2 - BN - hard-swish,
eleven inverted residuals ``[1x1 expand - BN - act] - depthwise kxk - BN - act - [SE] - 1x1 project - BN (+ x when the block keeps shape)``, then a
1x1 to 576 channels - BN - hard-swish.  Every BatchNorm has eps = 1e-3, momentum = 0.01.  Kernels: 1x1 convolutions on the implicit-GEMM kernels
(BatchNorm statistics in their epilogue in bf16 mode); depthwise 3x3 ``csrc/depthwise.hip``, 5x5 ``csrc/depthwise5x5.hip``; ReLU layers = the
BatchNorm apply kernels with their sign mask; hard-swish layers and squeeze-and-excitation ``csrc/mobilenet_v3.hip``.  Every channel count,
squeeze widths included, is a multiple of 8.
"""
import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from . import encoder as E
from .encoder_shuffle import dw_dgrad, dw_fwd, dw_wgrad, stem3x3_fwd, stem3x3_wgrad

#: (input channels, kernel, expanded channels, output channels, squeeze-and-excitation, activation, stride) of the eleven inverted residuals
SETTING = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
           (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
           (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
           (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
LAST = 576


def _make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _bn(c):
    return nn.BatchNorm2d(c, eps=0.001, momentum=0.01)


def conv_bn_act(cin, cout, k=1, stride=1, groups=1, act="HS"):
    """torchvision's ConvBNActivation: Sequential(Conv2d (no bias), BatchNorm2d, activation)"""
    a = nn.Hardswish(inplace=True) if act == "HS" else (nn.ReLU(inplace=True) if act == "RE" else nn.Identity())
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), _bn(cout), a)


class SqueezeExcitation(nn.Module):
    """Parameter holder: fc1 (C -> S) and fc2 (S -> C), 1x1 convolutions with bias; S = _make_divisible(C // 4, 8)"""

    def __init__(self, c):
        super().__init__()
        s = _make_divisible(c // 4, 8)
        self.fc1 = nn.Conv2d(c, s, 1)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(s, c, 1)


class InvertedResidual(nn.Module):
    """Parameter holder with torchvision's layout: ``block`` = [expand ConvBNActivation (exp != in)], depthwise ConvBNActivation,
    [SqueezeExcitation], project ConvBNActivation (Identity activation)."""

    def __init__(self, cin, k, exp, cout, se, act, stride):
        super().__init__()
        self.stride, self.act, self.k = stride, act, k
        self.use_res_connect = stride == 1 and cin == cout
        layers = []
        if exp != cin:
            layers.append(conv_bn_act(cin, exp, 1, act=act))
        layers.append(conv_bn_act(exp, exp, k, stride, groups=exp, act=act))
        if se:
            layers.append(SqueezeExcitation(exp))
        layers.append(conv_bn_act(exp, cout, 1, act=None))
        self.block = nn.Sequential(*layers)

    def parts(self):
        """((expand conv, bn) or None, (depthwise conv, bn), SE module or None, (project conv, bn)) looked up once"""
        p = self.__dict__.get("_parts")
        if p is None:
            mods = list(self.block)
            ex = (mods[0][0], mods[0][1]) if mods[0][0].groups == 1 else None
            dwm = mods[1] if ex is not None else mods[0]
            se = mods[-2] if isinstance(mods[-2], SqueezeExcitation) else None
            p = self.__dict__["_parts"] = (ex, (dwm[0], dwm[1]), se, (mods[-1][0], mods[-1][1]))
        return p


# ----------------------------------------------------------------------------- raw layer calls
def _mom(bn):
    return 0.1 if bn.momentum is None else float(bn.momentum)


def bn_hs_fwd(x, bn, training, tiles=None):
    """BatchNorm + hard-swish of a (..., C) NHWC tensor: (y, (mean, invstd)) in training mode, (y, None) in eval mode"""
    lib = L.lib()
    Cc = x.shape[-1]; rows = x.numel() // Cc
    y = torch.empty_like(x)
    dt = int(E._is_bf(x))
    if not training:
        L.check(lib.sat_bn_hswish_eval_fwd_t(dt, L.ptr(x), rows, Cc, L.ptr(bn.running_mean), L.ptr(bn.running_var), float(bn.eps), L.ptr(bn.weight),
                                             L.ptr(bn.bias), L.ptr(y), L.stream_ptr()), "sat_bn_hswish_eval_fwd_t")
        return y, None
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device); invstd = torch.empty_like(mean)
    scratch = E._bn_scratch(x.device, rows, Cc)
    ts, tr = (tiles[0], int(tiles[1])) if (tiles is not None and dt == 1) else (None, 0)
    L.check(lib.sat_bn_hswish_train_fwd_t(dt, L.ptr(x), rows, Cc, L.ptr(ts), tr, L.ptr(bn.weight), L.ptr(bn.bias), float(bn.eps), _mom(bn),
                                          L.ptr(bn.running_mean), L.ptr(bn.running_var), L.ptr(mean), L.ptr(invstd), L.ptr(y), L.ptr(scratch),
                                          L.stream_ptr()), "sat_bn_hswish_train_fwd_t")
    if E._defer[0]:
        E._tracked.append(bn.num_batches_tracked)
    else:
        bn.num_batches_tracked += 1
    return y, (mean, invstd)


def bn_hs_bwd(dy, x, stats, bn):
    """gradient of ``bn_hs_fwd``: (dx, dgamma, dbeta); the pre-activation is recomputed from x and the BatchNorm's parameters"""
    lib = L.lib()
    Cc = x.shape[-1]; rows = x.numel() // Cc
    dx = torch.empty_like(x)
    dgamma, dbeta = L.grad_buffer(bn.weight), L.grad_buffer(bn.bias)
    scratch = E._bn_scratch(x.device, rows, Cc)
    L.check(lib.sat_bn_hswish_train_bwd_t(int(E._is_bf(x)), L.ptr(dy), L.ptr(x), rows, Cc, L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(bn.weight), L.ptr(bn.bias),
                                          L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.ptr(scratch), L.stream_ptr()), "sat_bn_hswish_train_bwd_t")
    return dx, dgamma, dbeta


def act_fwd(x, bn, act, training, tiles=None):
    """BatchNorm + ReLU (the apply kernels' sign mask) or BatchNorm + hard-swish"""
    if act == "HS":
        return bn_hs_fwd(x, bn, training, tiles=tiles)
    return E.bn_fwd(x, bn, None, True, training, want_mask=True, tiles=tiles)


def act_bwd(dy, x, y, stats, bn, act):
    if act == "HS":
        return bn_hs_bwd(dy, x, stats, bn)
    return E.bn_bwd(dy, x, y, stats, bn, True)


def _dw5_weight(conv):
    w = conv.weight
    assert w.dtype == torch.float32 and w.shape[1] == 1 and tuple(w.shape[2:]) == (5, 5)
    return w if (w.is_contiguous() or w.is_contiguous(memory_format=torch.channels_last)) else w.contiguous()      # (C, 1, 5, 5): [C][25] either way


def dw5_fwd(x, conv):
    N, H, W, Cc = x.shape
    s = conv.stride[0]
    y = torch.empty(N, (H + 4 - 5) // s + 1, (W + 4 - 5) // s + 1, Cc, dtype=x.dtype, device=x.device)
    L.check(L.lib().sat_dwconv5x5_fwd_t(int(E._is_bf(x)), L.ptr(x), L.ptr(_dw5_weight(conv)), L.ptr(y), N, H, W, Cc, s, L.stream_ptr()), "sat_dwconv5x5_fwd")
    return y


def dw5_dgrad(dy, conv, x_shape):
    N, H, W, Cc = x_shape
    dx = torch.empty(N, H, W, Cc, dtype=dy.dtype, device=dy.device)
    L.check(L.lib().sat_dwconv5x5_dgrad_t(int(E._is_bf(dy)), L.ptr(dy), L.ptr(_dw5_weight(conv)), L.ptr(dx), N, H, W, Cc, conv.stride[0], L.stream_ptr()),
            "sat_dwconv5x5_dgrad")
    return dx


_scratch = {}


def _scratch_buf(device, tag, nbytes):
    """one grown-on-demand fp32 buffer per (device, stream, tag): consecutive launches on a stream are ordered, so they can share it"""
    key = (device.index, L.stream_ptr().value, tag)
    buf = _scratch.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = _scratch[key] = torch.empty(max(nbytes // 4 + 1, 1 << 16), dtype=torch.float32, device=device)
    return buf


def dw5_wgrad(dy, x, conv):
    """fp32 gradient of the (C, 1, 5, 5) filter, written to the parameter's gradient buffer"""
    lib = L.lib()
    N, H, W, Cc = x.shape
    s = conv.stride[0]
    buf = _scratch_buf(x.device, "dw5", lib.sat_dwconv5x5_wgrad_scratch_bytes(N, H, W, Cc, s))
    out = L.grad_buffer(conv.weight)
    dense = out.is_contiguous() or out.is_contiguous(memory_format=torch.channels_last)
    dst = out if dense else torch.empty(Cc, 1, 5, 5, dtype=torch.float32, device=x.device)
    L.check(lib.sat_dwconv5x5_wgrad_t(int(E._is_bf(x)), L.ptr(dy), L.ptr(x), L.ptr(dst), N, H, W, Cc, s, L.ptr(buf), L.stream_ptr()), "sat_dwconv5x5_wgrad")
    return dst


def dwk_fwd(x, conv):
    return dw5_fwd(x, conv) if conv.kernel_size[0] == 5 else dw_fwd(x, conv)


def dwk_dgrad(dy, conv, x_shape):
    return dw5_dgrad(dy, conv, x_shape) if conv.kernel_size[0] == 5 else dw_dgrad(dy, conv, x_shape)


def dwk_wgrad(dy, x, conv):
    return dw5_wgrad(dy, x, conv) if conv.kernel_size[0] == 5 else dw_wgrad(dy, x, conv)


def _fc(conv):
    """(S, C, 1, 1) / (C, S, 1, 1) weight of a 1x1 layer as the dense row-major matrix the SE kernels read"""
    w = conv.weight
    return w if (w.is_contiguous() or w.is_contiguous(memory_format=torch.channels_last)) else w.contiguous()


def se_fwd(x, se):
    """squeeze-and-excitation of an NHWC tensor: (y, (pool, h, z2, s)) - the vectors the backward reads"""
    N, H, W, Cc = x.shape
    S = se.fc1.out_channels
    f32 = dict(dtype=torch.float32, device=x.device)
    pool, z2, s = torch.empty(N, Cc, **f32), torch.empty(N, Cc, **f32), torch.empty(N, Cc, **f32)
    h = torch.empty(N, S, **f32)
    y = torch.empty_like(x)
    L.check(L.lib().sat_se_fwd_t(int(E._is_bf(x)), L.ptr(x), N, H * W, Cc, S, L.ptr(_fc(se.fc1)), L.ptr(se.fc1.bias), L.ptr(_fc(se.fc2)), L.ptr(se.fc2.bias),
                                 L.ptr(pool), L.ptr(h), L.ptr(z2), L.ptr(s), L.ptr(y), L.stream_ptr()), "sat_se_fwd_t")
    return y, (pool, h, z2, s)


def se_bwd(dy, x, rec, se, grads):
    """gradient of ``se_fwd``: fills the four parameter gradients, returns dx"""
    lib = L.lib()
    N, H, W, Cc = x.shape
    S = se.fc1.out_channels
    pool, h, z2, s = rec
    buf = _scratch_buf(x.device, "se", lib.sat_se_bwd_scratch_bytes(N, Cc, S))
    dx = torch.empty_like(x)
    dw1, db1 = L.grad_buffer(se.fc1.weight), L.grad_buffer(se.fc1.bias)
    dw2, db2 = L.grad_buffer(se.fc2.weight), L.grad_buffer(se.fc2.bias)
    L.check(lib.sat_se_bwd_t(int(E._is_bf(x)), L.ptr(dy), L.ptr(x), N, H * W, Cc, S, L.ptr(_fc(se.fc1)), L.ptr(_fc(se.fc2)), L.ptr(pool), L.ptr(h), L.ptr(z2),
                             L.ptr(s), L.ptr(dx), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(db2), L.ptr(buf), L.stream_ptr()), "sat_se_bwd_t")
    grads[se.fc1.weight], grads[se.fc1.bias], grads[se.fc2.weight], grads[se.fc2.bias] = dw1, db1, dw2, db2
    return dx


# ----------------------------------------------------------------------------- blocks and the whole trunk
class _BRec:
    __slots__ = ("blk", "x", "ce", "ae", "se", "d", "ad", "sd", "serec", "yse", "cp", "sp")


def _block_fwd(blk, x, training, Wt):
    conv = E.conv_fwd_stats if training else (lambda *a: (E.conv_fwd(*a), None))
    ex, (dwc, dbn), se, (pc, pbn) = blk.parts()
    r = _BRec(); r.blk, r.x = blk, x
    h = x
    if ex is not None:
        r.ce, tl = conv(x, Wt(ex[0].weight), 1, 0)
        r.ae, r.se = act_fwd(r.ce, ex[1], blk.act, training, tiles=tl)
        h = r.ae
    r.d = dwk_fwd(h, dwc)
    r.ad, r.sd = act_fwd(r.d, dbn, blk.act, training)
    r.yse = r.ad
    if se is not None:
        r.yse, r.serec = se_fwd(r.ad, se)
    r.cp, tl = conv(r.yse, Wt(pc.weight), 1, 0)
    out, r.sp = E.bn_fwd(r.cp, pbn, x if blk.use_res_connect else None, False, training, tiles=tl)
    return r, out


def _bn_g(grads, bn, res):
    dx, grads[bn.weight], grads[bn.bias] = res
    return dx


def _block_bwd(r, dout, grads, Wt, need_dx=True):
    """dout: gradient of the block's output (owned by the caller chain: it is overwritten when the block has the identity path)."""
    blk = r.blk
    ex, (dwc, dbn), se, (pc, pbn) = blk.parts()
    dcp = _bn_g(grads, pbn, E.bn_bwd(dout, r.cp, None, r.sp, pbn, False))
    grads[pc.weight] = E.conv_wgrad(dcp, r.yse, pc.weight, 1, 0, param=pc.weight)
    dad = E.conv_dgrad(dcp, Wt(pc.weight), r.yse.shape, 1, 0)
    if se is not None:
        dad = se_bwd(dad, r.ad, r.serec, se, grads)
    dd = _bn_g(grads, dbn, act_bwd(dad, r.d, r.ad, r.sd, dbn, blk.act))
    h = r.ae if ex is not None else r.x
    grads[dwc.weight] = dwk_wgrad(dd, h, dwc)
    if ex is None:
        return dwk_dgrad(dd, dwc, h.shape) if need_dx else None          # the first block: no expansion, stride 2 (no identity path)
    dae = dwk_dgrad(dd, dwc, h.shape)
    dce = _bn_g(grads, ex[1], act_bwd(dae, r.ce, r.ae, r.se, ex[1], blk.act))
    grads[ex[0].weight] = E.conv_wgrad(dce, r.x, ex[0].weight, 1, 0, param=ex[0].weight)
    if not need_dx:
        return None
    if blk.use_res_connect:          # dx = data gradient + dout: accumulated onto dout in place
        return E.conv_dgrad(dce, Wt(ex[0].weight), r.x.shape, 1, 0, out=dout, accumulate=True)
    return E.conv_dgrad(dce, Wt(ex[0].weight), r.x.shape, 1, 0)


class MobileNetV3EncoderFn(torch.autograd.Function):
    """img (B,3,H,W) fp32 in [0,1] -> annotations (B,D,h,w) fp32 (NHWC memory); ``enc.precision`` as in ``encoder.EncoderFn``."""

    @staticmethod
    def forward(ctx, img, enc, *params):
        try:
            return MobileNetV3EncoderFn._forward(ctx, img, enc, *params)
        finally:
            E._defer[0] = False

    @staticmethod
    def _forward(ctx, img, enc, *params):
        L.require_gpu(img, *params)
        if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
            raise ValueError("encoder input must be (B,3,H,W) fp32 in [0,1]")
        img = img.contiguous()
        training = enc.training
        E._defer[0] = True; del E._tracked[:]
        bf = enc.precision == "bf16"
        t = {}
        Wt = E._weight_reader(bf)
        conv = E.conv_fwd_stats if training else (lambda *a: (E.conv_fwd(*a), None))
        (conv1, bn1), blocks, (convL, bnL) = enc.layers()
        t["x0"], t["wp"], t["c0"], tl = stem3x3_fwd(enc[0], conv1, img, bf, training)
        t["a0"], t["s0"] = bn_hs_fwd(t["c0"], bn1, training, tiles=tl)
        x = t["a0"]
        recs = []
        for blk in blocks:
            r, x = _block_fwd(blk, x, training, Wt)
            recs.append(r)
        t["xL"] = x
        t["cL"], tl = conv(x, Wt(convL.weight), 1, 0)
        t["aL"], t["sL"] = bn_hs_fwd(t["cL"], bnL, training, tiles=tl)
        x = E._head_fwd(enc, t["aL"], t, Wt, bf)
        E._defer[0] = False
        if E._tracked:
            torch._foreach_add_(E._tracked, 1)
            del E._tracked[:]
        ctx.t, ctx.recs, ctx.enc, ctx.Wt, ctx.bf = t, recs, enc, Wt, bf
        ctx.params = params
        return x.permute(0, 3, 1, 2)            # (B, D, h, w) view over NHWC memory

    @staticmethod
    def backward(ctx, dann):
        enc, t, recs, Wt, bf = ctx.enc, ctx.t, ctx.recs, ctx.Wt, ctx.bf
        grads = {}
        d = E._head_bwd(enc, t, dann, grads, Wt, bf)
        if enc.trunk_trainable:
            (conv1, bn1), _, (convL, bnL) = enc.layers()
            dcL = _bn_g(grads, bnL, bn_hs_bwd(d, t["cL"], t["sL"], bnL))
            grads[convL.weight] = E.conv_wgrad(dcL, t["xL"], convL.weight, 1, 0, param=convL.weight)
            d = E.conv_dgrad(dcL, Wt(convL.weight), t["xL"].shape, 1, 0)
            for r in reversed(recs):
                d = _block_bwd(r, d, grads, Wt)
            dc0 = _bn_g(grads, bn1, bn_hs_bwd(d, t["c0"], t["s0"], bn1))
            grads[conv1.weight] = stem3x3_wgrad(dc0, t["x0"], t["wp"], conv1, bf)
        ctx.t = ctx.recs = ctx.Wt = None
        return (None, None, *[grads.get(p) if p.requires_grad else None for p in ctx.params])


class HipMobileNetV3Encoder(nn.Sequential):
    Fn = MobileNetV3EncoderFn
    single_bucket = True          # data-parallel exchange: one bucket for the whole trunk (0.93 M parameters)

    def __init__(self, norm, features, proj, out_size):
        mods = [norm, features] + ([proj] if proj is not None else [])
        super().__init__(*mods)
        self.__dict__["proj"] = proj              # not registered twice: index 2 already owns it
        self.out_size = out_size
        self.precision = "fp32"

    @property
    def trunk_trainable(self):
        return any(p.requires_grad for p in self[1][0].parameters())

    def layers(self):
        """((stem conv, bn), [inverted residuals], (last conv, bn)) looked up once"""
        ls = self.__dict__.get("_layers")
        if ls is None:
            f = list(self[1])
            ls = self.__dict__["_layers"] = ((f[0][0], f[0][1]), f[1:-1], (f[-1][0], f[-1][1]))
        return ls

    def forward(self, img):
        params = self.__dict__.get("_plist")
        if params is None:
            params = self.__dict__["_plist"] = list(self.parameters())
        return MobileNetV3EncoderFn.apply(img, self, *params)

    def _apply(self, fn, *a, **k):
        self.__dict__.pop("_plist", None)
        return super()._apply(fn, *a, **k)


def _load_torchvision_trunk(path, features):
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    sd = {k: v for k, v in sd.items() if not k.startswith("classifier.")}          # model.py:39 drops the classifier
    holder = nn.Module()
    holder.features = features
    missing, unexpected = holder.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not k.endswith("num_batches_tracked")]
    if missing or unexpected:
        raise RuntimeError("pretrained checkpoint %s does not fit: missing %s, unexpected %s" % (path, missing[:5], list(unexpected)[:5]))


def _probe_zero_image(features, size):
    """model.py:46-48 pushes one all-zero image through the train-mode trunk: its only lasting effect is on the BatchNorm buffers.
    Initialisation-time host arithmetic on a single image (torch CPU ops), not part of the step."""
    with torch.no_grad():
        def seq(x, mods):
            for m in mods:
                if isinstance(m, nn.BatchNorm2d):
                    x = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps); m.num_batches_tracked += 1
                elif isinstance(m, nn.Conv2d):
                    x = F.conv2d(x, m.weight, None, m.stride, m.padding, 1, m.groups)
                elif isinstance(m, SqueezeExcitation):
                    s = F.conv2d(F.relu(F.conv2d(x.mean((2, 3), keepdim=True), m.fc1.weight, m.fc1.bias)), m.fc2.weight, m.fc2.bias)
                    x = x * F.hardsigmoid(s)
                elif isinstance(m, nn.Sequential):
                    x = seq(x, m)
                elif isinstance(m, nn.Hardswish):
                    x = F.hardswish(x)
                elif isinstance(m, nn.ReLU):
                    x = F.relu(x)
            return x
        x = torch.zeros(1, 3, size, size)
        for m in features:
            x = (x + seq(x, m.block) if m.use_res_connect else seq(x, m.block)) if isinstance(m, InvertedResidual) else seq(x, m)


def build_features():
    """torchvision's module construction order, the classifier the reference drops included (RNG stream), then its initialisers over
    every module in order.  Returns ``features``."""
    feats = [conv_bn_act(3, 16, 3, 2, act="HS")]
    for cfg in SETTING:
        feats.append(InvertedResidual(*cfg))
    feats.append(conv_bn_act(SETTING[-1][3], LAST, 1, act="HS"))
    features = nn.Sequential(*feats)
    classifier = nn.Sequential(nn.Linear(LAST, 1024), nn.Hardswish(inplace=True), nn.Dropout(p=0.2, inplace=True), nn.Linear(1024, 1000))
    for mod in list(features.modules()) + list(classifier.modules()):
        if isinstance(mod, nn.Conv2d):
            nn.init.kaiming_normal_(mod.weight, mode="fan_out")
            if mod.bias is not None:
                nn.init.zeros_(mod.bias)
        elif isinstance(mod, nn.BatchNorm2d):
            nn.init.ones_(mod.weight); nn.init.zeros_(mod.bias)
        elif isinstance(mod, nn.Linear):
            nn.init.normal_(mod.weight, 0, 0.01); nn.init.zeros_(mod.bias)
    return features


def get_mobilenet_v3_encoder(args):
    """Reference get_encoder (model.py:16-63) for mobilenet_v3_small (called by ``encoder.get_encoder``)."""
    ckpt = E._pretrained_file("mobilenet_v3_small", getattr(args, "pretrained", False))
    features = build_features()
    if ckpt is None:
        # model.py:46-48: the zero image of the shape probe.  Zero biases: every activation stays 0 (SE: hardsigmoid(0) = 0.5 times 0), every
        # BatchNorm sees an all-zero batch: running_var = 0.99 * 1 + 0.01 * 0
        for sub in features.modules():
            if isinstance(sub, nn.BatchNorm2d):
                sub.running_var.fill_(1.0 - _mom(sub)); sub.num_batches_tracked.fill_(1)
    else:
        _load_torchvision_trunk(ckpt, features)
        for prm in features.parameters():
            prm.requires_grad = False
        _probe_zero_image(features, int(args.input_size))
    s = int(args.input_size)
    for _ in range(5):                # the stem and four stride-2 blocks: 3x3 / 5x5 windows with (k - 1) / 2 padding, stride 2
        s = (s - 1) // 2 + 1
    proj = None
    if getattr(args, "encoder_dim", None) is not None and args.encoder_dim != LAST:
        proj = nn.Conv2d(LAST, args.encoder_dim, kernel_size=1, stride=1, bias=True)      # model.py:53
    else:
        args.encoder_dim = LAST
    es = getattr(args, "encoder_size", None)
    enc = HipMobileNetV3Encoder(E.Normalize(args.mean, args.std, inplace=True), features, proj, es if (es is not None and es != s) else None)
    E._channels_last_(enc)
    E._shadow_(enc)
    return enc
