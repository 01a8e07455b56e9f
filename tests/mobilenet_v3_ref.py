"""TEST INFRASTRUCTURE ONLY -- the CPU restatement of torchvision 0.10's mobilenet_v3_small and of the reference's ``get_encoder`` for it
(model.py:38-39 keeps ``features``).  ``oracle/`` stays as it is, so the restatement lives here.

Sources: Howard et al. 2019, "Searching for MobileNetV3", table 2, and torchvision 0.10's ``_mobilenet_v3_conf("mobilenet_v3_small")``:
stem Conv 3 -> 16, 3x3, stride 2 - BN - Hardswish; eleven InvertedResidual blocks (``.block`` = [expand ConvBNActivation if exp != in],
depthwise kxk ConvBNActivation, [SqueezeExcitation], project ConvBNActivation with an Identity activation; identity path when stride 1 and
in == out); last Conv 96 -> 576, 1x1 - BN - Hardswish.  SqueezeExcitation(C): s = hardsigmoid(fc2(relu(fc1(mean_hw x)))), output x * s,
fc1 / fc2 1x1 Conv2d with bias, squeeze width _make_divisible(C // 4, 8).  Every BatchNorm is BatchNorm2d(eps = 0.001, momentum = 0.01).
Initialisation (after constructing the classifier the reference drops, for the RNG stream): Conv2d kaiming_normal_(fan_out), bias zeros;
BatchNorm ones / zeros; Linear normal_(0, 0.01), bias zeros.

``build_encoder(hp)`` restates ``oracle.sat_oracle.build_encoder`` for "mobilenet_v3_small" (Normalize, features, optional 1x1 projection,
optional resize, after the zero-image probe of model.py:46-48) and hands every other arch to the original.

``encoder_forward(enc, img)``: the same network with bf16 ROUNDING AT THE STORAGE POINTS OF THE HIP PATH (encoder_mobilenet_v3.py):
  the normalised image -> bf16;
  every convolution output -> bf16 (its gradient is stored bf16 too); the stem and the 1x1 convolutions read bf16 copies of their fp32
    filters (their gradients stay fp32); the depthwise 3x3 / 5x5 convolutions read the fp32 filters;
  every BatchNorm(+ residual)(+ ReLU | hard-swish) output -> bf16 (its gradient, a data-gradient output, is stored bf16 too);
  squeeze-and-excitation: pooled means, both 1x1 layers and the scale s in fp32 with the fp32 parameters, the output x * s -> bf16 (its
    gradient bf16 too);
  the optional 1x1 projection: bf16 x bf16 -> fp32 annotations + fp32 bias, its incoming gradient cast to bf16; the resize in fp32.
Only ``oracle.bf16_emulation.bf`` is reused."""
import torch
import torch.nn.functional as F
from torch import nn

from oracle import sat_oracle as O
from oracle.bf16_emulation import bf

_ORIGINAL_BUILD_ENCODER = O.build_encoder

#: (input channels, kernel, expanded channels, output channels, SE, activation, stride)
SMALL = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
         (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
         (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
         (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))


def make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def conv_bn_activation(cin, cout, k, stride=1, groups=1, act=nn.Hardswish):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout, eps=0.001, momentum=0.01),
                         act(inplace=True) if act is not nn.Identity else nn.Identity())


class SqueezeExcitationRef(nn.Module):
    def __init__(self, c):
        super().__init__()
        s = make_divisible(c // 4, 8)
        self.fc1 = nn.Conv2d(c, s, 1)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(s, c, 1)

    def scale(self, x):
        return F.hardsigmoid(self.fc2(self.relu(self.fc1(F.adaptive_avg_pool2d(x, 1)))))

    def forward(self, x):
        return self.scale(x) * x


class InvertedResidualRef(nn.Module):
    def __init__(self, cin, k, exp, cout, se, act, stride):
        super().__init__()
        a = nn.Hardswish if act == "HS" else nn.ReLU
        self.use_res_connect = stride == 1 and cin == cout
        layers = []
        if exp != cin:
            layers.append(conv_bn_activation(cin, exp, 1, act=a))
        layers.append(conv_bn_activation(exp, exp, k, stride, groups=exp, act=a))
        if se:
            layers.append(SqueezeExcitationRef(exp))
        layers.append(conv_bn_activation(exp, cout, 1, act=nn.Identity))
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        y = self.block(x)
        return y + x if self.use_res_connect else y


class MobileNetV3SmallOracle(nn.Module):
    """Children: features, avgpool, classifier - the reference keeps ``features`` (model.py:38-39)."""

    def __init__(self, num_classes=1000):
        super().__init__()
        feats = [conv_bn_activation(3, 16, 3, 2)]
        for cfg in SMALL:
            feats.append(InvertedResidualRef(*cfg))
        feats.append(conv_bn_activation(96, 576, 1))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(576, 1024), nn.Hardswish(inplace=True), nn.Dropout(p=0.2, inplace=True), nn.Linear(1024, num_classes))
        self.feature_dim = 576
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight); nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01); nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


def trunk_param_count():
    net = MobileNetV3SmallOracle()
    return sum(p.numel() for n, p in net.named_parameters() if not n.startswith("classifier.")), net.feature_dim


def build_encoder(hp):
    """oracle.sat_oracle.build_encoder with the mobilenet_v3_small branch (keys: 1.<i>.* features, 2.* 1x1 projection)"""
    if hp.encoder_arch != "mobilenet_v3_small":
        return _ORIGINAL_BUILD_ENCODER(hp)
    net = MobileNetV3SmallOracle()
    trunk = [net.features]
    probe = nn.Sequential(*trunk)(torch.zeros(1, 3, hp.input_size, hp.input_size))          # model.py:46-48
    final_dim, final_size = probe.shape[1], probe.shape[-1]
    if getattr(hp, "encoder_dim", None) is not None and hp.encoder_dim != final_dim:
        trunk.append(nn.Conv2d(final_dim, hp.encoder_dim, kernel_size=1, stride=1, bias=True))
    else:
        hp.encoder_dim = final_dim
    es = getattr(hp, "encoder_size", None)
    if es is not None:
        if es < final_size:
            trunk.append(nn.AdaptiveAvgPool2d((es, es)))
        elif es > final_size:
            trunk.append(nn.Upsample((es, es), mode="bilinear", align_corners=False))
    return nn.Sequential(O.NormalizeInplace(hp.mean, hp.std, inplace=True), *trunk)


# ----------------------------------------------------------------------------- bf16 storage emulation
class _RoundBoth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return bf(x)

    @staticmethod
    def backward(ctx, g):
        return bf(g)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return bf(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return bf(g)


rb, rf, rg = _RoundBoth.apply, _RoundFwd.apply, _RoundBwd.apply


def _conv(x, conv):
    w = rf(conv.weight) if conv.groups == 1 else conv.weight
    return rb(F.conv2d(x, w, None, conv.stride, conv.padding, 1, conv.groups))


def _bn_act(x, bn, act, residual=None):
    y = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
    if bn.training:
        bn.num_batches_tracked += 1
    if residual is not None:
        y = y + residual
    if isinstance(act, nn.Hardswish):
        y = F.hardswish(y)
    elif isinstance(act, nn.ReLU):
        y = F.relu(y)
    return rb(y)


def block_forward(blk, x):
    """one InvertedResidualRef with the storage rounding of the HIP path; the identity path is added inside the last BatchNorm"""
    h = x
    mods = list(blk.block)
    for i, m in enumerate(mods):
        if isinstance(m, SqueezeExcitationRef):
            h = rb(m.scale(h) * h)
        else:
            res = x if (i == len(mods) - 1 and blk.use_res_connect) else None
            h = _bn_act(_conv(h, m[0]), m[1], m[2], res)
    return h


def encoder_forward(enc, img):
    """``enc`` = build_encoder(hp) for mobilenet_v3_small; img (B, 3, H, W) fp32 in [0, 1] -> annotations (B, D, h, w) fp32"""
    mods = list(enc.children())
    norm = mods[0]
    m = torch.as_tensor(norm.mean, dtype=torch.float32).view(1, -1, 1, 1); s = torch.as_tensor(norm.std, dtype=torch.float32).view(1, -1, 1, 1)
    x = bf((img - m) / s)
    feats = list(mods[1])
    x = _bn_act(_conv(x, feats[0][0]), feats[0][1], feats[0][2])
    for blk in feats[1:-1]:
        x = block_forward(blk, x)
    x = _bn_act(_conv(x, feats[-1][0]), feats[-1][1], feats[-1][2])
    for mod in mods[2:]:
        if isinstance(mod, nn.Conv2d):
            x = rg(F.conv2d(x, rf(mod.weight), None)) + mod.bias.view(1, -1, 1, 1)
        else:
            x = mod(x)
    return x
