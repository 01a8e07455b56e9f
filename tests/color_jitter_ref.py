"""Test-side restatement of torchvision's ColorJitter on PIL images (T.ColorJitter, F_pil.adjust_brightness / contrast /
saturation / hue) as the arithmetic Pillow performs, in numpy.  The GPU kernels are checked against this module and against
Pillow itself (tests/golden/g13_color_jitter.npz); this module is checked against Pillow exhaustively where the domain allows.

Every function takes and returns uint8 arrays; pictures are (H, W, 3) RGB.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def luma(rgb):
    """Image.convert("L") of RGB bytes: ITU-R 601-2 in 16-bit fixed point."""
    rgb = rgb.astype(np.int64)
    return ((rgb[..., 0] * 19595 + rgb[..., 1] * 38470 + rgb[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, img, factor):
    """Image.blend(degenerate, img, factor) per byte: d + f * (img - d) in float32, each operation rounded on its own,
    truncated toward zero, clipped to [0, 255]."""
    d = np.asarray(d).astype(F32)
    t = d + F32(factor) * (np.asarray(img).astype(F32) - d)
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def contrast_mean(img):
    """ImageEnhance.Contrast's degenerate grey level: int(mean of L over the picture + 0.5), the mean taken as the exact
    integer sum over the pixel count in double."""
    s = int(luma(img).astype(np.int64).sum())
    return int(F64(s) / F64(luma(img).size) + 0.5)


def contrast(img, f):
    return blend(np.full(img.shape[:2] + (1,), contrast_mean(img), np.uint8), img, f)


def rgb_to_hsv(rgb):
    """Image.convert("HSV") of RGB bytes (Pillow's rgb2hsv: float32 ratios, double hue offsets and the fmod)."""
    rgb = rgb.astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(-1), rgb.min(-1)
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(F32)
    s = cr / np.where(mx == 0, 1, mx).astype(F32)
    rc, gc, bc = [(mx - c).astype(F32) / cr for c in (r, g, b)]
    h = np.where(r == mx, (bc - gc).astype(F64),
                 np.where(g == mx, F64(2.0) + rc.astype(F64) - bc.astype(F64), F64(4.0) + gc.astype(F64) - rc.astype(F64))).astype(F32)
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    H = np.clip(np.trunc(h.astype(F64) * 255.0), 0, 255).astype(np.int64)
    S = np.clip(np.trunc(s.astype(F64) * 255.0), 0, 255).astype(np.int64)
    H, S = np.where(flat, 0, H), np.where(flat, 0, S)
    return np.stack([H, S, mx], -1).astype(np.uint8)


def _round_half_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def hsv_to_rgb(hsv):
    """Image.convert("RGB") of HSV bytes (Pillow's hsv2rgb)."""
    hsv = hsv.astype(np.int64)
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    x = H.astype(F32).astype(F64) * 6.0 / 255.0
    i = np.floor(x)
    f = (x - i).astype(F32)
    fs = (S.astype(F32).astype(F64) / 255.0).astype(F32)
    v = V.astype(F32).astype(F64)
    p = np.clip(_round_half_away(v * (1.0 - fs.astype(F64))), 0, 255).astype(np.int64)
    q = np.clip(_round_half_away(v * (1.0 - (fs * f).astype(F64))), 0, 255).astype(np.int64)
    t = np.clip(_round_half_away(v * (1.0 - fs.astype(F64) * (1.0 - f.astype(F64)))), 0, 255).astype(np.int64)
    i = i.astype(np.int64) % 6
    cases = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.zeros(hsv.shape, np.int64)
    for k, (a, b, c) in enumerate(cases):
        m = i == k
        out[..., 0] = np.where(m, a, out[..., 0])
        out[..., 1] = np.where(m, b, out[..., 1])
        out[..., 2] = np.where(m, c, out[..., 2])
    out = np.where((S == 0)[..., None], V[..., None], out)
    return out.astype(np.uint8)


def hue_shift_byte(hue_factor):
    """F_pil.adjust_hue's byte offset: hue * 255 truncated toward zero, as a wrapping uint8 (-7.65 -> -7 -> 249)."""
    return int(np.trunc(F64(hue_factor) * 255.0))


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + shift) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


def jitter(img, order, b, c, s, shift):
    """T.ColorJitter.forward: the four adjustments in ``order`` (0 brightness, 1 contrast, 2 saturation, 3 hue)."""
    for op in order:
        if op == 0:
            img = brightness(img, b)
        elif op == 1:
            img = contrast(img, c)
        elif op == 2:
            img = saturation(img, s)
        else:
            img = hue(img, shift)
    return img
