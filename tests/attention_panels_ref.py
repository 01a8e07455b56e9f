"""CPU restatement of visualize.ipynb's make_visual and of util.py's load_square / prepare_image, with numpy and Pillow itself:
what sat_image_square_bicubic and sat_attention_panels (csrc/attention_panels.hip) must reproduce bit for bit.

* ``square`` / ``to_tensor``    crop_center's box arithmetic + ``Image.resize((size, size))`` (no filter: BICUBIC), ``T.ToTensor()``
* ``panels``                    numpy fp32 for the mask, ``Image.resize`` to enlarge it, ``Image.blend`` to lay it over the picture
* ``resample_int``              Pillow's BICUBIC resample in integers: oracle/image_oracle.py's restatement of Resample.c with its
                                "bicubic" filter; pins the kernel's arithmetic against Pillow without a GPU
* ``alpha_case`` / ``margin``   the attention maps the GPU test uses, generated from a seed, and the distance of every mask value
                                from a truncation boundary (tests/test_visualize.py asserts it for those very arrays)
"""
import io
import math

import numpy as np
from PIL import Image

from oracle import image_oracle as IO

#: (input (H, W), output size) pairs of the square tests; the last one has a side of exactly 32 x the output: 129 taps, the largest
#: shrink sat_image_square_bicubic accepts
SQUARE_CASES = [((7, 7), 32), ((14, 14), 256), ((5, 7), 32), ((1, 1), 8), ((1, 5), 16), ((37, 37), 16), ((61, 45), 32), ((480, 640), 256),
                ((256, 256), 224), ((32, 32), 32), ((128, 130), 4)]
#: (input (H, W), output (H, W)) pairs of the integer restatement: the list above, 5 x 7 as the mask path resizes it (no crop)
RESAMPLE_CASES = [((7, 7), (32, 32)), ((14, 14), (256, 256)), ((5, 7), (32, 32)), ((1, 1), (8, 8)), ((1, 5), (16, 16)), ((37, 37), (16, 16)),
                  ((45, 45), (32, 32)), ((480, 480), (256, 256)), ((256, 256), (224, 224)), ((32, 32), (32, 32)), ((128, 128), (4, 4))]


def picture(h, w, seed, channels=3):
    """a smooth gradient plus noise: every byte value, edges and flat parts"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = [(xx * 255.0 / max(w - 1, 1)), (yy * 255.0 / max(h - 1, 1)), ((xx + yy) % 64) * 4.0][:channels]
    a = np.stack(base, -1) + rs.randint(-40, 41, (h, w, channels))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a if channels > 1 else a[..., 0]


# ---------------------------------------------------------------------------------------------------------------- load_square
def crop_box(h, w):
    """util.py's crop_center(img, s, s) with s = min side: Pillow's (left, upper, right, lower)"""
    s = min(h, w)
    return ((w - s) // 2, (h - s) // 2, (w + s) // 2, (h + s) // 2)


def square(a, size):
    """crop_max_square of an (H, W, 3) uint8 array -> (size, size, 3) uint8"""
    img = Image.fromarray(a).crop(crop_box(a.shape[0], a.shape[1]))
    if size:
        img = img.resize((size, size))
    return np.asarray(img)


def to_tensor(sq):
    """T.ToTensor() of an (S, S, 3) uint8 picture: (3, S, S) float32, byte / 255"""
    return np.ascontiguousarray(sq.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


# ---------------------------------------------------------------------------------------------------------------- the integers
def resample_int(a, out_h, out_w):
    """``Image.resize((out_w, out_h), BICUBIC)`` of an (H, W) or (H, W, C) uint8 array"""
    return IO.resample_u8(np.asarray(a), out_h, out_w, "bicubic")


def blend_rule(p, m):
    """the overlay at opacity 0.75 in integers"""
    return (p + 3 * m) // 4


# ---------------------------------------------------------------------------------------------------------------- the panels
def mask_bytes(att, hw, power=None):
    """one (h * w,) float32 attention map -> the (h, w) uint8 mask: the notebook's numpy arithmetic; a flat map gives zeros"""
    att = np.asarray(att, np.float32).reshape(hw)
    mn, mx = np.min(att), np.max(att)
    if mx == mn:
        return np.zeros(hw, np.uint8)
    x = (att - mn) / (mx - mn)
    if power is not None:
        x = x ** power
    return np.uint8(x * 255)


def panels(sq, alpha, n, hw, power=5.0, opacity=0.75):
    """the (Tmax + 2, V, V, 3) panels of one picture: ``sq`` (V, V, 3) uint8, ``alpha`` (Tmax, h * w) float32, ``n`` caption length"""
    alpha = np.asarray(alpha, np.float32)
    V = sq.shape[0]
    out = np.zeros((alpha.shape[0] + 2, V, V, 3), np.uint8)
    out[0] = sq
    pic = Image.fromarray(sq)
    for t in range(n):
        mask = Image.fromarray(mask_bytes(alpha[t], hw, power)).convert("RGB").resize((V, V))
        out[1 + t] = np.asarray(Image.blend(pic, mask, opacity))
    total = alpha[:n].sum(0) if n else np.zeros(alpha.shape[1], np.float32)
    out[n + 1] = np.asarray(Image.fromarray(mask_bytes(total, hw)).convert("RGB").resize((V, V)))
    return out


#: name -> (seed, B, Tmax, V, (h, w), caption lengths, power, opacity): the cases of the GPU test.  The seeds are chosen so that
#: ``margin`` holds (tests/test_visualize.py asserts it); change one and that test says whether the new one will do.
PANEL_CASES = {
    "14x14_p5": (1, 3, 6, 32, (14, 14), (0, 1, 6), 5.0, 0.75),
    "7x7_p1": (1, 3, 6, 32, (7, 7), (0, 1, 6), 1.0, 0.5),
    "5x7_p5": (1, 3, 6, 32, (5, 7), (6, 0, 1), 5.0, 0.5),
    "1x1_flat": (1, 3, 6, 32, (1, 1), (0, 1, 6), 5.0, 0.75),
    "14x14_v256": (2, 3, 6, 256, (14, 14), (1, 6, 0), 5.0, 0.75),
}
MARGIN = 2e-4


def alpha_case(name):
    """(squares (B, V, V, 3) uint8, alpha (B, Tmax, h * w) float32 rows summing to one like a softmax, lengths (B,) int32)"""
    seed, B, Tmax, V, (h, w), lens, _, _ = PANEL_CASES[name]
    rs = np.random.RandomState(seed)
    e = rs.rand(B, Tmax, h * w).astype(np.float32) ** 3
    alpha = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    squares = np.stack([picture(V, V, seed * 100 + b) for b in range(B)])
    return squares, alpha, np.asarray(lens, np.int32)


def margin(att, power):
    """smallest distance of the exact (float64) 255 * x ** power of the map ``att`` from an integer k >= 1, over the elements that
    can flip: not the endpoints x = 0 and x = 1 (exact in any arithmetic).  inf for a flat map."""
    a = np.asarray(att, np.float64)
    mn, mx = a.min(), a.max()
    if mx == mn:
        return math.inf
    x = (a - mn) / (mx - mn)
    v = 255.0 * x ** power
    k = np.rint(v)
    live = (a != mn) & (a != mx) & (k >= 1)
    return float(np.abs(v - k)[live].min()) if live.any() else math.inf


def case_margin(name):
    """the smallest ``margin`` over every step map and every total of a case"""
    _, B, _, _, _, lens, power, _ = PANEL_CASES[name]
    _, alpha, _ = alpha_case(name)
    worst = math.inf
    for b in range(B):
        n = int(lens[b])
        for t in range(n):
            worst = min(worst, margin(alpha[b, t], power))
        if n:
            worst = min(worst, margin(alpha[b, :n].astype(np.float64).sum(0), 1.0))
    return worst


def jpeg_bytes(a, quality=90):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def png_bytes(a):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="PNG")
    return buf.getvalue()
