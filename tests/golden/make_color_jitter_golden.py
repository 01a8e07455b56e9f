"""Generate tests/golden/g13_color_jitter.npz with the installed Pillow:

    python tests/golden/make_color_jitter_golden.py

Every picture goes through the reference's train transform up to ToTensor on PIL images: crop, resize(BILINEAR), the
optional mirror, then T.ColorJitter's four adjustments in a given order, each done the way torchvision's functional_pil
does it (ImageEnhance.Brightness / Contrast / Color, and adjust_hue's HSV round trip with a wrapping uint8 hue offset).
The fixture holds the inputs, the per-picture parameters and the expected bytes; nothing here needs torchvision.
"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
S = 24


def adjust_hue(img, hue_factor):
    """F_pil.adjust_hue"""
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.uint8(int(hue_factor * 255) % 256)                # uint8 addition wraps across the 0 / 255 boundary
    h = Image.fromarray(np_h, "L")
    return Image.merge("HSV", (h, s, v)).convert("RGB")


def pil_chain(img, box, flip, order, b, c, s, hue):
    t, l, ch, cw = box
    p = Image.fromarray(img).crop((l, t, l + cw, t + ch)).resize((S, S), Image.BILINEAR)
    if flip:
        p = p.transpose(Image.FLIP_LEFT_RIGHT)
    for op in order:
        if op == 0:
            p = ImageEnhance.Brightness(p).enhance(b)
        elif op == 1:
            p = ImageEnhance.Contrast(p).enhance(c)
        elif op == 2:
            p = ImageEnhance.Color(p).enhance(s)
        else:
            p = adjust_hue(p, hue)
    return np.asarray(p)


def main():
    rng = np.random.default_rng(13)
    perms = list(itertools.permutations(range(4)))
    n = len(perms) + 6
    arrs, boxes, flips, orders, factors, hues = {}, [], [], [], [], []
    ends = [0.0, 2.0, 0.6, 1.4, 1.0]                                  # x = 1 and x = 0.4 range ends, identity
    hue_choices = [-0.03, 0.0, 0.03]                                  # byte shifts -7, 0, +7
    for i in range(n):
        h, w = int(rng.integers(S // 2, 3 * S)), int(rng.integers(S // 2, 3 * S))
        kind = i % 6
        if kind == 0:
            img = np.full((h, w, 3), rng.integers(0, 256, 3), np.uint8)                      # flat colour
        elif kind == 1:
            img = np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, axis=2)    # grey
        elif kind == 2:
            img = rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255                       # saturated primaries
        else:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ch, cw = int(rng.integers(max(1, h // 2), h + 1)), int(rng.integers(max(1, w // 2), w + 1))
        box = (int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1)), ch, cw)
        order = perms[i % len(perms)]
        if i < 15:
            f = [ends[(i + k) % len(ends)] for k in range(3)]
        else:
            f = [float(np.float32(rng.uniform(0.0, 2.0))) for _ in range(3)]
        hue = hue_choices[i % 3] if i < 12 else float(np.float32(rng.uniform(-0.03, 0.03)))
        flip = int(i % 4 == 1)
        arrs["in%d" % i] = img
        arrs["out%d" % i] = pil_chain(img, box, flip, order, f[0], f[1], f[2], hue)
        boxes.append(box); flips.append(flip); orders.append(order); factors.append(f); hues.append(hue)
    arrs.update(size=np.int64(S), boxes=np.array(boxes, np.int64), flips=np.array(flips, np.int64), orders=np.array(orders, np.int64),
                factors=np.array(factors, np.float32), hue_factors=np.array(hues, np.float64),
                hue_shifts=np.array([int(h * 255) for h in hues], np.int64))
    np.savez_compressed(os.path.join(HERE, "g13_color_jitter.npz"), **arrs)


if __name__ == "__main__":
    main()
