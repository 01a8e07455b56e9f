"""Generate tests/golden/g14_optical.npz with the installed Pillow:

    python tests/golden/make_optical_golden.py

Every picture goes through the reference's train transform up to ToTensor on PIL images: crop, resize(BILINEAR), the
optional mirror, the optional T.ColorJitter (ImageEnhance / adjust_hue in a given order), then one of the three "optical"
transforms of train.py:225-231 the way torchvision's functional_pil hands it to Pillow:

    RandomPerspective   Image.transform(size, PERSPECTIVE, coeffs, BILINEAR, fillcolor=(0, 0, 0))
    RandomAffine        Image.transform(size, AFFINE, matrix, NEAREST, fillcolor=(0, 0, 0))
    RandomRotation      Image.rotate(angle, NEAREST, fillcolor=(0, 0, 0))

The perspective coefficients and the affine matrix are torchvision's rules (tests/optical_ref.py); the rotation matrix is
Pillow's own.  The fixture holds the inputs, the per-picture parameters, the coefficients of the warp record and the expected
bytes; nothing here needs torchvision.
"""
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import optical_ref as R  # noqa: E402

S = 37
PERSPECTIVE, AFFINE, ROTATION = 0, 1, 2          # T.RandomChoice index


def adjust_hue(img, hue_shift):
    """F_pil.adjust_hue with its byte offset"""
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.uint8(hue_shift % 256)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_chain(img, box, flip, jitter, choice, param):
    t, l, ch, cw = box
    p = Image.fromarray(img).crop((l, t, l + cw, t + ch)).resize((S, S), Image.BILINEAR)
    if flip:
        p = p.transpose(Image.FLIP_LEFT_RIGHT)
    if jitter is not None:
        order, (b, c, s), shift = jitter
        for op in order:
            if op == 0:
                p = ImageEnhance.Brightness(p).enhance(b)
            elif op == 1:
                p = ImageEnhance.Contrast(p).enhance(c)
            elif op == 2:
                p = ImageEnhance.Color(p).enhance(s)
            else:
                p = adjust_hue(p, shift)
    if choice == ROTATION:
        return np.asarray(p.rotate(param, Image.NEAREST, fillcolor=(0, 0, 0)))
    kind = Image.PERSPECTIVE if choice == PERSPECTIVE else Image.AFFINE
    return np.asarray(p.transform((S, S), kind, tuple(param), Image.BILINEAR if choice == PERSPECTIVE else Image.NEAREST, fillcolor=(0, 0, 0)))


def main():
    rng = np.random.default_rng(14)
    gen = torch.Generator().manual_seed(14)
    dmax = int(1.0 * 0.5 * (S // 2))
    # s = 1 corner draws: the ends of every randint range, the ends of the angle and shear ranges
    far = [[dmax, dmax], [S - dmax - 1, dmax], [S - dmax - 1, S - dmax - 1], [dmax, S - dmax - 1]]
    near = [[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]]
    mixed = [[0, dmax], [S - 1, dmax], [S - dmax - 1, S - 1], [dmax, S - 1]]
    corner = {0: (PERSPECTIVE, far), 1: (AFFINE, (45.0, 45.0)), 2: (ROTATION, 45.0), 3: (PERSPECTIVE, near), 4: (AFFINE, (-45.0, -45.0)),
              5: (ROTATION, -45.0), 6: (PERSPECTIVE, mixed), 7: (AFFINE, (45.0, -45.0)), 8: (ROTATION, 0.0)}
    n = 32
    arrs = {}
    boxes, flips, has_jitter, orders, factors, shifts = [], [], [], [], [], []
    choices, strengths, angles, shears, endpoints, kinds, coeffs, all_fill = [], [], [], [], [], [], [], []
    for i in range(n):
        h, w = int(rng.integers(S // 2, 2 * S)), int(rng.integers(S // 2, 2 * S))
        if i % 4 == 3:
            y, x = np.mgrid[0:h, 0:w]
            img = np.stack([x * 255 // max(1, w - 1), y * 255 // max(1, h - 1), (x + y) * 127 // max(1, h + w - 2)], -1).astype(np.uint8)
        else:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ch, cw = int(rng.integers(max(1, h // 2), h + 1)), int(rng.integers(max(1, w // 2), w + 1))
        box = (int(rng.integers(0, h - ch + 1)), int(rng.integers(0, w - cw + 1)), ch, cw)
        flip = int((i // 2) % 2)
        jit = None
        if i % 2 == 0:
            jit = (tuple(int(o) for o in rng.permutation(4)), tuple(float(np.float32(f)) for f in rng.uniform(0.5, 1.5, 3)), int(rng.integers(-7, 8)))
        angle = shear = 0.0
        end = [[0, 0]] * 4
        fill = 0
        if i in corner:
            choice, p = corner[i]
            s = 1.0
        elif i >= n - 2:                                               # warps that map every output pixel outside the picture
            choice, s, fill = (AFFINE, PERSPECTIVE)[i - (n - 2)], 1.0, 1
        else:
            choice, s = i % 3, (0.1, 0.5, 1.0)[(i // 3) % 3]
            if choice == PERSPECTIVE:
                p = R.perspective_points(S, S, 0.5 * s, lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=gen).item()))[1]
            elif choice == AFFINE:
                p = tuple(float(torch.empty(1).uniform_(-45.0 * s, 45.0 * s, generator=gen).item()) for _ in range(2))
            else:
                p = float(torch.empty(1).uniform_(-45.0 * s, 45.0 * s, generator=gen).item())
        if fill:
            if choice == AFFINE:
                m = R.rotate_matrix(30.0, S)
                m[2] += 3 * S
                c8, kind = m + [0.0, 0.0], 0
            else:
                c8, kind = [1.0, 0.0, -2.0 * S, 0.0, 1.0, 0.0, 0.0, 0.0], 1
            param = c8[:6] if kind == 0 else c8
            pil_choice = AFFINE if kind == 0 else PERSPECTIVE
        elif choice == PERSPECTIVE:
            end = [list(q) for q in p]
            c8, kind = R.perspective_coeffs(near, end), 1
            param, pil_choice = c8, PERSPECTIVE
        elif choice == AFFINE:
            angle, shear = p
            m = R.affine_matrix(angle, shear, S)
            c8, kind, param, pil_choice = m + [0.0, 0.0], 0, m, AFFINE
        else:
            angle = p
            c8, kind, param, pil_choice = R.rotate_matrix(angle, S) + [0.0, 0.0], 0, angle, ROTATION
        arrs["in%d" % i] = img
        arrs["out%d" % i] = pil_chain(img, box, flip, jit, pil_choice, param)
        if fill:
            assert not arrs["out%d" % i].any()
        boxes.append(box); flips.append(flip); has_jitter.append(int(jit is not None))
        orders.append(jit[0] if jit else (0, 1, 2, 3)); factors.append(jit[1] if jit else (1.0, 1.0, 1.0)); shifts.append(jit[2] if jit else 0)
        choices.append(choice); strengths.append(s); angles.append(angle); shears.append(shear); endpoints.append(end)
        kinds.append(kind); coeffs.append(c8); all_fill.append(fill)
    arrs.update(size=np.int64(S), boxes=np.array(boxes, np.int64), flips=np.array(flips, np.int64), jitter=np.array(has_jitter, np.int64),
                orders=np.array(orders, np.int64), factors=np.array(factors, np.float32), hue_shifts=np.array(shifts, np.int64),
                choices=np.array(choices, np.int64), strengths=np.array(strengths, np.float64), angles=np.array(angles, np.float64),
                shears=np.array(shears, np.float64), endpoints=np.array(endpoints, np.int64), kinds=np.array(kinds, np.int64),
                coeffs=np.array(coeffs, np.float64), all_fill=np.array(all_fill, np.int64), corner_draws=np.array(sorted(corner), np.int64))
    np.savez_compressed(os.path.join(HERE, "g14_optical.npz"), **arrs)


if __name__ == "__main__":
    main()
