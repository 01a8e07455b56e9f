"""Test-side restatement of the reference's "optical" augmentation (train.py:225-231) on PIL images, in numpy:

    T.RandomChoice([T.RandomPerspective(distortion_scale=0.5 * s, p=1),
                    T.RandomAffine(degrees=45 * s, shear=45 * s),
                    T.RandomRotation(degrees=45 * s)])

The three matrix rules (torchvision 0.10's perspective coefficients and inverse affine matrix, Pillow's own Image.rotate
matrix) and the two samplers Pillow runs for them: Image.transform(AFFINE, NEAREST) in 16.16 fixed point and
Image.transform(PERSPECTIVE, BILINEAR) in double.  Both samplers take the inverse map (output pixel -> input point) and fill
with 0.  The GPU kernel is checked against this module and against Pillow itself (tests/golden/g14_optical.npz); this module
is checked against the installed Pillow in tests/test_optical.py.

Pictures are (H, W, 3) uint8 RGB.
"""
import math

import numpy as np
import torch

F64 = np.float64


# ------------------------------------------------------------------------------------------------------------ matrix rules
def affine_matrix(angle, shear_x, size):
    """torchvision 0.10 F.affine on a size x size PIL picture: _get_inverse_affine_matrix(center=[S*0.5, S*0.5], angle,
    translate=[0, 0], scale=1.0, shear=[shear_x, 0.0])."""
    cx = cy = size * 0.5
    tx = ty = 0
    scale = 1.0
    rot = math.radians(angle)
    sx = math.radians(shear_x)
    sy = math.radians(0.0)
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle, size):
    """Pillow's Image.rotate(angle) matrix about the picture's centre (no expand, no translate)."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx = cy = size / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def perspective_coeffs(startpoints, endpoints):
    """torchvision 0.10 _get_perspective_coeffs: the 8 coefficients that map each end point (output) onto its start point
    (input), a float32 least-squares solve ('gels') on the CPU."""
    a = torch.zeros(2 * len(startpoints), 8, dtype=torch.float)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b = torch.tensor(startpoints, dtype=torch.float).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.tolist()


def perspective_points(width, height, distortion_scale, randint):
    """T.RandomPerspective.get_params with ``randint(lo, hi)`` for each torch.randint(lo, hi, (1,)) draw: the start points
    (the picture's corners) and the drawn end points, topleft, topright, botright, botleft."""
    hw, hh = width // 2, height // 2
    dw, dh = int(distortion_scale * hw), int(distortion_scale * hh)
    tl = [randint(0, dw + 1), randint(0, dh + 1)]
    tr = [randint(width - dw - 1, width), randint(0, dh + 1)]
    br = [randint(width - dw - 1, width), randint(height - dh - 1, height)]
    bl = [randint(0, dw + 1), randint(height - dh - 1, height)]
    start = [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]]
    return start, [tl, tr, br, bl]


# ---------------------------------------------------------------------------------------------------------------- samplers
def _fix(v):
    """Pillow's 16.16 FIX(v) = floor(v * 65536 + 0.5)"""
    return int(math.floor(F64(v) * F64(65536.0) + F64(0.5)))


def _wrap32(v):
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)


def affine_fixed_ok(c, width, height):
    """Pillow's check_fixed at the four corners: when it fails Pillow samples in double instead (not restated here)."""
    for x, y in ((0, 0), (width, 0), (0, height), (width, height)):
        if not (abs(x * c[0] + y * c[1] + c[2]) < 32768.0 and abs(x * c[3] + y * c[4] + c[5]) < 32768.0):
            return False
    return True


def affine_nearest(img, c):
    """Image.transform(size, AFFINE, c, NEAREST, fillcolor=0) (Pillow's affine_fixed): 16.16 fixed point, the source pixel
    at (a2 + y*a1 + x*a0) >> 16, (a5 + y*a4 + x*a3) >> 16 with int32 running sums, 0 outside."""
    H, W = img.shape[:2]
    assert affine_fixed_ok(c, W, H)
    a0, a1, a3, a4 = _fix(c[0]), _fix(c[1]), _fix(c[3]), _fix(c[4])
    a2 = _fix(F64(c[2]) + F64(c[0]) * 0.5 + F64(c[1]) * 0.5)
    a5 = _fix(F64(c[5]) + F64(c[3]) * 0.5 + F64(c[4]) * 0.5)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = _wrap32(a2 + y * a1 + x * a0) >> 16
    yin = _wrap32(a5 + y * a4 + x * a3) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = img[np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    out[~inside] = 0
    return out


def perspective_bilinear(img, c):
    """Image.transform(size, PERSPECTIVE, c, BILINEAR, fillcolor=0) (Pillow's generic transform with bilinear_filter32RGB):
    the pixel centre mapped in double, 0 outside the picture, else two clamped rows blended in double and truncated."""
    H, W = img.shape[:2]
    c = [F64(v) for v in c]
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    xi, yi = x + 0.5, y + 0.5
    den = c[6] * xi + c[7] * yi + 1
    xo = (c[0] * xi + c[1] * yi + c[2]) / den
    yo = (c[3] * xi + c[4] * yi + c[5]) / den
    inside = (xo >= 0) & (xo < W) & (yo >= 0) & (yo < H)
    xo = np.where(inside, xo, 0.5) - 0.5
    yo = np.where(inside, yo, 0.5) - 0.5
    fx, fy = np.floor(xo), np.floor(yo)
    dx, dy = (xo - fx)[..., None], (yo - fy)[..., None]
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
    y0 = np.clip(fy, 0, H - 1)
    row2 = (fy + 1 >= 0) & (fy + 1 < H)
    y1 = np.clip(fy + 1, 0, H - 1)
    p = img.astype(np.int64)
    v1 = p[y0, x0] + (p[y0, x1] - p[y0, x0]).astype(F64) * dx            # BILINEAR(v, a, b, d): a + (b - a) * d
    v2 = p[y1, x0] + (p[y1, x1] - p[y1, x0]).astype(F64) * dx
    v2 = np.where(row2[..., None], v2, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)                          # (UINT8) v: truncated
    out[~inside] = 0
    return out


def warp(img, kind, c):
    """kind 0: affine map, NEAREST; kind 1: perspective map, BILINEAR (the sat_image_warp record)"""
    return affine_nearest(img, c) if kind == 0 else perspective_bilinear(img, c)
