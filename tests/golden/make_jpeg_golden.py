"""Generate tests/golden/g15_jpeg.npz with the installed Pillow:

    python tests/golden/make_jpeg_golden.py

Small JPEG files written by Pillow (``Image.save(..., "JPEG")``) and Pillow's decoded bytes,
``np.asarray(Image.open(f).convert("RGB"))``, for the files the GPU decoder takes: qualities 10, 75, 95 and 100 (noisy
content at 100), 4:4:4, 4:2:2, 4:2:0 and grayscale, sizes from 1x1 up, optimized Huffman tables, restart markers, and a
noise picture whose quantisation steps were scaled by 4 after encoding (IDCT outputs far outside [0, 255]).  Also a
few files it must hand to Pillow (progressive, CMYK, RGB kept as RGB with an Adobe marker, PNG), with ``gpu`` = 0.
    jpeg<i>   the file's bytes (uint8)          rgb<i>   the decoded (H, W, 3) bytes
    cases     one line per file: "name"         gpu      1 if the GPU decodes it
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def picture(h, w, seed, noise=12.0):
    """a smooth colour ramp plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, noise, (h, w, 3))), 0, 255).astype(np.uint8)


def encode(img, fmt="JPEG", **kw):
    buf = io.BytesIO()
    img.save(buf, fmt, **kw)
    return buf.getvalue()


def scale_dqt(data, factor):
    """the file with every quantisation step multiplied by ``factor`` (at most 255): the same coefficients dequantised to
    values far outside the sample range, so the IDCT output overshoots into range_limit's saturating zones"""
    d, i = bytearray(data), 2
    while d[i + 1] != 0xDA:
        seg = (d[i + 2] << 8) | d[i + 3]
        if d[i + 1] == 0xDB:
            for p in range(i + 4, i + 2 + seg, 65):
                d[p + 1:p + 65] = bytes(min(255, v * factor) for v in d[p + 1:p + 65])
        i += 2 + seg
    return bytes(d)


def cases():
    """(name, file bytes, GPU-decodable)"""
    out = []
    ss_name = {0: "444", 1: "422", 2: "420"}
    for q in (10, 75, 95, 100):
        for ss in (0, 1, 2):
            a = picture(33, 65, q * 10 + ss, noise=60.0 if q == 100 else 12.0)
            out.append(("q%d_%s_33x65" % (q, ss_name[ss]), encode(Image.fromarray(a), quality=q, subsampling=ss), True))
    for q in (10, 100):
        a = picture(33, 65, 900 + q, noise=60.0 if q == 100 else 12.0)[:, :, 1]
        out.append(("gray_q%d_33x65" % q, encode(Image.fromarray(a), quality=q), True))
    for h, w in ((1, 1), (1, 17), (17, 1), (15, 16), (17, 9), (3, 5), (5, 6)):
        for ss in (0, 1, 2):
            out.append(("q75_%s_%dx%d" % (ss_name[ss], h, w), encode(Image.fromarray(picture(h, w, h * 100 + w + ss)), quality=75, subsampling=ss), True))
        out.append(("gray_q75_%dx%d" % (h, w), encode(Image.fromarray(picture(h, w, h * 100 + w)[:, :, 0]), quality=75), True))
    a = picture(40, 57, 7)
    out.append(("optimize_420_40x57", encode(Image.fromarray(a), quality=90, optimize=True), True))
    out.append(("optimize_gray_40x57", encode(Image.fromarray(a[:, :, 2]), quality=90, optimize=True), True))
    for ss in (0, 1, 2):
        out.append(("rst_blocks1_%s_40x57" % ss_name[ss], encode(Image.fromarray(a), quality=85, subsampling=ss, restart_marker_blocks=1), True))
        out.append(("rst_rows1_%s_40x57" % ss_name[ss], encode(Image.fromarray(a), quality=85, subsampling=ss, restart_marker_rows=1), True))
    out.append(("rst_blocks3_gray_40x57", encode(Image.fromarray(a[:, :, 0]), quality=85, restart_marker_blocks=3), True))
    out.append(("rst_blocks9_optimize_420_40x57", encode(Image.fromarray(a), quality=85, restart_marker_blocks=9, optimize=True), True))
    noise = np.random.default_rng(11).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    out.append(("dqt_x4_overshoot_444_32x48", scale_dqt(encode(Image.fromarray(noise), quality=100, subsampling=0), 4), True))
    out.append(("progressive_40x57", encode(Image.fromarray(a), quality=85, progressive=True), False))
    out.append(("cmyk_40x57", encode(Image.fromarray(a).convert("CMYK"), quality=85), False))
    out.append(("adobe_rgb_40x57", encode(Image.fromarray(a), quality=85, keep_rgb=True), False))
    out.append(("png_40x57", encode(Image.fromarray(a), "PNG"), False))
    return out


def main():
    arrs, names, gpu = {}, [], []
    for i, (name, data, on_gpu) in enumerate(cases()):
        arrs["jpeg%d" % i] = np.frombuffer(data, np.uint8)
        arrs["rgb%d" % i] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        names.append(name)
        gpu.append(int(on_gpu))
    arrs.update(cases=np.array(names), gpu=np.array(gpu, np.int64))
    np.savez_compressed(os.path.join(HERE, "g15_jpeg.npz"), **arrs)


if __name__ == "__main__":
    main()
