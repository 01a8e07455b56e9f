"""Python restatement of progressive JPEG entropy decoding (libjpeg's jdphuff.c: DC first, DC refine, AC first, AC refine), independent
of the kernels of csrc/jpeg_decode.hip: every scan of a file that ``sat_amd.jpeg.parse(f, progressive=True)`` takes is decoded into
the coefficient array the baseline path leaves (components one after the other, every block of every MCU), and tests/jpeg_ref.py's
IDCT, upsampling and colour conversion make the pixels.  Pillow's bytes are what it must equal.

No progressive encoder is kept here: the parser admits exactly the two scan scripts Pillow writes (``jpeg.PROGRESSIONS``), so Pillow's
own files are all the tests need."""
import io

import numpy as np
from PIL import Image

from sat_amd import jpeg as J
import jpeg_ref as R


def picture(h, w, seed, noise=12.0):
    """the test picture of the JPEG tests: two ramps and a wave, plus noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, noise, (h, w, 3))), 0, 255).astype(np.uint8)


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def small_cases():
    """name -> progressive file: the smallest shapes at which each mechanism can go wrong.  17x9 4:2:0: the luma AC scans cover 3x2
    blocks of a 4x2 grid and the interleaved DC scan walks the padded grid; 8x8: one block; 33x65 gray: six scans, non-interleaved
    DC; 40x57 at quality 10 (EOB runs across block rows) and 100 (dense blocks, correction bits, ZRL in refinement), each with a
    restart marker per MCU row as well (EOBRUN and the predictors reset, several lanes per scan)."""
    out = {"420_17x9": encode(picture(17, 9, 1), progressive=True, subsampling=2),
           "422_1x1": encode(picture(1, 1, 2), progressive=True, subsampling=1),
           "444_8x8": encode(picture(8, 8, 3), progressive=True, subsampling=0),
           "gray_33x65": encode(picture(33, 65, 4)[:, :, 0], progressive=True),
           "gray_rst_33x65": encode(picture(33, 65, 4)[:, :, 0], progressive=True, restart_marker_rows=1)}
    for sub, name in ((2, "420"), (1, "422"), (0, "444")):
        for q in (10, 100):
            a = picture(40, 57, 10 + sub + q, noise=30.0)
            out["%s_q%d_40x57" % (name, q)] = encode(a, progressive=True, subsampling=sub, quality=q)
            out["%s_q%d_rst_40x57" % (name, q)] = encode(a, progressive=True, subsampling=sub, quality=q, restart_marker_rows=1)
    return out


class Bits:
    """the bits of one restart segment: 16-bit windows at every position (jpeg_ref.windows)"""

    def __init__(self, seg):
        self.win, self.nbits = R.windows(seg)
        self.pos = 0

    def huff(self, lut):
        e = lut[self.win[self.pos]]
        if e == 0:
            raise R.StreamError("bad Huffman code")
        self.pos += e >> 8
        return e & 255

    def get(self, n):
        if n == 0:
            return 0
        v = self.win[self.pos] >> (16 - n)
        self.pos += n
        return v


def extend(r, s):
    return r if s == 0 or r >= 1 << (s - 1) else r - (1 << s) + 1


def scan_blocks(hd, geo, base, sc):
    """the coefficient-array index of every block of the scan, in the order the scan codes them, and the component of each.
    An interleaved scan walks the padded MCU grid; a scan of one component is non-interleaved: one block per MCU, the
    ceil(dw / 8) x ceil(dh / 8) blocks that hold samples, in raster order."""
    if len(sc.comps) > 1:
        mx = geo[0]["bw"] // geo[0]["hs"]
        my = geo[0]["bh"] // geo[0]["vs"]
        out = []
        for m in range(mx * my):
            my_, mx_ = divmod(m, mx)
            for c in sc.comps:
                g = geo[c]
                for by in range(g["vs"]):
                    for bx in range(g["hs"]):
                        out.append((int(base[c]) + (my_ * g["vs"] + by) * g["bw"] + mx_ * g["hs"] + bx, c))
        return out, len(out) // (mx * my)
    c = sc.comps[0]
    g = geo[c]
    sw, sh = -(-g["dw"] // 8), -(-g["dh"] // 8)
    return [(int(base[c]) + by * g["bw"] + bx, c) for by in range(sh) for bx in range(sw)], 1


def decode_scan(data, hd, sc, coef, geo, base):
    blocks, per_mcu = scan_blocks(hd, geo, base, sc)
    n_mcu = len(blocks) // per_mcu
    ri = sc.restart_interval or n_mcu
    assert len(sc.segments) == -(-n_mcu // ri)
    nat = J.NATURAL_ORDER.tolist()
    dct = [R.lut16(*t) if t is not None else None for t in sc.dc]
    act = R.lut16(*sc.ac) if sc.ac is not None else None
    raw = bytes(data[sc.data_start:sc.data_end])
    p1, m1 = 1 << sc.al, -(1 << sc.al)
    for k, (s0, s1) in enumerate(sc.segments.tolist()):
        br = Bits(raw[s0:s1])
        pred = {c: 0 for c in sc.comps}                     # reset at every restart, as EOBRUN is
        eobrun = 0
        for bi, c in blocks[k * ri * per_mcu:min(n_mcu, (k + 1) * ri) * per_mcu]:
            blk = coef[bi]
            if sc.ss == 0 and sc.ah == 0:                   # DC first
                s = br.huff(dct[sc.comps.index(c)])
                if s > 15:
                    raise R.StreamError("bad Huffman code")
                pred[c] += extend(br.get(s), s)
                blk[0] = pred[c] << sc.al
            elif sc.ss == 0:                                # DC refine
                if br.get(1):
                    blk[0] |= p1
            elif sc.ah == 0:                                # AC first
                if eobrun > 0:
                    eobrun -= 1
                else:
                    i = sc.ss
                    while i <= sc.se:
                        rs = br.huff(act)
                        r, s = rs >> 4, rs & 15
                        if s:
                            i += r
                            if i > sc.se:
                                raise R.StreamError("coefficient index past the band")
                            blk[nat[i]] = extend(br.get(s), s) << sc.al
                        elif r == 15:
                            i += 15
                        else:
                            eobrun = (1 << r) + br.get(r) - 1
                            break
                        i += 1
            else:                                           # AC refine
                i = sc.ss
                if eobrun == 0:
                    while i <= sc.se:
                        rs = br.huff(act)
                        r, s = rs >> 4, rs & 15
                        if s:
                            s = p1 if br.get(1) else m1
                        elif r != 15:
                            eobrun = (1 << r) + br.get(r)
                            break
                        while i <= sc.se:
                            j = nat[i]
                            if blk[j] != 0:
                                if br.get(1) and (blk[j] & p1) == 0:
                                    blk[j] += p1 if blk[j] >= 0 else m1
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            i += 1
                        if s:
                            if i > sc.se:
                                raise R.StreamError("coefficient index past the band")
                            blk[nat[i]] = s
                        i += 1
                if eobrun > 0:
                    while i <= sc.se:
                        j = nat[i]
                        if blk[j] != 0 and br.get(1) and (blk[j] & p1) == 0:
                            blk[j] += p1 if blk[j] >= 0 else m1
                        i += 1
                    eobrun -= 1
            if br.pos > br.nbits:
                raise R.StreamError("ran out of data")


def decode_coefficients(data, hd):
    geo = R.comp_geometry(hd)
    base = np.concatenate([[0], np.cumsum([g["bw"] * g["bh"] for g in geo])])
    coef = np.zeros((int(base[-1]), 64), np.int64)
    try:
        for sc in hd.scans:
            decode_scan(data, hd, sc, coef, geo, base)
    except IndexError:
        raise R.StreamError("ran out of data") from None
    return coef.astype(np.int16), geo, base


def decode(data):
    """the (H, W, 3) bytes of Image.open(...).convert("RGB") of a progressive file the GPU path takes"""
    hd = J.parse(data, progressive=True)
    if hd.fallback or not hd.progressive:
        raise ValueError("not a GPU-decodable progressive file: %s" % hd.fallback)
    coef, geo, base = decode_coefficients(data, hd)
    planes = []
    for c, g in enumerate(geo):
        blk = R.idct_islow(coef[base[c]:base[c + 1]], hd.quant[c])
        pl = blk.reshape(g["bh"], g["bw"], 8, 8).transpose(0, 2, 1, 3).reshape(g["bh"] * 8, g["bw"] * 8)
        planes.append(pl[:g["dh"], :g["dw"]])
    H, W = hd.height, hd.width
    if hd.components == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2)
    up = [R.upsample(p, g, hd.h_samp, hd.v_samp)[:H, :W] for p, g in zip(planes, geo)]
    return R.ycc_to_rgb(*up)
