"""Numpy restatement of the integer pipeline of sat_jpeg_decode_batch (csrc/jpeg_decode.hip), independent of the kernels:
Huffman decoding (jdhuff.c), dequantisation + ISLOW IDCT through range_limit (jidctint.c, jdmaster.c), fancy upsampling
(jdsample.c) and YCbCr->RGB (jdcolor.c), for the files sat_amd.jpeg.parse accepts.  Pillow's bytes are what it must equal."""
import numpy as np

from sat_amd import jpeg as J

CB, P1 = 13, 2
F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
         f2562=20995, f3072=25172)


class StreamError(ValueError):
    pass


def lut16(bits, vals):
    """16-bit window -> (length, symbol); length 0: no code"""
    ln = np.zeros(1 << 16, np.int64)
    sym = np.zeros(1 << 16, np.int64)
    sizes, codes = J.huffman_codes(bits)
    for p, (length, code) in enumerate(zip(sizes, codes)):
        lo = code << (16 - length)
        ln[lo:lo + (1 << (16 - length))] = length
        sym[lo:lo + (1 << (16 - length))] = vals[p]
    return (ln << 8 | sym).tolist()


def windows(seg):
    """unstuffed bytes of a segment -> the 16-bit window at every bit position (zeros past the end), and the bit count"""
    b = np.frombuffer(seg, np.uint8)
    ff = np.flatnonzero(b[:-1] == 0xFF)
    if ff.size and np.any(b[ff + 1] != 0):
        raise StreamError("marker inside a segment")
    keep = np.ones(b.size, bool)
    keep[ff + 1] = False
    if b.size and b[-1] == 0xFF:
        raise StreamError("segment ends in 0xFF")
    u = b[keep].astype(np.int64)
    nbits = 8 * u.size
    pad = np.concatenate([u, np.zeros(16, np.int64)])
    w32 = (pad[:-3] << 24) | (pad[1:-2] << 16) | (pad[2:-1] << 8) | pad[3:]
    idx = np.arange(nbits + 64)
    win = (w32[idx >> 3] >> (16 - (idx & 7))) & 0xFFFF
    return win.tolist(), nbits


def decode_coefficients(data, hd):
    """(blocks, 64) int16 coefficients in natural order, components one after the other, every block of every MCU"""
    try:
        return _decode_coefficients(data, hd)
    except IndexError:                    # read past the zero padding of a segment
        raise StreamError("ran out of data") from None


def _decode_coefficients(data, hd):
    geo = comp_geometry(hd)
    nblk = [g["bw"] * g["bh"] for g in geo]
    base = np.concatenate([[0], np.cumsum(nblk)])
    coef = np.zeros((int(base[-1]), 64), np.int64)
    dct = [lut16(*t) for t in hd.dc]
    act = [lut16(*t) for t in hd.ac]
    nat = J.NATURAL_ORDER.tolist()
    mx = geo[0]["bw"] // geo[0]["hs"]
    total = mx * (geo[0]["bh"] // geo[0]["vs"])
    ri = hd.restart_interval or total
    scan = bytes(data[hd.data_start:hd.data_end])
    for k, (s0, s1) in enumerate(hd.segments.tolist()):
        win, nbits = windows(scan[s0:s1])
        pos = 0
        last = [0] * hd.components
        for m in range(k * ri, min(total, (k + 1) * ri)):
            my_, mx_ = divmod(m, mx)
            for c, g in enumerate(geo):
                for by in range(g["vs"]):
                    for bx in range(g["hs"]):
                        blk = coef[base[c] + (my_ * g["vs"] + by) * g["bw"] + mx_ * g["hs"] + bx]
                        e = dct[c][win[pos]]
                        if e == 0:
                            raise StreamError("bad Huffman code")
                        pos += e >> 8
                        s = e & 255
                        v = 0
                        if s:
                            r = win[pos] >> (16 - s)
                            pos += s
                            v = r if r >= 1 << (s - 1) else r - (1 << s) + 1
                        last[c] += v
                        blk[0] = np.int16(np.int64(last[c]).astype(np.int16))
                        i = 1
                        while i < 64:
                            e = act[c][win[pos]]
                            if e == 0:
                                raise StreamError("bad Huffman code")
                            pos += e >> 8
                            rs = e & 255
                            r, s = rs >> 4, rs & 15
                            if s:
                                i += r
                                if i > 63:
                                    raise StreamError("coefficient index past 63")
                                x = win[pos] >> (16 - s)
                                pos += s
                                blk[nat[i]] = x if x >= 1 << (s - 1) else x - (1 << s) + 1
                            elif r == 15:
                                i += 15
                            else:
                                break
                            i += 1
                        if pos > nbits:
                            raise StreamError("ran out of data")
    return coef.astype(np.int16), geo, base


def comp_geometry(hd):
    if hd.components == 1:
        return [dict(bw=(hd.width + 7) // 8, bh=(hd.height + 7) // 8, dw=hd.width, dh=hd.height, hs=1, vs=1)]
    mx, my = hd.mcus()
    out = []
    for c in range(3):
        hs, vs = (hd.h_samp, hd.v_samp) if c == 0 else (1, 1)
        out.append(dict(bw=mx * hs, bh=my * vs, dw=-(-hd.width * hs // hd.h_samp), dh=-(-hd.height * vs // hd.v_samp), hs=hs, vs=vs))
    return out


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_1d(x, sh):
    """jpeg_idct_islow's 1-D pass on x[0..7] (arrays), descaled by sh"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * F["f0541"]
    tmp2 = z1 + z3 * -F["f1847"]
    tmp3 = z1 + z2 * F["f0765"]
    tmp0 = (x[0] + x[4]) << CB
    tmp1 = (x[0] - x[4]) << CB
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["f1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["f0298"], tmp1 * F["f2053"], tmp2 * F["f3072"], tmp3 * F["f1501"]
    z1, z2, z3, z4 = z1 * -F["f0899"], z2 * -F["f2562"], z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [descale(tmp10 + tmp3, sh), descale(tmp11 + tmp2, sh), descale(tmp12 + tmp1, sh), descale(tmp13 + tmp0, sh),
            descale(tmp13 - tmp0, sh), descale(tmp12 - tmp1, sh), descale(tmp11 - tmp2, sh), descale(tmp10 - tmp3, sh)]


def range_limit_table():
    """IDCT_range_limit(cinfo)[0..1023] (jdmaster.c prepare_range_limit_table), indexed by x & 1023"""
    y = np.arange(1024)
    return np.where(y < 128, y + 128, np.where(y < 512, 255, np.where(y < 896, 0, y - 896))).astype(np.uint8)


def idct_islow(coef, q):
    """(N, 64) int16 natural order, (64,) quantisation -> (N, 8, 8) uint8"""
    x = coef.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(1, 8, 8)
    ws = np.stack(idct_1d([x[:, k, :] for k in range(8)], CB - P1), axis=1)          # (N, row k, col)
    ws = ws.astype(np.int32).astype(np.int64)                                         # libjpeg's int workspace
    out = np.stack(idct_1d([ws[:, :, k] for k in range(8)], CB + P1 + 3), axis=2)    # (N, row, col)
    return range_limit_table()[out.astype(np.int32) & 1023]


def upsample(p, g, hmax, vmax):
    """(dh, dw) samples of a component -> (vmax * dh, hmax * dw) (jdsample.c)"""
    if g["hs"] == hmax and g["vs"] == vmax:
        return p
    p = p.astype(np.int64)
    if g["dw"] <= 2:                                                    # h2v1_upsample / h2v2_upsample
        return np.repeat(np.repeat(p, 2, axis=1), vmax, axis=0)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    if vmax == 1:                                                       # h2v1_fancy_upsample
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        return out
    up = np.concatenate([p[:1], p[:-1]], axis=0)                       # h2v2_fancy_upsample: the row above / below, edges replicated
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    res = np.empty((2 * p.shape[0], 2 * p.shape[1]), np.int64)
    for v, far in ((0, up), (1, down)):
        cs = 3 * p + far
        csl = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        csr = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        res[v::2, 0::2] = (3 * cs + csl + 8) >> 4
        res[v::2, 1::2] = (3 * cs + csr + 7) >> 4
    return res


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = (a.astype(np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-46802 * cr + (-22554 * cb + 32768)) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """the (H, W, 3) bytes of Image.open(...).convert("RGB"); raises StreamError on a bad stream, ValueError for a file the GPU path
    does not take"""
    hd = J.parse(data)
    if hd.fallback:
        raise ValueError("not GPU-decodable: %s" % hd.fallback)
    coef, geo, base = decode_coefficients(data, hd)
    planes = []
    for c, g in enumerate(geo):
        blk = idct_islow(coef[base[c]:base[c + 1]], hd.quant[c])
        pl = blk.reshape(g["bh"], g["bw"], 8, 8).transpose(0, 2, 1, 3).reshape(g["bh"] * 8, g["bw"] * 8)
        planes.append(pl[:g["dh"], :g["dw"]])
    H, W = hd.height, hd.width
    if hd.components == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2)
    up = [upsample(p, g, hd.h_samp, hd.v_samp)[:H, :W] for p, g in zip(planes, geo)]
    return ycc_to_rgb(*up)
