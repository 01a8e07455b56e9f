"""Baseline JPEG decoding on the GPU, bit exact with Pillow's ``Image.open(f).convert("RGB")`` (libjpeg-turbo, JDCT_ISLOW,
fancy upsampling).

Host side of ``sat_jpeg_decode_batch`` (include/sat_hip.h): the header parser, which also decides whether a file is
decoded on the GPU or falls back to Pillow, the restart-marker scan, and the Huffman / quantisation tables in the layout
the kernels read.

GPU-decodable: Huffman-coded sequential 8-bit files (SOF0, SOF1) with one scan holding every component, either
1 component (grayscale) or 3 components that libjpeg reads as YCbCr, luma sampled h1v1, h2v1 or h2v2 and chroma 1x1, with
or without restart markers.  A file with restart markers is entropy-decoded by one thread per restart segment; a restart-free
file (most cameras, COCO) of at least ``parallel_min_bytes`` of data by one thread per ``subseq_bytes`` of it, the threads
synchronising on the device (include/sat_hip.h, ``sat_jpeg_decode_batch_ex``); the bytes that come out are the same.  Everything else (progressive, arithmetic-coded, 12-bit, lossless, CMYK / YCCK, Adobe RGB,
several scans, other sampling factors, non-JPEG bytes) is decoded by Pillow, as ``data.decode_rgb`` does.

Progressive files are taken on request only: ``parse(data, progressive=True)``, ``as_picture(item, progressive=True)``,
``read_jpeg_progressive`` and ``decode_jpeg_batch(..., progressive=True)``.  Admitted: Huffman-coded 8-bit SOF2 files with the same
components, sampling factors and colour rules as above whose scan script is one of ``PROGRESSIONS`` (libjpeg's
jpeg_simple_progression, which Pillow writes: ten scans for YCbCr, six for grayscale), valid by jdphuff.c's rules, complete down to
Al = 0 and closed by EOI, with or without restart markers.  Still Pillow's: any other scan script, an incomplete or cut progression,
arithmetic coding, CMYK / Adobe RGB.  The scans carry a dependency level each; the device runs one entropy launch per level
(``sat_jpeg_decode_progressive_batch``) and the baseline path's IDCT and colour kernels behind them.  Without the keyword every
function classifies as it always did.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

#: zigzag position -> natural (row-major) index: libjpeg's jpeg_natural_order
NATURAL_ORDER = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                          62, 63], dtype=np.int64)
LOOKAHEAD = 9                         # bits resolved by one table lookup on the device (sat_jpeg_htable.lookup)

_SOF_OTHER = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential", 0xC6: "differential progressive", 0xC7: "differential lossless",
              0xC9: "arithmetic", 0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCD: "arithmetic differential",
              0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}
_SAMPLING = ((1, 1), (2, 1), (2, 2))


class JpegHeader:
    """What the GPU decoder needs of one file.  ``fallback`` is None for a GPU-decodable file, else the reason it is not;
    ``height`` / ``width`` are set whenever the SOF marker was read, so the picture's shape is known either way."""

    def __init__(self):
        self.fallback = None
        self.height = self.width = None
        self.components = 0
        self.h_samp = self.v_samp = 1
        self.quant = []               # per component: (64,) uint16 in natural order, as latched at the scan
        self.dc = []                  # per component: (bits[17], huffval) of its DC table
        self.ac = []
        self.restart_interval = 0
        self.data_start = self.data_end = 0   # entropy-coded data of the scan in the file's bytes
        self.segments = None          # (n_segments, 2) uint32 (start, end) relative to data_start, RST markers excluded
        self.truncated = False
        self.progressive = False      # parse(progressive=True) took a SOF2 file: ``scans`` and ``levels`` describe it
        self.scans = []               # JpegScan records in file order
        self.levels = 0               # dependency levels of the scans: entropy launches on the device

    @property
    def shape(self):
        return (self.height, self.width)

    def mcus(self):
        """(MCU columns, MCU rows)"""
        mw, mh = 8 * self.h_samp, 8 * self.v_samp
        return (self.width + mw - 1) // mw, (self.height + mh - 1) // mh

    def blocks(self):
        """coefficient blocks of the scan, all components (every block of every MCU)"""
        mx, my = self.mcus()
        return mx * my * (self.h_samp * self.v_samp + (2 if self.components == 3 else 0))


class JpegScan:
    """One scan of a progressive file: the components it holds (indices into the frame), its band ``ss .. se`` and bit positions
    ``ah`` / ``al``, and the Huffman tables and restart interval in force at its SOS marker (libjpeg latches both per scan).
    ``segments``: as ``JpegHeader.segments``, relative to ``data_start``.  ``level``: the scan may run once every scan of a lower level
    is done."""

    def __init__(self, comps, ss, se, ah, al):
        self.comps, self.ss, self.se, self.ah, self.al = comps, ss, se, ah, al
        self.dc = [None] * len(comps)     # (bits[17], huffval) per component of the scan; None where the scan reads no such table
        self.ac = None
        self.restart_interval = 0
        self.data_start = self.data_end = 0
        self.segments = None
        self.level = 0

    @property
    def shape_key(self):
        return (tuple(self.comps), self.ss, self.se, self.ah, self.al)


def _u16(b, i):
    return (b[i] << 8) | b[i + 1]


def _check_huffman(bits, vals, is_dc):
    """jdhuff.c jpeg_make_d_derived_tbl's checks: None if libjpeg accepts the table, else the reason"""
    if sum(bits[1:]) > 256 or len(vals) < sum(bits[1:]):
        return "bad Huffman table"
    code = 0
    for length in range(1, 17):
        code += bits[length]
        if code > (1 << length):
            return "bad Huffman table"
        code <<= 1
    if is_dc and any(v > 15 for v in vals[:sum(bits[1:])]):
        return "bad DC Huffman table"
    return None


def _read_dht(b, p, end, dc, ac):
    """the tables of one DHT segment into ``dc`` / ``ac``; the reason libjpeg would refuse one, or None"""
    while p < end:
        tc, th = b[p] >> 4, b[p] & 15
        bits = [0] + list(b[p + 1:p + 17])
        cnt = sum(bits)
        vals = bytes(b[p + 17:p + 17 + cnt])
        why = _check_huffman(bits, vals, tc == 0)
        if why or tc > 1 or th > 3:
            return why or "bad Huffman table id"
        (dc if tc == 0 else ac)[th] = (bits, vals)
        p += 17 + cnt
    return None


def _read_dqt(b, p, end, quant):
    """the tables of one DQT segment into ``quant`` (natural order)"""
    while p < end:
        pq, tq = b[p] >> 4, b[p] & 15
        if pq:
            zz = np.frombuffer(bytes(b[p + 1:p + 129]), dtype=">u2").astype(np.uint16)
            p += 129
        else:
            zz = np.frombuffer(bytes(b[p + 1:p + 65]), dtype=np.uint8).astype(np.uint16)
            p += 65
        if tq > 3 or zz.size != 64:
            return "bad quantisation table"
        q = np.zeros(64, np.uint16)
        q[NATURAL_ORDER] = zz
        quant[tq] = q
    return None


def parse(data, progressive=False) -> JpegHeader:
    """Walk the markers up to the entropy-coded data of the first scan and find its restart markers.  With ``progressive`` a
    Huffman-coded 8-bit SOF2 file is walked through all of its scans (``hd.progressive``, ``hd.scans``) and taken when its
    progression is one the GPU decodes (``_progression``); without it every SOF2 file falls back, as before."""
    hd = JpegHeader()
    b = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray)) else data
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        hd.fallback = "not a JPEG"
        return hd
    quant, dc, ac = {}, {}, {}
    frame = None
    jfif = adobe = False
    adobe_transform = None
    i = 2
    try:
        while True:
            if i + 1 >= n:
                hd.fallback = "no scan"
                return hd
            if b[i] != 0xFF:
                hd.fallback = "bad marker"
                return hd
            while i < n and b[i] == 0xFF:
                i += 1
            m = b[i]
            i += 1
            if m in (0x01,) or 0xD0 <= m <= 0xD7:
                continue
            if m == 0xD9:
                hd.fallback = "no scan"
                return hd
            seg_len = _u16(b, i)
            if seg_len < 2 or i + seg_len > n:
                hd.fallback = "truncated header"
                return hd
            p, end = i + 2, i + seg_len
            if m in (0xC0, 0xC1) or (m == 0xC2 and progressive):
                hd.progressive = m == 0xC2
                if frame is not None:
                    hd.fallback = "two frames"
                    return hd
                prec, hd.height, hd.width, nf = b[p], _u16(b, p + 1), _u16(b, p + 3), b[p + 5]
                frame = [(b[p + 6 + 3 * k], b[p + 7 + 3 * k] >> 4, b[p + 7 + 3 * k] & 15, b[p + 8 + 3 * k]) for k in range(nf)]
                if prec != 8:
                    hd.fallback = "%d-bit samples" % prec
                elif hd.height == 0 or hd.width == 0:
                    hd.fallback = "no height (DNL) or width"
                elif nf not in (1, 3):
                    hd.fallback = "%d components" % nf
            elif m in _SOF_OTHER:
                hd.fallback = _SOF_OTHER[m]
                if end - p >= 5:
                    hd.height, hd.width = _u16(b, p + 1), _u16(b, p + 3)
                return hd
            elif m == 0xC4:
                why = _read_dht(b, p, end, dc, ac)
                if why:
                    hd.fallback = why
                    return hd
            elif m == 0xCC:
                hd.fallback = "arithmetic coding"
                return hd
            elif m == 0xDB:
                why = _read_dqt(b, p, end, quant)
                if why:
                    hd.fallback = why
                    return hd
            elif m == 0xDD:
                hd.restart_interval = _u16(b, p)
            elif m == 0xE0:
                jfif = jfif or (seg_len - 2 >= 14 and bytes(b[p:p + 5]) == b"JFIF\0")       # jdmarker.c examine_app0
            elif m == 0xEE:
                if seg_len - 2 >= 12 and bytes(b[p:p + 5]) == b"Adobe":                    # examine_app14
                    adobe, adobe_transform = True, b[p + 11]
            elif m == 0xDA:
                if frame is None:
                    hd.fallback = "scan before frame"
                    return hd
                if hd.fallback:
                    return hd
                ns = b[p]
                sel = [(b[p + 1 + 2 * k], b[p + 2 + 2 * k] >> 4, b[p + 2 + 2 * k] & 15) for k in range(ns)]
                ss, se, ahl = b[p + 1 + 2 * ns], b[p + 2 + 2 * ns], b[p + 3 + 2 * ns]
                if hd.progressive:
                    return _progressive(hd, b, i, frame, quant, dc, ac, jfif, adobe, adobe_transform)
                if ns != len(frame) or [s[0] for s in sel] != [f[0] for f in frame]:
                    hd.fallback = "more than one scan"
                    return hd
                if ss != 0 or se != 63 or ahl != 0:
                    hd.fallback = "not a sequential scan"
                    return hd
                return _finish(hd, b, end, frame, sel, quant, dc, ac, jfif, adobe, adobe_transform)
            i = end
    except IndexError:
        hd.fallback = "truncated header"
        return hd


def _frame_checks(hd, frame, jfif, adobe, adobe_transform):
    """the component, sampling-factor and colour rules of a GPU-decodable frame; False with ``hd.fallback`` set otherwise"""
    nf = len(frame)
    if nf == 3:
        # jdapimin.c default_decompress_parms: JFIF -> YCbCr; else Adobe transform 0 -> RGB; else component ids 'R','G','B' -> RGB
        if not jfif and adobe and adobe_transform == 0:
            hd.fallback = "Adobe RGB"
            return False
        if not jfif and not adobe and [f[0] for f in frame] == [82, 71, 66]:
            hd.fallback = "RGB components"
            return False
        if (frame[0][1], frame[0][2]) not in _SAMPLING or any((f[1], f[2]) != (1, 1) for f in frame[1:]):
            hd.fallback = "sampling factors"
            return False
        hd.h_samp, hd.v_samp = frame[0][1], frame[0][2]
    elif not (1 <= frame[0][1] <= 4 and 1 <= frame[0][2] <= 4):
        hd.fallback = "sampling factors"
        return False                  # one component: a non-interleaved scan, one block per MCU whatever the factors
    hd.components = nf
    return True


def _markers(b, start):
    """The vectorised marker scan: (bytes from ``start`` on, positions relative to ``start`` of every 0xFF that is followed by
    anything but 0x00, the byte that follows each)."""
    arr = np.frombuffer(bytes(b[start:]) if not isinstance(b, (bytes, bytearray)) else b, dtype=np.uint8,
                        offset=0 if not isinstance(b, (bytes, bytearray)) else start)
    ff = np.flatnonzero(arr[:-1] == 0xFF)
    nxt = arr[ff + 1]
    mk = nxt != 0
    return arr, ff[mk], nxt[mk]


def _segments(pos, code, data_end, units, ri, truncated):
    """The restart segments of a scan of ``units`` MCUs whose RST markers sit at ``pos`` (codes ``code``) of its ``data_end`` bytes:
    ((n_segments, 2) uint32, None), or (None, the reason the markers do not fit the restart interval)."""
    n_seg = (units + ri - 1) // ri if ri else 1
    if pos.size > n_seg - 1 or (pos.size < n_seg - 1 and not truncated):
        return None, "restart markers do not match the restart interval"
    if np.any(code != 0xD0 + (np.arange(code.size) & 7)):
        return None, "restart markers out of sequence"
    starts = np.concatenate([[0], pos + 2]).astype(np.int64)
    ends = np.concatenate([pos, [data_end]]).astype(np.int64)
    seg = np.full((n_seg, 2), data_end, dtype=np.uint32)          # a truncated file: the missing segments are empty
    seg[:starts.size, 0], seg[:starts.size, 1] = starts, ends
    return seg, None


def _finish(hd, b, start, frame, sel, quant, dc, ac, jfif, adobe, adobe_transform):
    nf = len(frame)
    if not _frame_checks(hd, frame, jfif, adobe, adobe_transform):
        return hd
    for (cid, h, v, tq), (_, td, ta) in zip(frame, sel):
        if tq not in quant or td not in dc or ta not in ac:
            hd.fallback = "missing table"
            return hd
        hd.quant.append(quant[tq])
        hd.dc.append(dc[td])
        hd.ac.append(ac[ta])
    # the end of the scan and its restart markers: it stops at the first marker that is no RST
    arr, pos, code = _markers(b, start)
    if pos.size and np.any(code == 0xFF):
        hd.fallback = "fill bytes in the scan"
        return hd
    rst = (code >= 0xD0) & (code <= 0xD7)
    stop = np.flatnonzero(~rst)
    if stop.size:
        data_end = int(pos[stop[0]])
        pos, code = pos[:stop[0]], code[:stop[0]]
    else:
        data_end = arr.size
        hd.truncated = True
        if arr.size and arr[-1] == 0xFF:
            data_end -= 1
    mx, my = hd.mcus() if nf == 3 else ((hd.width + 7) // 8, (hd.height + 7) // 8)
    hd.segments, why = _segments(pos, code, data_end, mx * my, hd.restart_interval, hd.truncated)
    if why:
        hd.fallback = why
        return hd
    hd.data_start, hd.data_end = start, start + data_end
    return hd


#: The progressions the GPU takes: exactly the ones the tests decode (tests/test_gpu_jpeg_progressive.py), which are the two that
#: libjpeg's jpeg_simple_progression - and so Pillow's ``progressive=True`` - writes: ten scans for YCbCr, six for grayscale.
#: A scan is (components, Ss, Se, Ah, Al).
_YCC = (0, 1, 2)
PROGRESSIONS = {
    "simple YCbCr": ((_YCC, 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                     ((0,), 1, 63, 2, 1), (_YCC, 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)),
    "simple grayscale": (((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
                         ((0,), 1, 63, 1, 0)),
}


def _progression(scans, nf):
    """Why the scans are not a progression the GPU decodes, or None.  jdphuff.c start_pass_phuff_decoder's rules (libjpeg only
    warns about the last three; here they send the file to Pillow), completeness - every coefficient of every component ends at
    Al = 0, else libjpeg smooths between blocks - and PROGRESSIONS.  Sets every scan's dependency level: 1 + the highest level
    of an earlier scan that touches one of the same (component, coefficient) cells.  The scans of one level touch disjoint
    cells, so the lanes of one entropy launch on the device never write (or refine) the same int16."""
    bit = np.full((nf, 64), -1, np.int64)         # libjpeg's coef_bits: the Al every cell has reached, -1 not seen yet
    level = np.full((nf, 64), -1, np.int64)
    for sc in scans:
        if sc.ss == 0:
            if sc.se != 0:
                return "progressive scan mixes DC and AC"
        elif len(sc.comps) != 1 or not sc.ss <= sc.se <= 63:
            return "bad progressive AC scan"
        if sc.al > 13 or (sc.ah and sc.al != sc.ah - 1):
            return "bad successive approximation"
        cells = (np.array(sc.comps), slice(sc.ss, sc.se + 1))
        if sc.ss and bit[sc.comps[0], 0] < 0:
            return "AC scan before the DC scan"
        if np.any(np.maximum(bit[cells], 0) != sc.ah) or (sc.ah == 0 and np.any(bit[cells] >= 0)):
            return "refinement out of order"
        sc.level = int(level[cells].max()) + 1
        bit[cells], level[cells] = sc.al, sc.level
    if np.any(bit != 0):
        return "incomplete progression"
    if tuple(sc.shape_key for sc in scans) not in PROGRESSIONS.values():
        return "untested progression"
    return None


def _progressive(hd, b, i, frame, quant, dc, ac, jfif, adobe, adobe_transform):
    """``parse`` from the first SOS marker (at ``b[i - 1]``, its length at ``b[i]``) of a SOF2 file to EOI."""
    nf = len(frame)
    if not _frame_checks(hd, frame, jfif, adobe, adobe_transform):
        return hd
    n = len(b)
    ids = [f[0] for f in frame]
    hd.quant = [None] * nf
    arr, pos, code = _markers(b, 0)
    # geometry of the scans: an interleaved scan walks the padded MCU grid; a scan of one component is non-interleaved, its MCU
    # one block, and covers the ceil(w / 8) x ceil(h / 8) blocks that hold samples of that component, which its restart
    # interval counts
    mx, my = hd.mcus() if nf == 3 else ((hd.width + 7) // 8, (hd.height + 7) // 8)
    own = []
    for c in range(nf):
        hs, vs = (hd.h_samp, hd.v_samp) if c == 0 and nf == 3 else (1, 1)
        hmax, vmax = (hd.h_samp, hd.v_samp) if nf == 3 else (1, 1)
        own.append((-(-hd.width * hs // (8 * hmax))) * (-(-hd.height * vs // (8 * vmax))))
    m = 0xDA
    while True:
        if m == 0xD9:
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            hd.fallback = "stray marker between scans"
            return hd
        seg_len = _u16(b, i)
        if seg_len < 2 or i + seg_len > n:
            hd.fallback = "truncated header"
            return hd
        p, end = i + 2, i + seg_len
        if m == 0xC4:
            why = _read_dht(b, p, end, dc, ac)
        elif m == 0xDB:
            why = _read_dqt(b, p, end, quant)
        elif m == 0xDD:
            hd.restart_interval, why = _u16(b, p), None
        elif m == 0xCC:
            why = "arithmetic coding"
        elif 0xC0 <= m <= 0xCF:
            why = "two frames"
        elif m == 0xDA:
            ns = b[p]
            sel = [(b[p + 1 + 2 * k], b[p + 2 + 2 * k] >> 4, b[p + 2 + 2 * k] & 15) for k in range(ns)]
            ss, se, ahl = b[p + 1 + 2 * ns], b[p + 2 + 2 * ns], b[p + 3 + 2 * ns]
            why = None
            if any(s[0] not in ids for s in sel) or not 1 <= ns <= nf:
                why = "scan of an unknown component"
            else:
                sc = JpegScan([ids.index(s[0]) for s in sel], ss, se, ahl >> 4, ahl & 15)
                if sorted(set(sc.comps)) != sc.comps or (ns > 1 and ns != nf):
                    why = "scan components"                   # out of order, repeated, or an interleaved scan of some components only
            if why is None:
                sc.restart_interval = hd.restart_interval
                for k, (c, (_, td, ta)) in enumerate(zip(sc.comps, sel)):
                    if hd.quant[c] is None:                   # jdinput.c latch_quant_tables: at the component's first scan
                        if frame[c][3] not in quant:
                            why = "missing table"
                            break
                        hd.quant[c] = quant[frame[c][3]]
                    if ss == 0 and sc.ah == 0:
                        sc.dc[k] = dc.get(td)
                    if ss:
                        sc.ac = ac.get(ta)
                if why is None and ((ss == 0 and sc.ah == 0 and None in sc.dc) or (ss and sc.ac is None)):
                    why = "missing table"
            if why is None:
                # the scan's data ends at the first marker that is no RST; the marker walk resumes there
                k0 = int(np.searchsorted(pos, end))
                stop = np.flatnonzero((code[k0:] < 0xD0) | (code[k0:] > 0xD7))
                if not stop.size:
                    why = "truncated"
                elif code[k0 + stop[0]] == 0xFF:
                    why = "fill bytes in the scan"
                else:
                    k1 = k0 + int(stop[0])
                    sc.data_start, sc.data_end = end, int(pos[k1])
                    sc.segments, why = _segments(pos[k0:k1] - end, code[k0:k1], sc.data_end - end, mx * my if ns > 1 else own[sc.comps[0]],
                                                 sc.restart_interval, False)
                    hd.scans.append(sc)
                    end = sc.data_end
        else:
            why = None                                        # APPn, COM, ...: skipped
        if why:
            hd.fallback = why
            return hd
        i = end
        if i + 1 >= n or b[i] != 0xFF:
            hd.fallback = "truncated"                         # no EOI behind the last scan: Pillow raises on such a file
            return hd
        while i < n and b[i] == 0xFF:
            i += 1
        if i >= n:
            hd.fallback = "truncated"
            return hd
        m = b[i]
        i += 1
    if any(q is None for q in hd.quant):
        hd.fallback = "incomplete progression"
        return hd
    hd.fallback = _progression(hd.scans, nf)
    if hd.fallback is None:
        hd.levels = 1 + max(sc.level for sc in hd.scans)
        hd.restart_interval = 0
        hd.data_start, hd.data_end = hd.scans[0].data_start, hd.scans[-1].data_end
    return hd


# ---------------------------------------------------------------------------------------------------------------------- tables
def huffman_codes(bits):
    """jpeg_make_d_derived_tbl: the canonical code of every symbol position and its length"""
    sizes = [length for length in range(1, 17) for _ in range(bits[length])]
    codes, code, si, p = [], 0, sizes[0] if sizes else 0, 0
    while p < len(sizes):
        while p < len(sizes) and sizes[p] == si:
            codes.append(code)
            code += 1
            p += 1
        code <<= 1
        si += 1
    return sizes, codes


def htable(bits, vals):
    """one sat_jpeg_htable: the LOOKAHEAD-bit lookup ((length << 8) | symbol, 0 for a longer code), maxcode / valoffset of
    every length (maxcode[17] = 0xFFFFF ends the search) and the symbols"""
    t = L.JpegHTable()
    sizes, codes = huffman_codes(bits)
    p = 0
    for length in range(1, 17):
        if bits[length]:
            t.valoffset[length] = p - codes[p]
            p += bits[length]
            t.maxcode[length] = codes[p - 1]
        else:
            t.maxcode[length] = -1
    t.maxcode[17], t.valoffset[17] = 0xFFFFF, 0
    look = np.zeros(1 << LOOKAHEAD, np.uint16)
    for p, (length, code) in enumerate(zip(sizes, codes)):
        if length <= LOOKAHEAD:
            lo = code << (LOOKAHEAD - length)
            look[lo:lo + (1 << (LOOKAHEAD - length))] = (length << 8) | vals[p]
    C.memmove(t.lookup, look.ctypes.data, look.nbytes)
    t.huffval[:len(vals)] = list(vals)
    return t


def qtable(q):
    t = L.JpegQTable()
    t.q[:] = [int(x) for x in q]
    return t


class TableSet:
    """The distinct quantisation and Huffman tables of a batch, deduplicated by content."""

    def __init__(self):
        self.quant, self.huff = [], []
        self._qi, self._hi = {}, {}

    def q(self, q):
        key = q.tobytes()
        if key not in self._qi:
            self._qi[key] = len(self.quant)
            self.quant.append(qtable(q))
        return self._qi[key]

    def h(self, tab):
        key = (tuple(tab[0]), tab[1])
        if key not in self._hi:
            self._hi[key] = len(self.huff)
            self.huff.append(htable(*tab))
        return self._hi[key]


def fill_desc(e, hd, tables):
    """the geometry and table fields of a sat_jpeg_desc; the offsets are the caller's"""
    e.height, e.width, e.components = hd.height, hd.width, hd.components
    e.h_samp, e.v_samp = hd.h_samp, hd.v_samp
    e.restart_interval, e.n_segments = hd.restart_interval, len(hd.segments)
    for c in range(3):
        k = min(c, hd.components - 1)
        e.quant[c], e.dc_table[c], e.ac_table[c] = tables.q(hd.quant[k]), tables.h(hd.dc[k]), tables.h(hd.ac[k])


# ---------------------------------------------------------------------------------------------------------------------- pictures
class JpegDecodeError(OSError):
    """A GPU-decoded picture whose entropy-coded data was bad (truncated, a bad Huffman code, ...).  Pillow raises OSError on such a
    file too."""


STATUS_TEXT = {1: "bad Huffman code", 2: "ran out of data (truncated file)", 4: "coefficient index past 63", 8: "bad restart segment",
               16: "marker inside the entropy-coded data"}


def status_text(code):
    return ", ".join(t for bit, t in STATUS_TEXT.items() if code & bit) or "status %d" % code


class JpegBytes(bytes):
    """The bytes of a GPU-decodable file, with its parsed header: the form in which such a picture travels from ``read_jpeg`` to
    the staging buffer.  ``shape`` is the (height, width, 3) of the decoded picture."""

    header: JpegHeader

    @property
    def shape(self):
        return (self.header.height, self.header.width, 3)


def pillow_decode(data):
    """data.decode_rgb on bytes: the fallback for the files the GPU decoder does not take"""
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def as_picture(item, progressive=False):
    """an (H, W, 3) array stays as it is; JPEG bytes become ``JpegBytes`` when the GPU takes them, else Pillow decodes them here.
    ``progressive``: the GPU also takes the progressive files ``parse(progressive=True)`` admits."""
    if isinstance(item, JpegBytes):
        return item
    if isinstance(item, (bytes, bytearray, memoryview)):
        hd = parse(item, progressive=progressive)
        if hd.fallback is None:
            jb = JpegBytes(item)
            jb.header = hd
            return jb
        return pillow_decode(item)
    return item


def read_jpeg(path):
    """A ``decode=`` function for ``data.CocoCaptionDataset``: the file's bytes (``JpegBytes``) when the GPU decodes it, else
    Pillow's pixels, decoded here on the loader's worker thread as ``data.decode_rgb`` does."""
    with open(path, "rb") as f:
        return as_picture(f.read())


def read_jpeg_progressive(path):
    """``read_jpeg`` that hands progressive files to the GPU as well (``as_picture(progressive=True)``)."""
    with open(path, "rb") as f:
        return as_picture(f.read(), progressive=True)


def _align(x, a):
    return (x + a - 1) // a * a


class JpegBatch:
    """The JPEG part of a staging buffer: [sat_jpeg_desc records | quantisation tables | Huffman tables | sat_jpeg_scan records |
    compressed], where compressed holds, per picture (per scan of a progressive picture), its restart-segment table and its
    entropy-coded data.  The records are the baseline files first, then the progressive ones (``n_baseline`` + ``n_progressive``);
    ``order[j]`` is the index in ``files`` of record j, and ``out_offsets``, ``shapes``, the status words and the info rows are in
    record order (which is the order of ``files`` when they are all of one kind).  The decoded pictures go to
    ``out_base + out_offsets[j]`` of the pixel buffer the caller hands to ``launch``."""

    def __init__(self, files, out_base=0):
        m = self.n = len(files)
        self.order = sorted(range(m), key=lambda j: bool(files[j].header.progressive))          # stable: file order within a kind
        nb = self.n_baseline = sum(1 for f in files if not f.header.progressive)
        self.n_progressive = m - nb
        self.desc = (L.JpegDesc * m)()
        tables = TableSet()
        parts, off, segs, blocks, out = [], 0, 0, 0, out_base
        scans = []                                # (level, record of its picture among the progressive ones, scan, segments_offset, data_offset)
        self.out_offsets, self.shapes = [], []
        for j, i in enumerate(self.order):
            f = files[i]
            hd = f.header
            e = self.desc[j]
            if j == nb:
                segs = blocks = 0                 # the progressive records are a batch of their own to the library
            if hd.progressive:
                e.height, e.width, e.components, e.h_samp, e.v_samp = hd.height, hd.width, hd.components, hd.h_samp, hd.v_samp
                for c in range(3):
                    e.quant[c] = tables.q(hd.quant[min(c, hd.components - 1)])
                for sc in hd.scans:
                    so = off
                    parts.append((off, sc.segments.tobytes()))
                    off += sc.segments.nbytes
                    scans.append((sc.level, j - nb, sc, so, off))
                    parts.append((off, memoryview(f)[sc.data_start:sc.data_end]))
                    off = _align(off + sc.data_end - sc.data_start, 8)
            else:
                fill_desc(e, hd, tables)
                e.segments_offset = off
                parts.append((off, hd.segments.tobytes()))
                off += hd.segments.nbytes
                e.data_offset, e.data_bytes = off, hd.data_end - hd.data_start
                parts.append((off, memoryview(f)[hd.data_start:hd.data_end]))
                off = _align(off + e.data_bytes, 8)
                e.segment_base = segs
                segs += len(hd.segments)
            e.block_offset, e.out_offset = blocks, out
            blocks += hd.blocks()
            self.out_offsets.append(out)
            self.shapes.append((hd.height, hd.width))
            out += hd.height * hd.width * 3
        self.out_bytes = out - out_base
        # the scan records, ordered by level (one entropy launch per level), then by picture and file order
        scans.sort(key=lambda t: t[0])
        self.scans = (L.JpegScan * len(scans))()
        segs = 0
        for r, (level, pic, sc, so, do) in zip(self.scans, scans):
            r.picture, r.level, r.n_components = pic, level, len(sc.comps)
            r.component[:len(sc.comps)] = sc.comps
            r.ss, r.se, r.ah, r.al = sc.ss, sc.se, sc.ah, sc.al
            for k, t in enumerate(sc.dc):
                r.dc_table[k] = tables.h(t) if t is not None else 0
            r.ac_table = tables.h(sc.ac) if sc.ac is not None else 0
            r.restart_interval, r.n_segments, r.segment_base = sc.restart_interval, len(sc.segments), segs
            r.segments_offset, r.data_offset, r.data_bytes = so, do, sc.data_end - sc.data_start
            segs += len(sc.segments)
        self.quant = (L.JpegQTable * len(tables.quant))(*tables.quant)
        self.huff = (L.JpegHTable * len(tables.huff))(*tables.huff)
        self.quant_off = _align(C.sizeof(self.desc), 16)
        self.huff_off = _align(self.quant_off + C.sizeof(self.quant), 16)
        self.scans_off = _align(self.huff_off + C.sizeof(self.huff), 16)
        self.comp_off = _align(self.scans_off + C.sizeof(self.scans), 16)
        self.comp_bytes = max(off, 8)
        self.nbytes = self.comp_off + self.comp_bytes
        self._parts = parts

    def write(self, buf):
        """fill ``buf`` (``nbytes`` uint8, numpy) with the region"""
        for o, obj in ((0, self.desc), (self.quant_off, self.quant), (self.huff_off, self.huff), (self.scans_off, self.scans)):
            if C.sizeof(obj):
                buf[o:o + C.sizeof(obj)] = np.frombuffer(obj, dtype=np.uint8)
        c = self.comp_off
        for o, blob in self._parts:
            buf[c + o:c + o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)

    def _desc(self, first):
        return C.c_void_p(C.addressof(self.desc) + first * C.sizeof(L.JpegDesc))

    def _workspaces(self, subseq_bytes=None, parallel_min_bytes=None):
        """workspace bytes of the baseline and of the progressive records (each a multiple of 16)"""
        base = prog = 0
        if self.n_baseline:
            opts = decode_opts(subseq_bytes, parallel_min_bytes)
            base = L.lib().sat_jpeg_decode_workspace_bytes_ex(self._desc(0), self.n_baseline, C.byref(opts))
            if base == 0:
                L.check(1, "sat_jpeg_decode_workspace_bytes_ex")
        if self.n_progressive:
            prog = L.lib().sat_jpeg_progressive_workspace_bytes(self._desc(self.n_baseline), self.n_progressive, C.cast(self.scans, C.c_void_p),
                                                                len(self.scans))
            if prog == 0:
                L.check(1, "sat_jpeg_progressive_workspace_bytes")
        return _align(base, 16) if prog else base, prog

    def workspace_bytes(self, subseq_bytes=None, parallel_min_bytes=None):
        return sum(self._workspaces(subseq_bytes, parallel_min_bytes))

    def launch(self, region_ptr, pixels_ptr, pixels_bytes, status, workspace, stream, subseq_bytes=None, parallel_min_bytes=None, info=None):
        """sat_jpeg_decode_batch_ex for the baseline records and sat_jpeg_decode_progressive_batch for the progressive ones, on the
        one stream, with the region at device address ``region_ptr``; ``status``: (n,) int32 device tensor; ``info``: None or an
        (n, 4) int32 device tensor (baseline: path, subsequences, synchronisation rounds, 0; progressive: 3, scans, levels, 0)"""
        opts = decode_opts(subseq_bytes, parallel_min_bytes)
        nb, npr = self.n_baseline, self.n_progressive
        info_ptr = 0
        if info is not None:
            L.require_gpu(info)
            assert info.dtype == status.dtype and info.numel() == 4 * self.n and info.is_contiguous()
            info_ptr = info.data_ptr()
            opts.info = info_ptr
        st = C.c_void_p(stream.cuda_stream)
        ws_base = self._workspaces(subseq_bytes, parallel_min_bytes)[0] if npr else workspace.numel()
        if nb:
            L.check(L.lib().sat_jpeg_decode_batch_ex(region_ptr + self.comp_off, self.comp_bytes, self._desc(0), region_ptr, nb,
                                                     region_ptr + self.quant_off, len(self.quant), region_ptr + self.huff_off, len(self.huff),
                                                     pixels_ptr, pixels_bytes, L.ptr(status), L.ptr(workspace), min(ws_base, workspace.numel()), st,
                                                     C.byref(opts)), "sat_jpeg_decode_batch_ex")
        if npr:
            L.check(L.lib().sat_jpeg_decode_progressive_batch(
                region_ptr + self.comp_off, self.comp_bytes, self._desc(nb), region_ptr + nb * C.sizeof(L.JpegDesc), npr,
                C.cast(self.scans, C.c_void_p), region_ptr + self.scans_off, len(self.scans), region_ptr + self.quant_off, len(self.quant),
                region_ptr + self.huff_off, len(self.huff), pixels_ptr, pixels_bytes, L.ptr(status) + 4 * nb, L.ptr(workspace) + ws_base,
                max(workspace.numel() - ws_base, 0), st, info_ptr + 16 * nb if info_ptr else None), "sat_jpeg_decode_progressive_batch")


#: ``parallel_min_bytes`` that keeps every picture on the one-thread-per-segment path
NEVER_PARALLEL = (1 << 63) - 1
#: the library's defaults (SAT_JPEG_SUBSEQ_BYTES_DEFAULT, SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT of include/sat_hip.h)
SUBSEQ_BYTES_DEFAULT = 128
PARALLEL_MIN_BYTES_DEFAULT = 2048


def decode_opts(subseq_bytes=None, parallel_min_bytes=None):
    """sat_jpeg_decode_opts; None: the library's default"""
    return L.JpegDecodeOpts(subseq_bytes=0 if subseq_bytes is None else int(subseq_bytes),
                            parallel_min_bytes=-1 if parallel_min_bytes is None else int(parallel_min_bytes), info=None)


def decode_jpeg_batch(items, device="cuda", check=True, subseq_bytes=None, parallel_min_bytes=None, return_info=False, progressive=False):
    """The decoded (H, W, 3) uint8 tensors on ``device`` of a list of JPEG byte strings (or ``JpegBytes``): the GPU decodes the
    files it takes, Pillow the others.  A bad stream raises ``JpegDecodeError``; with ``check=False`` the call returns
    ``(tensors, status)`` instead, status an (n,) int32 CPU tensor, 0 for a good picture (and for every Pillow-decoded one).
    ``subseq_bytes`` / ``parallel_min_bytes``: the options of ``sat_jpeg_decode_batch_ex`` (None: the library's defaults;
    ``parallel_min_bytes=0`` sends every restart-free picture to the many-thread path, ``NEVER_PARALLEL`` none).  With
    ``return_info`` an (n, 4) int32 CPU tensor comes back as the last value: per picture the path taken (0 one thread per restart
    segment, 1 one thread per subsequence, 2 the latter abandoned for the former), its subsequences, the synchronisation rounds
    run and 0; the row of a Pillow-decoded picture is all -1.  With ``progressive`` the GPU also decodes the progressive files
    ``parse(progressive=True)`` admits; the info row of such a picture is (3, its scans, its dependency levels, 0)."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise L.SatHipError("sat_amd decodes JPEG on the GPU only: got device %s (no CPU fallback)" % device)
    pics = [as_picture(x, progressive=progressive) for x in items]
    gpu = [i for i, p in enumerate(pics) if isinstance(p, JpegBytes)]
    out = [None] * len(pics)
    status = torch.zeros(len(pics), dtype=torch.int32)
    info = torch.full((len(pics), 4), -1, dtype=torch.int32)
    for i, p in enumerate(pics):
        if not isinstance(p, JpegBytes):
            out[i] = torch.from_numpy(np.array(p, dtype=np.uint8, copy=True)).to(device)
    if gpu:
        jb = JpegBatch([pics[i] for i in gpu])
        gpu = [gpu[k] for k in jb.order]          # record order: the baseline files, then the progressive ones
        host = torch.empty(jb.nbytes, dtype=torch.uint8).pin_memory()
        jb.write(host.numpy())
        stream = torch.cuda.current_stream(device)
        region = host.to(device, non_blocking=True)
        pixels = torch.empty(max(jb.out_bytes, 1), dtype=torch.uint8, device=device)
        st = torch.empty(jb.n, dtype=torch.int32, device=device)
        ws = torch.empty(jb.workspace_bytes(subseq_bytes, parallel_min_bytes), dtype=torch.uint8, device=device)
        inf = torch.empty(jb.n, 4, dtype=torch.int32, device=device) if return_info else None
        jb.launch(region.data_ptr(), pixels.data_ptr(), pixels.numel(), st, ws, stream, subseq_bytes, parallel_min_bytes, inf)
        st = st.cpu()
        if return_info:
            info[gpu] = inf.cpu()
        for j, i in enumerate(gpu):
            h, w = jb.shapes[j]
            out[i] = pixels[jb.out_offsets[j]:jb.out_offsets[j] + h * w * 3].view(h, w, 3)
            status[i] = st[j]
    if check:
        bad = [i for i in range(len(pics)) if status[i]]
        if bad:
            raise JpegDecodeError("corrupt JPEG data: " + "; ".join("picture %d: %s" % (i, status_text(int(status[i]))) for i in bad))
        return (out, info) if return_info else out
    return (out, status, info) if return_info else (out, status)
