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


def parse(data) -> JpegHeader:
    """Walk the markers up to the entropy-coded data of the first scan and find its restart markers."""
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
            if m in (0xC0, 0xC1):
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
                while p < end:
                    tc, th = b[p] >> 4, b[p] & 15
                    bits = [0] + list(b[p + 1:p + 17])
                    cnt = sum(bits)
                    vals = bytes(b[p + 17:p + 17 + cnt])
                    why = _check_huffman(bits, vals, tc == 0)
                    if why or tc > 1 or th > 3:
                        hd.fallback = why or "bad Huffman table id"
                        return hd
                    (dc if tc == 0 else ac)[th] = (bits, vals)
                    p += 17 + cnt
            elif m == 0xCC:
                hd.fallback = "arithmetic coding"
                return hd
            elif m == 0xDB:
                while p < end:
                    pq, tq = b[p] >> 4, b[p] & 15
                    if pq:
                        zz = np.frombuffer(bytes(b[p + 1:p + 129]), dtype=">u2").astype(np.uint16)
                        p += 129
                    else:
                        zz = np.frombuffer(bytes(b[p + 1:p + 65]), dtype=np.uint8).astype(np.uint16)
                        p += 65
                    if tq > 3 or zz.size != 64:
                        hd.fallback = "bad quantisation table"
                        return hd
                    q = np.zeros(64, np.uint16)
                    q[NATURAL_ORDER] = zz
                    quant[tq] = q
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


def _finish(hd, b, start, frame, sel, quant, dc, ac, jfif, adobe, adobe_transform):
    nf = len(frame)
    if nf == 3:
        # jdapimin.c default_decompress_parms: JFIF -> YCbCr; else Adobe transform 0 -> RGB; else component ids 'R','G','B' -> RGB
        if not jfif and adobe and adobe_transform == 0:
            hd.fallback = "Adobe RGB"
            return hd
        if not jfif and not adobe and [f[0] for f in frame] == [82, 71, 66]:
            hd.fallback = "RGB components"
            return hd
        if (frame[0][1], frame[0][2]) not in _SAMPLING or any((f[1], f[2]) != (1, 1) for f in frame[1:]):
            hd.fallback = "sampling factors"
            return hd
        hd.h_samp, hd.v_samp = frame[0][1], frame[0][2]
    elif not (1 <= frame[0][1] <= 4 and 1 <= frame[0][2] <= 4):
        hd.fallback = "sampling factors"
        return hd                     # one component: a non-interleaved scan, one block per MCU whatever the factors
    hd.components = nf
    for (cid, h, v, tq), (_, td, ta) in zip(frame, sel):
        if tq not in quant or td not in dc or ta not in ac:
            hd.fallback = "missing table"
            return hd
        hd.quant.append(quant[tq])
        hd.dc.append(dc[td])
        hd.ac.append(ac[ta])
    # the end of the scan and its restart markers: a vectorised scan for 0xFF followed by anything but 0x00
    arr = np.frombuffer(bytes(b[start:]) if not isinstance(b, (bytes, bytearray)) else b, dtype=np.uint8,
                        offset=0 if not isinstance(b, (bytes, bytearray)) else start)
    ff = np.flatnonzero(arr[:-1] == 0xFF)
    nxt = arr[ff + 1]
    mk = nxt != 0
    pos, code = ff[mk], nxt[mk]
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
    ri = hd.restart_interval
    n_seg = (mx * my + ri - 1) // ri if ri else 1
    if pos.size > n_seg - 1 or (pos.size < n_seg - 1 and not hd.truncated):
        hd.fallback = "restart markers do not match the restart interval"
        return hd
    if np.any(code != 0xD0 + (np.arange(code.size) & 7)):
        hd.fallback = "restart markers out of sequence"
        return hd
    starts = np.concatenate([[0], pos + 2]).astype(np.int64)
    ends = np.concatenate([pos, [data_end]]).astype(np.int64)
    seg = np.full((n_seg, 2), data_end, dtype=np.uint32)          # a truncated file: the missing segments are empty
    seg[:starts.size, 0], seg[:starts.size, 1] = starts, ends
    hd.segments = seg
    hd.data_start, hd.data_end = start, start + data_end
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


def as_picture(item):
    """an (H, W, 3) array stays as it is; JPEG bytes become ``JpegBytes`` when the GPU takes them, else Pillow decodes them here"""
    if isinstance(item, JpegBytes):
        return item
    if isinstance(item, (bytes, bytearray, memoryview)):
        hd = parse(item)
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


def _align(x, a):
    return (x + a - 1) // a * a


class JpegBatch:
    """The JPEG part of a staging buffer: [sat_jpeg_desc records | quantisation tables | Huffman tables | compressed], where
    compressed holds, per picture, its restart-segment table and its entropy-coded data.  The decoded pictures go to
    ``out_base + out_offsets[j]`` of the pixel buffer the caller hands to ``launch``."""

    def __init__(self, files, out_base=0):
        m = self.n = len(files)
        self.desc = (L.JpegDesc * m)()
        tables = TableSet()
        parts, off, segs, blocks, out = [], 0, 0, 0, out_base
        self.out_offsets, self.shapes = [], []
        for j, f in enumerate(files):
            hd = f.header
            e = self.desc[j]
            fill_desc(e, hd, tables)
            e.segments_offset = off
            parts.append((off, hd.segments.tobytes()))
            off += hd.segments.nbytes
            e.data_offset, e.data_bytes = off, hd.data_end - hd.data_start
            parts.append((off, memoryview(f)[hd.data_start:hd.data_end]))
            off = _align(off + e.data_bytes, 8)
            e.segment_base, e.block_offset, e.out_offset = segs, blocks, out
            segs += len(hd.segments)
            blocks += hd.blocks()
            self.out_offsets.append(out)
            self.shapes.append((hd.height, hd.width))
            out += hd.height * hd.width * 3
        self.out_bytes = out - out_base
        self.quant = (L.JpegQTable * len(tables.quant))(*tables.quant)
        self.huff = (L.JpegHTable * len(tables.huff))(*tables.huff)
        self.quant_off = _align(C.sizeof(self.desc), 16)
        self.huff_off = _align(self.quant_off + C.sizeof(self.quant), 16)
        self.comp_off = _align(self.huff_off + C.sizeof(self.huff), 16)
        self.comp_bytes = max(off, 8)
        self.nbytes = self.comp_off + self.comp_bytes
        self._parts = parts

    def write(self, buf):
        """fill ``buf`` (``nbytes`` uint8, numpy) with the region"""
        for o, obj in ((0, self.desc), (self.quant_off, self.quant), (self.huff_off, self.huff)):
            buf[o:o + C.sizeof(obj)] = np.frombuffer(obj, dtype=np.uint8)
        c = self.comp_off
        for o, blob in self._parts:
            buf[c + o:c + o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)

    def workspace_bytes(self, subseq_bytes=None, parallel_min_bytes=None):
        opts = decode_opts(subseq_bytes, parallel_min_bytes)
        need = L.lib().sat_jpeg_decode_workspace_bytes_ex(C.cast(self.desc, C.c_void_p), self.n, C.byref(opts))
        if need == 0:
            L.check(1, "sat_jpeg_decode_workspace_bytes_ex")
        return need

    def launch(self, region_ptr, pixels_ptr, pixels_bytes, status, workspace, stream, subseq_bytes=None, parallel_min_bytes=None, info=None):
        """sat_jpeg_decode_batch_ex with the region at device address ``region_ptr``; ``status``: (n,) int32 device tensor;
        ``info``: None or an (n, 4) int32 device tensor (path, subsequences, synchronisation rounds, 0 per picture)"""
        opts = decode_opts(subseq_bytes, parallel_min_bytes)
        if info is not None:
            L.require_gpu(info)
            assert info.dtype == status.dtype and info.numel() == 4 * self.n and info.is_contiguous()
            opts.info = info.data_ptr()
        L.check(L.lib().sat_jpeg_decode_batch_ex(region_ptr + self.comp_off, self.comp_bytes, C.cast(self.desc, C.c_void_p), region_ptr, self.n,
                                                 region_ptr + self.quant_off, len(self.quant), region_ptr + self.huff_off, len(self.huff),
                                                 pixels_ptr, pixels_bytes, L.ptr(status), L.ptr(workspace), workspace.numel(),
                                                 C.c_void_p(stream.cuda_stream), C.byref(opts)), "sat_jpeg_decode_batch_ex")


#: ``parallel_min_bytes`` that keeps every picture on the one-thread-per-segment path
NEVER_PARALLEL = (1 << 63) - 1
#: the library's defaults (SAT_JPEG_SUBSEQ_BYTES_DEFAULT, SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT of include/sat_hip.h)
SUBSEQ_BYTES_DEFAULT = 128
PARALLEL_MIN_BYTES_DEFAULT = 2048


def decode_opts(subseq_bytes=None, parallel_min_bytes=None):
    """sat_jpeg_decode_opts; None: the library's default"""
    return L.JpegDecodeOpts(subseq_bytes=0 if subseq_bytes is None else int(subseq_bytes),
                            parallel_min_bytes=-1 if parallel_min_bytes is None else int(parallel_min_bytes), info=None)


def decode_jpeg_batch(items, device="cuda", check=True, subseq_bytes=None, parallel_min_bytes=None, return_info=False):
    """The decoded (H, W, 3) uint8 tensors on ``device`` of a list of JPEG byte strings (or ``JpegBytes``): the GPU decodes the
    files it takes, Pillow the others.  A bad stream raises ``JpegDecodeError``; with ``check=False`` the call returns
    ``(tensors, status)`` instead, status an (n,) int32 CPU tensor, 0 for a good picture (and for every Pillow-decoded one).
    ``subseq_bytes`` / ``parallel_min_bytes``: the options of ``sat_jpeg_decode_batch_ex`` (None: the library's defaults;
    ``parallel_min_bytes=0`` sends every restart-free picture to the many-thread path, ``NEVER_PARALLEL`` none).  With
    ``return_info`` an (n, 4) int32 CPU tensor comes back as the last value: per picture the path taken (0 one thread per restart
    segment, 1 one thread per subsequence, 2 the latter abandoned for the former), its subsequences, the synchronisation rounds
    run and 0; the row of a Pillow-decoded picture is all -1."""
    import torch
    device = torch.device(device)
    if device.type != "cuda":
        raise L.SatHipError("sat_amd decodes JPEG on the GPU only: got device %s (no CPU fallback)" % device)
    pics = [as_picture(x) for x in items]
    gpu = [i for i, p in enumerate(pics) if isinstance(p, JpegBytes)]
    out = [None] * len(pics)
    status = torch.zeros(len(pics), dtype=torch.int32)
    info = torch.full((len(pics), 4), -1, dtype=torch.int32)
    for i, p in enumerate(pics):
        if not isinstance(p, JpegBytes):
            out[i] = torch.from_numpy(np.array(p, dtype=np.uint8, copy=True)).to(device)
    if gpu:
        jb = JpegBatch([pics[i] for i in gpu])
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
