"""CPU: the JPEG header parser and table builder (sat_amd/jpeg.py) and the numpy restatement of the GPU decoder's integer
pipeline (tests/jpeg_ref.py) against Pillow, byte for byte; the g15 fixture; the staging layout of a batch of JPEG bytes."""
import io
import os

import numpy as np
import pytest
import torch

import sat_amd  # noqa: F401
from sat_amd import data as D
from sat_amd import jpeg as J
import jpeg_ref as R

from PIL import Image


def picture(h, w, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, noise, (h, w, 3))), 0, 255).astype(np.uint8)


def encode(a, fmt="JPEG", **kw):
    buf = io.BytesIO()
    (a if isinstance(a, Image.Image) else Image.fromarray(a)).save(buf, fmt, **kw)
    return buf.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_jpeg.npz"), allow_pickle=False)


SIZES = [(1, 1), (1, 17), (17, 1), (15, 16), (17, 9), (33, 65)]


@pytest.mark.parametrize("quality", [10, 75, 95, 100])
@pytest.mark.parametrize("mode", ["444", "422", "420", "gray"])
def test_restatement_equals_pillow(quality, mode):
    for h, w in SIZES:
        a = picture(h, w, quality + h * 7 + w, noise=60.0 if quality == 100 else 12.0)     # high-frequency noise at 100
        if mode == "gray":
            f = encode(a[:, :, 0], quality=quality)
        else:
            f = encode(a, quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[mode])
        hd = J.parse(f)
        assert hd.fallback is None and hd.shape == (h, w)
        assert hd.components == (1 if mode == "gray" else 3)
        assert (hd.h_samp, hd.v_samp) == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[mode]
        assert np.array_equal(R.decode(f), pillow(f)), (h, w)


@pytest.mark.parametrize("ss", [0, 2])
def test_restatement_equals_pillow_480x640(ss):
    f = encode(picture(480, 640, 1), quality=90, subsampling=ss)
    assert np.array_equal(R.decode(f), pillow(f))


@pytest.mark.parametrize("kw", [dict(optimize=True), dict(restart_marker_blocks=1), dict(restart_marker_blocks=7), dict(restart_marker_rows=1),
                                dict(restart_marker_rows=2, optimize=True)])
@pytest.mark.parametrize("mode", ["444", "422", "420", "gray"])
def test_optimized_tables_and_restart_markers(kw, mode):
    a = picture(41, 70, 9)
    f = encode(a[:, :, 1], quality=80, **kw) if mode == "gray" else encode(a, quality=80, subsampling={"444": 0, "422": 1, "420": 2}[mode], **kw)
    hd = J.parse(f)
    assert hd.fallback is None
    if "restart_marker_blocks" in kw or "restart_marker_rows" in kw:
        assert hd.restart_interval > 0 and len(hd.segments) == -(-np.prod(hd.mcus()) // hd.restart_interval) > 1
    else:
        assert len(hd.segments) == 1
    assert np.array_equal(R.decode(f), pillow(f))


def test_classification_sends_other_files_to_pillow():
    a = picture(24, 40, 2)
    cases = {"progressive": encode(a, quality=80, progressive=True), "CMYK": encode(Image.fromarray(a).convert("CMYK"), quality=80),
             "Adobe RGB": encode(a, quality=80, keep_rgb=True), "PNG": encode(a, "PNG"), "empty": b"", "truncated header": encode(a)[:40]}
    for name, f in cases.items():
        hd = J.parse(f)
        assert hd.fallback is not None, name
        if name != "PNG" and name != "empty" and name != "truncated header":
            assert np.array_equal(J.as_picture(f), pillow(f)), name           # decoded by Pillow, as decode_rgb does
    assert J.parse(cases["progressive"]).shape == (24, 40)


def test_component_ids_and_adobe_transform_follow_libjpeg():
    """default_decompress_parms: JFIF -> YCbCr; without JFIF an Adobe transform 0 -> RGB (fallback), ids 'R','G','B' -> RGB"""
    f = encode(picture(16, 16, 3), quality=80)
    assert f[2:4] == b"\xff\xe0"
    app0 = 4 + ((f[4] << 8) | f[5])
    no_jfif = f[:2] + f[app0:]
    assert J.parse(no_jfif).fallback is None                                  # ids 1, 2, 3: YCbCr
    sof = no_jfif.index(b"\xff\xc0")
    rgb_ids = bytearray(no_jfif)
    for k, cid in enumerate(b"RGB"):
        rgb_ids[sof + 10 + 3 * k] = cid
    sos = rgb_ids.index(b"\xff\xda")
    for k, cid in enumerate(b"RGB"):
        rgb_ids[sos + 5 + 2 * k] = cid
    assert J.parse(bytes(rgb_ids)).fallback == "RGB components"
    adobe = lambda t: no_jfif[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + no_jfif[2:]     # noqa: E731
    assert J.parse(adobe(0)).fallback == "Adobe RGB"
    assert J.parse(adobe(1)).fallback is None
    assert np.array_equal(R.decode(adobe(1)), pillow(adobe(1)))


def test_fixture(g15):
    assert sum(os.path.getsize(p) for p in [os.path.join(os.path.dirname(__file__), "golden", "g15_jpeg.npz")]) < 1 << 20
    for i, name in enumerate(g15["cases"]):
        f = g15["jpeg%d" % i].tobytes()
        assert (J.parse(f).fallback is None) == bool(g15["gpu"][i]), name
        if g15["gpu"][i]:
            assert np.array_equal(R.decode(f), g15["rgb%d" % i]), name


def test_range_limit_is_libjpegs_table():
    """jdmaster.c prepare_range_limit_table, built the way libjpeg builds it, read at IDCT_range_limit = sample_range_limit + 128"""
    table = np.zeros(5 * 256 + 128, np.int64)
    srl = 256                                                                  # sample_range_limit
    table[srl:srl + 256] = np.arange(256)
    table[srl + 128 + 128:srl + 128 + 512] = 255
    table[srl + 128 + 1024 - 128:srl + 128 + 1024] = np.arange(128)
    assert np.array_equal(R.range_limit_table(), table[srl + 128:srl + 128 + 1024])
    x = np.array([-600, -513, -512, -129, -128, 0, 127, 128, 511, 512, 700])
    assert R.range_limit_table()[x & 1023].tolist() == [255, 255, 0, 0, 0, 128, 255, 255, 255, 0, 0]     # a wrap, not a clamp


def test_huffman_tables_decode_every_code():
    a = picture(20, 30, 4)
    hd = J.parse(encode(a, quality=60, optimize=True))
    for bits, vals in hd.dc + hd.ac:
        t = J.htable(bits, vals)
        sizes, codes = J.huffman_codes(bits)
        for p, (length, code) in enumerate(zip(sizes, codes)):
            if length <= J.LOOKAHEAD:
                e = t.lookup[code << (J.LOOKAHEAD - length)]
                assert (e >> 8, e & 255) == (length, vals[p])
            else:
                assert code <= t.maxcode[length] and t.huffval[code + t.valoffset[length]] == vals[p]
        assert t.maxcode[17] == 0xFFFFF


def test_truncated_file_keeps_its_shape_and_its_segments():
    f = encode(picture(64, 96, 5), quality=90, restart_marker_rows=1)
    hd = J.parse(f[:len(f) // 2])
    assert hd.fallback is None and hd.truncated and hd.shape == (64, 96)
    assert hd.segments[-1, 0] == hd.segments[-1, 1]                          # the missing segments are empty
    with pytest.raises(R.StreamError):
        R.decode(f[:len(f) // 2])


def test_staging_jpeg_bytes_draws_as_arrays_do():
    files = [encode(picture(50 + 9 * k, 70 - 4 * k, k), quality=85, subsampling=k % 3) for k in range(5)]
    files.append(encode(picture(30, 40, 9), quality=85, progressive=True))
    arrays = [pillow(f) for f in files]
    tf = D.BatchTransform(32, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=0.3)
    torch.manual_seed(3)
    da = tf.draw([a.shape[:2] for a in arrays])
    torch.manual_seed(3)
    st = tf.stage(files)
    torch.manual_seed(3)
    assert tf.draw([J.as_picture(f).shape[:2] for f in files]) == da
    assert st.jpeg is not None and st.jpeg.n == 5 and st.jpeg_index == [0, 1, 2, 3, 4]
    assert st.pixels_bytes == sum(a.size for a in arrays)
    assert st.desc[5].offset == 0 and [st.desc[i].offset for i in range(5)] == st.jpeg.out_offsets
    e = st.jpeg.desc
    assert [e[j].block_offset for j in range(5)] == list(np.cumsum([0] + [J.as_picture(f).header.blocks() for f in files[:4]]))
    assert st.host.numel() == st.head + arrays[5].size and st.device_bytes == st.head + st.pixels_bytes
