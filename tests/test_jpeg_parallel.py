"""CPU: the restatement of the many-lane entropy decoding (tests/jpeg_sync_ref.py) against the serial restatement
(tests/jpeg_ref.py) on pictures chosen for where lanes can go wrong; the _ex entry points of the C ABI: exported, bound, and
rejecting bad options without a GPU."""
import ctypes as C
import io

import numpy as np
import pytest

import sat_amd  # noqa: F401
from sat_amd import _lib as L
from sat_amd import jpeg as J
import jpeg_ref as R
import jpeg_sync_ref as S

from PIL import Image


def picture(h, w, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, noise, (h, w, 3))), 0, 255).astype(np.uint8)


def encode(a, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pictures():
    """name -> (file, the subseq_bytes it is decoded at): the pictures of tests/test_gpu_jpeg_parallel.py"""
    return {"noise_96x128_q100_444": (encode(picture(96, 128, 4, noise=70.0), quality=100, subsampling=0), (16, 32, 128)),
            "odd_97x131_q75_420": (encode(picture(97, 131, 5), quality=75, subsampling=2), (16,)),
            "optimized_64x96_q95_422": (encode(picture(64, 96, 6), quality=95, subsampling=1, optimize=True), (16,)),
            "flat_gray_256x256": (encode(np.full((256, 256), 128, np.uint8)), (16,)),
            "ramp_gray_64x256": (encode(np.repeat(np.linspace(0, 255, 256).astype(np.uint8)[None, :], 64, 0)), (16,))}


PICTURES = pictures()
CASES = [(name, s) for name, (_, ss) in PICTURES.items() for s in ss]


@pytest.fixture(scope="module")
def decoded():
    """the serial restatement's coefficients, once per picture"""
    out = {}
    for name, (f, _) in PICTURES.items():
        hd = J.parse(f)
        assert hd.fallback is None and len(hd.segments) == 1, name
        out[name] = (hd, R.decode_coefficients(f, hd)[0])
    return out


@pytest.mark.parametrize("name,subseq", CASES, ids=["%s-%d" % c for c in CASES])
def test_many_lanes_equal_the_serial_restatement(decoded, name, subseq):
    f = PICTURES[name][0]
    hd, ref = decoded[name]
    got, stats = S.decode_coefficients(f, hd, subseq)
    assert np.array_equal(got, ref)
    assert stats["subsequences"] == -(-(hd.data_end - hd.data_start) // subseq)
    assert 1 <= stats["iterations"] <= stats["subsequences"]


def test_the_pictures_have_the_properties_they_were_chosen_for(decoded):
    f = PICTURES["noise_96x128_q100_444"][0]
    hd, _ = decoded["noise_96x128_q100_444"]
    assert hd.data_end - hd.data_start == 47804
    assert -(-47804 // 16) == 2988 > 1024                                     # more subsequences than a workgroup has threads
    assert [S.stuffed_boundaries(f, hd, s) for s in (16, 32, 128)] == [15, 7, 2]
    for s in (16, 32, 128):
        assert S.decode_coefficients(f, hd, s)[1]["max_lane_rounds"] >= 2     # a lane that needs two or more rounds
    hd, _ = decoded["odd_97x131_q75_420"]
    assert (hd.h_samp, hd.v_samp, hd.components) == (2, 2, 3) and hd.height % 16 and hd.width % 16      # 6 slots, partial MCUs
    hd, _ = decoded["optimized_64x96_q95_422"]
    assert max(length for bits, _ in hd.dc + hd.ac for length in range(1, 17) if bits[length]) > J.LOOKAHEAD
    hd, ref = decoded["flat_gray_256x256"]
    assert hd.data_end - hd.data_start == 768 and hd.blocks() == 1024 and hd.blocks() / 48 > 20       # > 20 blocks a lane
    assert np.all(ref[1:, 0] == ref[0, 0]) and not ref[:, 1:].any()           # every DC difference behind the first is zero
    hd, ref = decoded["ramp_gray_64x256"]
    assert len(set(ref[:32, 0].tolist())) > 16                                # DC differences that are not zero, across lanes
    assert -(-(hd.data_end - hd.data_start) // 16) > 8


def test_a_marker_or_a_cut_stream_comes_up_short():
    f = PICTURES["optimized_64x96_q95_422"][0]
    hd = J.parse(f[:len(f) // 2])
    assert hd.fallback is None and hd.truncated
    with pytest.raises(S.ParallelShort):
        S.decode_coefficients(f[:len(f) // 2], hd, 16)


# ---------------------------------------------------------------------------------------------------------------------- C ABI
def test_ex_symbols_are_exported_and_bound():
    lib = L.lib()
    for name in ("sat_jpeg_decode_workspace_bytes_ex", "sat_jpeg_decode_batch_ex"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(L.JpegDecodeOpts) == 24
    assert (L.JpegDecodeOpts.subseq_bytes.offset, L.JpegDecodeOpts.parallel_min_bytes.offset, L.JpegDecodeOpts.info.offset) == (0, 8, 16)
    lib.sat_abi_version.restype = C.c_int
    assert lib.sat_abi_version() == 23


def batch():
    files = [J.as_picture(PICTURES[n][0]) for n in ("noise_96x128_q100_444", "flat_gray_256x256")]
    return J.JpegBatch(files)


def test_workspace_grows_as_the_subsequences_shrink():
    jb = batch()
    never = jb.workspace_bytes(parallel_min_bytes=J.NEVER_PARALLEL)
    sizes = [jb.workspace_bytes(s, 0) for s in (1024, 128, 32, 16)]
    assert never < sizes[0] < sizes[1] < sizes[2] < sizes[3]
    subs = lambda s: -(-47804 // s) - (-768 // s)                              # noqa: E731
    assert sizes[3] - sizes[1] == 24 * (subs(16) - subs(128))                 # 24 bytes of state per subsequence
    assert jb.workspace_bytes(16, 1000) == jb.workspace_bytes(16, 0) - 24 * 48     # the 768-byte picture stays serial
    assert jb.workspace_bytes() == jb.workspace_bytes(J.SUBSEQ_BYTES_DEFAULT, J.PARALLEL_MIN_BYTES_DEFAULT)
    lib = L.lib()
    assert lib.sat_jpeg_decode_workspace_bytes(C.cast(jb.desc, C.c_void_p), jb.n) == jb.workspace_bytes()


@pytest.mark.parametrize("subseq", [8, 12, 18, 130, -16, (1 << 20) + 4])
def test_workspace_bytes_ex_rejects_a_bad_subseq_bytes(subseq):
    jb = batch()
    lib = L.lib()
    opts = J.decode_opts(subseq, 0)
    assert lib.sat_jpeg_decode_workspace_bytes_ex(C.cast(jb.desc, C.c_void_p), jb.n, C.byref(opts)) == 0
    assert b"subseq_bytes" in lib.sat_last_error()
    with pytest.raises(L.SatHipError):
        jb.workspace_bytes(subseq, 0)


def test_decode_batch_ex_rejects_bad_options_without_a_gpu():
    """SAT_EINVAL with a message before anything is enqueued: the buffers below are never touched"""
    jb = batch()
    lib = L.lib()
    buf = np.zeros(4096, np.uint8)                                            # stands in for every device buffer
    ptr = buf.ctypes.data // 16 * 16 + 16
    desc = C.cast(jb.desc, C.c_void_p)

    def call(desc_host, ws_bytes, opts):
        return lib.sat_jpeg_decode_batch_ex(ptr, jb.comp_bytes, desc_host, ptr, jb.n, ptr, len(jb.quant), ptr, len(jb.huff), ptr, jb.out_bytes,
                                            ptr, ptr, ws_bytes, None, C.byref(opts) if opts is not None else None)
    for subseq in (8, 18, -4):
        assert call(desc, 1 << 40, J.decode_opts(subseq, 0)) == 1 and b"subseq_bytes" in lib.sat_last_error()
    assert call(desc, 1 << 40, J.decode_opts(16, -2)) == 1 and b"parallel_min_bytes" in lib.sat_last_error()
    assert call(None, 1 << 40, J.decode_opts(16, 0)) == 1 and b"null" in lib.sat_last_error()
    need = jb.workspace_bytes(16, 0)
    assert call(desc, need - 1, J.decode_opts(16, 0)) == 1 and b"workspace" in lib.sat_last_error()
    assert call(desc, jb.workspace_bytes() - 1, None) == 1 and b"workspace" in lib.sat_last_error()
    assert call(desc, jb.workspace_bytes(128, 0), J.decode_opts(16, 0)) == 1 and b"workspace" in lib.sat_last_error()


def test_python_options_reach_the_library():
    o = J.decode_opts()
    assert (o.subseq_bytes, o.parallel_min_bytes, o.info) == (0, -1, None)
    o = J.decode_opts(32, J.NEVER_PARALLEL)
    assert (o.subseq_bytes, o.parallel_min_bytes) == (32, (1 << 63) - 1)
    from sat_amd import data as D
    tf = D.BatchTransform(56, jpeg_subseq_bytes=32, jpeg_parallel_min_bytes=0)
    assert (tf.jpeg_subseq_bytes, tf.jpeg_parallel_min_bytes) == (32, 0)
    assert (D.BatchTransform(56).jpeg_subseq_bytes, D.BatchTransform(56).jpeg_parallel_min_bytes) == (None, None)
    import torch
    with pytest.raises(L.SatHipError):
        J.decode_jpeg_batch([PICTURES["flat_gray_256x256"][0]], "cpu", subseq_bytes=16, parallel_min_bytes=0, return_info=True)
    assert torch.iinfo(torch.int64).max == J.NEVER_PARALLEL
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sat_hip.h")).read()
    assert int(re.search(r"#define SAT_JPEG_SUBSEQ_BYTES_DEFAULT (\d+)", header).group(1)) == J.SUBSEQ_BYTES_DEFAULT
    assert int(re.search(r"#define SAT_JPEG_PARALLEL_MIN_BYTES_DEFAULT (\d+)", header).group(1)) == J.PARALLEL_MIN_BYTES_DEFAULT
