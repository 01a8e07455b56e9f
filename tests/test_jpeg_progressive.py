"""CPU: progressive JPEG on the host side.  The Python restatement of the four scan types (tests/jpeg_progressive_ref.py) against
Pillow, exactly; ``jpeg.parse(progressive=True)``: scans, bands, dependency levels, per-scan restart segments and tables, the files it
refuses and why; the defaults, which stay what they were (the option is opt-in); the new C-ABI entry points without a GPU.

The parser admits exactly the two scan scripts Pillow writes (``jpeg.PROGRESSIONS``): admission equals tested, so no progressive
encoder for other scripts is kept with the tests."""
import ctypes as C

import numpy as np
import pytest

import sat_amd  # noqa: F401
from sat_amd import _lib as L
from sat_amd import jpeg as J
import jpeg_progressive_ref as P

CASES = P.small_cases()
COLOUR = "420_q100_40x57"


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_pillow(name):
    assert np.array_equal(P.decode(CASES[name]), P.pillow(CASES[name]))


# ---------------------------------------------------------------------------------------------------------------------- parser
def test_scans_bands_and_levels_of_the_colour_script():
    hd = J.parse(CASES[COLOUR], progressive=True)
    assert hd.fallback is None and hd.progressive and (hd.height, hd.width, hd.components, hd.h_samp, hd.v_samp) == (40, 57, 3, 2, 2)
    assert tuple(sc.shape_key for sc in hd.scans) == J.PROGRESSIONS["simple YCbCr"]
    assert [sc.level for sc in hd.scans] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and hd.levels == 3
    assert [(sc.ss, sc.se, sc.ah, sc.al) for sc in hd.scans[:2]] == [(0, 0, 0, 1), (1, 5, 0, 2)]
    assert hd.blocks() == 4 * 3 * 6 and len(hd.quant) == 3
    for sc in hd.scans:
        assert len(sc.segments) == 1 and sc.segments[0].tolist() == [0, sc.data_end - sc.data_start]
        assert (sc.ac is not None) == (sc.ss > 0) and all((t is not None) == (sc.ss == 0 and sc.ah == 0) for t in sc.dc)
    assert CASES[COLOUR][hd.scans[-1].data_end:] == b"\xff\xd9"


def test_grayscale_levels():
    hd = J.parse(CASES["gray_33x65"], progressive=True)
    assert hd.fallback is None and hd.components == 1
    assert tuple(sc.shape_key for sc in hd.scans) == J.PROGRESSIONS["simple grayscale"]
    assert [sc.level for sc in hd.scans] == [0, 0, 0, 1, 1, 2] and hd.levels == 3


def test_restart_segments_and_tables_are_latched_per_scan():
    """4:2:0 with a restart marker per MCU row: the interleaved DC scans count MCUs of the padded 4 x 3 grid, the luma scans the
    8 x 5 blocks that hold samples, the chroma scans their 4 x 3; the DRI in front of every scan says so"""
    hd = J.parse(CASES["420_q100_rst_40x57"], progressive=True)
    assert hd.fallback is None
    assert [(sc.restart_interval, len(sc.segments)) for sc in hd.scans] == [(4, 3), (8, 5), (4, 3), (4, 3), (8, 5), (8, 5), (4, 3), (4, 3), (4, 3), (8, 5)]
    for sc in hd.scans:
        seg = sc.segments.astype(np.int64)
        assert seg[0, 0] == 0 and seg[-1, 1] == sc.data_end - sc.data_start and np.all(seg[1:, 0] == seg[:-1, 1] + 2)
    # every AC scan brings its own DHT under table id 0 or 1: what a scan holds is the table in force at its SOS
    y = [sc.ac for sc in hd.scans if sc.ss and sc.comps == [0]]
    assert len(y) == 4 and len({(tuple(b), v) for b, v in y}) > 1


# ---------------------------------------------------------------------------------------------------------------------- rejections
def _sos(f, sc):
    """offset of the scan's SOS marker"""
    return sc.data_start - (6 + 2 * len(sc.comps)) - 2


def test_refused_files_name_their_reason():
    f = CASES[COLOUR]
    hd = J.parse(f, progressive=True)
    cut = f[:_sos(f, hd.scans[6])]                                            # cut after scan 6: no EOI, incomplete
    assert J.parse(cut, progressive=True).fallback == "truncated"
    unrefined = f[:_sos(f, hd.scans[9])] + b"\xff\xd9"                        # the last luma refinement never comes
    assert J.parse(unrefined, progressive=True).fallback == "incomplete progression"
    wrong_ah = bytearray(f)
    assert wrong_ah[hd.scans[5].data_start - 1] == 0x21
    wrong_ah[hd.scans[5].data_start - 1] = 0x32
    assert J.parse(bytes(wrong_ah), progressive=True).fallback == "refinement out of order"
    bad_al = bytearray(f)
    bad_al[hd.scans[5].data_start - 1] = 0x20
    assert J.parse(bytes(bad_al), progressive=True).fallback == "bad successive approximation"
    no_dc = f[:_sos(f, hd.scans[0])] + f[hd.scans[0].data_end:]               # the first scan is now an AC scan
    assert J.parse(no_dc, progressive=True).fallback == "AC scan before the DC scan"
    mixed = bytearray(f)
    mixed[hd.scans[0].data_start - 2] = 5                                     # Se of the DC scan
    assert J.parse(bytes(mixed), progressive=True).fallback == "progressive scan mixes DC and AC"
    stray = f[:hd.scans[3].data_start + 1] + b"\xff\xff" + f[hd.scans[3].data_start + 1:]
    assert J.parse(stray, progressive=True).fallback in ("fill bytes in the scan", "restart markers do not match the restart interval")
    for bad in (cut, unrefined):
        assert J.parse(bad).fallback == "progressive"


def test_admission_equals_tested():
    """a valid, complete progression that is not one of PROGRESSIONS (the luma bands split at 6 / 7 instead of 5 / 6) falls back"""
    f = bytearray(CASES[COLOUR])
    hd = J.parse(bytes(f), progressive=True)
    assert (hd.scans[1].se, hd.scans[4].ss) == (5, 6)
    f[hd.scans[1].data_start - 2] = 6
    f[hd.scans[4].data_start - 3] = 7
    got = J.parse(bytes(f), progressive=True)
    assert got.fallback == "untested progression" and [sc.level for sc in got.scans] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert isinstance(J.as_picture(CASES[COLOUR], progressive=True), J.JpegBytes)


# ---------------------------------------------------------------------------------------------------------------------- defaults
def test_defaults_are_unchanged(tmp_path):
    f = CASES[COLOUR]
    hd = J.parse(f)
    assert hd.fallback == "progressive" and hd.shape == (40, 57) and not hd.scans
    a = J.as_picture(f)
    assert isinstance(a, np.ndarray) and np.array_equal(a, P.pillow(f))
    p = tmp_path / "p.jpg"
    p.write_bytes(f)
    assert isinstance(J.read_jpeg(str(p)), np.ndarray)
    got = J.read_jpeg_progressive(str(p))
    assert isinstance(got, J.JpegBytes) and got.shape == (40, 57, 3) and got.header.progressive
    base = P.encode(P.picture(40, 57, 1), quality=80, restart_marker_rows=1)
    h0, h1 = J.parse(base), J.parse(base, progressive=True)                   # a baseline file is read the same way with the option
    assert h0.fallback is None and h1.fallback is None and not h1.progressive
    assert np.array_equal(h0.segments, h1.segments) and (h0.data_start, h0.data_end) == (h1.data_start, h1.data_end)


# ---------------------------------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_exported_and_bound():
    lib = L.lib()
    for name in ("sat_jpeg_progressive_workspace_bytes", "sat_jpeg_decode_progressive_batch"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert C.sizeof(L.JpegScan) == 96 and C.sizeof(L.JpegDesc) == 112
    assert (L.JpegScan.picture.offset, L.JpegScan.ss.offset, L.JpegScan.dc_table.offset, L.JpegScan.restart_interval.offset) == (24, 48, 64, 80)
    lib.sat_abi_version.restype = C.c_int
    assert lib.sat_abi_version() == 23


def batch():
    files = [J.as_picture(CASES[n], progressive=True) for n in ("420_q100_rst_40x57", "gray_33x65")]
    files.insert(1, J.as_picture(P.encode(P.picture(24, 24, 2))))
    return J.JpegBatch(files)


def test_batch_layout():
    jb = batch()
    assert (jb.order, jb.n_baseline, jb.n_progressive, len(jb.scans)) == ([1, 0, 2], 1, 2, 16)
    assert [s.level for s in jb.scans] == sorted(s.level for s in jb.scans)
    segs = 0
    for s in jb.scans:
        assert s.segment_base == segs and s.segments_offset % 4 == 0
        segs += s.n_segments
    assert (jb.desc[1].block_offset, jb.desc[2].block_offset) == (0, 72) and jb.desc[1].reserved == 0
    base, prog = jb._workspaces()
    assert prog == 192 * (72 + 5 * 9) and jb.workspace_bytes() == base + prog and base % 16 == 0
    buf = np.zeros(jb.nbytes, np.uint8)
    jb.write(buf)
    sc = jb.scans[0]
    seg = buf[jb.comp_off + sc.segments_offset:][:8].view(np.uint32)
    assert seg[0] == 0 and sc.data_offset == sc.segments_offset + 8 * sc.n_segments


def test_progressive_entry_points_reject_bad_arguments_without_a_gpu():
    """SAT_EINVAL with a message before anything is enqueued: the buffers below are never touched"""
    jb = batch()
    lib = L.lib()
    buf = np.zeros(4096, np.uint8)
    ptr = buf.ctypes.data // 16 * 16 + 16
    nb, npr = jb.n_baseline, jb.n_progressive
    desc, scans = jb._desc(nb), C.cast(jb.scans, C.c_void_p)
    need = jb._workspaces()[1]
    assert lib.sat_jpeg_progressive_workspace_bytes(desc, npr, scans, len(jb.scans)) == need
    assert lib.sat_jpeg_progressive_workspace_bytes(None, npr, scans, len(jb.scans)) == 0 and b"null" in lib.sat_last_error()
    assert lib.sat_jpeg_progressive_workspace_bytes(desc, npr, None, 0) == 0 and b"null" in lib.sat_last_error()

    def call(desc_host=desc, scans_host=scans, ws=ptr, ws_bytes=1 << 40, n_scans=len(jb.scans)):
        return lib.sat_jpeg_decode_progressive_batch(ptr, jb.comp_bytes, desc_host, ptr, npr, scans_host, ptr, n_scans, ptr, len(jb.quant), ptr,
                                                     len(jb.huff), ptr, jb.out_bytes, ptr, ws, ws_bytes, None, None)
    assert call(desc_host=None) == 1 and b"null" in lib.sat_last_error()
    assert call(scans_host=None) == 1 and b"null" in lib.sat_last_error()
    assert call(ws=None) == 1 and b"workspace" in lib.sat_last_error()
    assert call(ws_bytes=need - 1) == 1 and b"workspace" in lib.sat_last_error()
    for field, value, text in (("picture", 2, b"picture"), ("level", 5, b"level"), ("se", 64, b"band"), ("al", 14, b"approximation"),
                               ("n_segments", 2, b"segments"), ("segment_base", 7, b"segment_base"), ("data_bytes", 1 << 40, b"outside"),
                               ("ac_table", 99, b"table"), ("n_components", 2, b"components")):
        s = jb.scans[6]                                                       # an AC first scan of level 0 in the middle of the array
        assert s.ss > 0 and s.ah == 0
        old = getattr(s, field)
        setattr(s, field, value)
        assert call() == 1 and text in lib.sat_last_error(), field
        setattr(s, field, old)
    assert call(ws_bytes=need - 1) == 1 and b"workspace" in lib.sat_last_error()          # the records are good again: the last check


def test_python_surface_refuses_the_cpu():
    with pytest.raises(L.SatHipError):
        J.decode_jpeg_batch([CASES[COLOUR]], "cpu", progressive=True)
