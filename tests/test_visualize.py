"""CPU: the arithmetic behind the attention overlays (csrc/attention_panels.hip, sat_amd/visualize.py) pinned against Pillow before
any GPU is involved: the integer restatement of the BICUBIC resample, util.py's crop_center box, the blend rule, the contact sheet's
grid, the rounding margin of the mask arrays the GPU test compares exactly, and the C ABI's argument checks (they return before
anything is launched, so they run without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

import attention_panels_ref as R


@pytest.mark.parametrize("shape_in,shape_out", R.RESAMPLE_CASES, ids=["%dx%d_to_%dx%d" % (a + b) for a, b in R.RESAMPLE_CASES])
def test_integer_restatement_equals_pillow_bicubic(shape_in, shape_out):
    noise = np.random.RandomState(3).randint(0, 256, shape_in + (3,)).astype(np.uint8)
    for channels in (3, 1):                                       # RGB and L
        for a in (R.picture(*shape_in, 7, channels), noise if channels == 3 else noise[..., 0]):
            want = np.asarray(Image.fromarray(a).resize((shape_out[1], shape_out[0]), Image.BICUBIC))
            assert np.array_equal(R.resample_int(a, *shape_out), want), (shape_in, shape_out, channels)


def test_default_resize_filter_is_bicubic_and_centre_crop_then_resize():
    a = R.picture(61, 45, 11)
    box = R.crop_box(61, 45)
    assert box == (0, 8, 45, 53)
    cropped = a[box[1]:box[3], box[0]:box[2]]
    assert np.array_equal(R.square(a, 32), R.resample_int(cropped, 32, 32))
    b = R.picture(480, 640, 12)
    assert np.array_equal(R.square(b, 256), R.resample_int(b[:, 80:560], 256, 256))


def test_grey_mask_resized_as_rgb_equals_the_l_mode_resize():
    for hw in ((7, 7), (14, 14), (10, 7), (1, 1), (1, 5)):
        m = R.picture(*hw, 5, 1).reshape(hw)
        rgb = np.asarray(Image.fromarray(m).convert("RGB").resize((64, 64)))
        assert all(np.array_equal(rgb[..., c], R.resample_int(m, 64, 64)) for c in range(3))


def test_crop_box_equals_the_reference_squares(golden_dir):
    """square_in / square_out of g11 were captured from util.py's crop_max_square(img, None): odd and even margins, both orientations"""
    g = np.load(os.path.join(golden_dir, "g11_input_pipeline.npz"))
    seen = set()
    for i in range(3):
        a, want = g["square_in%d" % i], g["square_out%d" % i]
        left, top, right, lower = R.crop_box(a.shape[0], a.shape[1])
        assert (right - left, lower - top) == want.shape[:2] == (min(a.shape[:2]),) * 2
        assert np.array_equal(a[top:lower, left:right], want)
        assert np.array_equal(R.square(a, None), want)
        seen.add(((a.shape[1] - want.shape[1]) % 2, a.shape[0] > a.shape[1]))
    assert len(seen) >= 2
    for h, w in ((5, 8), (8, 5), (6, 9), (9, 9), (1, 4)):         # the box is always min-side square, whatever the parities
        left, top, right, lower = R.crop_box(h, w)
        assert right - left == lower - top == min(h, w) and left == (w - min(h, w)) // 2 and top == (h - min(h, w)) // 2


def test_blend_rule_equals_image_blend():
    p, m = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    got = np.asarray(Image.blend(Image.fromarray(p), Image.fromarray(m), 0.75))
    assert np.array_equal(got, R.blend_rule(p.astype(np.int64), m.astype(np.int64)))
    f = (p.astype(np.float32) + np.float32(0.75) * (m.astype(np.float32) - p.astype(np.float32))).astype(np.uint8)
    assert np.array_equal(got, f)
    half = (p.astype(np.float32) + np.float32(0.5) * (m.astype(np.float32) - p.astype(np.float32))).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.blend(Image.fromarray(p), Image.fromarray(m), 0.5)), half)


@pytest.mark.parametrize("name", sorted(R.PANEL_CASES))
def test_mask_arrays_keep_their_distance_from_a_truncation_boundary(name):
    """The mask is uint8(255 * x ** power) by truncation after an fp32 subtract, divide, power and multiply: about ten ulp of relative
    error, 1.5e-4 absolute at 255.  The GPU test compares bytes exactly, so none of ITS arrays may hold an element whose exact value
    lies within 2e-4 of an integer k >= 1 (x = 0, x = 1 and what truncates to 0 cannot flip)."""
    assert R.case_margin(name) >= R.MARGIN, (name, R.case_margin(name))
    squares, alpha, lens = R.alpha_case(name)
    _, B, Tmax, V, (h, w), want_lens, _, _ = R.PANEL_CASES[name]
    assert squares.shape == (B, V, V, 3) and alpha.shape == (B, Tmax, h * w) and alpha.dtype == np.float32 and lens.tolist() == list(want_lens)


def test_reference_panels_layout():
    squares, alpha, lens = R.alpha_case("7x7_p1")
    for b in range(3):
        n = int(lens[b])
        p = R.panels(squares[b], alpha[b], n, (7, 7), 1.0, 0.5)
        assert p.shape == (8, 32, 32, 3) and np.array_equal(p[0], squares[b]) and not p[n + 2:].any()
        assert (p[n + 1][..., 0] == p[n + 1][..., 1]).all() and (p[n + 1][..., 0] == p[n + 1][..., 2]).all()
        assert p[n + 1].any() == (n > 0)                           # a blank caption: a zero "Total Attention"
    flat = R.panels(squares[0], np.full((6, 1), 1.0, np.float32), 2, (1, 1))
    assert np.array_equal(flat[1], R.blend_rule(squares[0].astype(np.int64), 0)) and not flat[3].any()


def _visual(lengths, V=16):
    import sat_amd  # noqa: F401
    from sat_amd import visualize as Z
    rs = np.random.RandomState(0)
    B, T = len(lengths), max(lengths)
    panels = rs.randint(0, 256, (B, T + 2, V, V, 3)).astype(np.uint8)
    words = [["w%d" % i for i in range(n)] for n in lengths]
    return Z, Z.Visual([list(range(n)) for n in lengths], words, [-1.5] * B, [3.25] * B, list(lengths), panels, ["pic%d" % b for b in range(B)])


def test_contact_sheet_grid_follows_the_notebook():
    Z, vis = _visual([0, 2, 3, 6, 10])
    want = {0: (2, 2, 2), 2: (4, 4, 2), 3: (5, 5, 2), 6: (8, 4, 3), 10: (12, 4, 4)}       # len -> (panels, columns, rows)
    for i, n in enumerate(vis.lengths):
        assert Z.sheet_grid(n, 4) == want[n]
        sheet = Z.contact_sheet(vis, i, references=["a cat", "a dog"], columns=4)
        assert (sheet.info["panels"], sheet.info["columns"], sheet.info["rows"]) == want[n] and sheet.info["panels"] == 2 + n
        assert sheet.mode == "RGB"
        pad, label = 4, 14
        assert sheet.size == (pad + want[n][1] * (16 + pad), pad + 4 * label + want[n][2] * (16 + label + pad))
        # the first panel sits under the title block, the last panel is "Total Attention"
        got = np.asarray(sheet)
        top = pad + 4 * label
        assert np.array_equal(got[top:top + 16, pad:pad + 16], vis.panels[i, 0])
        last = 1 + n
        x, y = pad + (last % want[n][1]) * (16 + pad), top + (last // want[n][1]) * (16 + label + pad)
        assert np.array_equal(got[y:y + 16, x:x + 16], vis.panels[i, last])
    assert Z.sheet_grid(5, 3) == (7, 3, 3) and Z.sheet_grid(2, 3) == (4, 4, 2)


def test_argument_errors_return_einval_before_any_launch():
    """every pointer below is a made-up non-null address: a call that got past its checks would have to touch it"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    fake = 1 << 20
    d = (L.ImageDesc * 2)()
    d[0].offset, d[0].height, d[0].width = 0, 40, 60
    d[1].offset, d[1].height, d[1].width = 7200, 33 * 8 + 1, 300
    host = C.cast(d, C.c_void_p)

    def err():
        return lib.sat_last_error().decode()

    good = lib.sat_image_square_bicubic_workspace_bytes(host, 2, 16)
    assert good > 0
    assert lib.sat_image_square_bicubic_workspace_bytes(host, 2, 8) == 0 and "shrinks by more than 32x" in err()      # 265 > 32 * 8
    assert lib.sat_image_square_bicubic_workspace_bytes(host, 2, 0) == 0 and "size 0" in err()
    assert lib.sat_image_square_bicubic_workspace_bytes(None, 2, 16) == 0 and "null" in err()
    sq = lambda *a: lib.sat_image_square_bicubic(*a)              # noqa: E731
    assert sq(None, 1 << 30, host, fake, 2, 16, fake, None, fake, good, None) == 1 and "null" in err()
    assert sq(fake, 1 << 30, host, fake, 2, 16, None, None, fake, good, None) == 1 and "null" in err()
    assert sq(fake, 1 << 30, host, fake, 2, 8, fake, None, fake, good, None) == 1 and "shrinks" in err()
    assert sq(fake, 1 << 30, host, fake, 2, -3, fake, None, fake, good, None) == 1 and "size -3" in err()
    assert sq(fake, 7200, host, fake, 2, 16, fake, None, fake, good, None) == 1 and "outside the pixel buffer" in err()
    assert sq(fake, 1 << 30, host, fake, 2, 16, fake, None, fake, good - 1, None) == 1 and "workspace" in err()
    ap = lambda *a: lib.sat_attention_panels(*a)                  # noqa: E731
    assert ap(None, fake, fake, 2, 6, 32, 7, 7, 5.0, 0.75, fake, None) == 1 and "null" in err()
    assert ap(fake, fake, fake, 2, 6, 32, 7, 7, 5.0, 0.75, None, None) == 1 and "null" in err()
    assert ap(fake, fake, fake, 2, 6, 32, 17, 16, 5.0, 0.75, fake, None) == 1 and "map 17x16" in err()                # above SAT_ATTENTION_MAX_MAP
    assert L.ATTENTION_MAX_MAP == 256 and L.BICUBIC_MAX_SHRINK == 32
    assert ap(fake, fake, fake, 2, 6, 32, 7, 7, 5.0, 1.25, fake, None) == 1 and "opacity" in err()
    assert ap(fake, fake, fake, 2, 6, 32, 7, 7, 5.0, -0.1, fake, None) == 1 and "opacity" in err()
    assert ap(fake, fake, fake, 2, 6, 32, 7, 7, 5.0, float("nan"), fake, None) == 1 and "opacity" in err()
    assert ap(fake, fake, fake, 2, 6, 0, 7, 7, 5.0, 0.75, fake, None) == 1 and "visual size 0" in err()
    assert ap(fake, fake, fake, 2, 6, -4, 7, 7, 5.0, 0.75, fake, None) == 1 and "visual size -4" in err()
    assert ap(fake, fake, fake, 2, 6, 8, 14, 14, 5.0, 0.75, fake, None) == 1 and "larger than" in err()
    assert ap(fake, fake, fake, 2, 6, 32, 7, 7, 0.0, 0.75, fake, None) == 1 and "power" in err()
    assert ap(fake, fake, fake, 0, 6, 32, 7, 7, 5.0, 0.75, fake, None) == 1 and "B=0" in err()
