"""CPU: ColorJitter of the input pipeline (train.py:223-224).  The numpy restatement (tests/color_jitter_ref.py) against the
installed Pillow - exhaustively where the domain is 2^24 or smaller - and against tests/golden/g13_color_jitter.npz (made by
tests/golden/make_color_jitter_golden.py); the host side of sat_amd.data (draws, staging) and the C ABI's validation of
the jitter records.  No kernel runs here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import color_jitter_ref as R
from oracle import image_oracle as IO


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_color_jitter.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def Image():
    return pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def all_rgb():
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_luma_equals_pillow_on_every_colour(Image, all_rgb):
    assert np.array_equal(R.luma(all_rgb), np.asarray(Image.fromarray(all_rgb).convert("L")))


def test_rgb_to_hsv_equals_pillow_on_every_colour(Image, all_rgb):
    assert np.array_equal(R.rgb_to_hsv(all_rgb), np.asarray(Image.fromarray(all_rgb).convert("HSV")))


def test_hsv_to_rgb_equals_pillow_on_every_triple(Image, all_rgb):
    hsv = Image.frombytes("HSV", (4096, 4096), all_rgb.tobytes())
    assert np.array_equal(R.hsv_to_rgb(all_rgb), np.asarray(hsv.convert("RGB")))


def test_blend_equals_pillow_on_every_byte_pair(Image):
    i = np.arange(1 << 16, dtype=np.uint32)
    d = (i >> 8).astype(np.uint8).reshape(256, 256)
    x = (i & 255).astype(np.uint8).reshape(256, 256)
    rng = np.random.default_rng(0)
    factors = [0.0, 1.0, 2.0, 0.6, 1.4, 0.5, 1.5, 1e-7, 1.9999999] + [float(np.float32(f)) for f in rng.uniform(0, 2, 24)]
    for f in factors:
        got = np.asarray(Image.blend(Image.fromarray(d), Image.fromarray(x), f))
        assert np.array_equal(R.blend(d, x, f), got), f


def test_enhancers_equal_pillow(Image):
    """brightness / contrast / saturation / hue on whole pictures against ImageEnhance and F_pil.adjust_hue"""
    from PIL import ImageEnhance
    rng = np.random.default_rng(1)
    for h, w in ((17, 23), (64, 48), (1, 1)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = Image.fromarray(img)
        for f in (0.0, 0.37, 1.0, 1.63, 2.0):
            assert np.array_equal(R.brightness(img, f), np.asarray(ImageEnhance.Brightness(p).enhance(f)))
            assert np.array_equal(R.contrast(img, f), np.asarray(ImageEnhance.Contrast(p).enhance(f)))
            assert np.array_equal(R.saturation(img, f), np.asarray(ImageEnhance.Color(p).enhance(f)))
        for shift in (-7, -1, 0, 3, 7, 127, -128):
            hh, s, v = p.convert("HSV").split()
            nh = ((np.asarray(hh).astype(np.int64) + shift) % 256).astype(np.uint8)
            want = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
            assert np.array_equal(R.hue(img, shift), np.asarray(want))
    assert R.hue_shift_byte(-0.03) == -7 and R.hue_shift_byte(0.03) == 7 and (-7) % 256 == 249


def test_g13_covers_the_stated_cases(g13):
    orders = {tuple(o) for o in g13["orders"].tolist()}
    assert len(orders) == 24
    f = g13["factors"]
    assert (f == 0).any() and (f == 2).any() and (f == np.float32(0.6)).any() and (f == np.float32(1.4)).any()
    assert {-7, 0, 7} <= set(g13["hue_shifts"].tolist())
    assert len({g13["in%d" % i].shape for i in range(len(orders))}) > 10             # ragged


def test_restated_chain_reproduces_g13(g13):
    S = int(g13["size"])
    for i in range(len(g13["boxes"])):
        t, l, h, w = g13["boxes"][i].tolist()
        x = IO.resample_u8(g13["in%d" % i][t:t + h, l:l + w], S, S)
        if g13["flips"][i]:
            x = x[:, ::-1]
        b, c, s = g13["factors"][i].tolist()
        assert R.hue_shift_byte(g13["hue_factors"][i]) == g13["hue_shifts"][i]
        assert np.array_equal(R.jitter(x, g13["orders"][i].tolist(), b, c, s, int(g13["hue_shifts"][i])), g13["out%d" % i]), "picture %d" % i


# ------------------------------------------------------------------------------------------------ host logic of the product
@pytest.fixture(scope="module")
def D():
    import sat_amd  # noqa: F401
    from sat_amd import data
    return data


def test_draws_follow_torchvision_order(D):
    """per picture: crop, flip, then randperm(4) and four uniform draws (brightness, contrast, saturation in
    [max(0, 1-x), 1+x], hue in [-0.03, 0.03]) - T.ColorJitter.get_params"""
    shapes = [(480, 640), (100, 100), (37, 200)]
    for x in (0.4, 1.0):
        tf = D.BatchTransform(64, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=x)
        torch.manual_seed(6)
        got = tf.draw(shapes)
        after = torch.get_rng_state()
        torch.manual_seed(6)
        for (h, w), d in zip(shapes, got):
            t, l, ch, cw = IO.random_resized_crop_params(h, w, (0.5, 1.0))
            flip = int(torch.rand(1).item() < 0.5)
            order = torch.randperm(4).tolist()
            lo = max(0.0, 1.0 - x)
            b, c, s = (float(torch.empty(1).uniform_(lo, 1.0 + x)) for _ in range(3))
            hue = float(torch.empty(1).uniform_(-0.03, 0.03))
            assert (d["crop_top"], d["crop_left"], d["crop_h"], d["crop_w"], d["flip"]) == (t, l, ch, cw, flip)
            assert tuple(d["jitter_order"]) == tuple(order) and (d["brightness"], d["contrast"], d["saturation"]) == (b, c, s)
            assert d["hue_shift"] == int(hue * 255) and -7 <= d["hue_shift"] <= 7
            assert lo <= min(b, c, s) and max(b, c, s) <= 1.0 + x
        assert torch.equal(torch.get_rng_state(), after)              # nothing drawn beyond the stated draws


def test_jitter_off_consumes_nothing_extra(D):
    shapes = [(480, 640), (64, 64), (30, 90)]
    for x in (0.0, 1.5, 7.0):                                        # train.py:223: off at 0 and silently off above 1
        torch.manual_seed(11)
        base = D.BatchTransform(64, train=True, aug_scale=0.5, aug_hflip=0.5).draw(shapes)
        after_base = torch.rand(1).item()
        torch.manual_seed(11)
        tf = D.BatchTransform(64, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=x)
        assert not tf.jitter
        got = tf.draw(shapes)
        assert got == base and torch.rand(1).item() == after_base
        assert not any(k in d for d in got for k in D.JITTER_KEYS)
    torch.manual_seed(11)
    D.BatchTransform(64, train=False, aug_color_jitter=0.5).draw(shapes)       # valid_transforms: no ColorJitter
    v = torch.rand(1).item()
    torch.manual_seed(11)
    assert torch.rand(1).item() == v


def test_negative_jitter_raises(D):
    with pytest.raises(ValueError):
        D.BatchTransform(64, train=True, aug_color_jitter=-0.1)
    assert D.BatchTransform(64, train=True, aug_color_jitter=1.0).jitter
    assert D.BatchTransform(64, train=True, aug_color_jitter=1e-3).jitter


def test_staged_batch_carries_jitter_records(D):
    from sat_amd import _lib as L
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((20, 31), (33, 17), (8, 8))]
    tf = D.BatchTransform(16, train=True, aug_color_jitter=0.4)
    torch.manual_seed(3)
    descs = tf.draw([im.shape[:2] for im in imgs])
    st = tf.stage(imgs, descs)
    buf = st.host.numpy()
    assert st.head % 256 == 0 and st.jitter_off % 16 == 0 and st.jitter_off >= C.sizeof(L.ImageDesc) * 3
    assert st.jitter_off + C.sizeof(L.ImageJitter) * 3 <= st.head
    back = (L.ImageJitter * 3).from_buffer_copy(buf[st.jitter_off:st.jitter_off + C.sizeof(L.ImageJitter) * 3].tobytes())
    for j, d in zip(back, descs):
        assert tuple(j.order) == tuple(d["jitter_order"]) and j.hue_shift == d["hue_shift"]
        assert (j.brightness, j.contrast, j.saturation) == tuple(float(np.float32(d[k])) for k in ("brightness", "contrast", "saturation"))
    for i, p in enumerate(imgs):
        assert np.array_equal(buf[st.head + st.desc[i].offset: st.head + st.desc[i].offset + p.size].reshape(p.shape), p)
    assert D.BatchTransform(16, train=True).stage(imgs).jitter is None
    mixed = [dict(d) for d in descs]
    for k in D.JITTER_KEYS:
        del mixed[1][k]
    with pytest.raises(ValueError):
        tf.stage(imgs, mixed)
    del mixed[0]["hue_shift"]
    with pytest.raises(ValueError):
        tf.stage(imgs, mixed)


def test_jitter_abi_validation_without_gpu(D):
    """bad records: a status and a message from the host checks, nothing launched (the device pointers are never used)"""
    from sat_amd import _lib as L
    lib = L.lib()
    img = np.zeros((10, 12, 3), np.uint8)
    st = D.StagedBatch([img], [dict(D.box_desc(10, 12, (0, 0, 10, 12), 8), jitter_order=(3, 1, 0, 2), brightness=0.5, contrast=1.5,
                                    saturation=1.0, hue_shift=-7)])
    desc = C.cast(st.desc, C.c_void_p)
    plain = lib.sat_image_batch_workspace_bytes(desc, 1, 8, 8)
    need = lib.sat_image_batch_jitter_workspace_bytes(desc, C.cast(st.jitter, C.c_void_p), 1, 8, 8)
    assert plain > 0 and need >= plain + 8 * 8 * 4 + 8
    assert lib.sat_image_batch_jitter_workspace_bytes(desc, None, 1, 8, 8) == plain
    fake = C.c_void_p(1 << 20)
    bad = [dict(order=(0, 1, 2, 2)), dict(order=(0, 1, 2, 4)), dict(order=(-1, 1, 2, 3)), dict(brightness=-0.5), dict(contrast=float("nan")),
           dict(saturation=float("inf")), dict(hue_shift=128), dict(hue_shift=-129)]
    for b in bad:
        j = L.ImageJitter()
        j.order[:] = list(b.get("order", (0, 1, 2, 3)))
        j.brightness, j.contrast, j.saturation = b.get("brightness", 1.0), b.get("contrast", 1.0), b.get("saturation", 1.0)
        j.hue_shift = b.get("hue_shift", 0)
        assert lib.sat_image_batch_jitter_workspace_bytes(desc, C.byref(j), 1, 8, 8) == 0, b
        rc = lib.sat_image_batch_transform_jitter(fake, st.pixels_bytes, desc, fake, C.byref(j), fake, 1, 8, 8, None, 0.0, fake, None, fake, need, None)
        assert rc != 0, b
        assert b"jitter" in lib.sat_last_error() or b"hue" in lib.sat_last_error(), b
    rc = lib.sat_image_batch_transform_jitter(fake, st.pixels_bytes, desc, fake, C.cast(st.jitter, C.c_void_p), None, 1, 8, 8, None, 0.0, fake, None,
                                              fake, need, None)
    assert rc != 0 and b"jitter" in lib.sat_last_error()
    rc = lib.sat_image_batch_transform_jitter(fake, st.pixels_bytes, desc, fake, C.cast(st.jitter, C.c_void_p), fake, 1, 8, 8, None, 0.0, fake, None,
                                              fake, plain, None)
    assert rc != 0 and b"workspace" in lib.sat_last_error()          # the plain workspace is too small for the jitter kernels
