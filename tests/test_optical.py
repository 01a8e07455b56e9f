"""CPU: the "optical" augmentation of the input pipeline (train.py:225-231).  The numpy restatement (tests/optical_ref.py)
against the installed Pillow and against tests/golden/g14_optical.npz (made by tests/golden/make_optical_golden.py); the
host side of sat_amd.data (draws, staging) and the C ABI's validation of the warp records.  No kernel runs here."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import color_jitter_ref as CJ
import optical_ref as R
from oracle import image_oracle as IO


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_optical.npz"), allow_pickle=False)


@pytest.fixture(autouse=True)
def keep_generator_states():
    """the draws below seed Python's ``random`` and torch's CPU generator: hand both back as they were"""
    py, th = random.getstate(), torch.get_rng_state()
    yield
    random.setstate(py)
    torch.set_rng_state(th)


@pytest.fixture(scope="module")
def Image():
    return pytest.importorskip("PIL.Image")


def _randint(gen):
    return lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=gen).item())


def _uniform(gen, s):
    return float(torch.empty(1).uniform_(-45.0 * s, 45.0 * s, generator=gen).item())


@pytest.mark.parametrize("S", [24, 37, 224])
def test_restatement_equals_pillow(Image, S):
    """the two samplers and the three matrix rules against Image.transform(AFFINE, NEAREST), Image.rotate(NEAREST) and
    Image.transform(PERSPECTIVE, BILINEAR), with matrices drawn as the reference draws them"""
    rng = np.random.default_rng(S)
    gen = torch.Generator().manual_seed(S)
    for s in (0.1, 0.5, 1.0):
        for _ in range(3 if S == 224 else 6):
            img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
            p = Image.fromarray(img)
            angle, shear = _uniform(gen, s), _uniform(gen, s)
            m = R.affine_matrix(angle, shear, S)
            assert np.array_equal(R.affine_nearest(img, m), np.asarray(p.transform((S, S), Image.AFFINE, m, Image.NEAREST, fillcolor=(0, 0, 0))))
            assert np.array_equal(R.affine_nearest(img, R.rotate_matrix(angle, S)), np.asarray(p.rotate(angle, Image.NEAREST, fillcolor=(0, 0, 0))))
            start, end = R.perspective_points(S, S, 0.5 * s, _randint(gen))
            c = R.perspective_coeffs(start, end)
            want = np.asarray(p.transform((S, S), Image.PERSPECTIVE, c, Image.BILINEAR, fillcolor=(0, 0, 0)))
            assert np.array_equal(R.perspective_bilinear(img, c), want), (S, s, end)
    img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    assert np.array_equal(R.affine_nearest(img, R.rotate_matrix(0.0, S)), np.asarray(Image.fromarray(img).rotate(0.0, Image.NEAREST)))
    assert np.array_equal(R.affine_nearest(img, R.rotate_matrix(0.0, S)), img)
    assert np.array_equal(R.affine_nearest(img, R.affine_matrix(0.0, 0.0, S)), img)


def test_perspective_truncates(Image):
    """(UINT8) v: the byte is truncated; rounding it would miss most pixels of a smooth picture"""
    S = 64
    y, x = np.mgrid[0:S, 0:S]
    img = np.stack([x * 4, y * 4, (x + y) * 2], -1).astype(np.uint8)
    c = R.perspective_coeffs(*R.perspective_points(S, S, 0.5, _randint(torch.Generator().manual_seed(1))))
    got = R.perspective_bilinear(img, c)
    assert np.array_equal(got, np.asarray(Image.fromarray(img).transform((S, S), Image.PERSPECTIVE, c, Image.BILINEAR)))


def test_g14_covers_the_stated_cases(g14):
    S = int(g14["size"])
    assert set(g14["choices"].tolist()) == {0, 1, 2} and set(g14["kinds"].tolist()) == {0, 1}
    j, f = g14["jitter"].astype(bool), g14["flips"].astype(bool)
    for kind in (0, 1):
        k = g14["kinds"] == kind
        assert (k & j).any() and (k & ~j).any() and (k & f).any() and (k & ~f).any()
    corner = g14["corner_draws"]
    assert set(g14["choices"][corner].tolist()) == {0, 1, 2} and (g14["strengths"][corner] == 1.0).all()
    d = int(0.5 * (S // 2))
    ends = g14["endpoints"][corner][g14["choices"][corner] == 0]
    assert [[d, d], [S - d - 1, d], [S - d - 1, S - d - 1], [d, S - d - 1]] in ends.tolist()      # every draw at its far end
    assert [[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]] in ends.tolist()                      # every draw at its near end
    assert {45.0, -45.0} <= set(g14["angles"][corner].tolist())
    assert {45.0, -45.0} <= set(g14["shears"][corner].tolist())
    assert 0.0 in g14["angles"][corner][g14["choices"][corner] == 2].tolist()                     # the exact identity
    fill = g14["all_fill"].astype(bool)
    assert set(g14["kinds"][fill].tolist()) == {0, 1}
    for i in np.flatnonzero(fill):
        assert not g14["out%d" % i].any()
    for i in range(len(g14["boxes"])):
        if not fill[i]:
            assert g14["out%d" % i].any()
    assert {0.1, 0.5, 1.0} <= set(g14["strengths"].tolist())
    assert len({g14["in%d" % i].shape for i in range(len(g14["boxes"]))}) > 10                    # ragged


def test_restated_chain_reproduces_g14(g14):
    S = int(g14["size"])
    start = [[0, 0], [S - 1, 0], [S - 1, S - 1], [0, S - 1]]
    for i in range(len(g14["boxes"])):
        c = g14["coeffs"][i].tolist()
        ch = int(g14["choices"][i])
        if not g14["all_fill"][i]:                 # the matrix rules give the record's coefficients
            if ch == 0:
                # a float32 least-squares solve: the LAPACK library picks its kernels by CPU, so the last bits of the solution
                # differ from one CPU to another (torchvision's do too).  The bytes below use the recorded coefficients.
                assert np.allclose(R.perspective_coeffs(start, g14["endpoints"][i].tolist()), c, rtol=1e-5, atol=1e-5)
            elif ch == 1:
                assert R.affine_matrix(g14["angles"][i], g14["shears"][i], S) + [0.0, 0.0] == c
            else:
                assert R.rotate_matrix(g14["angles"][i], S) + [0.0, 0.0] == c
        t, l, h, w = g14["boxes"][i].tolist()
        x = IO.resample_u8(g14["in%d" % i][t:t + h, l:l + w], S, S)
        if g14["flips"][i]:
            x = np.ascontiguousarray(x[:, ::-1])
        if g14["jitter"][i]:
            x = CJ.jitter(x, g14["orders"][i].tolist(), *g14["factors"][i].tolist(), int(g14["hue_shifts"][i]))
        assert np.array_equal(R.warp(x, int(g14["kinds"][i]), c), g14["out%d" % i]), "picture %d" % i


# ------------------------------------------------------------------------------------------------ host logic of the product
@pytest.fixture(scope="module")
def D():
    import sat_amd  # noqa: F401
    from sat_amd import data
    return data


def test_draws_follow_torchvision_order(D):
    """per picture: crop, flip, ColorJitter, then random.choice of the three transforms and the chosen one's torch draws:
    RandomPerspective torch.rand(1) + 8 randint, RandomAffine angle + shear_x, RandomRotation angle"""
    shapes = [(480, 640), (100, 100), (37, 200), (64, 64), (300, 200), (90, 120)] * 3
    S = 48
    for s in (0.3, 1.0):
        for jitter in (0.0, 0.4):
            tf = D.BatchTransform(S, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=jitter, aug_optical_strength=s)
            assert tf.optical
            random.seed(5); torch.manual_seed(6)
            got = tf.draw(shapes)
            after = random.getstate(), torch.get_rng_state()
            random.seed(5); torch.manual_seed(6)
            seen = set()
            for (h, w), d in zip(shapes, got):
                t, l, ch, cw = IO.random_resized_crop_params(h, w, (0.5, 1.0))
                flip = int(torch.rand(1).item() < 0.5)
                assert (d["crop_top"], d["crop_left"], d["crop_h"], d["crop_w"], d["flip"]) == (t, l, ch, cw, flip)
                if jitter:
                    order = torch.randperm(4).tolist()
                    lo = max(0.0, 1.0 - jitter)
                    b, c, sat = (float(torch.empty(1).uniform_(lo, 1.0 + jitter)) for _ in range(3))
                    hue = float(torch.empty(1).uniform_(-0.03, 0.03))
                    assert tuple(d["jitter_order"]) == tuple(order) and (d["brightness"], d["contrast"], d["saturation"]) == (b, c, sat)
                    assert d["hue_shift"] == int(hue * 255)
                else:
                    assert not any(k in d for k in D.JITTER_KEYS)
                k = random.choice((0, 1, 2))
                seen.add(k)
                if k == 0:
                    torch.rand(1)
                    start, end = R.perspective_points(S, S, 0.5 * s, lambda lo, hi: int(torch.randint(lo, hi, size=(1,)).item()))
                    assert d["warp_kind"] == 1 and list(d["warp_coeffs"]) == R.perspective_coeffs(start, end)
                else:
                    angle = float(torch.empty(1).uniform_(-45.0 * s, 45.0 * s).item())
                    if k == 1:
                        shear = float(torch.empty(1).uniform_(-45.0 * s, 45.0 * s).item())
                        m = R.affine_matrix(angle, shear, S)
                    else:
                        m = R.rotate_matrix(angle, S)
                    assert d["warp_kind"] == 0 and list(d["warp_coeffs"]) == m + [0.0, 0.0]
                    assert abs(angle) <= 45.0 * s
            assert seen == {0, 1, 2}
            assert random.getstate() == after[0] and torch.equal(torch.get_rng_state(), after[1])


def test_optical_off_draws_nothing(D):
    shapes = [(480, 640), (64, 64), (30, 90)]
    for jitter in (0.0, 0.5):
        random.seed(3); torch.manual_seed(11)
        base = D.BatchTransform(64, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=jitter).draw(shapes)
        py_after, torch_after = random.getstate(), torch.get_rng_state()
        for s in (0.0, 1.5, 7.0):                                    # train.py:225: off at 0 and silently off above 1
            random.seed(3); torch.manual_seed(11)
            tf = D.BatchTransform(64, train=True, aug_scale=0.5, aug_hflip=0.5, aug_color_jitter=jitter, aug_optical_strength=s)
            assert not tf.optical
            got = tf.draw(shapes)
            assert got == base and random.getstate() == py_after and torch.equal(torch.get_rng_state(), torch_after)
            assert not any(k in d for d in got for k in D.WARP_KEYS)
    random.seed(3); torch.manual_seed(11)
    py0, t0 = random.getstate(), torch.get_rng_state()
    D.BatchTransform(64, train=False, aug_optical_strength=0.5).draw(shapes)      # valid_transforms: no augmentation
    assert random.getstate() == py0 and torch.equal(torch.get_rng_state(), t0)


def test_negative_strength_raises(D):
    with pytest.raises(ValueError):
        D.BatchTransform(64, train=True, aug_optical_strength=-0.1)
    assert D.BatchTransform(64, train=True, aug_optical_strength=1.0).optical
    assert D.BatchTransform(64, train=True, aug_optical_strength=1e-3).optical
    assert not D.BatchTransform(64, train=True, aug_optical_strength=1.0 + 1e-9).optical


def test_staged_batch_carries_warp_records(D):
    from sat_amd import _lib as L
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((20, 31), (33, 17), (8, 8))]
    assert C.sizeof(L.ImageWarp) == 72 and C.alignment(L.ImageWarp) == 8
    for jitter in (0.0, 0.4):
        tf = D.BatchTransform(16, train=True, aug_color_jitter=jitter, aug_optical_strength=0.7)
        random.seed(1); torch.manual_seed(3)
        descs = tf.draw([im.shape[:2] for im in imgs])
        st = tf.stage(imgs, descs)
        buf = st.host.numpy()
        assert (st.jitter is not None) == bool(jitter) and st.warp is not None
        assert st.head % 256 == 0 and st.warp_off % 8 == 0 and st.warp_off >= C.sizeof(L.ImageDesc) * 3
        if jitter:
            assert st.warp_off >= st.jitter_off + C.sizeof(L.ImageJitter) * 3
        assert st.warp_off + C.sizeof(L.ImageWarp) * 3 <= st.head
        back = (L.ImageWarp * 3).from_buffer_copy(buf[st.warp_off:st.warp_off + C.sizeof(L.ImageWarp) * 3].tobytes())
        for wr, d in zip(back, descs):
            assert wr.kind == d["warp_kind"] and list(wr.coeffs) == list(d["warp_coeffs"])
        for i, p in enumerate(imgs):
            assert np.array_equal(buf[st.head + st.desc[i].offset: st.head + st.desc[i].offset + p.size].reshape(p.shape), p)
    assert D.BatchTransform(16, train=True).stage(imgs).warp is None
    six = [dict(d, warp_coeffs=tuple(d["warp_coeffs"])[:6], warp_kind=0) for d in descs]
    assert list(tf.stage(imgs, six).warp[0].coeffs) == list(six[0]["warp_coeffs"]) + [0.0, 0.0]
    mixed = [dict(d) for d in descs]
    del mixed[1]["warp_kind"]
    with pytest.raises(ValueError):
        tf.stage(imgs, mixed)


def test_warp_abi_validation_without_gpu(D):
    """bad records: a status and a message from the host checks, nothing launched (the device pointers are never used)"""
    from sat_amd import _lib as L
    lib = L.lib()
    S = 8
    img = np.zeros((10, 12, 3), np.uint8)
    rot = D.rotate_matrix(30.0, S, S) + [0.0, 0.0]
    st = D.StagedBatch([img], [dict(D.box_desc(10, 12, (0, 0, 10, 12), S), warp_kind=0, warp_coeffs=rot)])
    desc = C.cast(st.desc, C.c_void_p)
    plain = lib.sat_image_batch_workspace_bytes(desc, 1, S, S)
    need = lib.sat_image_batch_warp_workspace_bytes(desc, None, C.cast(st.warp, C.c_void_p), 1, S, S)
    assert plain > 0 and need >= plain + S * S * 3
    assert lib.sat_image_batch_warp_workspace_bytes(desc, None, None, 1, S, S) == plain
    fake = C.c_void_p(1 << 20)
    far = list(rot)
    far[2] += 40000.0
    tilt = list(rot)
    tilt[1] = 5000.0                                         # fine at (0, 0), out of range at the corners with y = H
    bad = [(2, rot, b"kind"), (-1, rot, b"kind"), (0, rot[:3] + [float("nan")] + rot[4:], b"finite"), (1, [1, 0, 0, 0, 1, 0, 0, float("inf")], b"finite"),
           (0, far, b"32768"), (0, tilt, b"32768")]
    for kind, coeffs, msg in bad:
        wr = L.ImageWarp()
        wr.kind = kind
        wr.coeffs[:] = [float(c) for c in coeffs]
        assert lib.sat_image_batch_warp_workspace_bytes(desc, None, C.byref(wr), 1, S, S) == 0, (kind, coeffs)
        assert msg in lib.sat_last_error(), lib.sat_last_error()
        rc = lib.sat_image_batch_transform_warp(fake, st.pixels_bytes, desc, fake, None, None, C.byref(wr), fake, 1, S, S, None, 0.0, fake, None, fake,
                                                need, None)
        assert rc != 0 and msg in lib.sat_last_error(), (kind, coeffs)
    ok = L.ImageWarp()
    ok.kind = 0
    ok.coeffs[:] = rot[:6] + [float("nan"), float("nan")]    # an affine record does not read coeffs[6..7]
    assert lib.sat_image_batch_warp_workspace_bytes(desc, None, C.byref(ok), 1, S, S) == need
    ok.kind = 1                                              # a perspective record does
    assert lib.sat_image_batch_warp_workspace_bytes(desc, None, C.byref(ok), 1, S, S) == 0
    rc = lib.sat_image_batch_transform_warp(fake, st.pixels_bytes, desc, fake, None, None, C.cast(st.warp, C.c_void_p), None, 1, S, S, None, 0.0, fake,
                                            None, fake, need, None)
    assert rc != 0 and b"warp" in lib.sat_last_error()
    rc = lib.sat_image_batch_transform_warp(fake, st.pixels_bytes, desc, fake, None, None, C.cast(st.warp, C.c_void_p), fake, 1, S, S, None, 0.0, fake,
                                            None, fake, plain, None)
    assert rc != 0 and b"workspace" in lib.sat_last_error()          # the plain workspace is too small for the warp stage
