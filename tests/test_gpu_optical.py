"""GPU: the "optical" augmentation of sat_image_batch_transform_warp / sat_amd.data.BatchTransform(aug_optical_strength=s)
against Pillow (tests/golden/g14_optical.npz) and the numpy restatement (tests/optical_ref.py, itself pinned to Pillow).
Bytes and fp32 results are compared EXACTLY."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import color_jitter_ref as CJ
import optical_ref as R
from oracle import image_oracle as IO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import sat_amd  # noqa: F401
    from sat_amd import data
    return data


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_optical.npz"), allow_pickle=False)


def restated(img, d, S):
    """crop + resize + flip (+ ColorJitter) + warp of one picture, from its descriptor dict"""
    x = IO.resample_u8(img[d["crop_top"]:d["crop_top"] + d["crop_h"], d["crop_left"]:d["crop_left"] + d["crop_w"]], S, S)
    if d["flip"]:
        x = np.ascontiguousarray(x[:, ::-1])
    if "jitter_order" in d:
        x = CJ.jitter(x, d["jitter_order"], d["brightness"], d["contrast"], d["saturation"], d["hue_shift"])
    return R.warp(x, d["warp_kind"], list(d["warp_coeffs"])) if "warp_kind" in d else x


def strip_warp(descs, D):
    return [{k: v for k, v in d.items() if k not in D.WARP_KEYS} for d in descs]


def test_bytes_equal_pillow_fixture(D, g14):
    S, n = int(g14["size"]), len(g14["boxes"])
    for with_jitter in (0, 1):
        idx = [i for i in range(n) if g14["jitter"][i] == with_jitter]
        imgs = [g14["in%d" % i] for i in idx]
        descs = []
        for i, im in zip(idx, imgs):
            d = D.box_desc(im.shape[0], im.shape[1], g14["boxes"][i].tolist(), S, flip=bool(g14["flips"][i]))
            if with_jitter:
                d.update(jitter_order=tuple(g14["orders"][i].tolist()), hue_shift=int(g14["hue_shifts"][i]),
                         **dict(zip(("brightness", "contrast", "saturation"), g14["factors"][i].tolist())))
            d.update(warp_kind=int(g14["kinds"][i]), warp_coeffs=g14["coeffs"][i].tolist())
            descs.append(d)
        tf = D.BatchTransform(S, train=True, aug_noise_std=0.02, aug_color_jitter=0.5 * with_jitter, aug_optical_strength=1.0)
        noise = torch.randn(len(idx), 3, S, S, generator=torch.Generator().manual_seed(4 + with_jitter))
        st = tf.stage(imgs, descs)
        assert st.warp is not None and (st.jitter is not None) == bool(with_jitter)
        out, raw = tf.run(st, torch.device("cuda"), noise=noise.cuda(), want_bytes=True)
        raw = raw.cpu()
        for k, i in enumerate(idx):
            assert np.array_equal(raw[k].numpy(), g14["out%d" % i]), "picture %d" % i
        want = raw.permute(0, 3, 1, 2).float().div(255) + noise * 0.02
        assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("s", [0.5, 1.0])
@pytest.mark.parametrize("jitter", [0.0, 0.4])
def test_ragged_224_batch_equals_restatement(D, s, jitter):
    """128 ragged pictures at S = 224 with real draws: the warped bytes equal the restatement's warp of the same batch's
    bytes without the warp (those are pinned by the plain and jitter tests), and a few pictures the whole restated chain"""
    rng = np.random.default_rng(int(s * 10) + int(jitter * 100))
    B, S = 128, 224
    shapes = [(int(rng.integers(120, 481)), int(rng.integers(120, 641))) for _ in range(B)]
    base = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    imgs = [np.ascontiguousarray(base[:h, (7 * i) % (641 - w):(7 * i) % (641 - w) + w]) for i, (h, w) in enumerate(shapes)]
    tf = D.BatchTransform(S, train=True, aug_scale=0.5, aug_hflip=0.5, aug_noise_std=0.01, aug_color_jitter=jitter, aug_optical_strength=s)
    random.seed(7); torch.manual_seed(7)
    descs = tf.draw(shapes)
    assert {d["warp_kind"] for d in descs} == {0, 1} and any(d["flip"] for d in descs)
    noise = torch.randn(B, 3, S, S, device="cuda")
    out, raw = tf.run(tf.stage(imgs, descs), torch.device("cuda"), noise=noise, want_bytes=True)
    _, pre = tf.run(tf.stage(imgs, strip_warp(descs, D)), torch.device("cuda"), noise=noise, want_bytes=True)
    raw, pre, out, noise = raw.cpu().numpy(), pre.cpu().numpy(), out.cpu(), noise.cpu()
    for i, d in enumerate(descs):
        want = R.warp(pre[i], d["warp_kind"], list(d["warp_coeffs"]))
        assert np.array_equal(raw[i], want), "picture %d (kind %d)" % (i, d["warp_kind"])
    assert torch.equal(out, torch.from_numpy(raw).permute(0, 3, 1, 2).float().div(255) + noise * 0.01)
    for i in (0, 1, 2, 77, 127):
        assert np.array_equal(raw[i], restated(imgs[i], descs[i], S)), "picture %d" % i


def test_batch_transform_end_to_end(D):
    """BatchTransform(aug_optical_strength=s)(images): draws, staging, one H2D copy and the kernels, against the restated
    chain of the same draws"""
    rng = np.random.default_rng(8)
    shapes = [(480, 640), (640, 427), (100, 100), (37, 200), (224, 224), (60, 45), (500, 333), (81, 81), (300, 64)] * 2
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    S = 64
    for jitter in (0.0, 0.8):
        tf = D.BatchTransform(S, train=True, aug_scale=0.3, aug_hflip=0.5, aug_noise_std=0.01, aug_color_jitter=jitter, aug_optical_strength=0.8)
        noise = torch.randn(len(imgs), 3, S, S, device="cuda")
        random.seed(21); torch.manual_seed(21)
        out = tf(imgs, noise=noise).cpu()
        random.seed(21); torch.manual_seed(21)
        descs = tf.draw(shapes)
        assert {d["warp_kind"] for d in descs} == {0, 1}
        for i, (im, d) in enumerate(zip(imgs, descs)):
            want = restated(im, d, S)
            assert torch.equal(out[i], torch.from_numpy(want).permute(2, 0, 1).float().div(255) + noise[i].cpu() * 0.01), "picture %d" % i


def test_null_warp_is_the_existing_entry_points(D):
    from sat_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(5)
    shapes = [(480, 640), (100, 100), (37, 200), (64, 48)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    S, n = 48, len(shapes)
    noise = torch.randn(n, 3, S, S, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for jitter in (0.0, 0.6):
        tf = D.BatchTransform(S, train=True, aug_scale=0.5, aug_color_jitter=jitter)
        torch.manual_seed(2)
        st = tf.stage(imgs)
        assert st.warp is None
        dev = st.host.cuda()
        desc = C.cast(st.desc, C.c_void_p)
        jit = (C.cast(st.jitter, C.c_void_p), dev.data_ptr() + st.jitter_off) if st.jitter is not None else (None, None)
        need = lib.sat_image_batch_warp_workspace_bytes(desc, jit[0], None, n, S, S)
        assert need == (lib.sat_image_batch_jitter_workspace_bytes(desc, jit[0], n, S, S) if jitter else lib.sat_image_batch_workspace_bytes(desc, n, S, S))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        res = []
        for which in ("old", "warp"):
            out = torch.empty(n, 3, S, S, device="cuda")
            raw = torch.empty(n, S, S, 3, dtype=torch.uint8, device="cuda")
            tail = (n, S, S, L.ptr(noise), 0.01, L.ptr(out), L.ptr(raw), L.ptr(ws), need, stream)
            head = (dev.data_ptr() + st.head, st.pixels_bytes, desc, dev.data_ptr())
            if which == "warp":
                rc = lib.sat_image_batch_transform_warp(*head, *jit, None, None, *tail)
            elif jitter:
                rc = lib.sat_image_batch_transform_jitter(*head, *jit, *tail)
            else:
                rc = lib.sat_image_batch_transform(*head, *tail)
            L.check(rc, which)
            res.append((out, raw))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_rejects_bad_warp(D):
    from sat_amd import _lib as L
    img = np.zeros((10, 12, 3), np.uint8)
    S = 8
    tf = D.BatchTransform(S, train=True, aug_optical_strength=0.5)
    rot = R.rotate_matrix(20.0, S) + [0.0, 0.0]
    far = list(rot)
    far[5] = -1e6
    for kind, coeffs in ((3, rot), (0, rot[:4] + [float("inf")] + rot[5:]), (1, rot[:6] + [float("nan"), 0.0]), (0, far)):
        d = dict(D.box_desc(10, 12, (0, 0, 10, 12), S), warp_kind=kind, warp_coeffs=coeffs)
        with pytest.raises(L.SatHipError):
            tf.run(tf.stage([img], [d]), torch.device("cuda"))
    d = dict(D.box_desc(10, 12, (0, 0, 10, 12), S), warp_kind=0, warp_coeffs=rot)
    out = tf.run(tf.stage([img], [d]), torch.device("cuda"))            # the stream is still usable
    assert out.shape == (1, 3, S, S) and bool(torch.isfinite(out).all())
