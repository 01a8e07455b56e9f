"""GPU: ColorJitter of sat_image_batch_transform_jitter / sat_amd.data.BatchTransform(aug_color_jitter=x) against Pillow
(tests/golden/g13_color_jitter.npz) and the numpy restatement (tests/color_jitter_ref.py, itself pinned to Pillow on every
colour).  Bytes and fp32 results are compared EXACTLY."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import color_jitter_ref as R
from oracle import image_oracle as IO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def D():
    import sat_amd  # noqa: F401
    from sat_amd import data
    return data


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_color_jitter.npz"), allow_pickle=False)


def jitter_fields(order, b, c, s, shift):
    return dict(jitter_order=tuple(int(o) for o in order), brightness=float(b), contrast=float(c), saturation=float(s), hue_shift=int(shift))


def restated(img, d, S):
    x = IO.resample_u8(img[d["crop_top"]:d["crop_top"] + d["crop_h"], d["crop_left"]:d["crop_left"] + d["crop_w"]], S, S)
    if d["flip"]:
        x = x[:, ::-1]
    return R.jitter(x, d["jitter_order"], d["brightness"], d["contrast"], d["saturation"], d["hue_shift"])


def test_bytes_equal_pillow_fixture(D, g13):
    S, n = int(g13["size"]), len(g13["boxes"])
    imgs = [g13["in%d" % i] for i in range(n)]
    descs = []
    for i in range(n):
        d = D.box_desc(imgs[i].shape[0], imgs[i].shape[1], g13["boxes"][i].tolist(), S, flip=bool(g13["flips"][i]))
        d.update(jitter_fields(g13["orders"][i], *g13["factors"][i].tolist(), g13["hue_shifts"][i]))
        descs.append(d)
    tf = D.BatchTransform(S, train=True, aug_noise_std=0.02, aug_color_jitter=1.0)
    noise = torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(4))
    out, raw = tf.run(tf.stage(imgs, descs), torch.device("cuda"), noise=noise.cuda(), want_bytes=True)
    raw = raw.cpu()
    for i in range(n):
        assert np.array_equal(raw[i].numpy(), g13["out%d" % i]), "picture %d" % i
    want = raw.permute(0, 3, 1, 2).float().div(255) + noise * 0.02
    assert torch.equal(out.cpu(), want)


def test_random_ragged_batch_equals_restatement(D):
    rng = np.random.default_rng(31)
    shapes = [(480, 640), (640, 427), (100, 100), (37, 200), (224, 224), (60, 45), (500, 333), (3, 3), (81, 81), (300, 64)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    imgs[3] = np.full(imgs[3].shape, 200, np.uint8)                                   # flat
    imgs[4] = np.repeat(imgs[4][..., :1], 3, axis=2)                                  # grey
    S = 64
    tf = D.BatchTransform(S, train=True, aug_scale=0.3, aug_hflip=0.5, aug_noise_std=0.01, aug_color_jitter=0.8)
    torch.manual_seed(17)
    descs = tf.draw(shapes)
    assert any(d["flip"] for d in descs) and len({d["jitter_order"] for d in descs}) > 3
    noise = torch.randn(len(imgs), 3, S, S)
    out, raw = tf.run(tf.stage(imgs, descs), torch.device("cuda"), noise=noise.cuda(), want_bytes=True)
    out, raw = out.cpu(), raw.cpu()
    for i, (im, d) in enumerate(zip(imgs, descs)):
        want = restated(im, d, S)
        assert np.array_equal(raw[i].numpy(), want), "picture %d" % i
        assert torch.equal(out[i], torch.from_numpy(want.copy()).permute(2, 0, 1).float().div(255) + noise[i] * 0.01)


def test_every_colour_through_the_hue_round_trip(D):
    """all 2^24 colours in one 4096 x 4096 picture (an identity resample, blend factors of 1) through the device's
    RGB -> HSV -> RGB with shifts 0 and +5"""
    a = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    tf = D.BatchTransform(4096, train=True, aug_noise_std=0.0, aug_color_jitter=0.5)
    for shift, order in ((0, (3, 0, 1, 2)), (5, (1, 2, 0, 3))):
        d = D.box_desc(4096, 4096, (0, 0, 4096, 4096), 4096)
        d.update(jitter_fields(order, 1.0, 1.0, 1.0, shift))
        _, raw = tf.run(tf.stage([img], [d]), torch.device("cuda"), want_bytes=True)
        got = raw[0].cpu().numpy()
        del raw
        assert np.array_equal(got, R.hue(img, shift)), "shift %d" % shift


def test_jitter_off_is_the_plain_transform(D):
    rng = np.random.default_rng(5)
    shapes = [(480, 640), (100, 100), (37, 200), (64, 48)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    S = 48
    noise = torch.randn(len(imgs), 3, S, S, device="cuda")
    outs = []
    for x in (0.0, 1.5, 4.0):
        tf = D.BatchTransform(S, train=True, aug_scale=0.5, aug_color_jitter=x)
        torch.manual_seed(2)
        st = tf.stage(imgs)
        assert st.jitter is None
        outs.append(tf.run(st, torch.device("cuda"), noise=noise, want_bytes=True))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    # the jitter entry point with NULL records is sat_image_batch_transform
    from sat_amd import _lib as L
    lib = L.lib()
    torch.manual_seed(2)
    st = D.BatchTransform(S, train=True, aug_scale=0.5).stage(imgs)
    dev = st.host.cuda()
    need = lib.sat_image_batch_workspace_bytes(C.cast(st.desc, C.c_void_p), len(imgs), S, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(len(imgs), 3, S, S, device="cuda")
    L.check(lib.sat_image_batch_transform_jitter(dev.data_ptr() + st.head, st.pixels_bytes, C.cast(st.desc, C.c_void_p), dev.data_ptr(), None, None,
                                                 len(imgs), S, S, L.ptr(noise), 0.01, L.ptr(out), None, L.ptr(ws), need,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "transform_jitter")
    assert torch.equal(out, outs[0][0])


def test_full_size_batch_finite_and_deterministic(D):
    g = torch.Generator().manual_seed(3)
    B, H, W, S = 128, 480, 640, 224
    base = torch.randint(0, 256, (4, H, W, 3), dtype=torch.uint8, generator=g).numpy()
    imgs = [base[i % 4] for i in range(B)]
    tf = D.BatchTransform(S, train=True, aug_color_jitter=0.4)
    torch.manual_seed(12)
    st = tf.stage(imgs)
    noise = torch.randn(B, 3, S, S, device="cuda")
    out1, raw1 = tf.run(st, torch.device("cuda"), noise=noise, want_bytes=True)
    out2, raw2 = tf.run(st, torch.device("cuda"), noise=noise, want_bytes=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out1).all()) and torch.equal(out1, out2) and torch.equal(raw1, raw2)
    descs = [dict(e) for e in _descs_of(st, D)]
    for i in (0, 77):
        assert np.array_equal(raw1[i].cpu().numpy(), restated(imgs[i], descs[i], S)), "picture %d" % i


def _descs_of(st, D):
    """the descriptor dicts a StagedBatch holds, jitter fields included"""
    for e, j in zip(st.desc, st.jitter):
        d = {k: getattr(e, k) for k, _ in e._fields_}
        d.update(jitter_fields(list(j.order), j.brightness, j.contrast, j.saturation, j.hue_shift))
        yield d


def test_rejects_bad_jitter(D):
    from sat_amd import _lib as L
    img = np.zeros((10, 12, 3), np.uint8)
    tf = D.BatchTransform(8, train=True, aug_color_jitter=0.5)
    good = jitter_fields((0, 1, 2, 3), 1.0, 1.0, 1.0, 0)
    for bad in (dict(jitter_order=(0, 0, 2, 3)), dict(jitter_order=(0, 1, 2, 5)), dict(brightness=-1.0), dict(saturation=float("nan")),
                dict(contrast=float("inf")), dict(hue_shift=200), dict(hue_shift=-129)):
        d = D.box_desc(10, 12, (0, 0, 10, 12), 8)
        d.update(good)
        d.update(bad)
        with pytest.raises(L.SatHipError):
            tf.run(tf.stage([img], [d]), torch.device("cuda"))
    d = D.box_desc(10, 12, (0, 0, 10, 12), 8)
    d.update(good)
    out = tf.run(tf.stage([img], [d]), torch.device("cuda"))            # the stream is still usable
    assert out.shape == (1, 3, 8, 8) and bool(torch.isfinite(out).all())
