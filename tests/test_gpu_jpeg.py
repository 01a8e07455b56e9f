"""GPU: sat_jpeg_decode_batch / sat_amd.jpeg against Pillow's bytes (g15, made by tests/golden/make_jpeg_golden.py) and the
numpy restatement (tests/jpeg_ref.py), compared EXACTLY; the transform fed JPEG bytes against the transform fed decode_rgb's
arrays; DeviceLoader over JPEG files; a truncated file."""
import io
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    import sat_amd  # noqa: F401
    from sat_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def D():
    import sat_amd  # noqa: F401
    from sat_amd import data
    return data


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_jpeg.npz"), allow_pickle=False)


def picture(h, w, seed, noise=12.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1), 128 + 100 * np.sin((x + 2 * y) / 5.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, noise, (h, w, 3))), 0, 255).astype(np.uint8)


def encode(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def test_every_fixture_picture_decodes_bit_exact(J, g15):
    files = [g15["jpeg%d" % i].tobytes() for i in range(len(g15["cases"]))]
    out = J.decode_jpeg_batch(files, "cuda")
    for i, name in enumerate(g15["cases"]):
        assert isinstance(J.as_picture(files[i]), J.JpegBytes) == bool(g15["gpu"][i]), name
        assert np.array_equal(out[i].cpu().numpy(), g15["rgb%d" % i]), name


def test_each_fixture_picture_alone(J, g15):
    for i, name in enumerate(g15["cases"]):
        if g15["gpu"][i]:
            (t,) = J.decode_jpeg_batch([g15["jpeg%d" % i].tobytes()], "cuda")
            assert np.array_equal(t.cpu().numpy(), g15["rgb%d" % i]), name


def test_large_pictures_match_pillow_and_the_restatement(J):
    import jpeg_ref as R
    a = picture(480, 640, 3)
    files = [encode(a, quality=90, subsampling=2), encode(a, quality=90, subsampling=0, restart_marker_rows=2),
             encode(a, quality=100, subsampling=1), encode(a[:, :, 1], quality=95), encode(picture(481, 643, 4, 70.0), quality=100, subsampling=2)]
    out = J.decode_jpeg_batch(files, "cuda")
    for k, f in enumerate(files):
        got = out[k].cpu().numpy()
        assert np.array_equal(got, pillow(f)), k
        if k in (0, 4):
            assert np.array_equal(got, R.decode(f)), k


def test_mixed_batch(J, g15):
    """GPU-decoded, restart-marker and fallback pictures in one call, in an interleaved order, with repeats"""
    names = list(g15["cases"])
    pick = [names.index(n) for n in ("png_40x57", "q75_420_17x9", "rst_rows1_422_40x57", "progressive_40x57", "gray_q10_33x65",
                                    "rst_blocks1_420_40x57", "cmyk_40x57", "q100_444_33x65", "q75_420_17x9", "adobe_rgb_40x57", "q75_422_1x1")]
    out = J.decode_jpeg_batch([g15["jpeg%d" % i].tobytes() for i in pick], "cuda")
    for t, i in zip(out, pick):
        assert np.array_equal(t.cpu().numpy(), g15["rgb%d" % i]), names[i]


def test_truncated_stream_sets_its_status_and_spares_the_others(J):
    a = picture(64, 96, 5)
    good = encode(a, quality=90)
    rst = encode(a, quality=90, restart_marker_rows=1)
    files = [good, good[:len(good) // 2], rst, rst[:len(rst) * 2 // 3], good]
    out, status = J.decode_jpeg_batch(files, "cuda", check=False)
    st = status.tolist()
    assert st[1] != 0 and st[3] != 0, st
    assert st[0] == st[2] == st[4] == 0, st
    for k in (0, 2, 4):
        assert np.array_equal(out[k].cpu().numpy(), pillow(files[k])), k
    with pytest.raises(J.JpegDecodeError, match="picture 1"):
        J.decode_jpeg_batch(files, "cuda")
    with pytest.raises(OSError):
        pillow(files[1])                     # Pillow raises on the truncated file too


@pytest.mark.parametrize("kw", [dict(), dict(aug_color_jitter=0.4, aug_optical_strength=0.5)], ids=["plain", "jitter_optical"])
def test_transform_of_jpeg_bytes_equals_transform_of_decoded_arrays(D, J, kw):
    files = [encode(picture(90 + 7 * k, 120 - 5 * k, 10 + k), quality=70 + 3 * k, subsampling=k % 3, **(dict(restart_marker_blocks=5) if k % 4 == 1 else {}))
             for k in range(8)]
    files.append(encode(picture(60, 80, 30), quality=80, progressive=True))              # falls back to Pillow
    arrays = [pillow(f) for f in files]
    tf = D.BatchTransform(56, train=True, aug_scale=0.5, aug_hflip=0.5, aug_noise_std=0.01, **kw)
    res = []
    for items in (arrays, files):
        torch.manual_seed(123)
        random.seed(123)
        staged = tf.stage(items)
        noise = torch.randn(len(items), 3, 56, 56, generator=torch.Generator().manual_seed(7)).cuda()
        res.append(tf.run(staged, torch.device("cuda"), noise=noise, want_bytes=True))
        if items is files:
            assert staged.jpeg is not None and staged.jpeg.n == 8
            assert staged.status.cpu().tolist() == [0] * 8
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0], res[1][0])


def _loader_batches(D, ds, seed):
    tf = D.BatchTransform(48, train=True, aug_scale=0.6, aug_hflip=0.5, aug_noise_std=0.0)
    torch.manual_seed(seed)
    loader = D.DeviceLoader(ds, batch_size=4, transform=tf, workers=2, prefetch=2)
    return [[t.cpu() for t in b] for b in loader]


def test_device_loader_read_jpeg_equals_decode_rgb(D, J, tmp_path):
    paths, caps, lens = [], [], []
    for k in range(10):
        kw = dict(quality=60 + 4 * k, subsampling=k % 3)
        if k == 3:
            kw["restart_marker_rows"] = 1
        if k == 7:
            kw["progressive"] = True
        p = tmp_path / ("%d.jpg" % k)
        p.write_bytes(encode(picture(70 + 3 * k, 90 - 2 * k, 40 + k), **kw))
        paths.append(str(p))
        caps.append([[1, 2 + k, 3, 0]])
        lens.append([3])
    meta = {"vocab_stoi": {"<UNK>": 0}, "train": {"img_paths": paths, "encoded_captions": caps, "lengths": lens}}
    ds_rgb = D.CocoCaptionDataset(meta, decode=D.decode_rgb)
    ds_jpg = D.CocoCaptionDataset(meta, decode=J.read_jpeg)
    assert isinstance(ds_jpg[0][0], J.JpegBytes) and isinstance(ds_jpg[7][0], np.ndarray)
    a, b = _loader_batches(D, ds_rgb, 5), _loader_batches(D, ds_jpg, 5)
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)
    # a truncated file: the loader raises on the consumer side and names the dataset index
    with open(paths[6], "rb") as f:
        data = f.read()
    with open(paths[6], "wb") as f:
        f.write(data[:len(data) // 2])
    assert isinstance(ds_jpg[6][0], J.JpegBytes)
    with pytest.raises(J.JpegDecodeError, match="dataset index 6"):
        _loader_batches(D, ds_jpg, 5)
