"""GPU: the many-lane entropy decoding of sat_jpeg_decode_batch_ex (restart-free pictures cut into subsequences) against
Pillow's bytes and against the same call kept on the serial lanes, compared EXACTLY; the path each picture reports; bad streams,
which must come out as the serial path leaves them; the options through BatchTransform and DeviceLoader."""
import io
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


def encode(a, fmt="JPEG", **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, fmt, **kw)
    return buf.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


NAMES = ["noise_96x128_q100_444", "odd_97x131_q75_420", "optimized_64x96_q95_422", "flat_gray_256x256", "ramp_gray_64x256"]


@pytest.fixture(scope="module")
def chosen():
    """the pictures of tests/test_jpeg_parallel.py and Pillow's bytes of each, once"""
    files = [encode(picture(96, 128, 4, noise=70.0), quality=100, subsampling=0), encode(picture(97, 131, 5), quality=75, subsampling=2),
             encode(picture(64, 96, 6), quality=95, subsampling=1, optimize=True), encode(np.full((256, 256), 128, np.uint8)),
             encode(np.repeat(np.linspace(0, 255, 256).astype(np.uint8)[None, :], 64, 0))]
    return files, [pillow(f) for f in files]


def data_bytes(J, f):
    hd = J.parse(f)
    assert hd.fallback is None and len(hd.segments) == 1
    return hd.data_end - hd.data_start


def test_fixture_pictures_on_the_parallel_path(J, g15):
    pick = []
    for i, name in enumerate(g15["cases"]):
        f = g15["jpeg%d" % i].tobytes()
        if g15["gpu"][i] and len(J.parse(f).segments) == 1:
            pick.append((i, name, f))
    assert len(pick) >= 10 and any("1x1" in n for _, n, _ in pick) and any("gray" in n for _, n, _ in pick)
    out, info = J.decode_jpeg_batch([f for _, _, f in pick], "cuda", subseq_bytes=16, parallel_min_bytes=0, return_info=True)
    for t, row, (i, name, f) in zip(out, info.tolist(), pick):
        assert np.array_equal(t.cpu().numpy(), g15["rgb%d" % i]), name
        nbytes = data_bytes(J, f)
        if nbytes > 16:
            assert row[0] == 1, (name, row)
        assert row[0] in (0, 1) and row[1] == (-(-nbytes // 16) if row[0] else 0) and row[3] == 0, (name, row)


@pytest.mark.parametrize("subseq", [16, 32, 128])
def test_chosen_pictures(J, chosen, subseq):
    files, want = chosen
    if subseq != 16:
        files, want = files[:1], want[:1]
    out, info = J.decode_jpeg_batch(files, "cuda", subseq_bytes=subseq, parallel_min_bytes=0, return_info=True)
    serial, sinfo = J.decode_jpeg_batch(files, "cuda", subseq_bytes=subseq, parallel_min_bytes=J.NEVER_PARALLEL, return_info=True)
    assert sinfo.tolist() == [[0, 0, 0, 0]] * len(files)
    for k, f in enumerate(files):
        print(NAMES[k], "subseq_bytes", subseq, "info", info[k].tolist())
        assert np.array_equal(out[k].cpu().numpy(), want[k]), NAMES[k]
        assert torch.equal(out[k], serial[k]), NAMES[k]
        path, subs, iters, zero = info[k].tolist()
        assert path == 1 and zero == 0, (NAMES[k], info[k].tolist())
        assert subs == -(-data_bytes(J, f) // subseq), NAMES[k]
        assert 1 <= iters <= subs, (NAMES[k], iters, subs)


def test_default_options(J, chosen):
    files, want = chosen
    out, info = J.decode_jpeg_batch(files, "cuda", return_info=True)
    for k, f in enumerate(files):
        assert np.array_equal(out[k].cpu().numpy(), want[k]), NAMES[k]
        nbytes = data_bytes(J, f)
        admitted = nbytes >= J.PARALLEL_MIN_BYTES_DEFAULT
        assert info[k].tolist()[:2] == ([1, -(-nbytes // J.SUBSEQ_BYTES_DEFAULT)] if admitted else [0, 0]), (NAMES[k], info[k].tolist())
    assert info[0, 0] == 1                                                    # 47,804 bytes: far above any sensible threshold
    assert J.decode_jpeg_batch(files[:1], "cuda")[0].equal(out[0])            # the plain call returns the tensors alone


def test_mixed_batch(J, chosen):
    a = picture(80, 112, 8)
    free, rst = encode(a, quality=92, subsampling=2), encode(a, quality=92, subsampling=2, restart_marker_rows=1)
    small, prog, png = encode(picture(24, 40, 9), quality=60), encode(a, quality=80, progressive=True), encode(a, "PNG")
    assert data_bytes(J, free) >= 2048 > data_bytes(J, small) and len(J.parse(rst).segments) > 1
    kinds = {"free": (free, 1), "rst": (rst, 0), "small": (small, 0), "prog": (prog, -1), "png": (png, -1)}
    order = ["png", "free", "rst", "small", "prog", "free", "small", "rst", "free"]
    files = [kinds[k][0] for k in order]
    out, info = J.decode_jpeg_batch(files, "cuda", parallel_min_bytes=2048, return_info=True)
    assert info[:, 0].tolist() == [kinds[k][1] for k in order]
    assert [r for r, k in zip(info.tolist(), order) if kinds[k][1] == -1] == [[-1] * 4] * 2
    want = {k: pillow(f) for k, (f, _) in kinds.items()}
    for t, k in zip(out, order):
        assert np.array_equal(t.cpu().numpy(), want[k]), k


@pytest.mark.parametrize("subseq", [16, None], ids=["16", "default"])
def test_bad_streams_come_out_as_the_serial_path_leaves_them(J, chosen, subseq):
    """bounded-input checks, as the truncated-file test of test_gpu_jpeg.py: cut files and a file with a random tail"""
    good = chosen[0][2]                                                       # the 64x96 picture
    hd = J.parse(good)
    n = len(good)
    tail0 = hd.data_start + 2 * (hd.data_end - hd.data_start) // 3
    noise = np.random.default_rng(11).integers(0, 256, hd.data_end - tail0, dtype=np.uint8)
    noise[noise == 0xFF] = 0xFE
    bad = [good[:n // 4], good[:n // 2], good[:n * 7 // 8], good[:tail0] + noise.tobytes() + good[hd.data_end:]]
    files = [good]
    for b in bad:
        files += [b, good]
    res = J.decode_jpeg_batch(files, "cuda", check=False, subseq_bytes=subseq, parallel_min_bytes=0, return_info=True)
    ref = J.decode_jpeg_batch(files, "cuda", check=False, subseq_bytes=subseq, parallel_min_bytes=J.NEVER_PARALLEL, return_info=True)
    (out, status, info), (out0, status0, info0) = res, ref
    print("status", status.tolist(), "paths", info[:, 0].tolist())
    assert info0[:, 0].tolist() == [0] * len(files)
    assert status.tolist() == status0.tolist()
    for k in range(len(files)):
        assert torch.equal(out[k], out0[k]), k
    for k in (1, 3, 5):
        assert status[k] != 0 and info[k, 0] == 2, (k, status.tolist(), info.tolist())
    assert info[7, 0] in (1, 2)
    for k in (0, 2, 4, 6, 8):
        assert status[k] == 0 and info[k, 0] == 1, (k, status.tolist(), info.tolist())
        assert np.array_equal(out[k].cpu().numpy(), chosen[1][2]), k


def test_pipeline_with_jpeg_options(D, J, tmp_path):
    files = [encode(picture(90 + 7 * k, 120 - 5 * k, 10 + k), quality=70 + 3 * k, subsampling=k % 3) for k in range(8)]
    assert all(len(J.parse(f).segments) == 1 for f in files)
    arrays = [pillow(f) for f in files]
    tf = D.BatchTransform(56, train=True, aug_scale=0.5, aug_hflip=0.5, aug_noise_std=0.01, jpeg_subseq_bytes=32, jpeg_parallel_min_bytes=0)
    res = []
    for items in (arrays, files):
        torch.manual_seed(123)
        random.seed(123)
        staged = tf.stage(items)
        noise = torch.randn(len(items), 3, 56, 56, generator=torch.Generator().manual_seed(7)).cuda()
        res.append(tf.run(staged, torch.device("cuda"), noise=noise, want_bytes=True))
        if items is files:
            assert staged.jpeg is not None and staged.jpeg.n == 8 and staged.status.cpu().tolist() == [0] * 8
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[1][0])
    # the same files through DeviceLoader
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("%d.jpg" % k)
        p.write_bytes(f)
        paths.append(str(p))
    meta = {"vocab_stoi": {"<UNK>": 0}, "train": {"img_paths": paths, "encoded_captions": [[[1, 2 + k, 3, 0]] for k in range(8)],
                                                  "lengths": [[3]] * 8}}
    batches = []
    for decode in (D.decode_rgb, J.read_jpeg):
        ds = D.CocoCaptionDataset(meta, decode=decode)
        tfl = D.BatchTransform(48, train=True, aug_scale=0.6, aug_hflip=0.5, aug_noise_std=0.0, jpeg_subseq_bytes=32, jpeg_parallel_min_bytes=0)
        torch.manual_seed(5)
        loader = D.DeviceLoader(ds, batch_size=4, transform=tfl, workers=2, prefetch=2)
        batches.append([[t.cpu() for t in b] for b in loader])
    assert isinstance(D.CocoCaptionDataset(meta, decode=J.read_jpeg)[0][0], J.JpegBytes)
    assert len(batches[0]) == len(batches[1]) == 2
    for x, y in zip(*batches):
        for s, t in zip(x, y):
            assert torch.equal(s, t)
