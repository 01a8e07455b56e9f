"""GPU: sat_jpeg_decode_progressive_batch / sat_amd.jpeg with ``progressive=True`` against Pillow's bytes, compared EXACTLY (integer
arithmetic: no tolerance): every scan shape of the two scripts Pillow writes, alone and in one batch, with and without restart
markers; mixed with every other kind of file; through BatchTransform, DeviceLoader, load_square_batch and SAT.caption_image; and a
damaged scan next to good pictures."""
import random

import numpy as np
import pytest
import torch

import jpeg_progressive_ref as P

pytestmark = pytest.mark.gpu

CASES = P.small_cases()


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
def want():
    """Pillow's pixels of every case, once"""
    return {name: P.pillow(f) for name, f in CASES.items()}


def test_all_cases_in_one_batch(J, want):
    names = list(CASES)
    out, status, info = J.decode_jpeg_batch([CASES[n] for n in names], "cuda", check=False, progressive=True, return_info=True)
    assert status.tolist() == [0] * len(names)
    for n, t, row in zip(names, out, info.tolist()):
        assert np.array_equal(t.cpu().numpy(), want[n]), n
        assert row == ([3, 6, 3, 0] if n.startswith("gray") else [3, 10, 3, 0]), n


@pytest.mark.parametrize("name", list(CASES))
def test_each_case_alone(J, want, name):
    (t,), status = J.decode_jpeg_batch([CASES[name]], "cuda", check=False, progressive=True)
    assert status.tolist() == [0]
    assert np.array_equal(t.cpu().numpy(), want[name])


def test_workload_size_matches_pillow_and_the_restatement(J):
    f = P.encode(P.picture(480, 640, 3, noise=70.0), progressive=True, quality=95, subsampling=2)
    (t,) = J.decode_jpeg_batch([f], "cuda", progressive=True)
    got = t.cpu().numpy()
    assert np.array_equal(got, P.pillow(f))
    assert np.array_equal(got, P.decode(f))


def _mixed():
    import io
    from PIL import Image
    a = P.picture(40, 57, 21)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, "JPEG")
    kinds = {"base": P.encode(a, quality=85, subsampling=2), "base_rst": P.encode(a, quality=85, subsampling=1, restart_marker_rows=1),
             "prog": CASES["420_q100_40x57"], "prog_rst": CASES["422_q10_rst_40x57"], "gray_prog": CASES["gray_33x65"], "png": buf.getvalue(),
             "cmyk": cmyk.getvalue()}
    order = ["prog", "png", "base", "prog_rst", "cmyk", "base_rst", "gray_prog", "prog", "base", "prog_rst"]
    return kinds, order


def test_mixed_batch_with_and_without_the_option(J):
    kinds, order = _mixed()
    files = [kinds[k] for k in order]
    ref = {k: P.pillow(f) for k, f in kinds.items()}
    out, info = J.decode_jpeg_batch(files, "cuda", progressive=True, return_info=True)
    off, info_off = J.decode_jpeg_batch(files, "cuda", return_info=True)
    for k, t, u, row, row_off in zip(order, out, off, info.tolist(), info_off.tolist()):
        assert np.array_equal(t.cpu().numpy(), ref[k]), k
        assert np.array_equal(u.cpu().numpy(), ref[k]), k
        if k in ("png", "cmyk"):
            assert row == row_off == [-1] * 4
        elif k.startswith("base"):
            assert row == row_off and row[3] == 0                                # what it is without the option
        else:
            assert row == ([3, 6, 3, 0] if k == "gray_prog" else [3, 10, 3, 0]) and row_off == [-1] * 4


def test_transform_of_progressive_bytes_equals_transform_of_decoded_arrays(D, J):
    names = ["420_q100_40x57", "444_q10_rst_40x57", "gray_33x65", "422_q100_rst_40x57"]
    files = [CASES[n] for n in names] + [P.encode(P.picture(60, 80, 30), quality=80, subsampling=2)]
    arrays = [P.pillow(f) for f in files]
    items = [J.as_picture(f, progressive=True) for f in files]
    assert all(isinstance(x, J.JpegBytes) for x in items)
    tf = D.BatchTransform(24, train=True, aug_scale=0.5, aug_hflip=0.5, aug_noise_std=0.01)
    res = []
    for batch in (arrays, items):
        torch.manual_seed(123)
        random.seed(123)
        staged = tf.stage(batch)
        noise = torch.randn(len(batch), 3, 24, 24, generator=torch.Generator().manual_seed(7)).cuda()
        res.append(tf.run(staged, torch.device("cuda"), noise=noise, want_bytes=True))
        if batch is items:
            assert staged.jpeg.n == 5 and staged.jpeg.n_progressive == 4 and staged.jpeg_index == [4, 0, 1, 2, 3]
            assert staged.status.cpu().tolist() == [0] * 5
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0], res[1][0])


def _loader_batches(D, ds, seed):
    tf = D.BatchTransform(32, train=True, aug_scale=0.6, aug_hflip=0.5, aug_noise_std=0.0)
    torch.manual_seed(seed)
    loader = D.DeviceLoader(ds, batch_size=4, transform=tf, workers=2, prefetch=2)
    return [[t.cpu() for t in b] for b in loader]


def test_device_loader_read_jpeg_progressive_equals_decode_rgb(D, J, tmp_path):
    paths, caps, lens = [], [], []
    for k in range(8):
        kw = dict(quality=60 + 5 * k, subsampling=k % 3, progressive=k % 2 == 0)
        if k in (2, 3):
            kw["restart_marker_rows"] = 1
        p = tmp_path / ("%d.jpg" % k)
        p.write_bytes(P.encode(P.picture(50 + 3 * k, 70 - 2 * k, 40 + k), **kw))
        paths.append(str(p))
        caps.append([[1, 2 + k, 3, 0]])
        lens.append([3])
    meta = {"vocab_stoi": {"<UNK>": 0}, "train": {"img_paths": paths, "encoded_captions": caps, "lengths": lens}}
    ds_rgb = D.CocoCaptionDataset(meta, decode=D.decode_rgb)
    ds_jpg = D.CocoCaptionDataset(meta, decode=J.read_jpeg_progressive)
    assert all(isinstance(ds_jpg[k][0], J.JpegBytes) for k in range(8)) and ds_jpg[0][0].header.progressive
    a, b = _loader_batches(D, ds_rgb, 5), _loader_batches(D, ds_jpg, 5)
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)


def test_a_damaged_refinement_scan_stays_inside_its_picture(J, want):
    """the entropy bytes of one AC-refinement scan replaced by seeded random bytes (every 0xFF followed by 0x00, so the parser still
    takes the file): the call returns and the good pictures next to it are exact.  Nothing is asserted about the damaged picture:
    random bits can be a valid stream."""
    name = "420_q100_40x57"
    f = bytearray(CASES[name])
    hd = J.parse(bytes(f), progressive=True)
    sc = hd.scans[5]
    assert sc.ah == 2 and sc.ss == 1
    n = sc.data_end - sc.data_start
    rnd = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8)
    ff = np.flatnonzero(rnd == 0xFF)
    rnd[ff] = 0xFE
    rnd[0:2] = (0xFF, 0x00)
    f[sc.data_start:sc.data_end] = rnd.tobytes()
    assert J.parse(bytes(f), progressive=True).fallback is None
    good = ["444_q100_40x57", "gray_rst_33x65"]
    out, status = J.decode_jpeg_batch([CASES[good[0]], bytes(f), CASES[good[1]]], "cuda", check=False, progressive=True)
    assert status[0] == 0 and status[2] == 0
    assert np.array_equal(out[0].cpu().numpy(), want[good[0]]) and np.array_equal(out[2].cpu().numpy(), want[good[1]])
    assert out[1].shape == (40, 57, 3)


def test_load_square_batch_and_caption_image(J):
    """a progressive file through the visualize entry points equals Pillow's decoded pixels through the same entry points (a
    baseline re-encoding of those pixels is not bit-equal to them, so the decoded array is the Pillow path here)"""
    import sat_amd  # noqa: F401
    from sat_amd import visualize as Z
    from test_gpu_visualize import _tiny_model
    f = P.encode(P.picture(70, 90, 5), progressive=True, quality=90, subsampling=2)
    a = P.pillow(f)
    sq = Z.load_square_batch([f], 48, progressive=True)
    assert torch.equal(sq, Z.load_square_batch([a], 48))
    assert torch.equal(sq, Z.load_square_batch([f], 48))                      # without the option Pillow decodes it: the same pixels
    model = _tiny_model()
    kw = dict(beamk=2, max_gen_length=5, visual_size=48, input_size=64)
    assert model.caption_image([f], progressive=True, **kw) == model.caption_image([a], **kw)
