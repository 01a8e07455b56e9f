"""GPU: the attention-overlay path (csrc/attention_panels.hip, sat_amd/visualize.py) against the CPU reference
(tests/attention_panels_ref.py: numpy + Pillow itself).  Everything is compared for exact equality: the squares' bytes, the fp32
tensors, the panels (the mask arrays keep the rounding margin tests/test_visualize.py asserts), and SAT.visualize against
SAT.caption + attention_panels on the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_panels_ref as R  # noqa: E402


def _mixed_items():
    """every input shape of the size list, one JPEG file the GPU decodes and one PNG file Pillow decodes; and what each decodes to"""
    from PIL import Image
    import io
    arrays = [R.picture(h, w, 20 + i) for i, ((h, w), _) in enumerate(R.SQUARE_CASES)]
    jpg, png = R.jpeg_bytes(R.picture(48, 70, 40)), R.png_bytes(R.picture(33, 21, 41))
    decoded = arrays + [np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB")), np.asarray(Image.open(io.BytesIO(png)).convert("RGB"))]
    return arrays + [jpg, png], decoded


def test_load_square_and_prepare_image_equal_pillow():
    import sat_amd  # noqa: F401
    from sat_amd import jpeg as J, visualize as Z
    items, decoded = _mixed_items()
    assert isinstance(J.as_picture(items[-2]), J.JpegBytes) and not isinstance(J.as_picture(items[-1]), J.JpegBytes)
    # one mixed batch: 1x1 ... 480x640 -> 32 (a 15x shrink, 61 taps, next to 5-tap enlargements)
    got = Z.load_square_batch(items, 32)
    assert got.shape == (len(items), 32, 32, 3) and got.dtype == torch.uint8 and got.is_cuda
    want = np.stack([R.square(a, 32) for a in decoded])
    assert np.array_equal(got.cpu().numpy(), want)
    ten = Z.prepare_image_batch(got)                              # ToTensor alone
    assert ten.shape == (len(items), 3, 32, 32) and ten.dtype == torch.float32
    assert np.array_equal(ten.cpu().numpy(), np.stack([R.to_tensor(s) for s in want]))
    # every (shape, size) pair of the list at its own size; 128 x 130 -> 4 is the largest shrink the entry point accepts (129 taps)
    for size in sorted({s for _, s in R.SQUARE_CASES}):
        arrays = [R.picture(h, w, 60 + i) for i, ((h, w), s) in enumerate(R.SQUARE_CASES) if s == size]
        got = Z.load_square_batch(arrays, size).cpu().numpy()
        for a, g in zip(arrays, got):
            assert np.array_equal(g, R.square(a, size)), (a.shape, size)


def test_load_square_then_prepare_image_chained():
    """prepare_image(load_square(path, 256), 224): the second resample reads the first one's bytes"""
    import sat_amd  # noqa: F401
    from sat_amd import visualize as Z
    pics = [R.picture(300, 420, 1), R.picture(257, 256, 2), R.jpeg_bytes(R.picture(200, 320, 3))]
    sq = Z.load_square_batch(pics, 256)
    ten = Z.prepare_image_batch(sq, 224)
    assert ten.shape == (3, 3, 224, 224)
    for b, s in enumerate(sq.cpu().numpy()):
        want = R.to_tensor(R.square(s, 224))
        assert np.array_equal(ten[b].cpu().numpy(), want), b
    assert np.array_equal(sq[0].cpu().numpy(), R.square(pics[0], 256))


_REFERENCE = {}


def _reference(name):
    """the case's inputs and its expected panels, computed once"""
    if name not in _REFERENCE:
        _, B, _, _, hw, _, power, opacity = R.PANEL_CASES[name]
        squares, alpha, lens = R.alpha_case(name)
        want = np.stack([R.panels(squares[b], alpha[b], int(lens[b]), hw, power, opacity) for b in range(B)])
        for a in (squares, alpha, lens, want):
            a.setflags(write=False)
        _REFERENCE[name] = (squares, alpha, lens, want)
    return _REFERENCE[name]


@pytest.mark.parametrize("name", sorted(R.PANEL_CASES))
def test_attention_panels_equal_the_reference(name):
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, visualize as Z
    _, B, Tmax, V, (h, w), _, power, opacity = R.PANEL_CASES[name]
    squares, alpha, lens, want = _reference(name)
    sq, al, ln = (torch.from_numpy(np.array(a)).cuda() for a in (squares, alpha, lens))
    # through the C ABI into a buffer with a canary behind the output
    n, tail = want.size, 4096
    buf = torch.full((n + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(L.lib().sat_attention_panels(L.ptr(sq), L.ptr(al), L.ptr(ln), B, Tmax, V, h, w, power, opacity, L.ptr(buf), L.stream_ptr()), "sat_attention_panels")
    got = buf.cpu().numpy()
    assert (got[n:] == 0xA5).all(), "wrote past the panels"
    got = got[:n].reshape(want.shape)
    for b in range(B):
        k = int(lens[b])
        assert np.array_equal(got[b, 0], squares[b]), (name, b)
        for t in range(k + 2):
            assert np.array_equal(got[b, t], want[b, t]), (name, b, t, int(np.abs(got[b, t].astype(int) - want[b, t]).max()))
        assert not got[b, k + 2:].any(), (name, b)
        if k == 0 or (h, w) == (1, 1):
            assert not got[b, k + 1].any()                       # the flat rule: a zero "Total Attention"
    assert np.array_equal(got, want)
    # and through the Python surface
    assert np.array_equal(Z.attention_panels(sq, al, ln, (h, w), power, opacity).cpu().numpy(), want)


def _tiny_model():
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=97, embed_dim=24, attention_dim=16, decoder_dim=40,
                deep_output=True)
    torch.manual_seed(42)
    return M.SAT(**vars(O.default_hparams(**over))).cuda().eval()


@pytest.fixture(scope="module")
def tiny_model():
    return _tiny_model()


@pytest.mark.parametrize("batch", [1, 3])
def test_visualize_equals_caption_plus_panels(tiny_model, batch):
    import sat_amd  # noqa: F401
    from sat_amd import visualize as Z
    model = tiny_model
    items = [R.picture(70, 90, 5), R.jpeg_bytes(R.picture(120, 80, 6)), R.picture(64, 64, 7)][:batch]
    kw = dict(beamk=3, max_gen_length=7, temperature=1.0, rescore_method="LN", rescore_reward=1.0)
    vis = model.visualize(items, visual_size=96, input_size=64, **kw)
    squares = Z.load_square_batch(items, 96)
    img = Z.prepare_image_batch(squares, 64)
    caps, scores, alphas, ppl = model.caption(img, return_all=True, **kw)
    assert len(vis) == batch and vis.panels.shape == (batch, 9, 96, 96, 3)
    hw = tuple(alphas[0][0].shape[1:])
    al = torch.zeros(batch, 7, hw[0] * hw[1])
    for b in range(batch):
        assert vis.captions[b] == caps[b][0] and vis.lengths[b] == len(caps[b][0]) and vis.words[b] == model.decode_seq(caps[b][0])
        assert vis.scores[b] == scores[b][0] and vis.perplexities[b] == ppl[b][0], (b, vis.scores[b], scores[b][0], vis.perplexities[b], ppl[b][0])
        al[b, :len(caps[b][0])] = alphas[b][0].reshape(len(caps[b][0]), -1)
    want = Z.attention_panels(squares, al.cuda(), torch.tensor(vis.lengths, dtype=torch.int32).cuda(), hw)
    assert torch.equal(vis.panels, want)
    assert any(vis.lengths) and bool(vis.panels[0, 1].ne(vis.panels[0, 0]).any())
    c2, w2, s2, p2 = model.caption_image(items, visual_size=96, input_size=64, **kw)
    assert (c2, w2, s2, p2) == (vis.captions, vis.words, vis.scores, vis.perplexities)
    sheet = Z.contact_sheet(vis, 0, references=["a reference caption"])
    assert sheet.info["panels"] == 2 + vis.lengths[0]


def test_argument_errors_give_einval_and_launch_nothing():
    """a null pointer, a map above the maximum, a shrink factor above the maximum, opacity outside [0, 1], V <= 0: status 1 with a
    message, and the output buffers keep their fill"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, visualize as Z
    lib = L.lib()
    sq = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device="cuda")
    al = torch.rand(2, 6, 49, device="cuda")
    ln = torch.tensor([2, 6], dtype=torch.int32, device="cuda")
    out = torch.full((2 * 8 * 32 * 32 * 3,), 0x5A, dtype=torch.uint8, device="cuda")

    def panels(square=sq, alpha=al, lens=ln, V=32, h=7, w=7, power=5.0, opacity=0.75, dst=out):
        rc = lib.sat_attention_panels(L.ptr(square), L.ptr(alpha), L.ptr(lens), 2, 6, V, h, w, power, opacity, L.ptr(dst), L.stream_ptr())
        return rc, lib.sat_last_error().decode()

    for kw, word in ((dict(square=None), "null"), (dict(alpha=None), "null"), (dict(lens=None), "null"), (dict(dst=None), "null"),
                     (dict(h=17, w=16), "map 17x16"), (dict(opacity=1.5), "opacity"), (dict(opacity=-0.25), "opacity"), (dict(V=0), "visual size 0"),
                     (dict(V=-32), "visual size -32")):
        rc, msg = panels(**kw)
        assert rc == 1 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    big = torch.zeros(1, 33 * 4 + 1, 140, 3, dtype=torch.uint8, device="cuda")          # side 133 -> 4: more than 32x
    d = (L.ImageDesc * 1)()
    d[0].offset, d[0].height, d[0].width = 0, 133, 140
    dd = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * 4 * 3,), 0x5A, dtype=torch.uint8, device="cuda")
    host = C.cast(d, C.c_void_p)
    for args, word in (((L.ptr(big), big.numel(), host, L.ptr(dd), 1, 4, L.ptr(dst), None), "shrinks by more than 32x"),
                       ((None, big.numel(), host, L.ptr(dd), 1, 8, L.ptr(dst), None), "null"),
                       ((L.ptr(big), big.numel(), host, L.ptr(dd), 1, 0, L.ptr(dst), None), "size 0")):
        rc = lib.sat_image_square_bicubic(*args, L.ptr(ws), ws.numel(), L.stream_ptr())
        assert rc == 1 and word in lib.sat_last_error().decode(), (word, rc, lib.sat_last_error())
    torch.cuda.synchronize()
    assert bool((dst == 0x5A).all())
    with pytest.raises(L.SatHipError, match="shrinks by more than 32x"):
        Z.load_square_batch([np.zeros((133, 140, 3), np.uint8)], 4)
    with pytest.raises(L.SatHipError, match="opacity"):
        Z.attention_panels(sq, al, ln, (7, 7), opacity=2.0)
