"""The reference's ``visualize.ipynb`` (``make_visual``) for a batch, on the device: picture files in, captions and attention
overlays out, with no per-picture host round trip.

* ``load_square_batch``     util.py's ``load_square``: decode (GPU JPEG decoder, Pillow for the files it does not take), centre-crop to
                            the largest square, ``Image.resize((size, size))`` = Pillow's BICUBIC, bit exact (sat_image_square_bicubic)
* ``prepare_image_batch``   util.py's ``prepare_image`` on those squares: the same resample once more, then ``T.ToTensor()``
* ``attention_panels``      the picture, one overlay per caption step, "Total Attention" (sat_attention_panels)
* ``visualize`` / ``caption_image``   the whole chain behind ``SAT.visualize`` / ``SAT.caption_image``
* ``contact_sheet``         the notebook's figure layout with Pillow, on the host

Where the notebook leaves the result open the project defines it: an overlay is ``Image.blend(picture, mask, opacity)``
(two stacked matplotlib ``imshow`` calls depend on the figure's DPI), and a flat attention map (0 / 0 in the notebook) gives a zero mask.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import constraints
from . import jpeg as J


class Visual:
    """What ``SAT.visualize`` returns.  Per picture b: ``captions[b]`` the winning token list, ``words[b]`` = ``decode_seq`` of it,
    ``scores[b]`` / ``perplexities[b]`` floats, ``lengths[b]``; ``panels`` (B, max_gen_length + 2, V, V, 3) uint8 on the device: panel 0
    the picture, 1 .. len the overlays, len + 1 "Total Attention", zero beyond.  ``names``: the pictures' file stems where known."""

    def __init__(self, captions, words, scores, perplexities, lengths, panels, names=None):
        self.captions, self.words, self.scores, self.perplexities, self.lengths, self.panels = captions, words, scores, perplexities, lengths, panels
        self.names = names if names is not None else [None] * len(captions)

    def __len__(self):
        return len(self.captions)


def _cuda(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise L.SatHipError("sat_amd renders on the GPU only: got device %s (no CPU fallback)" % device)
    return device


def _square_bicubic(pixels_ptr, pixels_bytes, desc, desc_dev_ptr, n, size, device, want_bytes, want_tensor):
    """sat_image_square_bicubic on n pictures described by ``desc`` (host ``ImageDesc`` array; its device copy at ``desc_dev_ptr``)"""
    lib = L.lib()
    need = lib.sat_image_square_bicubic_workspace_bytes(C.cast(desc, C.c_void_p), n, size)
    if need == 0:
        L.check(1, "sat_image_square_bicubic_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    raw = torch.empty(n, size, size, 3, dtype=torch.uint8, device=device) if want_bytes else None
    out = torch.empty(n, 3, size, size, dtype=torch.float32, device=device) if want_tensor else None
    L.check(lib.sat_image_square_bicubic(pixels_ptr, pixels_bytes, C.cast(desc, C.c_void_p), desc_dev_ptr, n, size, L.ptr(raw), L.ptr(out), L.ptr(ws),
                                         ws.numel(), L.stream_ptr()), "sat_image_square_bicubic")
    return raw, out


def _as_item(item, progressive=False):
    if isinstance(item, (str, os.PathLike)):
        return J.read_jpeg_progressive(item) if progressive else J.read_jpeg(item)
    if torch.is_tensor(item):
        item = item.cpu().numpy()
    return J.as_picture(item, progressive=progressive)


def _load_squares(items, size, device, progressive=False):
    """``load_square_batch`` plus the JPEG decoder's status words ((number of GPU-decoded files,) int32 on the device, or None) and the
    positions of those files in ``items``: the caller reads them when it reads everything else"""
    from .data import StagedBatch
    device = _cuda(device)
    size = int(size or 0)
    if size <= 0:
        raise L.SatHipError("load_square_batch: size=%r (the squares of one batch share one size > 0)" % (size,))
    pics = [_as_item(x, progressive) for x in items]
    if not pics:
        raise ValueError("load_square_batch: no picture")
    staged = StagedBatch(pics, [dict(height=int(p.shape[0]), width=int(p.shape[1])) for p in pics])
    stream = torch.cuda.current_stream(device)
    dev = torch.empty(staged.device_bytes, dtype=torch.uint8, device=device)
    dev[:staged.host.numel()].copy_(staged.host, non_blocking=True)
    status = None
    if staged.jpeg is not None:                 # the GPU decodes its files into the room behind the copied bytes
        jb = staged.jpeg
        jws = torch.empty(jb.workspace_bytes(), dtype=torch.uint8, device=device)
        status = torch.empty(jb.n, dtype=torch.int32, device=device)
        jb.launch(dev.data_ptr() + staged.jpeg_off, dev.data_ptr() + staged.head, staged.pixels_bytes, status, jws, stream)
    raw, _ = _square_bicubic(dev.data_ptr() + staged.head, staged.pixels_bytes, staged.desc, dev.data_ptr(), staged.n, size, device, True, False)
    return raw, status, staged.jpeg_index


def _raise_bad_jpeg(status, index):
    if status is None:
        return
    st = status.cpu().tolist() if torch.is_tensor(status) else list(status)
    bad = [(i, s) for i, s in zip(index, st) if s]
    if bad:
        raise J.JpegDecodeError("corrupt JPEG data: " + "; ".join("picture %d: %s" % (i, J.status_text(int(s))) for i, s in bad))


def load_square_batch(items, size, device="cuda", progressive=False):
    """util.py:141-143 ``load_square(path, size)`` for a batch: ``items`` are file paths, JPEG bytes (``jpeg.JpegBytes`` or plain bytes: the
    GPU decodes what it can, Pillow the rest) or decoded (H, W, 3) uint8 arrays of any shapes.  Returns (B, size, size, 3) uint8 on
    ``device``, the bytes ``crop_max_square`` leaves in the PIL image.  A corrupt GPU-decoded file raises ``jpeg.JpegDecodeError``.
    ``progressive``: the GPU also decodes the progressive files ``jpeg.parse(progressive=True)`` admits."""
    raw, status, index = _load_squares(items, size, device, progressive)
    _raise_bad_jpeg(status, index)
    return raw


def prepare_image_batch(squares, size=None):
    """util.py:146-149 ``prepare_image(img, size)`` for a batch of squares (B, V, V, 3) uint8 on the device: ``crop_max_square`` to
    ``size`` (BICUBIC again; nothing to crop), then ``T.ToTensor()``.  A falsy ``size`` is the ToTensor step alone.  Returns
    (B, 3, size, size) float32."""
    L.require_gpu(squares)
    if squares.dtype != torch.uint8 or squares.dim() != 4 or squares.shape[3] != 3 or squares.shape[1] != squares.shape[2]:
        raise ValueError("prepare_image_batch: expected (B, V, V, 3) uint8, got %s %s" % (tuple(squares.shape), squares.dtype))
    squares = squares.contiguous()
    B, V = int(squares.shape[0]), int(squares.shape[1])
    size = int(size) if size else V             # V -> V: every tap table is the identity, the bytes pass through both passes unchanged
    desc = (L.ImageDesc * B)()
    for b in range(B):
        desc[b].offset, desc[b].height, desc[b].width = b * V * V * 3, V, V
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(squares.device)
    _, out = _square_bicubic(squares.data_ptr(), squares.numel(), desc, desc_dev.data_ptr(), B, size, squares.device, False, True)
    return out


def attention_panels(squares, cap_alpha, cap_len, map_shape, power=5.0, opacity=0.75):
    """The panels of ``make_visual``: ``squares`` (B, V, V, 3) uint8, ``cap_alpha`` (B, Tmax, h * w) float32 and ``cap_len`` (B) int32 as
    ``evaluation.select_hypotheses(..., with_alpha=True)`` returns them, ``map_shape`` = (h, w).  Returns (B, Tmax + 2, V, V, 3) uint8
    (layout and arithmetic: include/sat_hip.h, sat_attention_panels)."""
    L.require_gpu(squares, cap_alpha, cap_len)
    h, w = int(map_shape[0]), int(map_shape[1])
    if squares.dtype != torch.uint8 or squares.dim() != 4 or squares.shape[3] != 3 or squares.shape[1] != squares.shape[2]:
        raise ValueError("attention_panels: squares must be (B, V, V, 3) uint8, got %s %s" % (tuple(squares.shape), squares.dtype))
    B, V = int(squares.shape[0]), int(squares.shape[1])
    if cap_alpha.dtype != torch.float32 or cap_alpha.dim() != 3 or cap_alpha.shape[0] != B or cap_alpha.shape[2] != h * w:
        raise ValueError("attention_panels: cap_alpha must be (%d, Tmax, %d) float32, got %s %s" % (B, h * w, tuple(cap_alpha.shape), cap_alpha.dtype))
    if cap_len.dtype != torch.int32 or tuple(cap_len.shape) != (B,):
        raise ValueError("attention_panels: cap_len must be (%d,) int32, got %s %s" % (B, tuple(cap_len.shape), cap_len.dtype))
    squares, cap_alpha, cap_len = squares.contiguous(), cap_alpha.contiguous(), cap_len.contiguous()
    Tmax = int(cap_alpha.shape[1])
    panels = torch.empty(B, Tmax + 2, V, V, 3, dtype=torch.uint8, device=squares.device)
    L.check(L.lib().sat_attention_panels(L.ptr(squares), L.ptr(cap_alpha), L.ptr(cap_len), B, Tmax, V, h, w, float(power), float(opacity), L.ptr(panels),
                                         L.stream_ptr()), "sat_attention_panels")
    return panels


def _names(items):
    return [os.path.splitext(os.path.basename(os.fspath(x)))[0] if isinstance(x, (str, os.PathLike)) else None for x in items]


@torch.no_grad()
def _search(model, items, opt, beamk, max_gen_length, temperature, rescore_method, rescore_reward, visual_size, input_size, with_alpha, progressive, mbr_corpus,
            mbr_reward, mbr_alpha):
    """load_square -> prepare_image -> encoder -> batched search -> the winning hypothesis of every picture, all enqueued back to back;
    ``opt``: the caller's ``constraints.SearchOptions``"""
    from . import evaluation as E
    if int(max_gen_length) < 1:
        raise ValueError("visualize: max_gen_length >= 1 (the batched search)")
    opt.resolve(model.hp.vocab_stoi, model.hp.vocab_size, len(items), beamk, max_gen_length)     # refuse before any launch, and before any picture is read
    constraints.check_mbr(rescore_method, mbr_corpus, mbr_reward, mbr_alpha, beamk, model.hp.vocab_size, max_gen_length)
    dev = model.embedding.weight.device
    model.eval()
    squares, status, index = _load_squares(items, visual_size, dev, progressive)
    img = prepare_image_batch(squares, input_size if input_size is not None else model.hp.get("input_size"))
    ann_bld, hw = model.encode(img)
    o = model._beam_search_device(ann_bld.contiguous(), beamk, max_gen_length, temperature, options=opt)
    sel = E.select_hypotheses(o, model.pad_idx, rescore_method, rescore_reward, with_alpha=with_alpha, mbr_corpus=mbr_corpus, mbr_reward=mbr_reward,
                              mbr_alpha=mbr_alpha)
    return squares, hw, sel, status, index


def _read(model, sel, status, index):
    """the one host read: tokens, lengths, scores, raw scores, steps (and the JPEG decoder's status words)"""
    B = sel["tokens"].shape[0]
    parts = [sel["tokens"].reshape(-1).double(), sel["lengths"].double(), sel["steps"].double(), sel["scores"].double(), sel["raw"].double()]
    if status is not None:
        parts.append(status.double())
    flat = torch.cat(parts).cpu()               # int32 and fp32 are exact in float64
    W = sel["tokens"].shape[1]
    tokens = flat[:B * W].reshape(B, W).to(torch.int64)
    lengths, steps, scores, raw = (flat[B * W + i * B: B * W + (i + 1) * B] for i in range(4))
    _raise_bad_jpeg(flat[B * W + 4 * B:].to(torch.int64).tolist() if status is not None else None, index)
    lengths = lengths.to(torch.int64).tolist()
    captions = [tokens[b, :lengths[b]].tolist() for b in range(B)]
    # model.py:415 on the host, as SAT.caption computes it: exp(-score / step) in fp32
    ppl = torch.exp(-raw.float() / steps.float()).tolist()
    return captions, [model.decode_seq(c) for c in captions], scores.float().tolist(), ppl, lengths


def visualize(model, items, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None, rescore_method=None,
              rescore_reward=1.0, visual_size=256, input_size=None, power=5.0, opacity=0.75, seed=None, progressive=False,
              topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
              mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None):
    """``make_visual`` without the figure, for a batch: returns a ``Visual``.  ``input_size`` None: the model's ``input_size``.  The winning
    caption is the one ``SAT.caption(..., return_all=True)`` lists first (the highest rescored value; among hypotheses with the very same
    value this picks the first to finish).  Everything stays on the device until one read of tokens and scores.
    ``topg`` / ``prefix`` (e.g. ``"a photo of"``) / ``banned`` / ``no_unk`` constrain the search, ``no_repeat_ngram`` / ``min_length`` /
    ``repetition_penalty`` are its history rules (``SATDecoder.beam_decode_batched``); ``rescore_method="MBR"`` with ``mbr_corpus`` /
    ``mbr_reward`` / ``mbr_alpha`` picks the caption by consensus (the score shown is its utility); ``beam_groups`` / ``diversity_penalty``: the
    diverse beam search ("Diverse beam search"); ``required`` (e.g. ``"dog frisbee"``): the words every caption must contain
    ("Required words")."""
    squares, hw, sel, status, index = _search(model, items, constraints.SearchOptions.from_kwargs(locals()), beamk, max_gen_length, temperature, rescore_method,
                                              rescore_reward, visual_size, input_size, with_alpha=True, progressive=progressive, mbr_corpus=mbr_corpus,
                                              mbr_reward=mbr_reward, mbr_alpha=mbr_alpha)
    panels = attention_panels(squares, sel["alphas"], sel["lengths"], hw, power, opacity)
    captions, words, scores, ppl, lengths = _read(model, sel, status, index)
    return Visual(captions, words, scores, ppl, lengths, panels, _names(items))


def caption_image(model, items, beamk=3, max_gen_length=32, temperature=1.0, sample_method="beam", sample_topk=3, decoder_noise=None,
                  rescore_method=None, rescore_reward=1.0, visual_size=256, input_size=None, seed=None, progressive=False,
                  topg=None, prefix=None, banned=None, no_unk=False, sample_topp=0.9, no_repeat_ngram=None, min_length=None, repetition_penalty=None,
                  mbr_corpus=None, mbr_reward=(1.0, 0.0), mbr_alpha=0.0, beam_groups=None, diversity_penalty=0.5, required=None):
    """``caption(prepare_image(load_square(path, visual_size), input_size))`` for a batch, without panels:
    ``(captions, words, scores, perplexities)``, one entry per picture.  ``topg`` / ``prefix`` / ``banned`` / ``no_unk``: as ``visualize``."""
    _, _, sel, status, index = _search(model, items, constraints.SearchOptions.from_kwargs(locals()), beamk, max_gen_length, temperature, rescore_method, rescore_reward,
                                       visual_size, input_size, with_alpha=False, progressive=progressive, mbr_corpus=mbr_corpus, mbr_reward=mbr_reward,
                                       mbr_alpha=mbr_alpha)
    captions, words, scores, ppl, _ = _read(model, sel, status, index)
    return captions, words, scores, ppl


# ---------------------------------------------------------------------------------------------------------------- the figure
def sheet_grid(caption_length, columns=4):
    """make_visual's grid: ``(panel count, columns, rows)``.  2 + len panels; a caption shorter than ``columns`` gets one row of them;
    rows = 1 + panels // columns (so a full last row is followed by an empty one, as in the notebook)."""
    num_figs = 2 + int(caption_length)
    if caption_length < columns:
        columns = num_figs
    return num_figs, columns, 1 + num_figs // columns


def contact_sheet(visual, index, references=None, columns=4, label_height=14, pad=4):
    """The notebook's figure for picture ``index`` of a ``Visual`` as a PIL image (host side, Pillow's default font): a title block (name,
    ``references`` = the ground-truth captions as strings, the prediction with score and perplexity), then the grid of ``sheet_grid``:
    the picture labelled ``<START>``, one overlay per word labelled with the word, "Total Attention" last."""
    from PIL import Image, ImageDraw
    n = int(visual.lengths[index])
    num_figs, columns, rows = sheet_grid(n, columns)
    panels = visual.panels[index, :num_figs]
    panels = panels.cpu().numpy() if torch.is_tensor(panels) else np.asarray(panels)
    V = panels.shape[1]
    labels = ["<START>"] + [str(w) for w in visual.words[index][:n]] + ["Total Attention"]
    title = []
    if visual.names[index]:
        title.append(str(visual.names[index]))
    for i, r in enumerate(references or []):
        title.append("Caption %d : %s" % (i, r))
    title.append("Prediction 0 (s=%.2f, p=%.2f) : %s" % (visual.scores[index], visual.perplexities[index], " ".join(visual.words[index])))
    title_h = pad + len(title) * label_height
    cell_w, cell_h = V + pad, V + label_height + pad
    sheet = Image.new("RGB", (pad + columns * cell_w, title_h + rows * cell_h), (255, 255, 255))
    draw = ImageDraw.Draw(sheet)
    for i, line in enumerate(title):
        draw.text((pad, pad + i * label_height), line, fill=(0, 0, 0))
    for i in range(num_figs):
        x, y = pad + (i % columns) * cell_w, title_h + (i // columns) * cell_h
        sheet.paste(Image.fromarray(np.ascontiguousarray(panels[i])), (x, y))
        draw.text((x, y + V + 1), labels[i], fill=(0, 0, 0))
    sheet.info.update(panels=num_figs, columns=columns, rows=rows)
    return sheet
