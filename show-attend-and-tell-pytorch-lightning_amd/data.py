"""Input pipeline with the per-picture transforms on the GPU.

Host-side mirror of the reference's data path:

* ``CocoCaptionDataset``   util.py:16-45 - same JSON (``vocab_stoi``, ``<split>.img_paths / encoded_captions / lengths``,
  preprocess.ipynb cell 17); ``__getitem__`` returns the *decoded bytes* (H, W, 3) uint8 instead of a transformed tensor.
* ``BucketSampler``        util.py:48-87 - same grouping and shuffle; additionally rank/world_size aware.
* ``BatchTransform``       train.py:208-233 - RandomResizedCrop | Resize+CenterCrop, RandomHorizontalFlip, ToTensor,
  ColorJitter (train.py:223-224), the "optical" RandomChoice of RandomPerspective / RandomAffine / RandomRotation
  (train.py:225-231), AddGaussianNoise (util.py:121-130) for a whole batch in three kernel launches, four with ColorJitter,
  one more with the optical augmentation (``sat_image_batch_transform[_jitter|_warp]``): the pictures are resampled,
  jittered and warped with Pillow's arithmetic bit for bit, the random draws are made on the host in the reference's order
  (crop parameters, then the flip coin, then ColorJitter's permutation and factors, then the optical choice and its
  parameters, per picture).
* ``DeviceLoader``         train.py:244-259 DataLoader(pin_memory=True): decode threads -> one pinned staging buffer per
  batch -> one H2D copy on a side stream -> transform; batches arrive as ``(img, caps, lengths)`` on the device.
* JPEG decoding on the GPU (``sat_amd.jpeg``): with ``CocoCaptionDataset(decode=jpeg.read_jpeg)`` the worker threads only read
  the files, the staging buffer carries the compressed bytes, and ``sat_jpeg_decode_batch`` decodes them in front of the
  transform, bit exact with ``decode_rgb``.  Files the GPU decoder does not take are decoded by Pillow on the worker threads.

There is no CPU path: the transform needs libsat_hip.so and a GPU.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import queue
import random
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib as L
from . import jpeg as J


def json_loader(path):
    """util.py:132-133"""
    with open(path) as f:
        return json.load(f)


def decode_rgb(path):
    """util.py:136-137 pil_loader, returned as an (H, W, 3) uint8 array."""
    from PIL import Image
    with open(path, "rb") as f:
        return np.asarray(Image.open(f).convert("RGB"))


class CocoCaptionDataset:
    """util.py:16-45.  ``root`` is prepended to relative ``img_paths``."""

    def __init__(self, jsonpath, split="train", root=None, decode=decode_rgb):
        self.json = json_loader(jsonpath) if isinstance(jsonpath, (str, os.PathLike)) else jsonpath
        self.split = split
        self.vocab_stoi = self.json["vocab_stoi"]
        self.vocab_itos = {v: k for k, v in self.vocab_stoi.items()}
        self.img_paths = self.json[split]["img_paths"]
        self.encoded_captions = self.json[split]["encoded_captions"]
        self.lengths = self.json[split]["lengths"]
        assert len(self.img_paths) == len(self.encoded_captions) == len(self.lengths)
        self.root, self.decode = root, decode

    def stoi(self, s):
        return int(self.vocab_stoi.get(s, self.vocab_stoi["<UNK>"]))

    def itos(self, i):
        return str(self.vocab_itos.get(int(i), "<UNK>"))

    def __len__(self):
        return len(self.img_paths)

    def __getitem__(self, idx):
        path = self.img_paths[idx]
        if self.root is not None and not os.path.isabs(path):
            path = os.path.join(self.root, path)
        return self.decode(path), torch.LongTensor(self.encoded_captions[idx]), torch.LongTensor(self.lengths[idx])


class BucketSampler:
    """util.py:48-87: indices grouped by the sample's total target count (sum of its caption lengths), groups in
    decreasing count, each group shuffled in place with ``np.random.shuffle`` at every ``__iter__``.

    ``world_size > 1``: every rank builds the same order (``seed`` + epoch drive a private RandomState instead of the
    global numpy generator), pads it to a multiple of ``batch_size * world_size`` by wrapping, and yields, of every run of
    ``batch_size * world_size`` indices, the ``batch_size`` that belong to ``rank``: the ranks' batches hold neighbouring
    lengths, and every rank sees the same number of batches."""

    def __init__(self, lengths, batch_size, indices=None, rank=0, world_size=1, seed=None):
        self.lengths, self.batch_size = lengths, batch_size
        self.indices = indices if indices else list(range(len(lengths)))
        assert 0 <= rank < world_size
        self.rank, self.world_size, self.seed, self.epoch = rank, world_size, seed, 0
        if world_size > 1 and seed is None:
            self.seed = 0
        len_map = OrderedDict()
        for i, length_list in zip(self.indices, self.lengths):
            len_map.setdefault(sum(length_list), []).append(i)
        self.grouped_indices = [idxs for _, idxs in reversed(sorted(len_map.items()))]

    def set_epoch(self, epoch):
        self.epoch = epoch

    def global_order(self):
        rs = np.random if self.seed is None else np.random.RandomState(self.seed + self.epoch)
        order = []
        for idxs in self.grouped_indices:
            if self.seed is not None:
                idxs = list(idxs)          # a seeded epoch does not depend on the epochs before it
            rs.shuffle(idxs)
            order.extend(idxs)
        return order

    def __iter__(self):
        order = self.global_order()
        if self.world_size == 1:
            return iter(order)
        run = self.batch_size * self.world_size
        padded = int(math.ceil(len(order) / run)) * run
        order = (order * (padded // len(order) + 1))[:padded]
        mine = []
        for start in range(0, padded, run):
            mine.extend(order[start + self.rank * self.batch_size: start + (self.rank + 1) * self.batch_size])
        return iter(mine)

    def __len__(self):
        if self.world_size == 1:
            return len(self.lengths)
        run = self.batch_size * self.world_size
        return int(math.ceil(len(self.lengths) / run)) * self.batch_size


# ----------------------------------------------------------------------------------------------------------------------
def resize_rule(h, w, size):
    """T.Resize(int): the smaller edge becomes ``size`` (torchvision 0.10 F.resize)."""
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def random_resized_crop_params(h, w, scale, ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """T.RandomResizedCrop.get_params (torchvision 0.10), drawing from the global torch CPU generator."""
    area = h * w
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        cw = int(round(math.sqrt(target_area * aspect)))
        ch = int(round(math.sqrt(target_area / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            i = torch.randint(0, h - ch + 1, size=(1,)).item()
            j = torch.randint(0, w - cw + 1, size=(1,)).item()
            return i, j, ch, cw
    in_ratio = float(w) / float(h)
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return (h - ch) // 2, (w - cw) // 2, ch, cw


def color_jitter_params(x, hue=0.03):
    """T.ColorJitter(brightness=x, contrast=x, saturation=x, hue=hue).get_params, drawing from the global torch CPU
    generator, as the fields of a picture's jitter record: the order of the adjustments (0 brightness, 1 contrast,
    2 saturation, 3 hue), the three blend factors and the hue byte shift F_pil.adjust_hue adds (hue * 255 truncated)."""
    fn_idx = torch.randperm(4)
    lo = max(0.0, 1.0 - x)
    b = float(torch.empty(1).uniform_(lo, 1.0 + x))
    c = float(torch.empty(1).uniform_(lo, 1.0 + x))
    s = float(torch.empty(1).uniform_(lo, 1.0 + x))
    h = float(torch.empty(1).uniform_(-hue, hue))
    return dict(jitter_order=tuple(fn_idx.tolist()), brightness=b, contrast=c, saturation=s, hue_shift=int(h * 255))


def perspective_params(width, height, distortion_scale):
    """T.RandomPerspective.get_params (torchvision 0.10), drawing from the global torch CPU generator: the picture's corners
    (start points) and the drawn end points, topleft, topright, botright, botleft."""
    hw, hh = width // 2, height // 2

    def randint(lo, hi):
        return int(torch.randint(lo, hi, size=(1,)).item())

    topleft = [randint(0, int(distortion_scale * hw) + 1), randint(0, int(distortion_scale * hh) + 1)]
    topright = [randint(width - int(distortion_scale * hw) - 1, width), randint(0, int(distortion_scale * hh) + 1)]
    botright = [randint(width - int(distortion_scale * hw) - 1, width), randint(height - int(distortion_scale * hh) - 1, height)]
    botleft = [randint(0, int(distortion_scale * hw) + 1), randint(height - int(distortion_scale * hh) - 1, height)]
    start = [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]]
    return start, [topleft, topright, botright, botleft]


def perspective_coeffs(startpoints, endpoints):
    """torchvision 0.10 F._get_perspective_coeffs: the 8 coefficients of the map from the end points (output) onto the
    start points (input), Pillow's PERSPECTIVE data; a float32 least-squares solve on the CPU."""
    a = torch.zeros(2 * len(startpoints), 8, dtype=torch.float)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b = torch.tensor(startpoints, dtype=torch.float).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.tolist()


def inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision 0.10 F._get_inverse_affine_matrix: Pillow's AFFINE data (output -> input) of rotation, shear, scale and
    translation about ``center``."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [x / scale for x in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rotate_matrix(angle, width, height):
    """Pillow's Image.rotate(angle) AFFINE data about the picture's centre (no expand, no translate)."""
    cx, cy = width / 2.0, height / 2.0
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def optical_params(s, size):
    """train.py:225-231 on a size x size PIL picture, as the fields of its warp record (sat_image_warp): T.RandomChoice picks
    with Python's ``random.choice``, then the chosen transform draws from the global torch CPU generator.
      RandomPerspective(0.5 * s, p=1): torch.rand(1) for the coin, 8 randint draws; perspective map, BILINEAR (kind 1)
      RandomAffine(45 * s, shear=45 * s): angle, then shear_x, uniform in [-45 s, 45 s]; affine map, NEAREST (kind 0)
      RandomRotation(45 * s): angle uniform in [-45 s, 45 s]; Image.rotate's own matrix, NEAREST (kind 0)"""
    k = random.choice((0, 1, 2))
    deg = [-45.0 * s, 45.0 * s]
    if k == 0:
        torch.rand(1)                                                    # RandomPerspective.forward: torch.rand(1) < p
        start, end = perspective_params(size, size, 0.5 * s)
        return dict(warp_kind=1, warp_coeffs=tuple(perspective_coeffs(start, end)))
    angle = float(torch.empty(1).uniform_(deg[0], deg[1]).item())
    if k == 1:
        shear_x = float(torch.empty(1).uniform_(deg[0], deg[1]).item())
        m = inverse_affine_matrix([size * 0.5, size * 0.5], angle, [0, 0], 1.0, [shear_x, 0.0])
    else:
        m = rotate_matrix(angle, size, size)
    return dict(warp_kind=0, warp_coeffs=tuple(m) + (0.0, 0.0))


def box_desc(h, w, box, size, flip=False):
    """descriptor fields of: crop ``box`` = (top, left, height, width) -> resize to size x size (-> flip)"""
    t, l, ch, cw = box
    return dict(height=h, width=w, crop_top=t, crop_left=l, crop_h=ch, crop_w=cw, resized_h=size, resized_w=size, out_top=0, out_left=0, flip=int(flip))


def center_desc(h, w, size):
    """descriptor fields of T.Resize(size) -> T.CenterCrop(size)"""
    rh, rw = resize_rule(h, w, size)
    return dict(height=h, width=w, crop_top=0, crop_left=0, crop_h=h, crop_w=w, resized_h=rh, resized_w=rw,
                out_top=int(round((rh - size) / 2.0)), out_left=int(round((rw - size) / 2.0)), flip=0)


#: descriptor-dict keys of the ColorJitter record of a picture (sat_image_jitter); the other keys are sat_image_desc fields
JITTER_KEYS = ("jitter_order", "brightness", "contrast", "saturation", "hue_shift")
#: descriptor-dict keys of the warp record of a picture (sat_image_warp): the kind (0 affine NEAREST, 1 perspective BILINEAR)
#: and the 8 coefficients of Pillow's inverse map (an affine map uses the first 6)
WARP_KEYS = ("warp_kind", "warp_coeffs")


class StagedBatch:
    """The pictures of one batch in one pinned host buffer: [descriptors | jitter records | warp records | pixels].
    The jitter records are there when the descriptor dicts carry ``JITTER_KEYS``, the warp records when they carry
    ``WARP_KEYS`` (in each case all of them or none).
    A picture is an (H, W, 3) uint8 array or the bytes of a JPEG file (``jpeg.JpegBytes``, or plain bytes, parsed here; a
    file the GPU decoder does not take is decoded by Pillow here).  With JPEG pictures the buffer is
    [descriptors | jitter | warp | JPEG region (jpeg.JpegBatch) | pixels of the array pictures]; the device buffer has room
    behind those pixels for the GPU-decoded ones, which ``run`` writes there before the transform reads them (``device_bytes``
    in all; ``head`` is where the pixels start, in both buffers).  ``jpeg_index[j]``: the picture of the j-th JPEG record."""

    def __init__(self, images, descs):
        images = [J.as_picture(im) for im in images]
        n = len(images)
        self.n = n
        self.desc = (L.ImageDesc * n)()
        has = {sum(k in d for k in JITTER_KEYS) for d in descs}
        if len(has) > 1 or has - {0, len(JITTER_KEYS)}:
            raise ValueError("ColorJitter fields (%s) must be given for every picture of a batch or for none" % ", ".join(JITTER_KEYS))
        self.jitter = (L.ImageJitter * n)() if has == {len(JITTER_KEYS)} else None
        has = {sum(k in d for k in WARP_KEYS) for d in descs}
        if len(has) > 1 or has - {0, len(WARP_KEYS)}:
            raise ValueError("warp fields (%s) must be given for every picture of a batch or for none" % ", ".join(WARP_KEYS))
        self.warp = (L.ImageWarp * n)() if has == {len(WARP_KEYS)} else None
        self.jitter_off = (C.sizeof(L.ImageDesc) * n + 15) // 16 * 16
        self.warp_off = (self.jitter_off + (C.sizeof(L.ImageJitter) * n if self.jitter is not None else 0) + 7) // 8 * 8
        head = self.warp_off + (C.sizeof(L.ImageWarp) * n if self.warp is not None else 0)
        head = (head + 255) // 256 * 256
        self.jpeg_index = [i for i, im in enumerate(images) if isinstance(im, J.JpegBytes)]
        arrays_bytes = sum(int(im.shape[0]) * int(im.shape[1]) * 3 for im in images if not isinstance(im, J.JpegBytes))
        self.jpeg, self.jpeg_off = None, head
        if self.jpeg_index:
            self.jpeg = J.JpegBatch([images[i] for i in self.jpeg_index], out_base=arrays_bytes)
            self.jpeg_index = [self.jpeg_index[k] for k in self.jpeg.order]        # record order: baseline files, then progressive ones
            head = (head + self.jpeg.nbytes + 255) // 256 * 256
        total = head + arrays_bytes
        self.device_bytes = total + (self.jpeg.out_bytes if self.jpeg is not None else 0)
        self.host = torch.empty(total, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else torch.empty(total, dtype=torch.uint8)
        buf = self.host.numpy()
        if self.jpeg is not None:
            self.jpeg.write(buf[self.jpeg_off:self.jpeg_off + self.jpeg.nbytes])
        jpeg_out = dict(zip(self.jpeg_index, self.jpeg.out_offsets)) if self.jpeg is not None else {}
        off = 0
        for i, (im, d) in enumerate(zip(images, descs)):
            e = self.desc[i]
            if i in jpeg_out:
                e.offset = jpeg_out[i]
            else:
                if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                    raise ValueError("picture %d: expected (H, W, 3) uint8, got %s %s" % (i, im.shape, im.dtype))
                nb = im.shape[0] * im.shape[1] * 3
                buf[head + off: head + off + nb] = im.reshape(-1)
                e.offset = off
                off += nb
            for k, v in d.items():
                if k not in JITTER_KEYS and k not in WARP_KEYS:
                    setattr(e, k, int(v))
            if self.jitter is not None:
                j = self.jitter[i]
                j.order[:] = [int(o) for o in d["jitter_order"]]
                j.brightness, j.contrast, j.saturation = float(d["brightness"]), float(d["contrast"]), float(d["saturation"])
                j.hue_shift = int(d["hue_shift"])
            if self.warp is not None:
                wr = self.warp[i]
                coeffs = [float(c) for c in d["warp_coeffs"]]
                if len(coeffs) not in (6, 8):
                    raise ValueError("picture %d: %d warp coefficients, expected 6 (affine) or 8 (perspective)" % (i, len(coeffs)))
                wr.kind = int(d["warp_kind"])
                wr.coeffs[:] = coeffs + [0.0] * (8 - len(coeffs))
        buf[:C.sizeof(L.ImageDesc) * n] = np.frombuffer(self.desc, dtype=np.uint8)
        if self.jitter is not None:
            buf[self.jitter_off:self.jitter_off + C.sizeof(L.ImageJitter) * n] = np.frombuffer(self.jitter, dtype=np.uint8)
        if self.warp is not None:
            buf[self.warp_off:self.warp_off + C.sizeof(L.ImageWarp) * n] = np.frombuffer(self.warp, dtype=np.uint8)
        self.head, self.pixels_bytes = head, self.device_bytes - head
        self.status = None          # run(): (number of JPEG records,) int32 device status words of the GPU decoder


class BatchTransform:
    """train.py:208-233 for a batch.  ``train=False``: Resize + CenterCrop + ToTensor (valid_transforms).
    ``train=True``: aug_scale == 1 -> Resize + CenterCrop, else RandomResizedCrop(scale=(aug_scale, 1)); a flip with
    probability aug_hflip when 0 < aug_hflip < 1; T.ColorJitter(x, x, x, hue=0.03) when aug_color_jitter = x is not 0 and
    at most 1 (a larger x is ignored, as the reference does; a negative one raises, as torchvision does);
    T.RandomChoice([RandomPerspective(0.5 s, p=1), RandomAffine(45 s, shear=45 s), RandomRotation(45 s)]) when
    aug_optical_strength = s is not 0 and at most 1 (the same rules; a negative s raises, as RandomAffine does); ToTensor;
    + N(0,1) * aug_noise_std.
    ``randn(shape, device)`` supplies the noise draws (default: ``torch.randn`` on the device).
    ``jpeg_subseq_bytes`` / ``jpeg_parallel_min_bytes``: the options of the GPU JPEG decoder for pictures that arrive as JPEG
    bytes (``jpeg.decode_jpeg_batch``; None: the library's defaults)."""

    def __init__(self, input_size, train=True, aug_scale=0.9, aug_hflip=0.5, aug_noise_std=0.01, randn=None, aug_color_jitter=0.0,
                 aug_optical_strength=0.0, jpeg_subseq_bytes=None, jpeg_parallel_min_bytes=None):
        if train and not (0 <= aug_scale <= 1.0):
            raise ValueError("Invalid value for aug_scale. Choose in the range {0,1}.")       # train.py:219-220
        x = float(aug_color_jitter)
        self.jitter = train and x != 0 and x <= 1.0                                           # train.py:223
        if self.jitter and x < 0:
            raise ValueError("If brightness is a single number, it must be non negative.")   # T.ColorJitter._check_input
        o = float(aug_optical_strength)
        self.optical = train and o != 0 and o <= 1.0                                          # train.py:225
        if self.optical and o < 0:
            raise ValueError("If degrees is a single number, it must be positive.")          # T.RandomAffine's _setup_angle
        self.size, self.train = int(input_size), train
        self.aug_scale, self.aug_hflip, self.noise_std, self.randn = aug_scale, aug_hflip, aug_noise_std, randn
        self.aug_color_jitter, self.aug_optical_strength = x, o
        self.jpeg_subseq_bytes, self.jpeg_parallel_min_bytes = jpeg_subseq_bytes, jpeg_parallel_min_bytes     # None: the library's defaults
        self._ws = self._jws = None

    def draw(self, shapes):
        """one descriptor per picture; consumes the torch CPU generator (and, for the optical choice, Python's ``random``)
        in the reference's per-sample order"""
        out = []
        for h, w in shapes:
            if not self.train or self.aug_scale == 1.0:
                d = center_desc(h, w, self.size)
            else:
                d = box_desc(h, w, random_resized_crop_params(h, w, (self.aug_scale, 1.0)), self.size)
            if self.train and 0 < self.aug_hflip < 1.0:
                d["flip"] = int(torch.rand(1).item() < self.aug_hflip)            # T.RandomHorizontalFlip.forward
            if self.jitter:
                d.update(color_jitter_params(self.aug_color_jitter))
            if self.optical:
                d.update(optical_params(self.aug_optical_strength, self.size))
            out.append(d)
        return out

    def stage(self, images, descs=None):
        """``images``: (H, W, 3) uint8 arrays and / or JPEG bytes; a JPEG picture's shape comes from its header, so the draws
        are the same whichever form a picture arrives in"""
        images = [J.as_picture(im) for im in images]
        return StagedBatch(images, descs if descs is not None else self.draw([im.shape[:2] for im in images]))

    def run(self, staged, device, stream=None, noise=None, want_bytes=False):
        """H2D copy of the staged batch + the kernels, on ``stream`` (default: current).  Returns the (n, 3, S, S) fp32
        batch (and the (n, S, S, 3) bytes PIL would hold when ``want_bytes``)."""
        lib = L.lib()
        device = torch.device(device)
        if device.type != "cuda":
            raise L.SatHipError("sat_amd computes on the GPU only: the batch transform got device %s (no CPU fallback)" % device)
        stream = stream if stream is not None else torch.cuda.current_stream(device)
        S, n = self.size, staged.n
        with torch.cuda.stream(stream):
            if staged.jpeg is None:
                dev = staged.host.to(device, non_blocking=True)
            else:                                   # room behind the copied bytes for the pictures the GPU decodes
                dev = torch.empty(staged.device_bytes, dtype=torch.uint8, device=device)
                dev[:staged.host.numel()].copy_(staged.host, non_blocking=True)
                jb = staged.jpeg
                need = jb.workspace_bytes(self.jpeg_subseq_bytes, self.jpeg_parallel_min_bytes)
                if self._jws is None or self._jws.numel() < need or self._jws.device != dev.device:
                    self._jws = torch.empty(need, dtype=torch.uint8, device=device)
                staged.status = torch.empty(jb.n, dtype=torch.int32, device=device)
                jb.launch(dev.data_ptr() + staged.jpeg_off, dev.data_ptr() + staged.head, staged.pixels_bytes, staged.status, self._jws, stream,
                          self.jpeg_subseq_bytes, self.jpeg_parallel_min_bytes)
            jit, warp = staged.jitter, staged.warp
            if warp is not None:
                need = lib.sat_image_batch_warp_workspace_bytes(C.cast(staged.desc, C.c_void_p), C.cast(jit, C.c_void_p) if jit is not None else None,
                                                                C.cast(warp, C.c_void_p), n, S, S)
            elif jit is None:
                need = lib.sat_image_batch_workspace_bytes(C.cast(staged.desc, C.c_void_p), n, S, S)
            else:
                need = lib.sat_image_batch_jitter_workspace_bytes(C.cast(staged.desc, C.c_void_p), C.cast(jit, C.c_void_p), n, S, S)
            if need == 0:
                L.check(1, "sat_image_batch_workspace_bytes")
            if self._ws is None or self._ws.numel() < need or self._ws.device != dev.device:
                self._ws = torch.empty(need, dtype=torch.uint8, device=device)
            out = torch.empty(n, 3, S, S, dtype=torch.float32, device=device)
            raw = torch.empty(n, S, S, 3, dtype=torch.uint8, device=device) if want_bytes else None
            if noise is None and self.train and self.noise_std:
                noise = (self.randn or (lambda shape, device: torch.randn(shape, device=device)))((n, 3, S, S), device)
            if noise is not None:
                L.require_gpu(noise)
                assert noise.shape == out.shape and noise.dtype == torch.float32 and noise.is_contiguous()
            tail = (n, S, S, L.ptr(noise) if noise is not None else None, float(self.noise_std if noise is not None else 0.0), L.ptr(out),
                    L.ptr(raw) if raw is not None else None, L.ptr(self._ws), self._ws.numel(), C.c_void_p(stream.cuda_stream))
            if warp is not None:
                jit_ptrs = (C.cast(jit, C.c_void_p), dev.data_ptr() + staged.jitter_off) if jit is not None else (None, None)
                L.check(lib.sat_image_batch_transform_warp(dev.data_ptr() + staged.head, staged.pixels_bytes, C.cast(staged.desc, C.c_void_p),
                                                           dev.data_ptr(), *jit_ptrs, C.cast(warp, C.c_void_p), dev.data_ptr() + staged.warp_off, *tail),
                        "sat_image_batch_transform_warp")
            elif jit is None:
                L.check(lib.sat_image_batch_transform(dev.data_ptr() + staged.head, staged.pixels_bytes, C.cast(staged.desc, C.c_void_p), dev.data_ptr(),
                                                      *tail), "sat_image_batch_transform")
            else:
                L.check(lib.sat_image_batch_transform_jitter(dev.data_ptr() + staged.head, staged.pixels_bytes, C.cast(staged.desc, C.c_void_p),
                                                             dev.data_ptr(), C.cast(jit, C.c_void_p), dev.data_ptr() + staged.jitter_off, *tail),
                        "sat_image_batch_transform_jitter")
            dev.record_stream(stream)
        return (out, raw) if want_bytes else out

    def __call__(self, images, device="cuda", descs=None, noise=None):
        return self.run(self.stage(images, descs), torch.device(device), noise=noise)


class DeviceLoader:
    """train.py:244-259: ``DataLoader(dataset, sampler=BucketSampler | shuffle, batch_size, num_workers, pin_memory=True)``
    with the transform moved behind the H2D copy.  Decoding runs in ``workers`` threads (PIL releases the GIL), staging and
    the copy + kernels of batch i+1 overlap the consumer's work on batch i (side stream, ``prefetch`` batches in flight).
    With a dataset whose ``decode`` is ``jpeg.read_jpeg`` the GPU decodes the pictures; the producer thread reads their status
    words after its side stream is done, and a bad stream raises ``jpeg.JpegDecodeError`` (naming the dataset index) on the
    consumer side, in place of the batch that held it."""

    def __init__(self, dataset, batch_size, transform, sampler=None, shuffle=False, workers=4, prefetch=2, device="cuda", drop_last=False):
        self.ds, self.batch_size, self.tf, self.sampler, self.shuffle = dataset, batch_size, transform, sampler, shuffle
        self.workers, self.prefetch, self.device, self.drop_last = max(1, workers), max(1, prefetch), torch.device(device), drop_last

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.ds)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def _index_batches(self):
        if self.sampler is not None:
            order = list(iter(self.sampler))
        elif self.shuffle:
            order = torch.randperm(len(self.ds)).tolist()
        else:
            order = list(range(len(self.ds)))
        for s in range(0, len(order), self.batch_size):
            b = order[s:s + self.batch_size]
            if len(b) == self.batch_size or not self.drop_last:
                yield b

    def __iter__(self):
        L.lib()
        side = torch.cuda.Stream(self.device)
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def produce():
            try:
                with ThreadPoolExecutor(self.workers) as pool:
                    for idxs in self._index_batches():
                        if stop.is_set():
                            return
                        samples = list(pool.map(self.ds.__getitem__, idxs))
                        staged = self.tf.stage([s[0] for s in samples])
                        caps = torch.stack([s[1] for s in samples])
                        lens = torch.stack([s[2] for s in samples])
                        img = self.tf.run(staged, self.device, stream=side)
                        with torch.cuda.stream(side):
                            caps_d = caps.pin_memory().to(self.device, non_blocking=True)
                            lens_d = lens.pin_memory().to(self.device, non_blocking=True)
                            if staged.status is not None:
                                status = torch.empty(staged.status.numel(), dtype=torch.int32).pin_memory()
                                status.copy_(staged.status, non_blocking=True)
                            done = torch.cuda.Event()
                            done.record(side)
                        if staged.status is not None:
                            done.synchronize()          # this thread waits for its own side stream; the consumer's stream does not
                            bad = [(idxs[staged.jpeg_index[j]], int(c)) for j, c in enumerate(status.tolist()) if c]
                            if bad:
                                q.put(J.JpegDecodeError("corrupt JPEG data: " + "; ".join("dataset index %d: %s" % (i, J.status_text(c))
                                                                                         for i, c in bad)))
                                return
                        q.put((img, caps_d, lens_d, done, staged))
                q.put(None)
            except BaseException as e:          # surfaces in the consumer
                q.put(e)

        th = threading.Thread(target=produce, daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                img, caps, lens, done, _staged = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(done)
                for t in (img, caps, lens):
                    t.record_stream(cur)
                yield img, caps, lens
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get(timeout=0.05)
                except queue.Empty:
                    pass
