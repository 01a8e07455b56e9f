"""visualize.ipynb's make_visual at batch size: 128 JPEG files of 480 x 640 (synthetic pictures, restart-free as cameras write them),
beam 3, max_gen_length 32, visual size 256, on the BASELINE configs[4] model (resnet50 encoder, synthetic weights).  The same files go,
in the same process and in alternating rounds, through
  (a) the notebook's loop: per picture Pillow decodes, ``load_square`` and ``prepare_image`` run in Pillow, ``SAT.caption`` searches a batch
      of one on the GPU, and numpy + Pillow build the panels (``Image.blend`` as the overlay), and
  (b) ``SAT.visualize``: decode, squares, search, selection and panels on the device, one host read per batch.
Wall clock around synchronised calls after a warm-up of each; median (min - max) of --repeats, reported as pictures per second.
    python tools/bench_visualize.py [--images 128] [--beamk 3] [--repeats 5] [--precision bf16] [--host-images 16] [--json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sat_amd  # noqa: E402,F401
from sat_amd import model as M  # noqa: E402


def synthetic_jpeg(seed, h=480, w=640, **kw):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([xx * 255.0 / (w - 1), yy * 255.0 / (h - 1), ((xx + yy) % 128) * 2.0], -1) + rs.randint(-24, 25, (h, w, 3))
    buf = io.BytesIO()
    Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90, **kw)
    return buf.getvalue()


def host_visual(model, data, kw, visual_size, input_size, power=5.0, opacity=0.75):
    """make_visual's arithmetic for one file, the overlay as Image.blend"""
    img = Image.open(io.BytesIO(data)).convert("RGB")
    s = min(img.size)
    sq = img.crop(((img.width - s) // 2, (img.height - s) // 2, (img.width + s) // 2, (img.height + s) // 2)).resize((visual_size, visual_size))
    ten = torch.from_numpy(np.asarray(sq.resize((input_size, input_size))).transpose(2, 0, 1).astype(np.float32) / np.float32(255)).unsqueeze(0)
    captions, scores, alphas, ppl = model.caption(ten.cuda(), return_all=True, **kw)
    atts = alphas[0][0].numpy()
    panels = [np.asarray(sq)]
    for att in list(atts) + [atts.sum(0)]:
        last = len(panels) == 1 + len(atts)
        x = (att - att.min()) / (att.max() - att.min())
        mask = Image.fromarray(np.uint8((x if last else x ** power) * 255)).convert("RGB").resize((visual_size, visual_size))
        panels.append(np.asarray(mask if last else Image.blend(sq, mask, opacity)))
    return captions[0][0], panels


def clock_s(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--host-images", type=int, default=16, help="pictures per round of the host loop (its rate does not depend on the count)")
    ap.add_argument("--beamk", type=int, default=3)
    ap.add_argument("--max-gen-length", type=int, default=32)
    ap.add_argument("--visual-size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--progressive", action="store_true", help="progressive files, decoded on the GPU (visualize(progressive=True))")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visualize.py measures on the GPU; there is no CPU path")
    hp, _, _, _ = bench.hparams("c2")
    torch.manual_seed(42)
    model = M.SAT(**hp).cuda().eval()
    model.set_precision(a.precision)
    files = [synthetic_jpeg(i, progressive=a.progressive) for i in range(a.images)]
    kw = dict(beamk=a.beamk, max_gen_length=a.max_gen_length, temperature=1.0, rescore_method="LN", rescore_reward=1.0)
    size = int(hp["input_size"])

    def path_a():
        return [host_visual(model, f, kw, a.visual_size, size) for f in files[:a.host_images]]

    def path_b():
        return model.visualize(files, visual_size=a.visual_size, input_size=size, progressive=a.progressive, **kw)

    ra, rb = path_a(), path_b()                          # warm-up; and the two paths' captions side by side
    same = sum(ra[i][0] == rb.captions[i] for i in range(len(ra)))
    rate = {"a": [], "b": []}
    for _ in range(a.repeats):                           # alternating rounds
        rate["a"].append(len(files[:a.host_images]) / clock_s(path_a)[0])
        rate["b"].append(len(files) / clock_s(path_b)[0])
    med = {k: statistics.median(v) for k, v in rate.items()}
    res = dict(images=a.images, host_images=a.host_images, beamk=a.beamk, max_gen_length=a.max_gen_length, visual_size=a.visual_size, input_size=size,
               precision=a.precision, repeats=a.repeats, progressive=a.progressive, mean_caption_length=sum(rb.lengths) / len(rb.lengths),
               host_loop_images_per_s=dict(median=med["a"], min=min(rate["a"]), max=max(rate["a"])),
               visualize_images_per_s=dict(median=med["b"], min=min(rate["b"]), max=max(rate["b"])), ratio=med["b"] / med["a"],
               captions_equal="%d of %d" % (same, len(ra)))
    if a.json:
        print(json.dumps(res))
    else:
        print("%d JPEG files of 480 x 640, beam %d, max_gen_length %d, visual size %d, input %d, %s; mean caption length %.1f" %
              (a.images, a.beamk, a.max_gen_length, a.visual_size, size, a.precision, res["mean_caption_length"]))
        print("  (a) host loop (%d pictures a round)  %9.1f pictures/s (min %.1f, max %.1f)" % (a.host_images, med["a"], min(rate["a"]), max(rate["a"])))
        print("  (b) SAT.visualize                   %9.1f pictures/s (min %.1f, max %.1f)   (b) / (a) = %.1fx" %
              (med["b"], min(rate["b"]), max(rate["b"]), res["ratio"]))
        print("  winning captions equal on %s pictures of the host round" % res["captions_equal"])


if __name__ == "__main__":
    main()
