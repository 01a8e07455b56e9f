"""Input pipeline: one C2-sized batch of decoded pictures (128 x 480x640 RGB bytes) -> (128, 3, 224, 224)
fp32 through sat_image_batch_transform, against Pillow doing the same crop + BILINEAR resize (+ numpy ToTensor) on the host.
With --color-jitter X the same batch also goes through T.ColorJitter(X, X, X, 0.03) (sat_image_batch_transform_jitter), and
both rates are reported from the same run.  With --optical S the same batch (with the ColorJitter draws too when
--color-jitter is given) also goes through the reference's RandomChoice of RandomPerspective / RandomAffine / RandomRotation
at strength S (sat_image_batch_transform_warp).
With --jpeg the batch arrives as JPEG files instead (Pillow-encoded 480x640, quality 90, 4:2:0, restart-free and again with
a restart marker per MCU row; or the first --batch files of --jpeg-dir): GPU decoding alone (sat_jpeg_decode_batch, bytes
resident), decoding + the transform with and without the H2D copy, and Pillow's decode_rgb on one host thread.
--subseq-bytes / --parallel-min-bytes set the options of sat_jpeg_decode_batch_ex (default: the library's); the paths the
pictures took and the mean number of synchronisation rounds are reported.
    python tools/bench_input_pipeline.py [--batch 128] [--size 224] [--color-jitter 0.4] [--optical 0.5]
    python tools/bench_input_pipeline.py --jpeg [--jpeg-dir DIR] [--subseq-bytes 128] [--parallel-min-bytes 2048]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import _lib as L  # noqa: E402
from sat_amd import data as D  # noqa: E402


def time_ms(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(tf, staged, noise, iters):
    """(with the H2D copy, kernels only) in ms per batch"""
    dev = torch.device("cuda")
    B, S = staged.n, tf.size
    with_copy_ms = time_ms(lambda: tf.run(staged, dev, noise=noise), iters)       # H2D copy of 118 MB + the kernels
    lib = L.lib()
    resident = staged.host.to(dev)                                               # kernels only: pixels already resident
    desc, jit, warp = C.cast(staged.desc, C.c_void_p), staged.jitter, staged.warp
    if warp is not None:
        need = lib.sat_image_batch_warp_workspace_bytes(desc, C.cast(jit, C.c_void_p) if jit is not None else None, C.cast(warp, C.c_void_p), B, S, S)
    elif jit is None:
        need = lib.sat_image_batch_workspace_bytes(desc, B, S, S)
    else:
        need = lib.sat_image_batch_jitter_workspace_bytes(desc, C.cast(jit, C.c_void_p), B, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, S, S, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernels():
        if warp is not None:
            jit_ptrs = (C.cast(jit, C.c_void_p), resident.data_ptr() + staged.jitter_off) if jit is not None else (None, None)
            L.check(lib.sat_image_batch_transform_warp(resident.data_ptr() + staged.head, staged.pixels_bytes, desc, resident.data_ptr(), *jit_ptrs,
                                                       C.cast(warp, C.c_void_p), resident.data_ptr() + staged.warp_off, B, S, S, L.ptr(noise),
                                                       0.01, L.ptr(out), None, L.ptr(ws), need, st), "transform_warp")
        elif jit is None:
            L.check(lib.sat_image_batch_transform(resident.data_ptr() + staged.head, staged.pixels_bytes, desc, resident.data_ptr(),
                                                  B, S, S, L.ptr(noise), 0.01, L.ptr(out), None, L.ptr(ws), need, st), "transform")
        else:
            L.check(lib.sat_image_batch_transform_jitter(resident.data_ptr() + staged.head, staged.pixels_bytes, desc, resident.data_ptr(),
                                                         C.cast(jit, C.c_void_p), resident.data_ptr() + staged.jitter_off, B, S, S, L.ptr(noise),
                                                         0.01, L.ptr(out), None, L.ptr(ws), need, st), "transform_jitter")
    return with_copy_ms, time_ms(kernels, iters)


def jpeg_rates(tf, files, iters, label, pool_threads=0):
    """decode alone / decode + transform with and without the H2D copy, images/s; Pillow per host thread, and with ``pool_threads``
    also Pillow on that many threads at once (what a loader's workers make of files the GPU does not take)"""
    from sat_amd import jpeg as J
    dev = torch.device("cuda")
    B = len(files)
    torch.manual_seed(0)
    staged = tf.stage(files)
    assert staged.jpeg is not None, "no GPU-decodable file"
    S = tf.size
    noise = torch.randn(B, 3, S, S, device=dev)
    with_copy_ms = time_ms(lambda: tf.run(staged, dev, noise=noise), iters)
    lib, jb = L.lib(), staged.jpeg
    resident = torch.empty(staged.device_bytes, dtype=torch.uint8, device=dev)
    resident[:staged.host.numel()].copy_(staged.host)
    status = torch.empty(jb.n, dtype=torch.int32, device=dev)
    info = torch.empty(jb.n, 4, dtype=torch.int32, device=dev)
    sb, pm = tf.jpeg_subseq_bytes, tf.jpeg_parallel_min_bytes
    jws = torch.empty(jb.workspace_bytes(sb, pm), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()
    base = resident.data_ptr()

    def decode():
        jb.launch(base + staged.jpeg_off, base + staged.head, staged.pixels_bytes, status, jws, stream, sb, pm, info)
    desc = C.cast(staged.desc, C.c_void_p)
    need = lib.sat_image_batch_workspace_bytes(desc, B, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, S, S, device=dev)

    def decode_transform():
        decode()
        L.check(lib.sat_image_batch_transform(base + staged.head, staged.pixels_bytes, desc, base, B, S, S, L.ptr(noise), 0.01, L.ptr(out), None,
                                              L.ptr(ws), need, C.c_void_p(stream.cuda_stream)), "transform")
    dec_ms = time_ms(decode, iters)
    assert not status.any().item(), "decode status %s" % status.tolist()
    dt_ms = time_ms(decode_transform, iters)
    n_cpu = min(B, 32)
    t0 = time.perf_counter()
    for f in files[:n_cpu]:
        J.pillow_decode(f)
    cpu_s = (time.perf_counter() - t0) / n_cpu
    pool = {}
    if pool_threads:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(pool_threads) as ex:
            list(ex.map(J.pillow_decode, files))                       # warm-up
            rates = []
            for _ in range(5):
                t0 = time.perf_counter()
                list(ex.map(J.pillow_decode, files))
                rates.append(B / (time.perf_counter() - t0))
        pool = {label + "pillow_decode_%dthreads_images_per_s" % pool_threads: dict(median=round(sorted(rates)[2], 1), min=round(min(rates), 1),
                                                                                    max=round(max(rates), 1))}
    mb = sum(len(f) for f in files) / 1e6
    inf = info.cpu()
    par = inf[:, 0] == 1
    paths = {label + "paths_serial_parallel_abandoned": [int((inf[:, 0] == k).sum()) for k in (0, 1, 2)],
             label + "mean_subsequences": round(float(inf[par, 1].float().mean()), 1) if par.any() else 0.0,
             label + "mean_sync_iterations": round(float(inf[par, 2].float().mean()), 2) if par.any() else 0.0}
    return {label + "decode_ms": round(dec_ms, 3), label + "decode_images_per_s": round(B / dec_ms * 1e3, 1),
            label + "decode_transform_ms": round(dt_ms, 3), label + "decode_transform_images_per_s": round(B / dt_ms * 1e3, 1),
            label + "decode_transform_with_h2d_ms": round(with_copy_ms, 3), label + "decode_transform_with_h2d_images_per_s": round(B / with_copy_ms * 1e3, 1),
            label + "compressed_MB": round(mb, 2), label + "h2d_bytes": int(staged.host.numel()), label + "segments": int(sum(jb.desc[j].n_segments for j in range(B))),
            label + "pillow_decode_1thread_images_per_s": round(1.0 / cpu_s, 1), **pool, **paths}


def main_jpeg(a):
    import io
    from PIL import Image
    B, S = a.batch, a.size
    tf = D.BatchTransform(S, train=True, aug_scale=0.9, aug_hflip=0.5, aug_noise_std=0.01, jpeg_subseq_bytes=a.subseq_bytes,
                          jpeg_parallel_min_bytes=a.parallel_min_bytes)
    res = {"metric": "input_pipeline_jpeg_images_per_s", "batch": B, "out": S, "subseq_bytes": a.subseq_bytes or "default",
           "parallel_min_bytes": "default" if a.parallel_min_bytes is None else a.parallel_min_bytes}
    if a.jpeg_dir:
        names = sorted(n for n in os.listdir(a.jpeg_dir) if n.lower().endswith((".jpg", ".jpeg")))[:B]
        files = []
        for n in names:
            with open(os.path.join(a.jpeg_dir, n), "rb") as f:
                files.append(f.read())
        from sat_amd import jpeg as J
        gpu = [f for f in files if isinstance(J.as_picture(f), J.JpegBytes)]
        res.update({"jpeg_dir_files": len(files), "jpeg_dir_gpu_decodable": len(gpu)})
        res.update(jpeg_rates(tf, gpu, a.iters, "dir_"))
    else:
        H, W = 480, 640
        rng = np.random.default_rng(0)
        y, x = np.mgrid[0:H, 0:W]
        base = []
        for k in range(8):
            ramp = np.stack([x * 255.0 / W, y * 255.0 / H, 128 + 100 * np.sin((x + (k + 1) * y) / (9.0 + k))], -1)
            base.append(np.clip(np.rint(ramp + rng.normal(0, 10, (H, W, 3))), 0, 255).astype(np.uint8))

        def enc(im, **kw):
            buf = io.BytesIO()
            Image.fromarray(im).save(buf, "JPEG", quality=90, subsampling=2, **kw)
            return buf.getvalue()
        res["source"] = "%dx%d q90 4:2:0" % (H, W)
        if a.progressive:                                     # the same pictures as progressive files, decoded on the GPU on request
            from sat_amd import jpeg as J
            res["source"] += " progressive"
            for label, kw in (("progressive_", {}), ("progressive_rst_rows1_", dict(restart_marker_rows=1))):
                files = [J.as_picture(enc(base[i % 8], progressive=True, **kw), progressive=True) for i in range(B)]
                assert all(isinstance(f, J.JpegBytes) and f.header.progressive for f in files)
                res.update(jpeg_rates(tf, files, a.iters, label, pool_threads=16))
            print(json.dumps(res))
            return
        res.update(jpeg_rates(tf, [enc(base[i % 8]) for i in range(B)], a.iters, ""))
        res.update(jpeg_rates(tf, [enc(base[i % 8], restart_marker_rows=1) for i in range(B)], a.iters, "rst_rows1_"))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--color-jitter", type=float, default=0.0, help="also time T.ColorJitter(X, X, X, 0.03) on the same batch")
    ap.add_argument("--optical", type=float, default=0.0, help="also time the optical augmentation of strength S on the same batch")
    ap.add_argument("--jpeg", action="store_true", help="time GPU JPEG decoding (+ the transform) of a batch of JPEG files instead")
    ap.add_argument("--jpeg-dir", default=None, help="with --jpeg: the first --batch *.jpg files of this directory instead of synthetic ones")
    ap.add_argument("--subseq-bytes", type=int, default=None, help="with --jpeg: bytes per subsequence of a restart-free picture (default: the library's)")
    ap.add_argument("--parallel-min-bytes", type=int, default=None,
                    help="with --jpeg: least data bytes of a restart-free picture decoded by subsequences (default: the library's; 0 all; 2^63-1 none)")
    ap.add_argument("--progressive", action="store_true",
                    help="with --jpeg: encode the synthetic pictures progressively and decode them on the GPU (as_picture(progressive=True)); also "
                         "times Pillow on 16 threads, which is what decodes such files without the option")
    a = ap.parse_args()
    if a.jpeg or a.jpeg_dir or a.progressive:
        return main_jpeg(a)
    H, W, S, B = 480, 640, a.size, a.batch
    rng = np.random.default_rng(0)
    base = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    imgs = [base[i % 8] for i in range(B)]
    tf = D.BatchTransform(S, train=True, aug_scale=0.9, aug_hflip=0.5, aug_noise_std=0.01)
    torch.manual_seed(0)
    descs = tf.draw([(H, W)] * B)
    dev = torch.device("cuda")
    t0 = time.perf_counter()
    staged = tf.stage(imgs, descs)
    stage_s = time.perf_counter() - t0
    noise = torch.randn(B, 3, S, S, device=dev)
    with_copy_ms, kern_ms = measure(tf, staged, noise, a.iters)
    src_bytes = sum(d["crop_h"] * d["crop_w"] * 3 for d in descs)
    alg_bytes = src_bytes + 2 * 4 * sum(d["crop_h"] for d in descs) * S + 2 * B * 3 * S * S * 4     # box read, RGBX intermediate w+r, noise read + fp32 write
    res = {"metric": "input_pipeline_images_per_s", "batch": B, "source": "%dx%d u8" % (H, W), "out": S,
           "kernels_ms": round(kern_ms, 4), "kernels_images_per_s": round(B / kern_ms * 1e3, 1),
           "algorithmic_GBps": round(alg_bytes / kern_ms / 1e6, 1),
           "with_h2d_ms": round(with_copy_ms, 3), "with_h2d_images_per_s": round(B / with_copy_ms * 1e3, 1),
           "h2d_bytes": int(staged.host.numel()), "host_stage_ms": round(stage_s * 1e3, 2)}
    jdescs = None
    if a.color_jitter:
        x = a.color_jitter
        tfj = D.BatchTransform(S, train=True, aug_scale=0.9, aug_hflip=0.5, aug_noise_std=0.01, aug_color_jitter=x)
        if not tfj.jitter:
            raise SystemExit("--color-jitter %g: the reference applies no jitter for this value (0 < x <= 1)" % x)
        torch.manual_seed(1)
        jdescs = [dict(d, **D.color_jitter_params(x)) for d in descs]                # same crops, jitter draws added
        jw_ms, jk_ms = measure(tfj, tfj.stage(imgs, jdescs), noise, a.iters)
        # the same two timings of the plain batch again, after the jitter runs (drift between the two halves of the run)
        w2_ms, k2_ms = measure(tf, staged, noise, a.iters)
        res.update({"color_jitter": x, "jitter_kernels_ms": round(jk_ms, 4), "jitter_kernels_images_per_s": round(B / jk_ms * 1e3, 1),
                    "jitter_with_h2d_ms": round(jw_ms, 3), "jitter_with_h2d_images_per_s": round(B / jw_ms * 1e3, 1),
                    "plain_again_kernels_ms": round(k2_ms, 4), "plain_again_with_h2d_ms": round(w2_ms, 3)})
    if a.optical:
        o = a.optical
        tfo = D.BatchTransform(S, train=True, aug_scale=0.9, aug_hflip=0.5, aug_noise_std=0.01, aug_color_jitter=a.color_jitter, aug_optical_strength=o)
        if not tfo.optical:
            raise SystemExit("--optical %g: the reference applies no optical augmentation for this value (0 < s <= 1)" % o)
        random.seed(2)
        torch.manual_seed(2)
        odescs = [dict(d, **D.optical_params(o, S)) for d in (jdescs or descs)]          # same crops (and jitter), warp draws added
        ow_ms, ok_ms = measure(tfo, tfo.stage(imgs, odescs), noise, a.iters)
        w3_ms, k3_ms = measure(tf, staged, noise, a.iters)
        res.update({"optical": o, "optical_with_jitter": bool(jdescs), "optical_kinds": [sum(d["warp_kind"] == k for d in odescs) for k in (0, 1)],
                    "optical_kernels_ms": round(ok_ms, 4), "optical_kernels_images_per_s": round(B / ok_ms * 1e3, 1),
                    "optical_with_h2d_ms": round(ow_ms, 3), "optical_with_h2d_images_per_s": round(B / ow_ms * 1e3, 1),
                    "plain_after_optical_kernels_ms": round(k3_ms, 4), "plain_after_optical_with_h2d_ms": round(w3_ms, 3)})
    # host: Pillow on one thread, a sample of the same batch
    from PIL import Image
    n_cpu = min(B, 32)
    t0 = time.perf_counter()
    for im, d in zip(imgs[:n_cpu], descs[:n_cpu]):
        p = Image.fromarray(im).crop((d["crop_left"], d["crop_top"], d["crop_left"] + d["crop_w"], d["crop_top"] + d["crop_h"])).resize((S, S), Image.BILINEAR)
        if d["flip"]:
            p = p.transpose(Image.FLIP_LEFT_RIGHT)
        x = torch.from_numpy(np.asarray(p).copy()).permute(2, 0, 1).float().div(255)
        x = x + torch.randn(x.size()) * 0.01
    cpu_s = (time.perf_counter() - t0) / n_cpu
    res.update({"pillow_1thread_images_per_s": round(1.0 / cpu_s, 1), "pillow_sample": n_cpu})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
