"""What the activation regularisers cost ("Activation regularisation"), at BASELINE configs[1]'s decoder shape: N = 640
captions, T1 = 21 steps, n = 512, ragged lengths (bench.synthetic_batch(..., ragged=True), U{8..21}).  Device events, warm-up first,
profiler off.
  1. sat_activation_reg_fwd (partial + finish) and sat_activation_reg_bwd on (T1, N, n) states, each against the same arithmetic from
     torch ops on the device (masked squares and differences, autograd for the gradient); alternating rounds, results compared first.
  2. The bytes each must move at least over its time, against the HBM peak: forward the live rows once; backward the live rows once and
     dH's live rows read and written (the neighbouring rows come from the cache or cost up to two more reads).
  3. ``SAT.training_step`` + backward with ``ar_alpha=2, tar_beta=1`` next to the same model with both at 0, same process, alternating.
    python tools/bench_activation_reg.py [--repeats 10] [--launches 20] [--step-repeats 8] [--no-step] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sat_amd  # noqa: E402,F401
from sat_amd import _lib as L  # noqa: E402
from sat_amd import model as M  # noqa: E402

HBM_PEAK_GBS = bench.PEAK_HBM_GBS


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def torch_terms(h, live, P, Q):
    """(ar, tar) from torch ops: h (T1, N, n), live (T1, N, 1) as 0 / 1 floats; rows that are not live hold zeros here"""
    n = h.shape[-1]
    ar = (h * h * live).sum() / (P * n)
    d = (h[1:] - h[:-1]) * live[1:]
    tar = (d * d).sum() / (Q * n)
    return ar, tar


def kernel_bench(a):
    hp, T, B, R = bench.hparams("c2")
    _, _, lengths = bench.synthetic_batch(B, R, T, hp["vocab_size"], 1234, True, px=8)
    N, T1, n = B * R, T - 1, hp["decoder_dim"]
    lens = lengths.reshape(-1)
    P, Q = int(lens.sum()), int((lens - 1).clamp_min(0).sum())
    g = torch.Generator().manual_seed(5)
    live = (torch.arange(T1).unsqueeze(1) < lens.unsqueeze(0)).unsqueeze(-1)
    h = ((torch.rand(T1, N, n, generator=g) * 2 - 1) * live).cuda()
    live_f = live.float().cuda()
    lens32 = lens.to(torch.int32).cuda()
    lib = L.lib()
    scratch = torch.empty(lib.sat_activation_reg_scratch_bytes(N, T1, n), dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    gscale = torch.tensor([2.0, 1.0], device="cuda")
    dH = torch.zeros(T1, N, n, device="cuda")

    def fwd():
        L.check(lib.sat_activation_reg_fwd(L.ptr(h), L.ptr(lens32), N, T1, n, P, Q, L.ptr(scratch), L.ptr(out), L.stream_ptr()), "sat_activation_reg_fwd")

    def bwd():
        L.check(lib.sat_activation_reg_bwd(L.ptr(h), L.ptr(lens32), N, T1, n, P, Q, L.ptr(gscale), L.ptr(dH), L.stream_ptr()), "sat_activation_reg_bwd")

    def torch_fwd():
        with torch.no_grad():
            return torch_terms(h, live_f, P, Q)

    def torch_bwd():
        ha = h.detach().requires_grad_()
        ar, tar = torch_terms(ha, live_f, P, Q)
        (2.0 * ar + 1.0 * tar).backward()
        return ha.grad

    fwd(); bwd()
    ar_t, tar_t = torch_fwd(); grad_t = torch_bwd()
    torch.cuda.synchronize()
    agree = dict(ar_kernel=float(out[0]), ar_torch=float(ar_t), tar_kernel=float(out[1]), tar_torch=float(tar_t),
                 grad_max_abs_diff=float((dH - grad_t).abs().max()), grad_max_abs=float(grad_t.abs().max()))
    del grad_t
    for _ in range(3):
        fwd(); bwd(); torch_fwd(); torch_bwd()
    torch.cuda.synchronize()
    ms = {"fwd": [], "bwd": [], "torch_fwd": [], "torch_bwd": []}
    for _ in range(a.repeats):                                   # alternating rounds
        for k, fn in (("fwd", fwd), ("bwd", bwd), ("torch_fwd", torch_fwd), ("torch_bwd", torch_bwd)):
            ms[k].append(event_ms(lambda: [fn() for _ in range(a.launches)])[0] / a.launches)
    row = n * 4
    least = dict(fwd=P * row, bwd=3 * P * row)                   # the live rows once | the live rows once, dH's live rows read and written
    res = dict(N=N, T1=T1, n=n, P=P, Q=Q, agree=agree, least_bytes=least, **{k + "_ms": spread(v) for k, v in ms.items()})
    for k in ("fwd", "bwd"):
        gbs = least[k] / (res[k + "_ms"]["median"] * 1e-3) / 1e9
        res[k + "_least_bytes_gbs"], res[k + "_share_of_hbm_peak"] = gbs, gbs / HBM_PEAK_GBS
    return res


def step_bench(a):
    hp, T, B, R = bench.hparams("c2")
    models = {}
    for name, over in (("off", {}), ("on", dict(ar_alpha=2.0, tar_beta=1.0))):
        torch.manual_seed(42)
        m = M.SAT(**dict(hp, **over)).cuda().train()
        m.set_precision(a.precision)
        m.__dict__["_sat_global_step"] = 2                       # past encoder_finetune_after: the encoder trains, as in bench.py's headline
        models[name] = m
    img, caps, lengths = bench.synthetic_batch(B, R, T, hp["vocab_size"], 1234, True, px=hp["input_size"])
    batch = (img.cuda(), caps.cuda(), lengths)

    def step(m):
        m.zero_grad(set_to_none=True)
        out = m.training_step(batch, 0)
        out["loss"].backward()
        return out

    for _ in range(3):
        for m in models.values():
            step(m)
    torch.cuda.synchronize()
    ms = {"off": [], "on": []}
    for _ in range(a.step_repeats):                              # alternating rounds
        for name, m in models.items():
            ms[name].append(event_ms(lambda: step(m))[0])
    out = step(models["on"])
    return dict(images=B, captions=B * R, packed_rows=int(lengths.sum()), precision=a.precision, ar=float(out["ar"]), tar=float(out["tar"]),
                step_off_ms=spread(ms["off"]), step_on_ms=spread(ms["on"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-step", action="store_true", help="the kernels and the torch composition only")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_activation_reg.py measures on the GPU; there is no CPU path")
    res = dict(repeats=a.repeats, launches=a.launches, kernels=kernel_bench(a))
    torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_bench(a)
    if a.json:
        print(json.dumps(res))
        return
    k = res["kernels"]
    print("activation regularisers at N = %d, T1 = %d, n = %d (P = %d live rows, Q = %d pairs); median (min - max) of %d rounds of %d" %
          (k["N"], k["T1"], k["n"], k["P"], k["Q"], a.repeats, a.launches))
    ag = k["agree"]
    print("  ar %.8f (torch %.8f), tar %.8f (torch %.8f), max |gradient difference| %.2e of %.2e" %
          (ag["ar_kernel"], ag["ar_torch"], ag["tar_kernel"], ag["tar_torch"], ag["grad_max_abs_diff"], ag["grad_max_abs"]))
    for name, label in (("fwd", "forward pair"), ("bwd", "backward")):
        r, t = k[name + "_ms"], k["torch_" + name + "_ms"]
        print("  %-14s %7.1f us (%.1f - %.1f)  %.0f GB/s of the %.1f MB it must move = %.0f%% of the %.0f GB/s HBM peak;  torch ops %7.1f us (%.1f - %.1f) = %.1fx" % (
            label, 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"], k[name + "_least_bytes_gbs"], k["least_bytes"][name] / 1e6,
            100 * k[name + "_share_of_hbm_peak"], HBM_PEAK_GBS, 1e3 * t["median"], 1e3 * t["min"], 1e3 * t["max"], t["median"] / r["median"]))
    if "step" in res:
        s = res["step"]
        off, on = s["step_off_ms"], s["step_on_ms"]
        print("  training_step + backward, %d images x %d captions (%d packed rows), %s: off %.3f ms (%.3f - %.3f), on %.3f ms (%.3f - %.3f); ar %.6f tar %.6f" % (
            s["images"], s["captions"] // s["images"], s["packed_rows"], s["precision"], off["median"], off["min"], off["max"], on["median"], on["min"],
            on["max"], s["ar"], s["tar"]))


if __name__ == "__main__":
    main()
