"""What distillation costs ("Distillation"), at BASELINE configs[1] (resnet50, V = 6400, 128 images x 5 captions x 21 steps =
13440 packed rows) with M = 1, 2, 4 teachers (synthetic weights, pictures and captions).  Device events, warm-up first, profiler off.
  1. The loss kernels on (P, V) logits, forward + backward, in both forms: "fused" (sat_distill_fwd writes the gradient, sat_distill_bwd
     scales it in place) and "split" (sat_distill_bwd produces it from the row scratch); the bytes every form has to move at least
     (each of the M + 1 logit matrices read once, the gradient written once) over the time, against the HBM peak.
  2. The same loss and gradient composed from torch ops on the same tensors (log_softmax, the mixture or product, kl_div, cross_entropy,
     autograd): the yardstick.  Alternating rounds with 1; the two results are compared first.
  3. ``SAT.distill_step`` + backward next to ``SAT.training_step`` + backward on the same batch (no optimizer step in either), and one
     more distillation step split into the teachers' passes and the student's pass.
    python tools/bench_distill.py [--members 1 2 4] [--step-members 1 2 4] [--combine arithmetic] [--alpha 0.5] [--temperature 2.0]
                                  [--repeats 10] [--launches 5] [--step-repeats 5] [--no-step] [--json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sat_amd  # noqa: E402,F401
from sat_amd import _lib as L  # noqa: E402
from sat_amd import distill  # noqa: E402
from sat_amd import model as M  # noqa: E402
from sat_amd.ensemble import Ensemble  # noqa: E402

HBM_PEAK_GBS = bench.PEAK_HBM_GBS            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (a float4 copy measures 6.29 TB/s)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def torch_pair(z, ts, w, combine, y, tau, alpha, smoothing):
    """the loss and its gradient from torch ops: what a user without the kernel would write"""
    z = z.detach().requires_grad_()
    ls = [torch.log_softmax(t / tau, -1) for t in ts]
    if combine == "geometric":
        q = torch.softmax(sum(wi * l for wi, l in zip(w, ls)), -1)
    else:
        q = sum(wi * l.exp() for wi, l in zip(w, ls))
    hard = F.cross_entropy(z, y, label_smoothing=smoothing)
    soft = F.kl_div(torch.log_softmax(z / tau, -1), q, reduction="batchmean")
    loss = (1.0 - alpha) * hard + alpha * tau * tau * soft
    loss.backward()
    return loss.detach(), z.grad


def kernel_bench(a, P, V, m):
    g = torch.Generator().manual_seed(3 + m)
    z = (torch.randn(P, V, generator=g) * 3.0).cuda()
    ts = [(torch.randn(P, V, generator=g) * 3.0).cuda() for _ in range(m)]
    y32 = torch.randint(0, V, (P,), generator=g).to(torch.int32).cuda()
    y64 = y32.long()
    w = [1.0 / m] * m
    tau, alpha, smoothing = a.temperature, a.alpha, 0.1
    f32 = dict(dtype=torch.float32, device="cuda")
    lse, tlse, cnorm, rows = torch.empty(P, 2, **f32), torch.empty(P, m, **f32), torch.empty(P, **f32), torch.empty(P, 2, **f32)
    correct, out, dl = torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(4, **f32), torch.empty(P, V, **f32)
    one = torch.ones(1, **f32)
    tarr = (C.c_void_p * m)(*[t.data_ptr() for t in ts])
    warr = (C.c_float * m)(*w)
    cmb = L.ENSEMBLE_COMBINE[a.combine]
    lib = L.lib()

    def pair(fused):
        L.check(lib.sat_distill_fwd(L.ptr(z), tarr, warr, m, cmb, L.ptr(y32), P, V, 1.0 / tau, alpha, smoothing, L.ptr(lse), L.ptr(tlse), L.ptr(cnorm),
                                    L.ptr(rows), L.ptr(correct), L.ptr(out), L.ptr(dl) if fused else None, L.stream_ptr()), "sat_distill_fwd")
        L.check(lib.sat_distill_bwd(L.ptr(z), tarr, warr, m, cmb, L.ptr(y32), P, V, 1.0 / tau, alpha, smoothing, L.ptr(lse), L.ptr(tlse), L.ptr(cnorm),
                                    L.ptr(one), int(fused), L.ptr(dl), L.stream_ptr()), "sat_distill_bwd")

    # the two sides compute the same thing
    pair(True)
    loss_t, grad_t = torch_pair(z, ts, w, a.combine, y64, tau, alpha, smoothing)
    torch.cuda.synchronize()
    agree = dict(loss_kernel=float(out[0]), loss_torch=float(loss_t), grad_max_abs_diff=float((dl - grad_t).abs().max()), grad_max_abs=float(grad_t.abs().max()))
    del grad_t
    for _ in range(2):                                           # warm-up of all three
        pair(True); pair(False); torch_pair(z, ts, w, a.combine, y64, tau, alpha, smoothing)
    torch.cuda.synchronize()
    ms = {"fused": [], "split": [], "torch": []}
    for _ in range(a.repeats):                                   # alternating rounds
        ms["fused"].append(event_ms(lambda: [pair(True) for _ in range(a.launches)])[0] / a.launches)
        ms["split"].append(event_ms(lambda: [pair(False) for _ in range(a.launches)])[0] / a.launches)
        ms["torch"].append(event_ms(lambda: [torch_pair(z, ts, w, a.combine, y64, tau, alpha, smoothing) for _ in range(a.launches)])[0] / a.launches)
    least_bytes = (m + 2) * P * V * 4                            # M teachers and the student read once, the gradient written once
    res = dict(members=m, P=P, V=V, least_bytes=least_bytes, agree=agree, **{k + "_ms": spread(v) for k, v in ms.items()})
    for k in ("fused", "split"):
        gbs = least_bytes / (res[k + "_ms"]["median"] * 1e-3) / 1e9
        res[k + "_least_bytes_gbs"], res[k + "_share_of_hbm_peak"] = gbs, gbs / HBM_PEAK_GBS
    return res


def step_bench(a, m):
    hp, T, B, R = bench.hparams("c2")
    torch.manual_seed(42)
    student = M.SAT(**hp).cuda().train()
    student.set_precision(a.precision)
    student.__dict__["_sat_global_step"] = 2                     # past encoder_finetune_after: the encoder trains, as in bench.py's headline
    teachers = []
    for i in range(m):
        torch.manual_seed(100 + i)
        t = M.SAT(**hp).cuda().eval()
        t.set_precision(a.precision)
        teachers.append(t)
    teacher = Ensemble(teachers, None, a.combine)
    img, caps, lengths = bench.synthetic_batch(B, R, T, hp["vocab_size"], 1234, ragged=False, px=hp["input_size"])
    batch = (img.cuda(), caps.cuda(), lengths)

    def distill_step():
        student.zero_grad(set_to_none=True)
        student.distill_step(batch, teacher, alpha=a.alpha, temperature=a.temperature)["loss"].backward()

    def xe_step():
        student.zero_grad(set_to_none=True)
        student.training_step(batch, 0)["loss"].backward()

    for _ in range(2):
        distill_step(); xe_step()
    torch.cuda.synchronize()
    ms = {"distill": [], "xe": []}
    for _ in range(a.step_repeats):                              # alternating rounds
        ms["distill"].append(event_ms(distill_step)[0])
        ms["xe"].append(event_ms(xe_step)[0])
    student.zero_grad(set_to_none=True)
    t_ms, tl = event_ms(lambda: distill.teacher_logits(teacher, batch[0], batch[1], batch[2]))

    def student_pass():
        ann, _ = student.encode(batch[0])
        distill.loss(student, ann, batch[1], batch[2], tl, teacher.weights, teacher.combine, a.alpha, a.temperature).backward()
    s_ms, _ = event_ms(student_pass)
    return dict(members=m, images=B, captions=B * R, packed_rows=int(lengths.sum()), precision=a.precision, distill_step_ms=spread(ms["distill"]),
                training_step_ms=spread(ms["xe"]), teacher_passes_ms=t_ms, student_pass_ms=s_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 2, 4], help="teachers of the kernel measurement (1 and 2)")
    ap.add_argument("--step-members", type=int, nargs="+", default=None, help="teachers of the whole-step measurement (3); default: --members")
    ap.add_argument("--combine", default="arithmetic", choices=list(L.ENSEMBLE_COMBINE))
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--rows", type=int, default=640 * 21)
    ap.add_argument("--vocab", type=int, default=6400)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-step", action="store_true", help="the kernels and the torch composition only")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distill.py measures on the GPU; there is no CPU path")
    res = dict(combine=a.combine, alpha=a.alpha, temperature=a.temperature, repeats=a.repeats, launches=a.launches, kernels=[], steps=[])
    for m in a.members:
        res["kernels"].append(kernel_bench(a, a.rows, a.vocab, m))
        torch.cuda.empty_cache()
    if not a.no_step:
        for m in a.step_members or a.members:
            res["steps"].append(step_bench(a, m))
            torch.cuda.empty_cache()
    if a.json:
        print(json.dumps(res))
        return
    print("distillation loss, forward + backward, %s, alpha %g, tau %g, smoothing 0.1; median (min - max) of %d rounds of %d" %
          (a.combine, a.alpha, a.temperature, a.repeats, a.launches))
    for k in res["kernels"]:
        print("  M = %d, P = %d, V = %d: loss %.6f (torch %.6f), max |gradient difference| %.2e of %.2e" % (
            k["members"], k["P"], k["V"], k["agree"]["loss_kernel"], k["agree"]["loss_torch"], k["agree"]["grad_max_abs_diff"], k["agree"]["grad_max_abs"]))
        for name in ("fused", "split"):
            r = k[name + "_ms"]
            print("    %-28s %8.3f ms (%.3f - %.3f)  %.0f GB/s of the %.2f GB it must move = %.0f%% of the %.0f GB/s HBM peak" % (
                "kernels, " + name, r["median"], r["min"], r["max"], k[name + "_least_bytes_gbs"], k["least_bytes"] / 1e9,
                100 * k[name + "_share_of_hbm_peak"], HBM_PEAK_GBS))
        r = k["torch_ms"]
        print("    %-28s %8.3f ms (%.3f - %.3f)  = %.1fx the fused kernels" % ("torch ops + autograd", r["median"], r["min"], r["max"],
                                                                              r["median"] / k["fused_ms"]["median"]))
    for s in res["steps"]:
        d, x = s["distill_step_ms"], s["training_step_ms"]
        print("  M = %d, %d images x %d captions (%d packed rows), %s: distill_step %.2f ms (%.2f - %.2f), training_step %.2f ms (%.2f - %.2f); "
              "teachers' passes %.2f ms, student's pass %.2f ms" % (s["members"], s["images"], s["captions"] // s["images"], s["packed_rows"], s["precision"],
                                                                    d["median"], d["min"], d["max"], x["median"], x["min"], x["max"], s["teacher_passes_ms"],
                                                                    s["student_pass_ms"]))


if __name__ == "__main__":
    main()
