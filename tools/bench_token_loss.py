"""What the token losses cost ("Token losses"), at BASELINE configs[1]'s loss shape: P = 13440 packed rows (640 captions of
21 steps), V = 6400, T = 22.  Device events, warm-up first, profiler off, alternating rounds in one process.
  1. The forward + backward pair sat_token_loss_fwd + _bwd for "ce+fl" (gamma 2), for the unlikelihood on top of the cross entropy
     ("ul", alpha 1) and for both, against two baselines: the pair sat_ce_label_smooth_fwd + _bwd (the yardstick: the same bytes but for
     P (T - 1) ids and gathers) and the same loss and gradient from torch ops (log_softmax, a (P, V) scatter mask for the candidates,
     autograd).  The captions are random words of the vocabulary, so nearly every context id is a candidate of its own: the most
     candidates a row can have.  Results are compared before anything is timed.
  2. ``SAT.training_step`` + backward with ``token_loss="ce+fl", ul_alpha=1`` next to the same model with the defaults.
    python tools/bench_token_loss.py [--repeats 10] [--launches 20] [--step-repeats 8] [--no-step] [--json]
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
from sat_amd import decoder as Dk  # noqa: E402
from sat_amd import model as M  # noqa: E402

FORMS = {"ce+fl": (1.0, 1.0, 2.0, 0.0), "ul": (1.0, 0.0, 2.0, 1.0), "ce+fl+ul": (1.0, 1.0, 2.0, 1.0)}      # ce_weight, focal_weight, gamma, ul_alpha
SMOOTHING = 0.1
CLAMP = 1e-5


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def candidate_mask(caps, src_row, targets, V, pad):
    """(P, V) 0 / 1 floats from torch ops: what the kernels never build"""
    N, T = caps.shape
    P = src_row.numel()
    t, i = src_row.long() // N, src_row.long() % N
    ctx = caps.long()[i, 1:]                                         # (P, T - 1): context id k of the row's caption
    live = (torch.arange(T - 1, device=caps.device).unsqueeze(0) < t.unsqueeze(1)) & (ctx != pad) & (ctx != targets.long().unsqueeze(1))
    mask = torch.zeros(P, V, device=caps.device)
    mask.scatter_(1, ctx, live.float())                              # a 1 wherever some live context id points (duplicates write the same 1 ...)
    dead = torch.zeros(P, V, device=caps.device).scatter_(1, ctx, (~live).float())
    return torch.where((dead > 0) & (mask == 0), torch.zeros_like(mask), mask), live      # ... and a masked id that is also live elsewhere stays


def torch_loss(z, y, mask, form):
    cw, fw, gamma, ua = form
    logp = torch.log_softmax(z, dim=-1)
    nll = -logp.gather(1, y.long().unsqueeze(1)).squeeze(1)
    loss = z.new_zeros(())
    if cw:
        loss = loss + cw * ((1.0 - SMOOTHING) * nll + SMOOTHING * (-logp.mean(dim=-1))).mean()
    if fw:
        loss = loss + fw * ((-torch.expm1(-nll)) ** gamma * nll).mean()
    if ua:
        loss = loss + ua * (-(torch.log((-torch.expm1(logp)).clamp(min=CLAMP)) * mask).sum(dim=-1)).mean()
    return loss


def kernel_bench(a):
    hp, T, B, R = bench.hparams("c2")
    V, N = hp["vocab_size"], B * R
    _, caps, lengths = bench.synthetic_batch(B, R, T, V, 1234, False, px=8)
    plan = Dk.PackPlan(lengths.reshape(-1), T, torch.device("cuda"))
    P = plan.P
    caps_i32 = caps.reshape(N, T).to(torch.int32).cuda().contiguous()
    targets = plan.pack(caps.reshape(N, T)[:, 1:].cuda().unsqueeze(-1)).squeeze(-1).to(torch.int32).contiguous()
    pad = int(hp["vocab_stoi"]["<PAD>"])
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(P, V, generator=g) * 2.0).cuda()
    lib = L.lib()
    f32 = dict(dtype=torch.float32, device="cuda")
    lse, aux, rows4, rows1 = torch.empty(P, **f32), torch.empty(P, 2, **f32), torch.empty(P, 4, **f32), torch.empty(P, **f32)
    correct = torch.empty(P, dtype=torch.int32, device="cuda")
    out6, out2, one, dl = torch.empty(6, **f32), torch.empty(2, **f32), torch.ones(1, **f32), torch.empty(P, V, **f32)

    def ce_pair(forward=True, backward=True):
        if forward:
            L.check(lib.sat_ce_label_smooth_fwd(L.ptr(z), L.ptr(targets), P, V, SMOOTHING, L.ptr(lse), L.ptr(rows1), L.ptr(correct), L.ptr(out2), L.stream_ptr()),
                    "sat_ce_label_smooth_fwd")
        if backward:
            L.check(lib.sat_ce_label_smooth_bwd(L.ptr(z), L.ptr(targets), L.ptr(lse), P, V, SMOOTHING, L.ptr(one), L.ptr(dl), L.stream_ptr()), "sat_ce_label_smooth_bwd")

    def token_pair(form, forward=True, backward=True):
        cw, fw, gamma, ua = form
        head = (L.ptr(z), L.ptr(targets), P, V, SMOOTHING, cw, fw, gamma, ua, L.ptr(caps_i32), L.ptr(plan.src_row), N, T, pad)
        if forward:
            L.check(lib.sat_token_loss_fwd(*head, L.ptr(lse), L.ptr(aux), L.ptr(rows4), L.ptr(correct), L.ptr(out6), L.stream_ptr()), "sat_token_loss_fwd")
        if backward:
            L.check(lib.sat_token_loss_bwd(*head, L.ptr(lse), L.ptr(aux), L.ptr(one), L.ptr(dl), L.stream_ptr()), "sat_token_loss_bwd")

    def torch_pair(form):
        za = z.detach().requires_grad_()
        mask = candidate_mask(caps_i32, plan.src_row, targets, V, pad)[0] if form[3] else None
        loss = torch_loss(za, targets, mask, form)
        loss.backward()
        return loss.detach(), za.grad

    agree = {}
    for name, form in FORMS.items():
        token_pair(form)
        loss_t, grad_t = torch_pair(form)
        torch.cuda.synchronize()
        agree[name] = dict(loss_kernel=float(out6[0]), loss_torch=float(loss_t), grad_max_abs_diff=float((dl - grad_t).abs().max()),
                           grad_max_abs=float(grad_t.abs().max()), mean_candidates=float(candidate_mask(caps_i32, plan.src_row, targets, V, pad)[0].sum()) / P)
        del grad_t
    calls = [("ce_pair", ce_pair)] + [("token_" + k, (lambda f: lambda: token_pair(f))(f)) for k, f in FORMS.items()]
    calls += [("ce_fwd", lambda: ce_pair(True, False)), ("ce_bwd", lambda: ce_pair(False, True))]
    calls += [("token_ce+fl+ul_fwd", lambda: token_pair(FORMS["ce+fl+ul"], True, False)), ("token_ce+fl+ul_bwd", lambda: token_pair(FORMS["ce+fl+ul"], False, True))]
    calls += [("torch_" + k, (lambda f: lambda: torch_pair(f))(f)) for k, f in FORMS.items()]
    for _ in range(3):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in calls}
    for _ in range(a.repeats):                                   # alternating rounds
        for k, fn in calls:
            n = a.launches if not k.startswith("torch_") else max(1, a.launches // 10)
            ms[k].append(event_ms(lambda: [fn() for _ in range(n)])[0] / n)
    res = dict(P=P, V=V, T=T, N=N, agree=agree, logits_mb=P * V * 4 / 1e6, **{k + "_ms": spread(v) for k, v in ms.items()})
    for k in FORMS:
        res["ratio_to_ce_pair_" + k] = res["token_%s_ms" % k]["median"] / res["ce_pair_ms"]["median"]
        res["torch_over_kernel_" + k] = res["torch_%s_ms" % k]["median"] / res["token_%s_ms" % k]["median"]
    return res


def step_bench(a):
    hp, T, B, R = bench.hparams("c2")
    models = {}
    for name, over in (("off", {}), ("on", dict(token_loss="ce+fl", focal_gamma=2.0, ul_alpha=1.0))):
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
    return dict(images=B, captions=B * R, packed_rows=int(lengths.sum()), precision=a.precision, step_off_ms=spread(ms["off"]), step_on_ms=spread(ms["on"]),
                **{k: float(out[k]) for k in ("ce", "fl", "ul", "repeat_mass")})


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
        raise SystemExit("bench_token_loss.py measures on the GPU; there is no CPU path")
    res = dict(repeats=a.repeats, launches=a.launches, kernels=kernel_bench(a))
    torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_bench(a)
    if a.json:
        print(json.dumps(res))
        return
    k = res["kernels"]
    print("token losses at P = %d, V = %d, T = %d (%.0f MB of logits); median (min - max) of %d rounds of %d" %
          (k["P"], k["V"], k["T"], k["logits_mb"], a.repeats, a.launches))
    r = k["ce_pair_ms"]
    print("  %-34s %7.1f us (%.1f - %.1f)" % ("sat_ce_label_smooth_fwd + _bwd", 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"]))
    for name in FORMS:
        r, t, ag = k["token_%s_ms" % name], k["torch_%s_ms" % name], k["agree"][name]
        print("  %-34s %7.1f us (%.1f - %.1f) = %.3fx the cross-entropy pair;  torch ops %8.1f us (%.1f - %.1f) = %.1fx;  loss %.6f (torch %.6f), "
              "max |gradient difference| %.2e of %.2e, %.1f candidates a row" % (
                  "sat_token_loss_fwd + _bwd, " + name, 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"], k["ratio_to_ce_pair_" + name], 1e3 * t["median"],
                  1e3 * t["min"], 1e3 * t["max"], k["torch_over_kernel_" + name], ag["loss_kernel"], ag["loss_torch"], ag["grad_max_abs_diff"], ag["grad_max_abs"],
                  ag["mean_candidates"]))
    f, b = k["token_ce+fl+ul_fwd_ms"], k["token_ce+fl+ul_bwd_ms"]
    cf, cb = k["ce_fwd_ms"], k["ce_bwd_ms"]
    print("  by phase: ce+fl+ul forward %.1f us (%.1f - %.1f), backward %.1f us (%.1f - %.1f);  cross entropy forward %.1f us (%.1f - %.1f), backward %.1f us (%.1f - %.1f)" % (
        1e3 * f["median"], 1e3 * f["min"], 1e3 * f["max"], 1e3 * b["median"], 1e3 * b["min"], 1e3 * b["max"], 1e3 * cf["median"], 1e3 * cf["min"], 1e3 * cf["max"],
        1e3 * cb["median"], 1e3 * cb["min"], 1e3 * cb["max"]))
    if "step" in res:
        s = res["step"]
        off, on = s["step_off_ms"], s["step_on_ms"]
        print("  training_step + backward, %d images x %d captions (%d packed rows), %s: plain %.3f ms (%.3f - %.3f), ce+fl with ul_alpha=1 %.3f ms (%.3f - %.3f); "
              "ce %.4f fl %.4f ul %.6f repeat mass %.6f" % (s["images"], s["captions"] // s["images"], s["packed_rows"], s["precision"], off["median"], off["min"],
                                                          off["max"], on["median"], on["min"], on["max"], s["ce"], s["fl"], s["ul"], s["repeat_mass"]))


if __name__ == "__main__":
    main()
