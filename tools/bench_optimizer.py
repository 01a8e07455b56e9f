"""What averaged weights cost in the optimizer step ("Averaged weights"): one ``FusedOptimizer.step()`` over the parameter set
of BASELINE configs[1] (C2: resnet50 + decoder as ``bench.py`` builds the model - bf16 filter copies present, gradients in the persistent
buckets, so the step runs on its fast path) for

    adam                    the plain fused step                                   28 B / element (p rw, g r, exp_avg rw, exp_avg_sq rw)
    adam + ema              the same launch with the average taken in the pass     36 B / element (+ ema rw)
    asgd                    torch.optim.ASGD's step, lambd = 0                     20 B / element (p rw, g r, ax rw)
    adam, then foreach lerp the unfused alternative: the plain step, then
                            ``torch._foreach_lerp_`` over every parameter          40 B / element (+ p r, ema rw)

(+ 2 B for every filter element that has a bf16 copy, in all four).  The variants are timed in alternation, ``--rounds`` windows of
``--steps`` steps each between device events; the line of a variant is the median window, with the fastest and slowest beside it.
    python tools/bench_optimizer.py [--steps 50] [--rounds 7] [--ema-decay 0.999] [--json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="optimizer steps per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="timed windows per variant (alternating)")
    ap.add_argument("--ema-decay", type=float, default=0.999)
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    model, opt, sync, batch, _ = bench._build_train("c2", dev, batch=4)      # the gradients of one real (small) train step, left in place
    opt.zero_grad(set_to_none=True)
    model.training_step(batch, 0)["loss"].backward()
    sync.finish()
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    n = sum(p.numel() for p in params)
    n_shadow = sum(p.numel() for p in params if getattr(p, "_sat_bf16_shadow", None) is not None)

    def build(kind, ema):
        model.hp.opt, model.hp.ema_decay, model.hp.asgd_lambd = kind, ema, 0.0
        return model.configure_optimizers()

    plain, with_ema, asgd, unfused = build("adam", 0.0), build("adam", a.ema_decay), build("asgd", 0.0), build("adam", 0.0)
    emas = [p.detach().clone() for p in params]
    datas = [p.detach() for p in params]

    def unfused_step():
        unfused.step()
        torch._foreach_lerp_(emas, datas, 1.0 - a.ema_decay)

    variants = [("adam", plain.step, 28), ("adam + ema (fused)", with_ema.step, 36), ("asgd", asgd.step, 20),
                ("adam, then foreach lerp", unfused_step, 40)]
    for _, fn, _ in variants:           # warm: tables built and uploaded, state created, the fast path reached
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, fn, _ in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.steps)
    fast = {"adam": plain, "adam + ema (fused)": with_ema, "asgd": asgd, "adam, then foreach lerp": unfused}
    rows = []
    for name, _, per_elem in variants:
        ms = statistics.median(times[name])
        nbytes = per_elem * n + 2 * n_shadow
        rows.append(dict(variant=name, ms=round(ms, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                         bytes_per_element=per_elem, gbytes_per_s=round(nbytes / ms / 1e6, 1),
                         fast_path_steps=getattr(fast[name], "fast_path_steps", 0)))
    out = dict(tool="bench_optimizer", config="c2", tensors=len(params), elements=n, elements_with_bf16_copy=n_shadow, steps=a.steps, rounds=a.rounds,
               ema_decay=a.ema_decay, device=torch.cuda.get_device_name(0), rows=rows)
    if a.json:
        print(json.dumps(out))
        return
    print("C2 parameter set: %d tensors, %.2f M elements (%.2f M with a bf16 copy); %d x %d steps per variant" % (len(params), n / 1e6, n_shadow / 1e6, a.rounds, a.steps))
    for r in rows:
        print("%-26s %8.4f ms / step (%.4f - %.4f)   %2d B/element   %7.1f GB/s" % (r["variant"], r["ms"], r["ms_min"], r["ms_max"], r["bytes_per_element"],
                                                                               r["gbytes_per_s"]))


if __name__ == "__main__":
    main()
