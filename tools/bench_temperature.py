"""Temperature-scaling calibration at the reference protocol's size: P = 70,560 packed rows (42 batches x 16 images x 5 captions x
21 steps, seq_len = 22), V = 6400 and V = 10000.  Times, on the same GPU and the same buffers,
  (a) ``fit_temperature`` with the reference constants (70 Nesterov-SGD steps; csrc/temperature.hip: one read of the logits per
      iteration), as the Python call and as the bare ``sat_temperature_fit`` enqueue on preallocated buffers, and
  (b) the reference's own loop (temperature_scaling.py:51-59) through stock torch ops: ``F.cross_entropy(logits / T, targets)``,
      autograd, ``torch.optim.SGD``.
hipEvent timing of whole fits after a warm-up fit of each; min / median / max over --repeats.  Reports ms per fit, ms per
iteration, and the logits bytes per iteration over the time, against the copy rate DESIGN.md uses for this chip (6.3 TB/s).
    python tools/bench_temperature.py [--rows 70560] [--vocab 6400 10000] [--repeats 7] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import _lib as L  # noqa: E402
from sat_amd import calibration  # noqa: E402

COPY_RATE = 6.3e12          # bytes/s, DESIGN.md section 5
REFERENCE = dict(init=1.5, lr=1e-2, momentum=0.8, nesterov=True, iters=70)


def timed(fn, repeats):
    fn()                                          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def torch_loop(logits, targets, init, lr, momentum, nesterov, iters):
    t = (torch.ones(1) * init).to(logits.device).detach().requires_grad_(True)
    opt = torch.optim.SGD([t], lr=lr, momentum=momentum, nesterov=nesterov)
    for _ in range(iters):
        loss = F.cross_entropy(logits / t, targets)
        loss.backward()
        opt.step()
        opt.zero_grad()
    return t.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=70560)
    ap.add_argument("--vocab", type=int, nargs="+", default=[6400, 10000])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_temperature.py measures on the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    lib = L.lib()
    iters = REFERENCE["iters"]
    for V in a.vocab:
        P = a.rows
        g = torch.Generator(device=dev).manual_seed(1)
        logits = torch.randn(P, V, generator=g, device=dev)
        targets = torch.randint(0, V, (P,), generator=g, device=dev)
        wrong = torch.rand(P, generator=g, device=dev) < 0.1
        hit = torch.where(wrong, (targets + 1 + torch.randint(0, V - 1, (P,), generator=g, device=dev)) % V, targets)
        logits[torch.arange(P, device=dev), hit] += 8.0
        t32 = targets.to(torch.int32)
        ws = torch.empty(lib.sat_temperature_workspace_bytes(P, V), dtype=torch.uint8, device=dev)
        t_trace = torch.empty(iters + 1, dtype=torch.float32, device=dev)
        l_trace = torch.empty(iters, dtype=torch.float32, device=dev)

        def bare():
            L.check(lib.sat_temperature_fit(L.ptr(logits), L.ptr(t32), P, V, REFERENCE["init"], REFERENCE["lr"], REFERENCE["momentum"], 1, iters,
                                            L.ptr(t_trace), L.ptr(l_trace), L.ptr(ws), L.stream_ptr()), "sat_temperature_fit")

        fit = calibration.fit_temperature(logits, targets, **REFERENCE)
        t_ref = float(torch_loop(logits, targets, **REFERENCE))
        rows = {"sat_temperature_fit": timed(bare, a.repeats),
                "fit_temperature": timed(lambda: calibration.fit_temperature(logits, targets, **REFERENCE), a.repeats),
                "torch_loop": timed(lambda: torch_loop(logits, targets, **REFERENCE), a.repeats)}
        nbytes = P * V * 4
        res = dict(P=P, V=V, logits_bytes=nbytes, iters=iters, T_hip=fit.temperature, T_torch=t_ref, repeats=a.repeats)
        for k, ms in rows.items():
            med = statistics.median(ms)
            res[k] = dict(ms_per_fit_min=min(ms), ms_per_fit_median=med, ms_per_fit_max=max(ms), ms_per_iteration=med / iters,
                          logits_bytes_per_s=nbytes * iters / (med * 1e-3), share_of_copy_rate=nbytes * iters / (med * 1e-3) / COPY_RATE)
        res["speedup_torch_over_fit_temperature"] = res["torch_loop"]["ms_per_fit_median"] / res["fit_temperature"]["ms_per_fit_median"]
        if a.json:
            print(json.dumps(res))
        else:
            print("P=%d V=%d (%.2f GB of logits), %d iterations; T: hip %.6f, torch loop %.6f" % (P, V, nbytes / 1e9, iters, fit.temperature, t_ref))
            for k in rows:
                r = res[k]
                print("  %-20s %8.2f ms/fit (min %.2f, max %.2f)  %7.3f ms/iteration  %6.2f TB/s of logits = %4.1f %% of the 6.3 TB/s copy rate"
                      % (k, r["ms_per_fit_median"], r["ms_per_fit_min"], r["ms_per_fit_max"], r["ms_per_iteration"], r["logits_bytes_per_s"] / 1e12,
                         100 * r["share_of_copy_rate"]))
            print("  torch loop / fit_temperature = %.1fx" % res["speedup_torch_over_fit_temperature"])
        del logits, ws


if __name__ == "__main__":
    main()
