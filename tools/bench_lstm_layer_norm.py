"""What the layer-normalised LSTM cell costs ("Layer-normalised LSTM"), at BASELINE configs[1]'s decoder shape: n = 512,
N = 640 caption rows with gate rows embedded in the (A + D + 4n)-wide step buffer, ragged lengths.  Device events, warm-up first,
profiler off, the two sides of every comparison alternating in one process.
  1. The two cell kernels (sat_lstm_ln_cell_fwd / _bwd, the backward with its parameter-gradient partials) next to the plain pair
     (sat_lstm_cell_pointwise_fwd / _bwd) on the same buffers, and the finishing sum (sat_lstm_ln_param_grads); the bytes each launch
     has to move over its time, against the HBM peak.
  2. ``SAT.training_step`` + backward at C2 with and without ``lstm_layer_norm``.
  3. The batched beam-5 search of C5 (64 images, max_gen_length 20, decode only) with and without.
    python tools/bench_lstm_layer_norm.py [--repeats 10] [--launches 50] [--step-repeats 8] [--search-repeats 8] [--no-step] [--no-search] [--json]
"""
import argparse
import ctypes as C
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


def kernel_bench(a):
    hp, T, B, R = bench.hparams("c2")
    A, D, n = hp["attention_dim"], hp["encoder_dim"], hp["decoder_dim"]
    N, ld = B * R, A + D + 4 * n
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).cuda()
    pre, hc, dhc = rnd(N, ld), torch.empty(N, ld, device="cuda"), torch.empty(N, ld, device="cuda")
    gy, c_prev, h_prev, dh_out = rnd(N, 4 * n), rnd(N, n), rnd(N, n), rnd(N, n)
    c_new, h_new = torch.empty(N, n, device="cuda"), torch.empty(N, n, device="cuda")
    dh0, dc0 = rnd(N, n), rnd(N, n)
    dh_carry, dc_carry = dh0.clone(), dc0.clone()
    hb = torch.empty(N, n, dtype=torch.bfloat16, device="cuda")
    dgb = torch.empty(N, ld, dtype=torch.bfloat16, device="cuda")
    live = (torch.rand(N, generator=g) > 0.2).to(torch.int32).cuda()          # a fifth of the captions has ended
    gw, gb, cw, cb = 1 + 0.5 * rnd(4 * n), 0.5 * rnd(4 * n), 1 + 0.5 * rnd(n), 0.5 * rnd(n)
    xhat, rstd = torch.empty(N, 5 * n, device="cuda"), torch.empty(N, 5, device="cuda")
    lib = L.lib()
    slots = lib.sat_lstm_ln_slots(N)
    part = torch.zeros(slots, 10 * n, device="cuda")
    grads = [torch.empty(w, device="cuda") for w in (4 * n, 4 * n, n, n)]
    scratch = torch.empty(16 * n, device="cuda")
    gates, dgates = hc[:, A + D:], dhc[:, A + D:]
    st = L.stream_ptr

    def ln_fwd():
        L.check(lib.sat_lstm_ln_cell_fwd(L.ptr(gates), ld, L.ptr(gy), L.ptr(c_prev), L.ptr(h_prev), L.ptr(c_new), L.ptr(h_new), L.ptr(live), L.ptr(hb), L.ptr(gw),
                                         L.ptr(gb), L.ptr(cw), L.ptr(cb), L.ptr(xhat), L.ptr(rstd), N, n, st()), "sat_lstm_ln_cell_fwd")

    def plain_fwd():
        L.check(lib.sat_lstm_cell_pointwise_fwd(L.ptr(gates), ld, L.ptr(gy), L.ptr(c_prev), L.ptr(h_prev), L.ptr(c_new), L.ptr(h_new), L.ptr(live), L.ptr(hb), N, n, st()),
                "sat_lstm_cell_pointwise_fwd")

    def ln_bwd():
        L.check(lib.sat_lstm_ln_cell_bwd(L.ptr(gates), ld, L.ptr(c_prev), L.ptr(xhat), L.ptr(rstd), L.ptr(dh_out), L.ptr(dh_carry), L.ptr(dc_carry), L.ptr(dgates), ld,
                                         L.ptr(live), L.ptr(dgb), L.ptr(gw), L.ptr(cw), L.ptr(cb), L.ptr(part), N, n, st()), "sat_lstm_ln_cell_bwd")

    def plain_bwd():
        L.check(lib.sat_lstm_cell_pointwise_bwd(L.ptr(gates), ld, L.ptr(c_prev), L.ptr(c_new), L.ptr(dh_out), L.ptr(dh_carry), L.ptr(dc_carry), L.ptr(dgates), ld,
                                                L.ptr(live), L.ptr(dgb), N, n, st()), "sat_lstm_cell_pointwise_bwd")

    def finish():
        L.check(lib.sat_lstm_ln_param_grads(L.ptr(part), slots, n, *[L.ptr(t) for t in grads], L.ptr(scratch), st()), "sat_lstm_ln_param_grads")

    # the forward kernels activate the gates in place: every timed forward launch starts from the pre-activations again (the copy is
    # timed on its own and taken off); the backward kernels read activated gates, which both forwards leave in the same place
    def fresh():
        hc.copy_(pre)

    def carries():
        dh_carry.copy_(dh0); dc_carry.copy_(dc0)

    fns = {"copy_gates": (fresh, None), "ln_fwd": (ln_fwd, fresh), "plain_fwd": (plain_fwd, fresh), "copy_carries": (carries, None), "ln_bwd": (ln_bwd, carries),
           "plain_bwd": (plain_bwd, carries), "finish": (finish, None)}
    fresh(); ln_fwd()
    for _ in range(3):
        for fn, prep in fns.values():
            if prep:
                prep()
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.repeats):                                   # alternating rounds
        for k, (fn, prep) in fns.items():
            if k == "ln_bwd":                                    # ... on the gates and saved values of its own forward
                fresh(); ln_fwd()
            if k == "plain_bwd":
                fresh(); plain_fwd()

            def burst():
                for _ in range(a.launches):
                    if prep:
                        prep()
                    fn()
            ms[k].append(event_ms(burst)[0] / a.launches)
    res = {k + "_ms": spread(v) for k, v in ms.items()}
    for k, base in (("ln_fwd", "copy_gates"), ("plain_fwd", "copy_gates"), ("ln_bwd", "copy_carries"), ("plain_bwd", "copy_carries")):
        res[k + "_net_ms"] = spread([x - y for x, y in zip(ms[k], ms[base])])
    nl = int(live.sum())
    f4 = 4.0
    # bytes a launch has to move (live rows; dead rows move the state / zero the gates): gates read + written, gy, c_prev, c, h, bf16 h (+ saved 5n + 5)
    least = dict(plain_fwd=nl * n * (f4 * (4 + 4 + 4 + 1 + 1 + 1) + 2), ln_fwd=nl * n * (f4 * (4 + 4 + 4 + 1 + 1 + 1 + 5) + 2) + nl * 5 * f4,
                 # gates, c_prev, c or saved rows, dh_out, the two carries read and written, dgates fp32 + bf16 (+ one pass over the slots, read and written)
                 plain_bwd=nl * n * (f4 * (4 + 1 + 1 + 1 + 4 + 4) + 8), ln_bwd=nl * n * (f4 * (4 + 1 + 5 + 1 + 4 + 4) + 8) + nl * 5 * f4 + slots * 10 * n * 2 * f4,
                 finish=slots * 10 * n * f4)
    res.update(rows=N, live_rows=nl, n=n, ld=ld, slots=slots, least_bytes=least)
    for k, b in least.items():
        t = res[k + "_net_ms"]["median"] if k + "_net_ms" in res else res[k + "_ms"]["median"]
        res[k + "_gbs"] = b / (t * 1e-3) / 1e9 if t > 0 else float("nan")
    # one more pass over the saved rows at the HBM peak on top of the plain backward: the yardstick DESIGN.md compares the backward with
    res["saved_pass_ms_at_peak"] = nl * (5 * n + 5) * f4 / (HBM_PEAK_GBS * 1e9) * 1e3
    return res


def make_model(hp, over, precision, train):
    torch.manual_seed(42)
    m = M.SAT(**dict(hp, **over)).cuda()
    m.train(train)
    m.set_precision(precision)
    return m


CASES = (("plain", {}), ("layer_norm", dict(lstm_layer_norm=True)))


def step_bench(a):
    hp, T, B, R = bench.hparams("c2")
    models = {}
    for name, over in CASES:
        m = make_model(hp, over, a.precision, True)
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
    ms = {name: [] for name in models}
    for _ in range(a.step_repeats):                              # alternating rounds
        for name, m in models.items():
            ms[name].append(event_ms(lambda: step(m))[0])
    return dict(images=B, captions=B * R, packed_rows=int(lengths.sum()), precision=a.precision, **{"step_%s_ms" % k: spread(v) for k, v in ms.items()})


def search_bench(a, images=64, max_len=20, beamk=5):
    hp, _, _, _ = bench.hparams("c2")
    models = {name: make_model(hp, over, a.precision, False) for name, over in CASES}
    img = torch.rand(images, 3, hp["input_size"], hp["input_size"], device="cuda")
    anns = {}
    with torch.no_grad():
        for name, m in models.items():
            ann, hw = m.encode(img)
            anns[name] = (ann.contiguous(), hw)
        run = lambda name: models[name].beam_decode_batched(*anns[name], beamk=beamk, max_gen_length=max_len)
        for _ in range(2):
            for name in models:
                run(name)
        torch.cuda.synchronize()
        ms = {name: [] for name in models}
        for _ in range(a.search_repeats):
            for name in models:
                ms[name].append(event_ms(lambda: run(name))[0])
    return dict(images=images, beamk=beamk, max_gen_length=max_len, precision=a.precision, **{"search_%s_ms" % k: spread(v) for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--step-repeats", type=int, default=8)
    ap.add_argument("--search-repeats", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lstm_layer_norm.py measures on the GPU; there is no CPU path")
    res = dict(repeats=a.repeats, launches=a.launches, kernels=kernel_bench(a))
    torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_bench(a)
        torch.cuda.empty_cache()
    if not a.no_search:
        res["search"] = search_bench(a)
    if a.json:
        print(json.dumps(res))
        return
    k = res["kernels"]
    print("LSTM cell at n = %d, %d rows (%d live), gate rows of stride %d; median (min - max) of %d rounds of %d launches" % (k["n"], k["rows"], k["live_rows"], k["ld"], a.repeats, a.launches))
    for name, label in (("plain_fwd", "plain forward"), ("ln_fwd", "normalised forward"), ("plain_bwd", "plain backward"), ("ln_bwd", "normalised backward + partials")):
        r, raw = k[name + "_net_ms"], k[name + "_ms"]
        print("  %-32s %7.2f us (%.2f - %.2f) net of the reset copy (%.2f us with it)  %.1f MB -> %.0f GB/s = %.0f%% of the %.0f GB/s HBM peak" % (
            label, 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"], 1e3 * raw["median"], k["least_bytes"][name] / 1e6, k[name + "_gbs"],
            100 * k[name + "_gbs"] / HBM_PEAK_GBS, HBM_PEAK_GBS))
    r = k["finish_ms"]
    print("  %-32s %7.2f us (%.2f - %.2f)  %d slots, four column sums" % ("finishing sum (once a step)", 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"], k["slots"]))
    print("  one pass over the saved rows at the HBM peak: %.2f us" % (1e3 * k["saved_pass_ms_at_peak"]))
    if "step" in res:
        s = res["step"]
        print("  training_step + backward, %d images x %d captions (%d packed rows), %s:" % (s["images"], s["captions"] // s["images"], s["packed_rows"], s["precision"]))
        for name, _ in CASES:
            r = s["step_%s_ms" % name]
            print("    %-12s %.3f ms (%.3f - %.3f)" % (name, r["median"], r["min"], r["max"]))
    if "search" in res:
        s = res["search"]
        print("  batched beam-%d search, %d images, max_gen_length %d, decode only, %s:" % (s["beamk"], s["images"], s["max_gen_length"], s["precision"]))
        for name, _ in CASES:
            r = s["search_%s_ms" % name]
            print("    %-12s %.3f ms (%.3f - %.3f) = %.0f images/s" % (name, r["median"], r["min"], r["max"], s["images"] / (r["median"] * 1e-3)))


if __name__ == "__main__":
    main()
