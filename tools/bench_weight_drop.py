"""What weight-drop and variational dropout cost ("Weight-drop and variational dropout"), at BASELINE configs[1]'s decoder
shape: A = 128, D = 512, n = 512 (Wcat is 2688 x 512), N = 640 captions, ragged lengths.  Device events, warm-up first, profiler off.
  1. The packing launch (sat_decoder_pack_weights: Wcat, its bf16 copy, bcat) plain and with weight_drop = 0.5, alternating rounds; the
     bytes it moves (every source element once, fp32 and bf16 copies written) over its time, against the HBM peak.
  2. The gradient-mask launch (sat_weight_drop_grad) on one and on two (4n, n) matrices: one read and one write of every element.
  3. ``SAT.training_step`` + backward: plain, with ``weight_drop=0.5``, and with ``dropout=0.3, embedding_dropout=0.2`` per step against
     the same rates under ``variational_dropout=True``; same process, alternating.
    python tools/bench_weight_drop.py [--repeats 10] [--launches 50] [--step-repeats 8] [--no-step] [--json]
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
from sat_amd import decoder as Dk  # noqa: E402
from sat_amd import model as M  # noqa: E402

HBM_PEAK_GBS = bench.PEAK_HBM_GBS
SEED = 123456789


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def kernel_bench(a):
    hp, T, B, R = bench.hparams("c2")
    A, D, m, n, V = hp["attention_dim"], hp["encoder_dim"], hp["embed_dim"], hp["decoder_dim"], hp["vocab_size"]
    HCW = A + D + 4 * n
    g = torch.Generator().manual_seed(5)
    rnd = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).cuda()
    tens = dict(att_dec=rnd(A, n), beta_w=rnd(D, n), w_hh=rnd(4 * n, n), beta_b=rnd(D), b_ih=rnd(4 * n), b_hh=rnd(4 * n))
    params = Dk._params_struct(tens)
    wcat, wcat_b, bcat = torch.empty(HCW, n, device="cuda"), torch.empty(HCW, n, dtype=torch.bfloat16, device="cuda"), torch.empty(HCW, device="cuda")
    lib = L.lib()
    dims = {name: Dk.decoder_dims(B, R, T, 49, D, A, m, n, V, 0, True, 0, 1, weight_drop=p, dropout_seed=SEED) for name, p in (("plain", 0.0), ("masked", 0.5))}

    def pack(name):
        L.check(lib.sat_decoder_pack_weights(C.byref(dims[name]), C.byref(params), L.ptr(wcat), L.ptr(wcat_b), L.ptr(bcat), L.stream_ptr()), "sat_decoder_pack_weights")

    grads = {1: rnd(1, 4 * n, n), 2: rnd(2, 4 * n, n)}

    def grad_mask(layers):
        Dk.weight_drop_grad_(grads[layers], 0.5, SEED)

    # agreement first: the masked pack differs from the plain one in the W_hh rows only, by the host mask
    pack("plain"); plain = wcat.clone()
    pack("masked")
    mask = torch.from_numpy(Dk.weight_drop_scale_reference(SEED, 1, n, 0.5))[0].cuda()
    agree = dict(head_rows_equal=bool(torch.equal(wcat[:A + D], plain[:A + D])), w_hh_rows_equal_mask=bool(torch.equal(wcat[A + D:], plain[A + D:] * mask)),
                 kept_share=float((mask > 0).float().mean()))
    fns = {"pack_plain": lambda: pack("plain"), "pack_masked": lambda: pack("masked"), "grad_mask_1": lambda: grad_mask(1), "grad_mask_2": lambda: grad_mask(2)}
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(a.repeats):                                   # alternating rounds
        for k, fn in fns.items():
            ms[k].append(event_ms(lambda: [fn() for _ in range(a.launches)])[0] / a.launches)
    pack_bytes = HCW * n * (4 + 4 + 2) + HCW * 4 * 3             # sources read once, fp32 and bf16 copies written, the bias rows
    least = dict(pack_plain=pack_bytes, pack_masked=pack_bytes, grad_mask_1=4 * n * n * 8, grad_mask_2=2 * 4 * n * n * 8)
    res = dict(A=A, D=D, n=n, wcat_rows=HCW, agree=agree, least_bytes=least, **{k + "_ms": spread(v) for k, v in ms.items()})
    for k in fns:
        gbs = least[k] / (res[k + "_ms"]["median"] * 1e-3) / 1e9
        res[k + "_gbs"], res[k + "_share_of_hbm_peak"] = gbs, gbs / HBM_PEAK_GBS
    return res


STEP_CASES = (("plain", {}), ("weight_drop", dict(weight_drop=0.5)), ("dropout", dict(dropout=0.3, embedding_dropout=0.2)),
              ("variational", dict(dropout=0.3, embedding_dropout=0.2, variational_dropout=True)))


def step_bench(a):
    hp, T, B, R = bench.hparams("c2")
    models = {}
    for name, over in STEP_CASES:
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
    ms = {name: [] for name in models}
    for _ in range(a.step_repeats):                              # alternating rounds
        for name, m in models.items():
            ms[name].append(event_ms(lambda: step(m))[0])
    return dict(images=B, captions=B * R, packed_rows=int(lengths.sum()), precision=a.precision, **{"step_%s_ms" % k: spread(v) for k, v in ms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--step-repeats", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--no-step", action="store_true", help="the kernels only")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_drop.py measures on the GPU; there is no CPU path")
    res = dict(repeats=a.repeats, launches=a.launches, kernels=kernel_bench(a))
    torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_bench(a)
    if a.json:
        print(json.dumps(res))
        return
    k = res["kernels"]
    print("weight-drop at A = %d, D = %d, n = %d (Wcat %d x %d); median (min - max) of %d rounds of %d" % (k["A"], k["D"], k["n"], k["wcat_rows"], k["n"], a.repeats, a.launches))
    ag = k["agree"]
    print("  masked pack: W_d / W_beta rows unchanged %s, W_hh rows = plain * host mask %s, kept share %.4f" % (ag["head_rows_equal"], ag["w_hh_rows_equal_mask"], ag["kept_share"]))
    for name, label in (("pack_plain", "pack, plain"), ("pack_masked", "pack, weight_drop 0.5"), ("grad_mask_1", "gradient mask, 1 layer"), ("grad_mask_2", "gradient mask, 2 layers")):
        r = k[name + "_ms"]
        print("  %-24s %7.1f us (%.1f - %.1f)  %.0f GB/s of the %.1f MB it moves = %.0f%% of the %.0f GB/s HBM peak" % (
            label, 1e3 * r["median"], 1e3 * r["min"], 1e3 * r["max"], k[name + "_gbs"], k["least_bytes"][name] / 1e6, 100 * k[name + "_share_of_hbm_peak"], HBM_PEAK_GBS))
    if "step" in res:
        s = res["step"]
        print("  training_step + backward, %d images x %d captions (%d packed rows), %s:" % (s["images"], s["captions"] // s["images"], s["packed_rows"], s["precision"]))
        for name, _ in STEP_CASES:
            r = s["step_%s_ms" % name]
            print("    %-12s %.3f ms (%.3f - %.3f)" % (name, r["median"], r["min"], r["max"]))


if __name__ == "__main__":
    main()
