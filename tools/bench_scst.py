"""What a self-critical step costs next to a cross-entropy step, at BASELINE configs[1] (resnet50, V = 6400, 128 images, bf16) with K = 5
samples of up to S = 20 words per image (synthetic weights, pictures and references).  Device events, warm-up first, profiler off.
  1. ``SAT.scst_step`` + backward against ``SAT.training_step`` + backward on a 128 x 5-caption batch, in the same process and in
     alternating rounds (no optimizer step in either); median (min - max) of --repeats.
  2. One more self-critical step split by events around its layers (sat_amd/scst.py): encoder + sampling, greedy baseline, scoring +
     prepare, gradient pass (forward + backward).
  3. At the (P, V) the step produced: the pair sat_policy_nll_fwd + _bwd against the pair sat_ce_label_smooth_fwd + _bwd on the same
     logits, alternating, --pair-repeats rounds of --pair-launches launches each: median (min - max) per pair.
    python tools/bench_scst.py [--images 128] [--samples 5] [--max-gen-length 20] [--baseline mean] [--repeats 7] [--json]
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
from sat_amd import evaluation as E  # noqa: E402
from sat_amd import model as M  # noqa: E402
from sat_amd import scst  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--max-gen-length", type=int, default=20)
    ap.add_argument("--baseline", default="mean", choices=list(scst.BASELINES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pair-repeats", type=int, default=15)
    ap.add_argument("--pair-launches", type=int, default=10)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scst.py measures on the GPU; there is no CPU path")
    hp, T, _, R = bench.hparams("c2")
    torch.manual_seed(42)
    model = M.SAT(**hp).cuda().train()
    model.set_precision(a.precision)
    model.__dict__["_sat_global_step"] = 2                       # past encoder_finetune_after: the encoder trains, as in bench.py's headline
    V, K, S = hp["vocab_size"], a.samples, a.max_gen_length
    img, caps, lengths = bench.synthetic_batch(a.images, R, T, V, 1234, ragged=True, px=hp["input_size"])
    batch = (img.cuda(), caps.cuda(), lengths)
    rc = E.ReferenceCorpus(V, expected_positions=8 * E.ReferenceCorpus.positions(lengths))
    rc.add(caps, lengths)
    for i in range(7):                                           # a corpus a few batches large, so that document frequencies differ
        _, c, l = bench.synthetic_batch(a.images, R, T, V, 2000 + i, ragged=True, px=8)
        rc.add(c, l)
    rc.check()
    kw = dict(samples=K, baseline=a.baseline, max_gen_length=S, temperature=1.0)

    def scst_step(seed):
        model.zero_grad(set_to_none=True)
        out = model.scst_step(batch, rc, seed=seed, **kw)
        out["loss"].backward()
        return out

    def xe_step():
        model.zero_grad(set_to_none=True)
        out = model.training_step(batch, 0)
        out["loss"].backward()
        return out

    for i in range(2):                                           # warm-up: code objects, allocator, packing plans
        scst_step(i); xe_step()
    torch.cuda.synchronize()
    ms = {"scst": [], "xe": []}
    for i in range(a.repeats):                                   # alternating rounds
        ms["scst"].append(event_ms(lambda: scst_step(10 + i))[0])
        ms["xe"].append(event_ms(xe_step)[0])

    # ---- the split of one more step, layer by layer
    split = {}
    ids = scst.special_ids(model)
    model.zero_grad(set_to_none=True)
    model.eval()
    with torch.no_grad():
        def sample():
            ann, _ = model.encode(batch[0])
            return (ann.contiguous(),) + tuple(scst.sample(model, ann.contiguous(), K, S, 1.0, seed=99))
        split["encoder_and_sample"], (ann, tokens, lens) = event_ms(sample)
        refs_d, rl_d = batch[1].to(torch.int32).contiguous(), batch[2].cuda().to(torch.int32).contiguous()

        def greedy():
            g_tok, g_len = scst.greedy(model, ann, S)
            return scst.rewards(g_tok, g_len, refs_d, rl_d, rc, 1)
        split["greedy_baseline"], sg = event_ms(greedy)

        def score():
            sc = scst.rewards(tokens, lens, refs_d, rl_d, rc, K)
            return scst.prepare(tokens, lens, sc, K, ids, a.baseline, (1.0, 0.0), sg if a.baseline == "greedy" else None)
        split["scoring_and_prepare"], prep = event_ms(score)
    model.train()
    lengths_host = prep["lengths"].cpu()

    def gradient():
        ann_g, _ = model.encode(batch[0])
        loss = scst.loss(model, ann_g, prep["caps"], lengths_host, prep["step_weight"], None, 1.0)
        loss.backward()
    split["gradient_pass"], _ = event_ms(gradient)
    if a.baseline != "greedy":
        split["greedy_baseline"] = 0.0                           # not part of the step with this baseline (measured above for reference only)

    # ---- the loss kernels on their own at the step's (P, V)
    P = int(lengths_host.sum())
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(P, V, generator=g) * 3.0).cuda()
    targets = torch.randint(1, V - 3, (P,), generator=g).to(torch.int32).cuda()
    weight = (torch.rand(P, generator=g) - 0.5).cuda()
    idd = torch.tensor(ids, dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    lse, logq, rowl, out, dl = torch.empty(P, **f32), torch.empty(P, **f32), torch.empty(P, **f32), torch.empty(2, **f32), torch.empty(P, V, **f32)
    correct = torch.empty(P, dtype=torch.int32, device="cuda")
    lib = L.lib()
    N = a.images * K

    def policy_pair():
        for _ in range(a.pair_launches):
            L.check(lib.sat_policy_nll_fwd(L.ptr(logits), L.ptr(targets), L.ptr(weight), P, V, 1.0, L.ptr(idd), N, 1.0 / P, L.ptr(lse), L.ptr(logq),
                                           L.ptr(out), L.stream_ptr()), "sat_policy_nll_fwd")
            L.check(lib.sat_policy_nll_bwd(L.ptr(logits), L.ptr(targets), L.ptr(weight), L.ptr(lse), P, V, 1.0, L.ptr(idd), N, 1.0 / P, None, L.ptr(dl),
                                           L.stream_ptr()), "sat_policy_nll_bwd")

    def ce_pair():
        for _ in range(a.pair_launches):
            L.check(lib.sat_ce_label_smooth_fwd(L.ptr(logits), L.ptr(targets), P, V, 0.0, L.ptr(lse), L.ptr(rowl), L.ptr(correct), L.ptr(out),
                                                L.stream_ptr()), "sat_ce_label_smooth_fwd")
            L.check(lib.sat_ce_label_smooth_bwd(L.ptr(logits), L.ptr(targets), L.ptr(lse), P, V, 0.0, None, L.ptr(dl), L.stream_ptr()),
                    "sat_ce_label_smooth_bwd")

    policy_pair(); ce_pair()
    torch.cuda.synchronize()
    pair = {"policy": [], "ce": []}
    for _ in range(a.pair_repeats):                              # alternating rounds
        pair["policy"].append(event_ms(policy_pair)[0] / a.pair_launches)
        pair["ce"].append(event_ms(ce_pair)[0] / a.pair_launches)

    res = dict(images=a.images, samples=K, max_gen_length=S, baseline=a.baseline, precision=a.precision, repeats=a.repeats, vocab=V,
               scst_step_ms=spread(ms["scst"]), training_step_ms=spread(ms["xe"]), scst_split_ms=split,
               sample_length_mean=float(lens.float().mean()), packed_rows=P, xe_packed_rows=int(lengths.sum()),
               policy_pair_ms=spread(pair["policy"]), ce_pair_ms=spread(pair["ce"]), pair_repeats=a.pair_repeats, pair_launches=a.pair_launches)
    if a.json:
        print(json.dumps(res))
        return
    print("%d images x %d samples of up to %d words, baseline %s, %s; forward + backward, no optimizer step" % (a.images, K, S, a.baseline, a.precision))
    for name, key in (("scst_step", "scst_step_ms"), ("training_step (%d x %d captions)" % (a.images, R), "training_step_ms")):
        print("  %-40s %8.2f ms (min %.2f, max %.2f)" % (name, res[key]["median"], res[key]["min"], res[key]["max"]))
    print("  scst_step by layer: encoder + sample %.2f, greedy baseline %.2f, scoring + prepare %.2f, gradient pass %.2f ms"
          % (split["encoder_and_sample"], split["greedy_baseline"], split["scoring_and_prepare"], split["gradient_pass"]))
    print("  samples of %.1f words on average: %d packed rows (the cross-entropy batch packs %d)" % (res["sample_length_mean"], P, res["xe_packed_rows"]))
    for name, key in (("sat_policy_nll_fwd + _bwd", "policy_pair_ms"), ("sat_ce_label_smooth_fwd + _bwd", "ce_pair_ms")):
        print("  %-40s %8.4f ms (min %.4f, max %.4f) at P = %d, V = %d" % (name, res[key]["median"], res[key]["min"], res[key]["max"], P, V))


if __name__ == "__main__":
    main()
