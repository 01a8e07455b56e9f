"""One trial of the reference's evaluate.ipynb at its size: 4 batches of 128 images x 5 references, max_gen_length 32, beam 5 and
beam 20, on the BASELINE configs[4] model (resnet50 encoder, synthetic weights and pictures).  The same batches go, in the same
process and in alternating rounds, through
  (a) ``SAT.val_batch``        search on the device, then back-trace, BLEU / GLEU and the cosine loop on the host, and
  (b) ``SAT.val_batch_stats``  selection, statistics and cosine on the device; one host read per trial (``evaluation.evaluate``).
hipEvent timing of whole trials after a warm-up trial of each; median (min - max) of --repeats, reported per batch.  Path (a) is also
split, by host clocks around synchronised sections of one more trial, into encoder, search, read-back + back-trace and score_captions.
    python tools/bench_evaluate.py [--beams 5 20] [--batches 4] [--images 128] [--repeats 5] [--precision bf16] [--json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import sat_amd  # noqa: E402,F401
from sat_amd import evaluation as E  # noqa: E402
from sat_amd import model as M  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def clock_ms(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--max-gen-length", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_evaluate.py measures on the GPU; there is no CPU path")
    hp, T, _, R = bench.hparams("c2")
    torch.manual_seed(42)
    model = M.SAT(**hp).cuda().eval()
    model.set_precision(a.precision)
    batches = []
    for i in range(a.batches):
        img, caps, lengths = bench.synthetic_batch(a.images, R, T, hp["vocab_size"], 100 + i, ragged=True, px=hp["input_size"])
        batches.append((img.cuda(), caps.cuda(), lengths.cuda()))
    for beamk in a.beams:
        kw = dict(beamk=beamk, max_gen_length=a.max_gen_length, temperature=1.0, rescore_method="LN")

        def path_a():
            per = [model.val_batch(b, **kw) for b in batches]
            return {k: sum(p[k] for p in per) / len(per) for k in per[0]}

        def path_b():
            return E.evaluate(model, batches, **kw)["batch_mean"]

        ra, rb = path_a(), path_b()                      # warm-up: code objects, allocator; and the two paths' results side by side
        torch.cuda.synchronize()
        ms = {"a": [], "b": []}
        for _ in range(a.repeats):                       # alternating rounds
            ms["a"].append(event_ms(path_a)[0] / a.batches)
            ms["b"].append(event_ms(path_b)[0] / a.batches)
        # split of path (a), one more trial: host clocks around synchronised sections
        split = dict(encoder=0.0, search=0.0, readback_backtrace=0.0, score_captions=0.0)
        with torch.no_grad():
            for img, caps, lengths in batches:
                t, (ann, hw) = clock_ms(lambda: model.encode(img)); split["encoder"] += t
                ann = ann.contiguous()
                t_s, _ = clock_ms(lambda: model._beam_search_device(ann, beamk, a.max_gen_length, 1.0, "beam", 3, None, None, None, None, False))
                t_d, out = clock_ms(lambda: model.beam_decode_batched(ann, hw, beamk, a.max_gen_length, 1.0, "LN", 0.5, False))
                split["search"] += t_s; split["readback_backtrace"] += max(0.0, t_d - t_s)
                t, _ = clock_ms(lambda: model.score_captions(out[0], caps, lengths, out[3])); split["score_captions"] += t
        split = {k: v / a.batches for k, v in split.items()}
        med_a, med_b = statistics.median(ms["a"]), statistics.median(ms["b"])
        res = dict(beamk=beamk, images=a.images, references=R, batches=a.batches, max_gen_length=a.max_gen_length, precision=a.precision, repeats=a.repeats,
                   val_batch_ms_per_batch=dict(median=med_a, min=min(ms["a"]), max=max(ms["a"])),
                   val_batch_stats_ms_per_batch=dict(median=med_b, min=min(ms["b"]), max=max(ms["b"])),
                   val_batch_split_ms_per_batch=split, ratio=med_a / med_b,
                   bleu_gleu_equal=all(ra[k] == rb[k] for k in ("bleu1", "bleu2", "bleu3", "bleu4", "gleu")),
                   cosine_a=ra["cosine_similarity"], cosine_b=rb["cosine_similarity"], perplexity_a=ra["perplexity"], perplexity_b=rb["perplexity"])
        if a.json:
            print(json.dumps(res))
        else:
            print("beam %d, %d batches of %d images x %d references, max_gen_length %d, %s" % (beamk, a.batches, a.images, R, a.max_gen_length, a.precision))
            print("  (a) val_batch        %8.2f ms per batch (min %.2f, max %.2f)" % (med_a, min(ms["a"]), max(ms["a"])))
            print("      of which: encoder %.2f, search %.2f, read-back + back-trace %.2f, score_captions %.2f" %
                  (split["encoder"], split["search"], split["readback_backtrace"], split["score_captions"]))
            print("  (b) val_batch_stats  %8.2f ms per batch (min %.2f, max %.2f)   (a) / (b) = %.2fx" % (med_b, min(ms["b"]), max(ms["b"]), med_a / med_b))
            print("  BLEU / GLEU equal: %s; cosine %.7f / %.7f; perplexity %.6f / %.6f" %
                  (res["bleu_gleu_equal"], ra["cosine_similarity"], rb["cosine_similarity"], ra["perplexity"], rb["perplexity"]))


if __name__ == "__main__":
    main()
