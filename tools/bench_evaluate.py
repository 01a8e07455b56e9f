"""One trial of the reference's evaluate.ipynb at its size: 4 batches of 128 images x 5 references, max_gen_length 32, beam 5 and
beam 20, on the BASELINE configs[4] model (resnet50 encoder, synthetic weights and pictures).  The same batches go, in the same
process and in alternating rounds, through
  (a) ``SAT.val_batch``        search on the device, then back-trace, BLEU / GLEU and the cosine loop on the host, and
  (b) ``SAT.val_batch_stats``  selection, statistics and cosine on the device; one host read per trial (``evaluation.evaluate``).
hipEvent timing of whole trials after a warm-up trial of each; median (min - max) of --repeats, reported per batch.  Path (a) is also
split, by host clocks around synchronised sections of one more trial, into encoder, search, read-back + back-trace and score_captions.
--cider measures instead what CIDEr-D and ROUGE-L cost at beam 5: the per-batch time of ``val_batch_stats`` without and with
``corpus=`` (alternating rounds, hipEvents), the host clock of ``metrics.cider_d`` + ``metrics.rouge_l`` on the same tokens (already
on the host as lists: the read-back is not counted), and the one-off build of the document-frequency table for --split-images images.
--chrf measures the same for chrF: ``val_batch_stats`` without and with ``chrf=`` (alternating rounds, hipEvents), the host clock of
``metrics.chrf`` on the same tokens (already on the host as lists), and the build of the ``VocabChars``.  The synthetic vocabulary is
spelled with pseudo-words of 1..12 letters (5 on average, about an English caption's), drawn from a seed.
    python tools/bench_evaluate.py [--beams 5 20] [--batches 4] [--images 128] [--repeats 5] [--precision bf16] [--json]
    python tools/bench_evaluate.py --cider [--split-images 5000] [--batches 4] [--images 128] [--repeats 5] [--json]
--mbr measures consensus reranking (``rescore_method="MBR"``) at beam 5 and beam 20: the per-batch time of ``val_batch_stats`` with
``"LN"`` (today's path) and with ``"MBR"`` at rewards (1, 0) and (0.5, 0.5) in alternating rounds (hipEvents), the three new launches
on their own on one batch's search buffers, and the host clock of ``metrics.consensus_utilities`` on the same hypotheses.
    python tools/bench_evaluate.py --chrf [--batches 4] [--images 128] [--repeats 5] [--json]
    python tools/bench_evaluate.py --mbr [--beams 5 20] [--split-images 5000] [--batches 4] [--images 128] [--repeats 5] [--json]
--diversity measures the beam-diversity statistics (``with_diversity=True``) at beam 5 and beam 20: the per-batch time of
``evaluation.evaluate`` without and with the flag in alternating rounds (hipEvents), the work it replaces -- one batch's finished
hypotheses copied to the host, rebuilt as lists and put through ``metrics.diversity_stats`` (host clock, with and without the copy) --
and ``sat_caption_diversity`` alone (20 launches between two hipEvents) on that batch's hypotheses and, once, on 128 synthetic images
at the limits: 32 hypotheses of 128 tokens over 5 words (every sort at its full 4096 pairs).
    python tools/bench_evaluate.py --diversity [--beams 5 20] [--batches 4] [--images 128] [--repeats 5] [--json]
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
from sat_amd import metrics  # noqa: E402
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


def bench_cider(a, model, batches, hp, T, R):
    """--cider: val_batch_stats without / with corpus, the host scorer on the same tokens, the table build"""
    kw = dict(beamk=5, max_gen_length=a.max_gen_length, temperature=1.0, rescore_method="LN")
    n_chunks = max(1, a.split_images // a.images)
    split = [bench.synthetic_batch(a.images, R, T, hp["vocab_size"], 500 + i, ragged=True, px=8)[1:] for i in range(n_chunks)]
    split = [(c.cuda(), l.cuda()) for c, l in split]
    positions = sum(E.ReferenceCorpus.positions(l) for _, l in split)

    def build():
        rc = E.ReferenceCorpus(hp["vocab_size"], expected_positions=positions)
        for c, l in split:
            rc.add(c, l)
        return rc

    build().check()                                      # warm-up: code objects, allocator
    build_ms = [event_ms(build)[0] for _ in range(a.repeats)]
    rc = build().check()

    def plain():
        return E.evaluate(model, batches, **kw)

    def with_corpus():
        return E.evaluate(model, batches, corpus=rc, **kw)

    def host():
        out = []
        for img, caps, lengths in batches:
            tok, ln, _, _ = model.caption_tokens(img, **kw)
            hyps = [t[:n] for t, n in zip(tok.tolist(), ln.tolist())]
            refs = [[c[1:n] for c, n in zip(cs, ns)] for cs, ns in zip(caps.tolist(), lengths.tolist())]
            t0 = time.perf_counter()
            df = host.df
            c = metrics.cider_d(refs, hyps, df=df, n_images=rc.images)
            r = [metrics.rouge_l(rf, h) for rf, h in zip(refs, hyps)]
            out.append(((time.perf_counter() - t0) * 1e3, sum(c) / len(c), sum(r) / len(r)))
        return out

    host.df = rc.to_dict()
    plain(); got = with_corpus(); want = host()
    torch.cuda.synchronize()
    ms = {"plain": [], "corpus": []}
    for _ in range(a.repeats):                           # alternating rounds
        ms["plain"].append(event_ms(plain)[0] / a.batches)
        ms["corpus"].append(event_ms(with_corpus)[0] / a.batches)
    host_ms = [statistics.median(t for t, _, _ in host()) for _ in range(a.repeats)]
    res = dict(beamk=5, images=a.images, references=R, batches=a.batches, repeats=a.repeats, precision=a.precision, split_images=rc.images,
               table_capacity=rc.capacity, distinct_ngrams=len(host.df),
               val_batch_stats_ms_per_batch=dict(median=statistics.median(ms["plain"]), min=min(ms["plain"]), max=max(ms["plain"])),
               val_batch_stats_corpus_ms_per_batch=dict(median=statistics.median(ms["corpus"]), min=min(ms["corpus"]), max=max(ms["corpus"])),
               host_cider_rouge_ms_per_batch=dict(median=statistics.median(host_ms), min=min(host_ms), max=max(host_ms)),
               table_build_ms=dict(median=statistics.median(build_ms), min=min(build_ms), max=max(build_ms)),
               cider_device=got["batch_mean"]["cider"], cider_host=sum(c for _, c, _ in want) / len(want),
               rouge_l_device=got["batch_mean"]["rouge_l"], rouge_l_host=sum(r for _, _, r in want) / len(want))
    if a.json:
        print(json.dumps(res))
        return
    print("beam 5, %d batches of %d images x %d references, %s; corpus of %d images, %d distinct n-grams in %d slots" %
          (a.batches, a.images, R, a.precision, rc.images, len(host.df), rc.capacity))
    for name, key in (("val_batch_stats", "val_batch_stats_ms_per_batch"), ("val_batch_stats(corpus=)", "val_batch_stats_corpus_ms_per_batch"),
                      ("host cider_d + rouge_l (tokens already on the host)", "host_cider_rouge_ms_per_batch"), ("table build, once per split", "table_build_ms")):
        print("  %-52s %8.3f ms (min %.3f, max %.3f)" % (name, res[key]["median"], res[key]["min"], res[key]["max"]))
    print("  CIDEr-D device %.12f host %.12f; ROUGE-L device %.12f host %.12f" %
          (res["cider_device"], res["cider_host"], res["rouge_l_device"], res["rouge_l_host"]))


def synthetic_spelling(model, seed=7):
    """gives every id of the synthetic vocabulary a pseudo-word: 1..12 lower-case letters, 5 on average, from ``seed``"""
    import numpy as np
    rs = np.random.RandomState(seed)
    itos = dict(model.hp.vocab_itos)
    for i in range(model.hp.vocab_size):
        if i not in itos:
            itos[i] = "".join(chr(97 + c) for c in rs.randint(0, 26, size=int(np.clip(rs.poisson(4.0) + 1, 1, 12))))
    model.hp.vocab_itos = itos


def bench_chrf(a, model, batches, hp, T, R):
    """--chrf: val_batch_stats without / with chrf, the host scorer on the same tokens, the VocabChars build"""
    kw = dict(beamk=5, max_gen_length=a.max_gen_length, temperature=1.0, rescore_method="LN")
    synthetic_spelling(model)
    E.VocabChars.from_model(model)                       # warm-up
    build_ms = [clock_ms(lambda: E.VocabChars.from_model(model))[0] for _ in range(a.repeats)]
    chars = E.VocabChars.from_model(model)

    def plain():
        return E.evaluate(model, batches, **kw)

    def with_chrf():
        return E.evaluate(model, batches, chrf=chars, **kw)

    def host():
        out = []
        for img, caps, lengths in batches:
            tok, ln, _, _ = model.caption_tokens(img, **kw)
            hyps = [model.decode_seq(t[:n]) for t, n in zip(tok.tolist(), ln.tolist())]
            refs = [[model.decode_seq(c[1:n]) for c, n in zip(cs, ns)] for cs, ns in zip(caps.tolist(), lengths.tolist())]
            t0 = time.perf_counter()
            c = metrics.corpus_chrf(refs, hyps)
            out.append(((time.perf_counter() - t0) * 1e3, c, sum(len(metrics.chrf_text(h)) for h in hyps) / len(hyps)))
        return out

    plain(); got = with_chrf(); want = host()
    torch.cuda.synchronize()
    ms = {"plain": [], "chrf": []}
    for _ in range(a.repeats):                           # alternating rounds
        ms["plain"].append(event_ms(plain)[0] / a.batches)
        ms["chrf"].append(event_ms(with_chrf)[0] / a.batches)
    host_ms = [statistics.median(t for t, _, _ in host()) for _ in range(a.repeats)]
    spread = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    res = dict(beamk=5, images=a.images, references=R, batches=a.batches, repeats=a.repeats, precision=a.precision, vocab_size=chars.vocab_size,
               vocab_characters=int(chars.word_chars.numel()), max_word_chars=chars.max_word_chars,
               hypothesis_characters_mean=sum(n for _, _, n in want) / len(want),
               val_batch_stats_ms_per_batch=spread(ms["plain"]), val_batch_stats_chrf_ms_per_batch=spread(ms["chrf"]),
               host_chrf_ms_per_batch=spread(host_ms), vocab_chars_build_ms=spread(build_ms),
               chrf_device=got["batch_mean"]["chrf"], chrf_host=sum(c for _, c, _ in want) / len(want))
    if a.json:
        print(json.dumps(res))
        return
    print("beam 5, %d batches of %d images x %d references, %s; %d words spelled with %d characters, hypotheses of %.1f characters on average" %
          (a.batches, a.images, R, a.precision, chars.vocab_size, res["vocab_characters"], res["hypothesis_characters_mean"]))
    for name, key in (("val_batch_stats", "val_batch_stats_ms_per_batch"), ("val_batch_stats(chrf=)", "val_batch_stats_chrf_ms_per_batch"),
                      ("host metrics.chrf (words already on the host)", "host_chrf_ms_per_batch"), ("VocabChars build, once per model", "vocab_chars_build_ms")):
        print("  %-52s %8.3f ms (min %.3f, max %.3f)" % (name, res[key]["median"], res[key]["min"], res[key]["max"]))
    print("  chrF device %.12f host %.12f" % (res["chrf_device"], res["chrf_host"]))


def bench_mbr(a, model, batches, hp, T, R):
    """--mbr: val_batch_stats with "LN" and with "MBR", the three launches alone, the host specification on the same hypotheses"""
    n_chunks = max(1, a.split_images // a.images)
    rc = E.ReferenceCorpus(hp["vocab_size"], expected_positions=n_chunks * a.images * R * 4 * T)
    for i in range(n_chunks):
        caps, lengths = bench.synthetic_batch(a.images, R, T, hp["vocab_size"], 500 + i, ragged=True, px=8)[1:]
        rc.add(caps.cuda(), lengths.cuda())
    rc.check()
    df = rc.to_dict()
    spread = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    rewards = {"mbr_cider": (1.0, 0.0), "mbr_mixed": (0.5, 0.5)}
    for beamk in a.beams:
        kw = dict(beamk=beamk, max_gen_length=a.max_gen_length, temperature=1.0)
        paths = {"ln": lambda: E.evaluate(model, batches, rescore_method="LN", **kw)}
        for name, reward in rewards.items():
            paths[name] = (lambda reward: lambda: E.evaluate(model, batches, rescore_method="MBR", mbr_corpus=rc, mbr_reward=reward, **kw))(reward)
        for fn in paths.values():                        # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):                       # alternating rounds
            for k, fn in paths.items():
                ms[k].append(event_ms(fn)[0] / a.batches)
        # the three launches alone, on the buffers one batch's search leaves
        with torch.no_grad():
            ann, _ = model.encode(batches[0][0])
            o = model._beam_search_device(ann.contiguous(), beamk, a.max_gen_length, 1.0, "beam", 3, None, None, None, None, False)
        launches = {"hypotheses": [], "mbr_cider": [], "mbr_mixed": [], "select_at": []}
        sel = E.select_hypotheses(o, model.pad_idx, "MBR", mbr_corpus=rc)
        for _ in range(a.repeats + 1):                   # the first round warms up
            t, (ht, hl) = event_ms(lambda: E.finished_hypotheses(o, model.pad_idx)); launches["hypotheses"].append(t)
            for name, reward in rewards.items():
                launches[name].append(event_ms(lambda: E.consensus_utilities(ht, hl, o["fin_count"], o["fin_score"], rc, reward, 0.0))[0])
            launches["select_at"].append(event_ms(lambda: E.select_hypotheses(o, model.pad_idx, "MBR", mbr_corpus=rc))[0])
        launches = {k: v[1:] for k, v in launches.items()}
        launches["select_at"] = [max(0.0, t - h - c) for t, h, c in zip(launches["select_at"], launches["hypotheses"], launches["mbr_cider"])]
        # the host specification on the same hypotheses (already on the host as lists: the read-back is not counted)
        tok, ln, cnt, lp = ht.cpu().tolist(), hl.cpu().tolist(), o["fin_count"].cpu().tolist(), o["fin_score"].cpu().tolist()
        hyps = [[tok[b][f][:ln[b][f]] for f in range(cnt[b])] for b in range(len(cnt))]
        host = {}
        for name, reward in rewards.items():
            t0 = time.perf_counter()
            us = [metrics.consensus_utilities(h, s[:len(h)], df, rc.images, reward, 0.0) for h, s in zip(hyps, lp)]
            host[name] = (time.perf_counter() - t0) * 1e3
        dev = E.consensus_utilities(ht, hl, o["fin_count"], o["fin_score"], rc, rewards["mbr_mixed"], 0.0)[0].cpu().tolist()
        worst = max([abs(g - w) for gu, wu in zip(dev, us) for g, w in zip(gu, wu)] or [0.0])
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = dict(beamk=beamk, images=a.images, references=R, batches=a.batches, max_gen_length=a.max_gen_length, precision=a.precision, repeats=a.repeats,
                   corpus_images=rc.images, val_batch_stats_ms_per_batch={k: spread(v) for k, v in ms.items()},
                   mbr_increment_ms={k: med[k] - med["ln"] for k in rewards}, mbr_ratio_to_ln={k: med[k] / med["ln"] for k in rewards},
                   launches_ms={k: spread(v) for k, v in launches.items()}, host_consensus_utilities_ms_per_batch=host,
                   finished_hypotheses_mean=sum(cnt) / len(cnt), worst_device_minus_host=worst, winners_not_first_finished=int((sel["winner"] != 0).sum()))
        if a.json:
            print(json.dumps(res))
            continue
        print("beam %d, %d batches of %d images x %d references, max_gen_length %d, %s; corpus of %d images; %.1f finished hypotheses per image" %
              (beamk, a.batches, a.images, R, a.max_gen_length, a.precision, rc.images, res["finished_hypotheses_mean"]))
        for k, label in (("ln", 'val_batch_stats(rescore_method="LN")'), ("mbr_cider", '"MBR", reward (1, 0)'), ("mbr_mixed", '"MBR", reward (0.5, 0.5)')):
            extra = "" if k == "ln" else "   %+.3f ms, %.3fx of LN" % (res["mbr_increment_ms"][k], res["mbr_ratio_to_ln"][k])
            print("  %-40s %8.3f ms per batch (min %.3f, max %.3f)%s" % (label, med[k], min(ms[k]), max(ms[k]), extra))
        for k, label in (("hypotheses", "sat_beam_hypotheses"), ("mbr_cider", "sat_caption_mbr (1, 0)"), ("mbr_mixed", "sat_caption_mbr (0.5, 0.5)"),
                         ("select_at", "sat_beam_select_at (by difference)")):
            v = res["launches_ms"][k]
            print("  %-40s %8.3f ms (min %.3f, max %.3f)" % (label, v["median"], v["min"], v["max"]))
        print("  host metrics.consensus_utilities: %.1f ms (1, 0), %.1f ms (0.5, 0.5) per batch; worst |device - host| %.2e" %
              (host["mbr_cider"], host["mbr_mixed"], worst))


def bench_diversity(a, model, batches, hp, T, R):
    """--diversity: evaluate without / with the flag, the host specification on the same hypotheses, the kernel alone"""
    import numpy as np
    spread = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))

    def kernel_ms(ht, hl, cnt, launches=20):
        def run():
            for _ in range(launches):
                E.diversity_statistics(ht, hl, cnt)
        run()
        return spread([event_ms(run)[0] / launches for _ in range(a.repeats)])

    rs = np.random.RandomState(3)
    lim_tok = torch.from_numpy(rs.randint(0, 5, size=(a.images, 32, 128)).astype(np.int32)).cuda()
    lim_len = torch.full((a.images, 32), 128, dtype=torch.int32, device="cuda")
    lim_cnt = torch.full((a.images,), 32, dtype=torch.int32, device="cuda")
    limits = kernel_ms(lim_tok, lim_len, lim_cnt)
    for beamk in a.beams:
        kw = dict(beamk=beamk, max_gen_length=a.max_gen_length, temperature=1.0, rescore_method="LN")
        paths = {"off": lambda: E.evaluate(model, batches, **kw), "on": lambda: E.evaluate(model, batches, with_diversity=True, **kw)}
        for fn in paths.values():                        # warm-up: code objects, allocator
            fn()
        got = paths["on"]()["diversity"]
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(a.repeats):                       # alternating rounds
            for k, fn in paths.items():
                ms[k].append(event_ms(fn)[0] / a.batches)
        with torch.no_grad():
            ann, _ = model.encode(batches[0][0])
            o = model._beam_search_device(ann.contiguous(), beamk, a.max_gen_length, 1.0, "beam", 3, None, None, None, None, False)
        ht, hl = E.finished_hypotheses(o, model.pad_idx)
        alone = kernel_ms(ht, hl, o["fin_count"])

        def host():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tok, ln, cnt = ht.cpu().tolist(), hl.cpu().tolist(), o["fin_count"].cpu().tolist()
            hyps = [[tok[b][f][:ln[b][f]] for f in range(cnt[b])] for b in range(len(cnt))]
            t1 = time.perf_counter()
            rows = [metrics.diversity_stats(h) for h in hyps]
            t2 = time.perf_counter()
            return (t2 - t0) * 1e3, (t2 - t1) * 1e3, rows, cnt

        host_ms = [host() for _ in range(a.repeats)]
        rows, cnt = host_ms[0][2], host_ms[0][3]
        equal = E.diversity_statistics(ht, hl, o["fin_count"]).cpu().tolist() == rows
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = dict(beamk=beamk, images=a.images, references=R, batches=a.batches, max_gen_length=a.max_gen_length, precision=a.precision, repeats=a.repeats,
                   evaluate_ms_per_batch={k: spread(v) for k, v in ms.items()}, increment_ms=med["on"] - med["off"], ratio=med["on"] / med["off"],
                   host_copy_rebuild_stats_ms_per_batch=spread([t for t, _, _, _ in host_ms]), host_stats_only_ms_per_batch=spread([t for _, t, _, _ in host_ms]),
                   kernel_ms=alone, kernel_at_limits_ms=limits, finished_hypotheses_mean=sum(cnt) / len(cnt), device_equals_host=equal, diversity=got)
        if a.json:
            print(json.dumps(res))
            continue
        print("beam %d, %d batches of %d images x %d references, max_gen_length %d, %s; %.1f finished hypotheses per image" %
              (beamk, a.batches, a.images, R, a.max_gen_length, a.precision, res["finished_hypotheses_mean"]))
        for k, label in (("off", "evaluate"), ("on", "evaluate(with_diversity=True)")):
            extra = "" if k == "off" else "   %+.3f ms, %.4fx" % (res["increment_ms"], res["ratio"])
            print("  %-44s %8.3f ms per batch (min %.3f, max %.3f)%s" % (label, med[k], min(ms[k]), max(ms[k]), extra))
        for key, label in (("host_copy_rebuild_stats_ms_per_batch", "host: copy + lists + metrics.diversity_stats"), ("host_stats_only_ms_per_batch", "host: metrics.diversity_stats alone"),
                           ("kernel_ms", "sat_caption_diversity, K = %d, width = %d" % (beamk, a.max_gen_length + 1)),
                           ("kernel_at_limits_ms", "sat_caption_diversity, K = 32, width = 128")):
            v = res[key]
            print("  %-44s %8.3f ms (min %.3f, max %.3f)" % (label, v["median"], v["min"], v["max"]))
        print("  device == host: %s; %s" % (equal, ", ".join("%s %s" % (k, ("%.4f" % v) if isinstance(v, float) else v) for k, v in got.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, nargs="+", default=[5, 20])
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--max-gen-length", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--cider", action="store_true", help="measure CIDEr-D / ROUGE-L: val_batch_stats with and without corpus=, the host scorer, the build")
    ap.add_argument("--chrf", action="store_true", help="measure chrF: val_batch_stats with and without chrf=, the host scorer, the VocabChars build")
    ap.add_argument("--mbr", action="store_true", help="measure consensus reranking: val_batch_stats with LN and with MBR, the three launches, the host")
    ap.add_argument("--diversity", action="store_true", help="measure the beam-diversity statistics: evaluate with and without with_diversity, the host, the kernel alone")
    ap.add_argument("--split-images", type=int, default=5000, help="--cider / --mbr: images in the corpus the table is built from")
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
    if a.cider:
        return bench_cider(a, model, batches, hp, T, R)
    if a.chrf:
        return bench_chrf(a, model, batches, hp, T, R)
    if a.mbr:
        return bench_mbr(a, model, batches, hp, T, R)
    if a.diversity:
        return bench_diversity(a, model, batches, hp, T, R)
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
