"""The reference's evaluate.ipynb as a command (dev/todo.txt: "new eval script"): checkpoint + dataset json in, a table of decode
parameters and metrics out.  Without --trials: one pass over the split at the given decode parameters, printing the notebook's mean
of per-batch metrics and the corpus-level score of the whole split.  With --trials N: the notebook's random search (N draws from its
parameter ranges, each scored over the first --max-batches batches), written as csv with its 13 columns plus ``<metric>_corpus``.
--cider: CIDEr-D and ROUGE-L as well; the n-gram document frequencies of the evaluated split are built once on the device
(``evaluation.ReferenceCorpus``) and every batch and trial is scored against them (columns cider, rouge_l, cider_corpus, rouge_l_corpus).
--chrf [--chrf-beta 3.0]: chrF as well (character n-grams, n = 1..6, across word boundaries); the vocabulary's spelling is put on the
device once (``evaluation.VocabChars``) and every batch and trial is scored over it (columns chrf, chrf_corpus).  Combinable with --cider.
--rescore-method MBR [--mbr-split train --mbr-reward 1.0 0.0 --mbr-alpha 0.0]: consensus reranking of every beam; the document
frequencies come from the named split's references (one more ``ReferenceCorpus``, built once).  With --trials, "MBR" joins the
notebook's rescore methods.
--diversity: how different the finished hypotheses of an image are, over the whole split: distinct-1..4, mBLEU-1..4, the share of
unique hypotheses, their number and the vocabulary the selected captions use (``evaluation.DiversityStats``; one pass only, not with
--trials); printed, and written under "diversity" in --out.
All work is in sat_amd/evaluation.py: a batch is decoded and scored on the device, one host read per pass.
    python tools/evaluate.py CHECKPOINT [--json DATASET.json] [--root IMAGE_DIR] [--split test] [--batch N] [--max-batches M]
                             [--trials N --seed S --out results.csv]  [--cider]  [--chrf --chrf-beta 3.0]  [--diversity]  [--beamk 5 --temperature 1.0 --rescore-method LN ...]
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import data as D  # noqa: E402
from sat_amd import evaluation as E  # noqa: E402
from sat_amd.model import SAT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--json", default=None, help="dataset json; default: the one recorded in the checkpoint's hyper-parameters")
    ap.add_argument("--root", default=None, help="directory the json's relative image paths start from")
    ap.add_argument("--split", default="test")
    ap.add_argument("--batch", type=int, default=None, help="default: the checkpoint's training batch size, as the notebook")
    ap.add_argument("--max-batches", type=int, default=None, help="default: the whole split (4 with --trials, as the notebook)")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--trials", type=int, default=0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--out", default=None, help="csv (with --trials) or json (without) to write")
    ap.add_argument("--cider", action="store_true", help="also CIDEr-D and ROUGE-L against the document frequencies of the evaluated split")
    ap.add_argument("--chrf", action="store_true", help="also chrF over the characters of the vocabulary's spelling")
    ap.add_argument("--chrf-beta", type=float, default=3.0, help="chrF: the weight of recall over precision")
    ap.add_argument("--diversity", action="store_true", help="also distinct-n, mBLEU, unique hypotheses and vocabulary over every finished hypothesis of the split")
    ap.add_argument("--beamk", type=int, default=5)
    ap.add_argument("--max-gen-length", type=int, default=32)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--sample-method", default="beam", choices=["beam", "multinomial", "topk", "nucleus", "ancestral"])
    ap.add_argument("--sample-topk", type=int, default=3)
    ap.add_argument("--sample-topp", type=float, default=0.9, help="nucleus sampling: the share of the probability mass the candidates of a hypothesis carry, (0, 1]")
    ap.add_argument("--decoder-noise", type=float, default=0.0)
    ap.add_argument("--rescore-method", default="LN", choices=["NONE", "LN", "WR", "BAR", "MBR"])
    ap.add_argument("--rescore-reward", type=float, default=0.5)
    ap.add_argument("--mbr-split", default="train", help="MBR: the split whose references give the document frequencies")
    ap.add_argument("--mbr-reward", type=float, nargs=2, default=[1.0, 0.0], metavar=("W_CIDER", "W_ROUGE"), help="MBR: the weights of CIDEr-D and ROUGE-L in the gain")
    ap.add_argument("--mbr-alpha", type=float, default=0.0, help="MBR: a hypothesis votes with exp(alpha * (its raw score - the best)); 0 = uniform")
    ap.add_argument("--topg", type=int, default=None, help="top-g clipping: only the G best words of every hypothesis are candidates (beam sampling)")
    ap.add_argument("--no-unk", action="store_true", help="never emit <UNK>")
    ap.add_argument("--no-repeat-ngram", type=int, default=None, help="no n-gram of this size is said twice in a caption (0 / unset = off)")
    ap.add_argument("--min-length", type=int, default=None, help="<END> stays masked until a caption has this many words")
    ap.add_argument("--repetition-penalty", type=float, default=None, help="CTRL's penalty on the logits of the words already said (1.0 = off)")
    ap.add_argument("--beam-groups", type=int, default=None, help="diverse beam search: split the beam into this many groups (a divisor of --beamk; beam sampling)")
    ap.add_argument("--diversity-penalty", type=float, default=0.5, help="what a group pays per hypothesis an earlier group kept with the same word at a step")
    ap.add_argument("--ensemble", nargs="+", default=None, metavar="CKPT", help="ensemble decoding: further checkpoints over the same vocabulary; one search over all of them (beam sampling)")
    ap.add_argument("--ensemble-weights", type=float, nargs="+", default=None, help="one weight per model, CHECKPOINT first (default: uniform; normalised to sum 1)")
    ap.add_argument("--ensemble-combine", default="arithmetic", choices=["arithmetic", "geometric"], help="mix the models' distributions, or multiply them")
    a = ap.parse_args()
    if a.diversity and a.trials > 0:
        ap.error("--diversity goes with one pass over the split, not with --trials (the random search's table has no diversity columns)")

    ckpt = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    model = SAT(**dict(ckpt["hyper_parameters"]))
    model.load_state_dict(ckpt["state_dict"])
    model = model.cuda()
    if a.ensemble:
        from sat_amd.ensemble import Ensemble
        model = Ensemble([model] + Ensemble.from_checkpoints(a.ensemble).models, a.ensemble_weights, a.ensemble_combine)
    ds = D.CocoCaptionDataset(a.json or model.hparams.json, a.split, root=a.root)
    loader = D.DeviceLoader(ds, a.batch or model.hparams.batch, D.BatchTransform(model.hparams.input_size, train=False), workers=a.workers)
    corpus = E.ReferenceCorpus.from_dataset(ds).check() if a.cider else None
    chars = E.VocabChars.from_model(model) if a.chrf else None
    mbr = {}
    if a.rescore_method == "MBR":
        mbr_ds = ds if a.mbr_split == a.split else D.CocoCaptionDataset(a.json or model.hparams.json, a.mbr_split, root=a.root)
        mbr = dict(mbr_corpus=corpus if (corpus is not None and mbr_ds is ds) else E.ReferenceCorpus.from_dataset(mbr_ds).check(),
                   mbr_reward=tuple(a.mbr_reward), mbr_alpha=a.mbr_alpha)
    shown = E.HEADERS + (list(E.CONSENSUS_KEYS) if a.cider else []) + (list(E.CHRF_KEYS) if a.chrf else [])
    if a.trials > 0:
        space = dict(E.NOTEBOOK_SPACE, rescore_methods=E.NOTEBOOK_SPACE["rescore_methods"] + ["MBR"]) if mbr else E.NOTEBOOK_SPACE
        rows = E.random_search(model, loader, a.trials, space=space, seed=a.seed, max_batches=a.max_batches or 4, corpus=corpus, chrf=chars,
                               chrf_beta=a.chrf_beta, **mbr)
        cols = list(rows[0])
        for r in sorted(rows, key=lambda r: -r["bleu4"]):
            print("  ".join("%s=%s" % (k, ("%.4f" % r[k]) if isinstance(r[k], float) else r[k]) for k in shown))
        if a.out:
            with open(a.out, "w", newline="") as f:
                w = csv.DictWriter(f, fieldnames=cols)
                w.writeheader(); w.writerows(rows)
        return
    res = E.evaluate(model, loader, max_batches=a.max_batches, seed=a.seed, corpus=corpus, with_diversity=a.diversity, **(dict(chrf=chars, chrf_beta=a.chrf_beta) if a.chrf else {}), beamk=a.beamk, max_gen_length=a.max_gen_length, temperature=a.temperature,
                     sample_method=a.sample_method, sample_topk=a.sample_topk, sample_topp=a.sample_topp, decoder_noise=a.decoder_noise,
                     rescore_method=None if a.rescore_method == "NONE" else a.rescore_method, rescore_reward=a.rescore_reward, topg=a.topg,
                     no_unk=a.no_unk, no_repeat_ngram=a.no_repeat_ngram, min_length=a.min_length, repetition_penalty=a.repetition_penalty,
                     beam_groups=a.beam_groups, diversity_penalty=a.diversity_penalty, **mbr)
    print("%d images in %d batches" % (res["images"], res["batches"]))
    for k in E.METRIC_KEYS + (E.CONSENSUS_KEYS if a.cider else ()) + (E.CHRF_KEYS if a.chrf else ()):
        print("%-18s batch mean %.6f   corpus %.6f" % (k, res["batch_mean"][k], res["corpus"][k]))
    if a.diversity:
        for k, v in res["diversity"].items():
            print("%-18s %s" % (k, ("%.6f" % v) if isinstance(v, float) else v))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
