"""The reference's visualize.ipynb as a command: checkpoint + dataset json in, one ``<image name>_result.jpg`` per picture out (the
picture, one attention overlay per predicted word, "Total Attention", under a title block with the references and the prediction).
The pictures are decoded, squared, captioned and rendered on the device in batches (sat_amd/visualize.py); the host only lays the
panels out with Pillow.
    python tools/visualize.py CHECKPOINT [--json DATASET.json] [--root IMAGE_DIR] [--split test] (--idx I [I ...] | --count N [--seed S])
                              --out DIR [--batch 32] [--visual-size 256] [--input-size 224] [--beamk 3 --temperature 1.0
                              --sample-method beam --sample-topk 3 --decoder-noise 0.0 --rescore-method LN --rescore-reward 1.0]
                              [--rescore-method MBR --mbr-split train --mbr-reward 1.0 0.0 --mbr-alpha 0.0]   consensus reranking: the caption
                              that agrees most with the rest of its beam; document frequencies from the named split's references
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import data as D  # noqa: E402
from sat_amd import visualize as Z  # noqa: E402
from sat_amd.model import SAT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--json", default=None, help="dataset json; default: the one recorded in the checkpoint's hyper-parameters")
    ap.add_argument("--root", default=None, help="directory the json's relative image paths start from")
    ap.add_argument("--split", default="test")
    ap.add_argument("--idx", type=int, nargs="+", default=None, help="indices into the split")
    ap.add_argument("--count", type=int, default=None, help="instead of --idx: this many random pictures (np.random.randint, as the notebook)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--visual-size", type=int, default=256)
    ap.add_argument("--input-size", type=int, default=None, help="default: the checkpoint's input_size")
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--beamk", type=int, default=3)
    ap.add_argument("--max-gen-length", type=int, default=32)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--sample-method", default="beam", choices=["beam", "multinomial", "topk", "nucleus"])
    ap.add_argument("--sample-topk", type=int, default=3)
    ap.add_argument("--sample-topp", type=float, default=0.9, help="nucleus sampling: the share of the probability mass the candidates of a hypothesis carry, (0, 1]")
    ap.add_argument("--decoder-noise", type=float, default=0.0)
    ap.add_argument("--rescore-method", default="LN", choices=["NONE", "LN", "WR", "BAR", "MBR"])
    ap.add_argument("--rescore-reward", type=float, default=1.0)
    ap.add_argument("--mbr-split", default="train", help="MBR: the split whose references give the document frequencies")
    ap.add_argument("--mbr-reward", type=float, nargs=2, default=[1.0, 0.0], metavar=("W_CIDER", "W_ROUGE"), help="MBR: the weights of CIDEr-D and ROUGE-L in the gain")
    ap.add_argument("--mbr-alpha", type=float, default=0.0, help="MBR: a hypothesis votes with exp(alpha * (its raw score - the best)); 0 = uniform")
    ap.add_argument("--progressive", action="store_true", help="decode progressive JPEG files on the GPU as well (default: Pillow decodes them)")
    ap.add_argument("--topg", type=int, default=None, help="top-g clipping: only the G best words of every hypothesis are candidates (beam sampling)")
    ap.add_argument("--prefix", default=None, help='words every caption starts with, e.g. "a photo of" (each must be in the vocabulary)')
    ap.add_argument("--no-unk", action="store_true", help="never emit <UNK>")
    ap.add_argument("--no-repeat-ngram", type=int, default=None, help="no n-gram of this size is said twice in a caption (0 / unset = off)")
    ap.add_argument("--min-length", type=int, default=None, help="<END> stays masked until a caption has this many words")
    ap.add_argument("--repetition-penalty", type=float, default=None, help="CTRL's penalty on the logits of the words already said (1.0 = off)")
    ap.add_argument("--beam-groups", type=int, default=None, help="diverse beam search: split the beam into this many groups (a divisor of --beamk; beam sampling)")
    ap.add_argument("--diversity-penalty", type=float, default=0.5, help="what a group pays per hypothesis an earlier group kept with the same word at a step")
    ap.add_argument("--required", default=None, help='words every caption must contain, e.g. "dog frisbee" (the same for every picture; beam sampling)')
    ap.add_argument("--ensemble", nargs="+", default=None, metavar="CKPT", help="ensemble decoding: further checkpoints over the same vocabulary; one search over all of them (beam sampling)")
    ap.add_argument("--ensemble-weights", type=float, nargs="+", default=None, help="one weight per model, CHECKPOINT first (default: uniform; normalised to sum 1)")
    ap.add_argument("--ensemble-combine", default="arithmetic", choices=["arithmetic", "geometric"], help="mix the models' distributions, or multiply them")
    a = ap.parse_args()
    if (a.idx is None) == (a.count is None):
        ap.error("give either --idx or --count")

    ckpt = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    model = SAT(**dict(ckpt["hyper_parameters"]))
    model.load_state_dict(ckpt["state_dict"])
    model = model.cuda()
    if a.ensemble:
        from sat_amd.ensemble import Ensemble
        model = Ensemble([model] + Ensemble.from_checkpoints(a.ensemble).models, a.ensemble_weights, a.ensemble_combine)
    ds = D.CocoCaptionDataset(a.json or model.hparams.json, a.split, root=a.root)
    mbr = {}
    if a.rescore_method == "MBR":
        from sat_amd import evaluation as E
        mbr_ds = ds if a.mbr_split == a.split else D.CocoCaptionDataset(a.json or model.hparams.json, a.mbr_split, root=a.root)
        mbr = dict(mbr_corpus=E.ReferenceCorpus.from_dataset(mbr_ds).check(), mbr_reward=tuple(a.mbr_reward), mbr_alpha=a.mbr_alpha)
    idx = a.idx if a.idx is not None else np.random.RandomState(a.seed).randint(0, len(ds), a.count).tolist()
    os.makedirs(a.out, exist_ok=True)
    for start in range(0, len(idx), a.batch):
        chunk = idx[start:start + a.batch]
        paths = [ds.img_paths[i] if a.root is None or os.path.isabs(ds.img_paths[i]) else os.path.join(a.root, ds.img_paths[i]) for i in chunk]
        vis = model.visualize(paths, beamk=a.beamk, max_gen_length=a.max_gen_length, temperature=a.temperature, sample_method=a.sample_method,
                              sample_topk=a.sample_topk, sample_topp=a.sample_topp, decoder_noise=a.decoder_noise, rescore_method=None if a.rescore_method == "NONE" else a.rescore_method,
                              rescore_reward=a.rescore_reward, visual_size=a.visual_size, input_size=a.input_size, seed=a.seed, progressive=a.progressive,
                              topg=a.topg, prefix=a.prefix, no_unk=a.no_unk, no_repeat_ngram=a.no_repeat_ngram, min_length=a.min_length,
                              repetition_penalty=a.repetition_penalty, beam_groups=a.beam_groups, diversity_penalty=a.diversity_penalty, required=a.required, **mbr)
        for j, i in enumerate(chunk):
            refs = [" ".join(ds.itos(t) for t in c[1:n]) for c, n in zip(ds.encoded_captions[i], ds.lengths[i])]
            name = os.path.join(a.out, "%s_result.jpg" % vis.names[j])
            Z.contact_sheet(vis, j, references=refs, columns=a.columns).save(name)
            print("idx = %d  %s  (s=%.2f, p=%.2f) : %s" % (i, name, vis.scores[j], vis.perplexities[j], " ".join(vis.words[j])))


if __name__ == "__main__":
    main()
