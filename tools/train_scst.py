"""Self-critical fine-tuning of a trained captioner (the usual second training stage): checkpoint + dataset json in, a checkpoint
optimised for CIDEr-D (and / or ROUGE-L) out.  Every step samples --samples captions per picture from the model's own distribution,
scores them on the device against the document frequencies of the training split (``evaluation.ReferenceCorpus``, built once) and
back-propagates the advantage-weighted log-likelihood (``SAT.scst_step``; DESIGN.md 5, "Self-critical training").  The encoder stays
frozen unless --train-encoder; Adam with a constant --lr drives the parameters that train.
    python tools/train_scst.py CHECKPOINT --out TUNED.ckpt [--json DATASET.json] [--root IMAGE_DIR] [--steps 1000] [--samples 5]
                               [--baseline mean|greedy] [--reward-cider 1.0 --reward-rouge 0.0] [--max-gen-length 20] [--temperature 1.0]
                               [--batch N] [--lr 5e-5] [--seed S] [--log-every 20] [--train-encoder] [--ema-decay D]
--ema-decay D keeps an exponential moving average of the trained weights in the optimizer step (``FusedOptimizer(ema_decay=D)``; DESIGN.md 5,
"Averaged weights") and writes the AVERAGED weights into the checkpoint.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import data as D  # noqa: E402
from sat_amd import evaluation as E  # noqa: E402
from sat_amd.model import SAT  # noqa: E402
from sat_amd.optim import FusedOptimizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--out", required=True, help="where the fine-tuned checkpoint goes (same layout as the input)")
    ap.add_argument("--json", default=None, help="dataset json; default: the one recorded in the checkpoint's hyper-parameters")
    ap.add_argument("--root", default=None, help="directory the json's relative image paths start from")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--baseline", default="mean", choices=["mean", "greedy"])
    ap.add_argument("--reward-cider", type=float, default=1.0)
    ap.add_argument("--reward-rouge", type=float, default=0.0)
    ap.add_argument("--max-gen-length", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None, help="default: the checkpoint's training batch size")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--seed", type=int, default=None, help="step i samples with seed + i")
    ap.add_argument("--log-every", type=int, default=20)
    ap.add_argument("--train-encoder", action="store_true")
    ap.add_argument("--ema-decay", type=float, default=0.0, help="in (0, 1): save the exponential moving average of the weights (0 = off)")
    a = ap.parse_args()

    ckpt = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    model = SAT(**dict(ckpt["hyper_parameters"]))
    model.load_state_dict(ckpt["state_dict"])
    model = model.cuda().train()
    for p in model.encoder.parameters():
        p.requires_grad = bool(a.train_encoder)
    ds = D.CocoCaptionDataset(a.json or model.hparams.json, "train", root=a.root)
    loader = D.DeviceLoader(ds, a.batch or model.hparams.batch, D.BatchTransform(model.hparams.input_size, train=True), shuffle=True, workers=a.workers,
                            drop_last=True)
    corpus = E.ReferenceCorpus.from_dataset(ds).check()
    trained = [p for p in model.parameters() if p.requires_grad]
    opt = FusedOptimizer(trained, kind="adam", lr=a.lr, ema_decay=a.ema_decay) if a.ema_decay else torch.optim.Adam(trained, lr=a.lr)
    step, logs = 0, []
    while step < a.steps:
        for batch in loader:
            opt.zero_grad(set_to_none=True)
            out = model.scst_step(batch, corpus, samples=a.samples, baseline=a.baseline, reward=(a.reward_cider, a.reward_rouge),
                                  max_gen_length=a.max_gen_length, temperature=a.temperature, seed=None if a.seed is None else a.seed + step)
            out["loss"].backward()
            opt.step()
            logs.append(torch.stack([out[k].detach().float() for k in ("loss", "reward", "baseline_reward", "advantage_abs", "sample_length")]))
            step += 1
            if step % a.log_every == 0 or step == a.steps:       # one host read per log line
                m = torch.stack(logs).mean(0).tolist(); logs = []
                print("step %6d  loss %+.5f  reward %.4f  baseline %.4f  |advantage| %.4f  words %.2f" % (step, *m), flush=True)
            if step >= a.steps:
                break
    if a.ema_decay:         # the averaged weights go into the checkpoint: swap them in, save, swap back (BatchNorm buffers are the live ones)
        with opt.averaged_weights():
            ckpt["state_dict"] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    else:
        ckpt["state_dict"] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ckpt["scst"] = dict(steps=step, samples=a.samples, baseline=a.baseline, reward=(a.reward_cider, a.reward_rouge), max_gen_length=a.max_gen_length,
                        temperature=a.temperature, lr=a.lr, ema_decay=a.ema_decay)
    torch.save(ckpt, a.out)
    print("wrote %s%s" % (a.out, " (exponential moving average of the weights, decay %g)" % a.ema_decay if a.ema_decay else ""))


if __name__ == "__main__":
    main()
