"""Distil one or several trained captioners into one student: student checkpoint + teacher checkpoints + dataset json in, a student
checkpoint out that decodes at single-model cost.  Every step teacher-forces the teachers (frozen, eval mode) and the student on the same
captions and back-propagates ``(1 - alpha) * cross entropy + alpha * tau^2 * KL(teachers || student)`` (``SAT.distill_step``; DESIGN.md 5,
"Distillation").  --targets teacher trains on the teachers' own best beam caption of every picture instead of the references
(sequence-level distillation).  The student may have another encoder or other sizes than the teachers; the vocabulary is shared.  The
student's encoder stays frozen unless --train-encoder; Adam with a constant --lr drives the parameters that train.
    python tools/train_distill.py STUDENT.ckpt --teacher A.ckpt [B.ckpt ...] --out DISTILLED.ckpt [--weights 1 1 ...]
                                  [--combine arithmetic|geometric] [--alpha 0.5] [--temperature 2.0] [--targets references|teacher]
                                  [--beamk 3] [--max-gen-length 20] [--json DATASET.json] [--root IMAGE_DIR] [--steps 1000] [--batch N]
                                  [--lr 1e-4] [--log-every 20] [--train-encoder] [--ema-decay D]
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
from sat_amd import distill  # noqa: E402
from sat_amd.ensemble import Ensemble  # noqa: E402
from sat_amd.model import SAT  # noqa: E402
from sat_amd.optim import FusedOptimizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint", help="the student: a trained or freshly initialised SAT checkpoint")
    ap.add_argument("--teacher", nargs="+", required=True, help="one or more teacher checkpoints (one vocabulary, the student's)")
    ap.add_argument("--weights", type=float, nargs="+", default=None, help="one weight per teacher (normalised to sum 1); default: equal")
    ap.add_argument("--combine", default="arithmetic", choices=["arithmetic", "geometric"])
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--targets", default="references", choices=list(distill.TARGETS))
    ap.add_argument("--beamk", type=int, default=3)
    ap.add_argument("--max-gen-length", type=int, default=20)
    ap.add_argument("--out", required=True, help="where the distilled checkpoint goes (same layout as the input)")
    ap.add_argument("--json", default=None, help="dataset json; default: the one recorded in the student's hyper-parameters")
    ap.add_argument("--root", default=None, help="directory the json's relative image paths start from")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=None, help="default: the student's training batch size")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-4)
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
    teacher = Ensemble.from_checkpoints(a.teacher, a.weights, a.combine, device="cuda")
    for m in teacher.models:
        m.eval()
        for p in m.parameters():
            p.requires_grad = False
    distill.check_step_args(model, teacher, a.alpha, a.temperature, a.targets, a.beamk, a.max_gen_length)      # refuse before the data is read
    ds = D.CocoCaptionDataset(a.json or model.hparams.json, "train", root=a.root)
    loader = D.DeviceLoader(ds, a.batch or model.hparams.batch, D.BatchTransform(model.hparams.input_size, train=True), shuffle=True, workers=a.workers,
                            drop_last=True)
    trained = [p for p in model.parameters() if p.requires_grad]
    opt = FusedOptimizer(trained, kind="adam", lr=a.lr, ema_decay=a.ema_decay) if a.ema_decay else torch.optim.Adam(trained, lr=a.lr)
    step, logs = 0, []
    while step < a.steps:
        for batch in loader:
            opt.zero_grad(set_to_none=True)
            out = model.distill_step(batch, teacher, alpha=a.alpha, temperature=a.temperature, targets=a.targets, beamk=a.beamk,
                                     max_gen_length=a.max_gen_length)
            out["loss"].backward()
            opt.step()
            logs.append(torch.stack([out[k].detach().float() for k in ("loss", "hard", "soft", "accuracy")]))
            step += 1
            if step % a.log_every == 0 or step == a.steps:       # one host read per log line
                m = torch.stack(logs).mean(0).tolist(); logs = []
                print("step %6d  loss %.5f  cross entropy %.5f  KL %.5f  accuracy %.4f" % (step, *m), flush=True)
            if step >= a.steps:
                break
    if a.ema_decay:         # the averaged weights go into the checkpoint: swap them in, save, swap back (BatchNorm buffers are the live ones)
        with opt.averaged_weights():
            ckpt["state_dict"] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    else:
        ckpt["state_dict"] = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ckpt["distill"] = dict(steps=step, teachers=list(a.teacher), weights=teacher.weights, combine=a.combine, alpha=a.alpha, temperature=a.temperature,
                           targets=a.targets, beamk=a.beamk, max_gen_length=a.max_gen_length, lr=a.lr, ema_decay=a.ema_decay)
    torch.save(ckpt, a.out)
    print("wrote %s%s" % (a.out, " (exponential moving average of the weights, decay %g)" % a.ema_decay if a.ema_decay else ""))


if __name__ == "__main__":
    main()
