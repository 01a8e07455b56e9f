"""The reference's temperature_scaling.py as a command: checkpoint + dataset json in, fitted temperature and its trace out.

Loads the checkpoint (Lightning layout: ``hyper_parameters`` + ``state_dict``), runs the frozen model teacher-forced over the
first 42 validation batches of 16 pictures (Resize + CenterCrop to the model's input size, no shuffling), and fits T with the
reference's constants.  All work is in sat_amd/calibration.py; pass the result as ``temperature=`` to ``caption()`` / ``val_batch()``.
    python tools/temperature_scaling.py CHECKPOINT [--json DATASET.json] [--root IMAGE_DIR] [--batch 16] [--max-batches 42] [--out FIT.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402,F401
from sat_amd import data as D  # noqa: E402
from sat_amd.model import SAT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--json", default=None, help="dataset json; default: the one recorded in the checkpoint's hyper-parameters")
    ap.add_argument("--root", default=None, help="directory the json's relative image paths start from")
    ap.add_argument("--split", default="val")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--max-batches", type=int, default=42)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--init", type=float, default=1.5)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--momentum", type=float, default=0.8)
    ap.add_argument("--no-nesterov", action="store_true")
    ap.add_argument("--iters", type=int, default=70)
    ap.add_argument("--out", default=None, help="write {temperature, trace, losses} as json")
    a = ap.parse_args()

    ckpt = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    model = SAT(**dict(ckpt["hyper_parameters"]))
    model.load_state_dict(ckpt["state_dict"])
    model = model.cuda()
    ds = D.CocoCaptionDataset(a.json or model.hparams.json, a.split, root=a.root)
    loader = D.DeviceLoader(ds, a.batch, D.BatchTransform(model.hparams.input_size, train=False), workers=a.workers)
    fit = model.calibrate_temperature(loader, max_batches=a.max_batches, init=a.init, lr=a.lr, momentum=a.momentum,
                                      nesterov=not a.no_nesterov, iters=a.iters)
    for k, (t, loss) in enumerate(zip(fit.trace.tolist(), fit.losses.tolist())):
        print("step %3d  temperature %.6f  loss %.6f" % (k, t, loss))
    print("temperature = %.6f" % fit.temperature)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(temperature=fit.temperature, trace=fit.trace.tolist(), losses=fit.losses.tolist()), f)


if __name__ == "__main__":
    main()
