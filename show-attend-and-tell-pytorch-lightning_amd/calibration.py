"""Temperature-scaling calibration: the reference's ``temperature_scaling.py`` on the fused HIP loss/gradient kernels.

The reference runs the frozen model teacher-forced over validation batches, keeps every packed logit row and fits one scalar
``T`` by 70 Nesterov-SGD steps on ``F.cross_entropy(logits / T, targets)`` (temperature_scaling.py:29-59).  The fitted value is
what ``caption(temperature=...)`` / ``val_batch(temperature=...)`` take.  Here every iteration is one streaming read of the
logits (csrc/temperature.hip): nothing of the logits' size is written, ``T`` stays on the device until the fit is over.

Python is plumbing only: shapes, device memory, the stream.  There is no CPU path.
"""
import math
from collections import namedtuple

import torch
from torch.nn.utils.rnn import PackedSequence

from . import _lib as L

#: most temperatures one pass of ``nll_at`` evaluates (SAT_TEMPERATURE_MAX of include/sat_hip.h); longer lists go in chunks
MAX_TEMPERATURES = 8

#: ``temperature``: the fitted T (float); ``trace``: T before every step and after the last (iters + 1 values, trace[0] == init);
#: ``losses``: the loss at trace[k] (iters values)
TemperatureFit = namedtuple("TemperatureFit", ["temperature", "trace", "losses"])


def _rows(logits, targets):
    """(P, V) fp32 logits and (P,) int32 targets on the GPU, from the PackedSequence pair of ``train_batch`` or plain tensors."""
    if isinstance(logits, PackedSequence):
        logits = logits.data
    if isinstance(targets, PackedSequence):
        targets = targets.data
    L.require_gpu(logits, targets)
    if logits.dim() != 2 or targets.dim() != 1 or targets.shape[0] != logits.shape[0] or logits.shape[0] == 0 or logits.shape[1] == 0:
        raise ValueError("expected logits (P, V) and targets (P,), got %s and %s" % (tuple(logits.shape), tuple(targets.shape)))
    if targets.is_floating_point():
        raise ValueError("targets must be class indices, got %s" % targets.dtype)
    logits = logits.detach().to(torch.float32).contiguous()
    V = logits.shape[1]
    lo, hi = int(targets.min()), int(targets.max())
    if lo < 0 or hi >= V:
        raise ValueError("targets outside [0, %d): min %d, max %d" % (V, lo, hi))
    return logits, targets.detach().to(device=logits.device, dtype=torch.int32).contiguous()


def _workspace(lib, P, V, device):
    nbytes = lib.sat_temperature_workspace_bytes(P, V)
    if nbytes == 0:
        raise L.SatHipError("sat_temperature_workspace_bytes: %s" % lib.sat_last_error().decode(errors="replace"))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def nll_at(logits, targets, temperatures):
    """``(loss, dloss_dT)`` of ``F.cross_entropy(logits / T, targets)`` at every T of ``temperatures``: two fp32 tensors of
    ``len(temperatures)`` on the logits' device.  Up to 8 temperatures share one read of the logits."""
    lib = L.lib()
    logits, targets = _rows(logits, targets)
    temps = [float(t) for t in temperatures]
    if not temps or not all(t > 0.0 and math.isfinite(t) for t in temps):
        raise ValueError("temperatures must be positive finite numbers, got %r" % (temps,))
    P, V = logits.shape
    with torch.cuda.device(logits.device):
        ws = _workspace(lib, P, V, logits.device)
        t_dev = torch.tensor(temps, dtype=torch.float32, device=logits.device)
        loss, grad = torch.empty_like(t_dev), torch.empty_like(t_dev)
        for i in range(0, len(temps), MAX_TEMPERATURES):
            n = min(MAX_TEMPERATURES, len(temps) - i)
            L.check(lib.sat_temperature_nll(L.ptr(logits), L.ptr(targets), P, V, L.ptr(t_dev[i:]), n, L.ptr(loss[i:]), L.ptr(grad[i:]),
                                            L.ptr(ws), L.stream_ptr()), "sat_temperature_nll")
    return loss, grad


def fit_temperature(logits, targets, init=1.5, lr=1e-2, momentum=0.8, nesterov=True, iters=70):
    """temperature_scaling.py:51-59: ``iters`` steps of ``torch.optim.SGD([T], lr, momentum, nesterov)`` on
    ``F.cross_entropy(logits / T, targets)`` from ``T = init``; the defaults are the reference script's constants.

    Raises ``SatHipError`` if T becomes non-positive or non-finite on the way (a learning rate too large for these logits); the
    exception carries ``trace`` and ``losses`` as far as they got."""
    lib = L.lib()
    logits, targets = _rows(logits, targets)
    iters = int(iters)
    if nesterov and not momentum > 0:
        raise ValueError("Nesterov momentum requires a momentum (torch.optim.SGD)")
    P, V = logits.shape
    with torch.cuda.device(logits.device):
        ws = _workspace(lib, P, V, logits.device)
        t_trace = torch.empty(max(iters, 0) + 1, dtype=torch.float32, device=logits.device)
        loss_trace = torch.empty(max(iters, 1), dtype=torch.float32, device=logits.device)
        L.check(lib.sat_temperature_fit(L.ptr(logits), L.ptr(targets), P, V, float(init), float(lr), float(momentum), int(bool(nesterov)), iters,
                                        L.ptr(t_trace), L.ptr(loss_trace), L.ptr(ws), L.stream_ptr()), "sat_temperature_fit")
        trace, losses = t_trace.cpu(), loss_trace.cpu()          # the only time T visits the host
    bad = (~(torch.isfinite(trace) & (trace > 0))).nonzero()
    if bad.numel():
        k = int(bad[0])
        err = L.SatHipError("fit_temperature: T = %g after step %d (init=%g lr=%g momentum=%g): the fit was stopped there; use a smaller lr"
                            % (float(trace[k]), k, init, lr, momentum))
        err.trace, err.losses = trace, losses          # what was computed up to there, for the post-mortem
        raise err
    return TemperatureFit(float(trace[-1]), trace, losses)


def collect_logits(model, batches, max_batches=42):
    """temperature_scaling.py:29-48: ``train_batch(batch, epsilon=1)`` of the frozen model (eval mode, no_grad) over the first
    ``max_batches`` batches (the reference's ``if i > 40: break`` after the append keeps 42); packed rows concatenated in batch
    order.  The model's train/eval mode is restored on return."""
    device = next(model.parameters()).device
    was_training = model.training
    logits, targets = [], []
    model.eval()
    try:
        with torch.no_grad():
            for i, (img, caps, lengths) in enumerate(batches):
                if i >= max_batches:
                    break
                lp, tp, _ = model.train_batch((img.to(device), caps.to(device), lengths), epsilon=1)
                logits.append(lp.data)
                targets.append(tp.data)
    finally:
        model.train(was_training)
    if not logits:
        raise ValueError("collect_logits: no batches")
    return torch.cat(logits), torch.cat(targets)


def calibrate_temperature(model, batches, max_batches=42, **fit_kwargs):
    """``collect_logits`` then ``fit_temperature``: the whole of temperature_scaling.py.  Changes nothing in the model."""
    logits, targets = collect_logits(model, batches, max_batches)
    return fit_temperature(logits, targets, **fit_kwargs)
