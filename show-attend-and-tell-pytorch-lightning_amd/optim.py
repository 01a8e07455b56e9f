"""Multi-tensor optimizer step on the HIP library: the optimizers ``SAT.configure_optimizers`` builds
(reference model.py:723-757: SGD / Adam / AdamW over per-module parameter groups) and Lightning's gradient clipping
(train.py:93-96, 273-274: ``clip_grad_value_`` / ``clip_grad_norm_``) in one launch over every parameter tensor.

``FusedOptimizer`` is a ``torch.optim.Optimizer``: ``param_groups`` (so the reference's LR schedulers drive it unchanged)
and the per-parameter ``state`` keys of torch's own optimizers (``step``, ``exp_avg``, ``exp_avg_sq`` /
``momentum_buffer``), so optimizer checkpoints stay interchangeable.

Averaged weights are taken in the same launch (``sat_optimizer_step_avg``): ``kind="asgd"`` is ``torch.optim.ASGD`` (state ``step``,
``eta``, ``mu``, ``ax``; ``start_averaging()`` is the NT-ASGD switch, ``NonMonotonicTrigger`` its criterion) and ``ema_decay=d`` keeps
an exponential moving average ``ema`` beside SGD / Adam / AdamW.  ``swap_averaged()`` / ``averaged_weights()`` put the average into
the parameters and back.  Only parameters are averaged: BatchNorm's running statistics are the live ones, as with
``torch.optim.swa_utils.AveragedModel(use_buffers=False)``."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L

KINDS = {"sgd": 0, "adam": 1, "adamw": 2, "asgd": 3}


def asgd_coefficients(lr, lambd, alpha, t0, step):
    """``(eta, mu)`` as ``torch.optim.ASGD`` stores them after step ``step`` (1-based) and uses them in step ``step + 1``: python double
    arithmetic rounded once to float32.  ``lr`` is the group's learning rate at that moment, so a scheduler acts one step late."""
    lr, step = float(lr), float(step)
    eta = lr / ((1 + lambd * lr * step) ** alpha)
    mu = 1 / max(1, step - t0)
    return float(np.float32(eta)), float(np.float32(mu))


class NonMonotonicTrigger:
    """The non-monotonic criterion of NT-ASGD (Merity et al. 2017, Alg. 1) on a logged validation metric: ``update(v)`` appends ``v``
    and returns True the first time ``len(log) > n`` and ``v`` is worse than the best of ``log[:-n-1]`` (the checks made at least ``n``
    checks ago).  ``mode="max"`` for metrics that grow (bleu4 and the other monitors), ``"min"`` for a loss.  Fires once."""

    def __init__(self, n=5, mode="max"):
        if mode not in ("max", "min") or int(n) < 0:
            raise ValueError("NonMonotonicTrigger(n=%r, mode=%r)" % (n, mode))
        self.n, self.mode, self.log, self.fired = int(n), mode, [], False

    def update(self, value):
        self.log.append(float(value))
        if self.fired or len(self.log) <= self.n:
            return False
        past = self.log[:-self.n - 1]
        if not past:
            return False
        worse = self.log[-1] < max(past) if self.mode == "max" else self.log[-1] > min(past)
        self.fired = bool(worse)
        return self.fired


def _same_layout(a, b):
    """same memory order: equal strides on every dimension that has more than one element (size-1 dimensions of a
    channels_last 1x1 filter carry arbitrary strides)"""
    return a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


class FusedOptimizer(torch.optim.Optimizer):
    def __init__(self, params, kind="adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.0, nesterov=False,
                 grad_clip=None, clip_value=0.0, lambd=1e-4, alpha=0.75, t0=1e6, ema_decay=0.0):
        if kind not in KINDS:
            raise ValueError("kind=%r (sgd / adam / adamw / asgd)" % (kind,))
        if kind == "adamw" and weight_decay == 0.0:
            weight_decay = 1e-2                        # torch.optim.AdamW's default for groups that do not set it
        ema_decay = float(ema_decay or 0.0)
        if ema_decay != 0.0 and not 0.0 < ema_decay < 1.0:
            raise ValueError("ema_decay=%r is not in (0, 1)" % (ema_decay,))
        if lambd < 0.0:
            raise ValueError("lambd=%r is negative" % (lambd,))
        if kind == "asgd":
            # torch.optim.ASGD's groups (momentum / nesterov / betas / eps have no meaning for it), so that its state_dict() loads here
            if ema_decay:
                raise ValueError("kind='asgd' keeps its own average (ax): ema_decay cannot be combined with it")
            defaults = dict(lr=lr, lambd=lambd, alpha=alpha, t0=t0, weight_decay=weight_decay)
        else:
            defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov)
        super().__init__(params, defaults)
        self.kind = kind
        self.ema_decay = ema_decay
        self._avg_name = "ax" if kind == "asgd" else ("ema" if ema_decay else None)      # state key of the averaged weights
        self._swapped = False
        self.set_clipping(grad_clip, clip_value)
        self._chunks = None
        self._sig = None
        self.last_grad_norm = None                     # device scalar after a step with norm clipping

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._fast_key = None                          # the state tensors were replaced: rebuild the pointer table on the next step

    def set_clipping(self, algorithm, value):
        """train.py:93-96: ``--grad_clip value|norm`` with ``--clip_value`` (0 = off)."""
        if algorithm not in (None, "value", "norm"):
            raise ValueError("grad_clip=%r" % (algorithm,))
        self.grad_clip, self.clip_value = (algorithm, float(value)) if value and value > 0 else (None, 0.0)

    def _tables(self, entries, dev):
        sig = tuple((p.data_ptr(), p.numel()) for p, _ in entries)
        if sig != self._sig:
            ce = L.lib().sat_optimizer_chunk_elems()
            rows = [(ti, 0, s) for ti, (p, _) in enumerate(entries) for s in range(0, p.numel(), ce)]
            arr = np.array(rows, dtype=[("tensor", np.int32), ("reserved", np.int32), ("start", np.int64)])
            self._chunks = torch.from_numpy(arr.view(np.uint8).copy()).to(dev)
            self._n_chunks = len(rows)
            # The pointer table is rebuilt on the host every step and uploaded asynchronously.  The host may run a step or more
            # ahead of the GPU, so a pinned table must not be rewritten before its previous upload has executed: a small ring
            # of pinned tables, each with the event of its last upload (and no upload at all while the table is unchanged).
            nbytes = len(entries) * C.sizeof(L.OptTensor)
            self._avg_off = nbytes
            if self._avg_name is not None:             # one address of averaged weights per tensor, behind the table: one block, one upload
                nbytes += len(entries) * C.sizeof(C.c_void_p)
            self._ring = [[torch.empty(nbytes, dtype=torch.uint8).pin_memory(), None] for _ in range(3)]
            self._ring_pos = 0
            self._uploaded = None
            self._dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._scratch = torch.empty(self._n_chunks, dtype=torch.float64, device=dev)
            self._coef = torch.ones(2, dtype=torch.float32, device=dev)
            self._sig = sig
        return self._chunks

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        host = self._host_step()
        if host is None:
            return loss
        g0, beta1, beta2, step, chunks, avg_coef = host
        return self._launch(L.lib(), g0, beta1, beta2, step, chunks, loss, avg_coef)

    # ---- the step in two halves for a replayed launch (graph.GraphedTrainStep): everything the host does - step counters, the pointer /
    # learning-rate table and its upload, the hyper-parameters of this step written to DEVICE memory - and the kernel launches, which read
    # nothing but device memory and can therefore sit in a captured graph
    @torch.no_grad()
    def step_host(self):
        host = self._host_step()
        if host is None:
            raise RuntimeError("FusedOptimizer.step_host: no parameter has a gradient")
        g0, beta1, beta2, step, _, avg_coef = host
        hyper = self._hyper(g0, beta1, beta2, step)
        dev = self._dev.device
        self.prepare_device_step(dev)
        self._hyper_pos = (self._hyper_pos + 1) % len(self._hyper_ring)
        slot = self._hyper_ring[self._hyper_pos]
        if slot[1] is not None:
            slot[1].synchronize()                      # the upload that last read this pinned block has executed (the host may run steps ahead)
        C.memmove(slot[0].data_ptr(), C.addressof(hyper), C.sizeof(L.OptHyper))
        if avg_coef is None:
            self._hyper_dev.copy_(slot[0], non_blocking=True)
        else:                                          # the averaging coefficient of this step follows the hyper-parameters in the pinned block
            n = C.sizeof(L.OptHyper)
            avg = self._avg_hyper(g0, avg_coef)
            C.memmove(slot[0].data_ptr() + n, C.addressof(avg), C.sizeof(L.OptAvgHyper))
            self._hyper_dev.copy_(slot[0][:n], non_blocking=True)
            self._avg_hyper_dev.copy_(slot[0][n:], non_blocking=True)
        ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(dev)); slot[1] = ev

    def step_device(self):
        """the launches of one step (gradient-norm coefficient when clipping by norm, the update), hyper-parameters from device memory"""
        lib = L.lib()
        if getattr(self, "_hyper_dev", None) is None:
            raise RuntimeError("FusedOptimizer.step_device before step_host")
        coef = None
        if self.grad_clip == "norm":
            L.check(lib.sat_grad_clip_coef(L.ptr(self._dev), L.ptr(self._chunks), self._n_chunks, self.clip_value, L.ptr(self._scratch),
                                           L.ptr(self._coef), L.stream_ptr()), "sat_grad_clip_coef")
            coef = self._coef
            self.last_grad_norm = self._coef[1]
        if self._avg_name is not None:
            L.check(lib.sat_optimizer_step_avg_dev(L.ptr(self._dev), self._dev.data_ptr() + self._avg_off, L.ptr(self._chunks), self._n_chunks,
                                                   L.ptr(self._hyper_dev), L.ptr(self._avg_hyper_dev), L.ptr(coef), L.stream_ptr()),
                    "sat_optimizer_step_avg_dev")
            return
        L.check(lib.sat_optimizer_step_dev(L.ptr(self._dev), L.ptr(self._chunks), self._n_chunks, L.ptr(self._hyper_dev), L.ptr(coef), L.stream_ptr()),
                "sat_optimizer_step_dev")

    def prepare_device_step(self, dev):
        """device / pinned blocks of the hyper-parameters (allocated once, before a capture)"""
        if getattr(self, "_hyper_dev", None) is None or self._hyper_dev.device != dev:
            n = C.sizeof(L.OptHyper)
            self._hyper_dev = torch.zeros(n, dtype=torch.uint8, device=dev)
            if self._avg_name is not None:
                self._avg_hyper_dev = torch.zeros(C.sizeof(L.OptAvgHyper), dtype=torch.uint8, device=dev)
                n += C.sizeof(L.OptAvgHyper)
            self._hyper_ring = [[torch.empty(n, dtype=torch.uint8).pin_memory(), None] for _ in range(4)]
            self._hyper_pos = 0

    def table_signature(self):
        """what ``_tables`` keys the chunk / pointer tables by, for the parameters that hold a gradient now"""
        return tuple((p.data_ptr(), p.numel()) for g in self.param_groups for p in g["params"] if p.grad is not None)

    def device_buffers(self):
        """addresses a captured ``step_device`` has baked in (graph.py re-captures when they move)"""
        bufs = (self._dev, self._chunks, self._scratch, self._coef, self._hyper_dev)
        if self._avg_name is not None:
            bufs += (self._avg_hyper_dev,)             # the averaged-state addresses live in self._dev, behind the table
        return tuple(t.data_ptr() for t in bufs)

    def _host_step(self):
        lib = L.lib()
        entries = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    entries.append((p, group))
        if not entries:
            return None
        L.require_gpu(*[p for p, _ in entries])
        dev = entries[0][0].device
        if self._swapped:
            raise RuntimeError("FusedOptimizer: the averaged weights are swapped into the parameters (swap_averaged): swap back before stepping")
        g0 = self.param_groups[0]
        asgd, avg_name = self.kind == "asgd", self._avg_name
        if asgd:
            beta1 = beta2 = 0.0
            for g in self.param_groups:
                if g["lambd"] != g0["lambd"] or g["t0"] != g0["t0"]:
                    raise ValueError("FusedOptimizer: lambd and t0 must be the same in every group (lr, alpha and weight_decay may differ)")
                if g["lambd"] < 0:
                    raise ValueError("FusedOptimizer: lambd=%r is negative" % (g["lambd"],))
        else:
            beta1, beta2 = g0["betas"]
            for g in self.param_groups:
                if tuple(g["betas"]) != (beta1, beta2) or g["eps"] != g0["eps"] or g["momentum"] != g0["momentum"] or g["nesterov"] != g0["nesterov"]:
                    raise ValueError("FusedOptimizer: betas / eps / momentum / nesterov must be the same in every group (lr and weight_decay may differ)")
        # Fast path: the same tensors, gradient addresses, learning rates and weight decays as the step before - the table on the device is
        # current, nothing to rebuild or upload (the per-parameter loop below is ~1.2 ms of host time at C2, 2.5 ms for resnet101, and C1 / C3
        # are host-bound).  Gradients living in persistent buckets (dist.GradSync) or reallocated at the same addresses hit it every step.
        # Everything the table on the device points at is part of the key: the bf16 filter copies (remade by encoder.py whenever a parameter
        # changed behind the optimizer's back - load_state_dict, broadcast, clamping - or created later by set_precision) and the state
        # tensors (replaced by anything but this class's load_state_dict) would otherwise be written through stale addresses.
        state = self.state
        mv_key = []
        for p, _ in entries:
            st = state.get(p)
            if not st or (avg_name is not None and avg_name not in st):      # an average that starts now (a checkpoint saved without one)
                mv_key = None
                break
            if self.kind == "sgd":
                m = st.get("momentum_buffer"); mv_key.append(0 if m is None else m.data_ptr())
            elif not asgd:
                mv_key.append(st["exp_avg"].data_ptr()); mv_key.append(st["exp_avg_sq"].data_ptr())
            if avg_name is not None:
                mv_key.append(st[avg_name].data_ptr())
        shadows = [getattr(p, "_sat_bf16_shadow", None) for p, _ in entries]
        # ASGD: the step size in the table is the eta stored after the step before (one per group; with lambd == 0 and a constant lr it never
        # moves and the table stays; with lambd > 0 it changes every step and every step takes the slow path)
        rates = (getattr(self, "_asgd_etas", None), tuple([g["weight_decay"] for g in self.param_groups])) if asgd else \
            tuple([(g["lr"], g["weight_decay"]) for g in self.param_groups])
        fast_key = (tuple([p.grad.data_ptr() for p, _ in entries]), rates,
                    tuple([p.data_ptr() for p, _ in entries]), tuple([0 if s is None else s.data_ptr() for s in shadows]),
                    None if mv_key is None else tuple(mv_key))
        if mv_key is not None and fast_key == getattr(self, "_fast_key", None) and self._fast_ok:
            self.fast_path_steps = getattr(self, "fast_path_steps", 0) + 1
            self._fast_steps += 1                      # every state["step"] is a view of this one tensor (see below)
            step = float(self._fast_steps[0])
            for q in self._fast_shadowed:
                q._sat_shadow_version = q._version
            return g0, beta1, beta2, step, self._chunks, self._avg_coef(step)
        chunks = self._tables(entries, dev)
        self._ring_pos = (self._ring_pos + 1) % len(self._ring)
        slot = self._ring[self._ring_pos]
        if slot[1] is not None:
            slot[1].synchronize()                      # the upload that last read this pinned table has executed
        host = slot[0]
        table = (L.OptTensor * len(entries)).from_buffer(host.numpy())
        avg_table = None if avg_name is None else (C.c_void_p * len(entries)).from_buffer(host.numpy(), self._avg_off)
        steps = []          # the per-parameter step counters (torch's state layout), advanced together below
        etas, mus = [], []  # ASGD: what torch keeps per parameter as 0-dim tensors (on the device after a loaded checkpoint: read once, here)
        for i, (p, group) in enumerate(entries):
            dense = p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))      # KRSC filters
            if p.dtype != torch.float32 or not dense:
                raise ValueError("FusedOptimizer: parameters must be dense fp32 (contiguous or channels_last)")
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                if self.kind == "sgd":
                    st["momentum_buffer"] = torch.zeros_like(p) if group["momentum"] != 0 else None
                elif asgd:
                    st["eta"] = torch.tensor(float(group["lr"]), dtype=torch.float32); st["mu"] = torch.tensor(1.0)
                    st["ax"] = torch.zeros_like(p)     # mu == 1 until step t0: the kernel stores p itself
                else:
                    st["exp_avg"] = torch.zeros_like(p); st["exp_avg_sq"] = torch.zeros_like(p)
            if avg_name == "ema" and "ema" not in st:
                st["ema"] = p.detach().clone()         # starts at the current weights, also in a run resumed from a checkpoint without it
            steps.append(st["step"])
            grad = p.grad if _same_layout(p.grad, p) else torch.empty_like(p).copy_(p.grad)     # element i of g <-> element i of p
            m = st.get("momentum_buffer") if self.kind == "sgd" else (None if asgd else st["exp_avg"])
            v = None if self.kind == "sgd" or asgd else st["exp_avg_sq"]
            t = table[i]
            t.p = p.data_ptr(); t.g = grad.data_ptr(); t.m = 0 if m is None else m.data_ptr(); t.v = 0 if v is None else v.data_ptr()
            t.n = p.numel(); t.lr = float(group["lr"]); t.weight_decay = float(group["weight_decay"])
            if asgd:
                etas.append(float(st["eta"])); mus.append(float(st["mu"]))
                t.lr = etas[-1]
            if avg_name is not None:
                a = st[avg_name]
                if a.dtype != torch.float32 or a.device != p.device:
                    raise ValueError("FusedOptimizer: state[%r] must be fp32 on the parameter's device" % avg_name)
                if not _same_layout(a, p):             # element i of the average <-> element i of p
                    a = st[avg_name] = torch.empty_like(p).copy_(a)
                avg_table[i] = a.data_ptr()
            sh = getattr(p, "_sat_bf16_shadow", None)      # bf16 filter copy of the encoder (encoder.py): kept current by this step
            t.shadow_bf16 = sh.data_ptr() if (sh is not None and _same_layout(sh, p)) else 0
            if t.shadow_bf16:
                p._sat_shadow_version = p._version
            entries[i] = (p, group, grad)              # keep a re-laid-out gradient alive until the launch
        # torch's state layout keeps one 0-dim "step" tensor per parameter; here they are views of ONE host tensor, so the fast path advances all
        # of them with a single add (a foreach add over ~170 host scalars was 0.4 ms a step).  state_dict() / load_state_dict() see ordinary
        # 0-dim tensors; after a load the addresses in the fast key change and this path re-gathers them.
        sv = torch.stack(steps) + 1
        step = float(sv[0])
        if float(sv.min()) != float(sv.max()):
            raise ValueError("FusedOptimizer: parameters are at different step counts %s" % sorted(set((sv - 1).tolist())))
        for i, (p, _, _) in enumerate(entries):
            self.state[p]["step"] = sv[i]
        steps = sv
        if asgd:
            if min(mus) != max(mus):
                raise ValueError("FusedOptimizer: parameters hold different averaging coefficients mu %s" % sorted(set(mus)))
            # like "step": views of one host tensor each, rewritten in place after every step (_avg_coef)
            self._asgd_eta_t, self._asgd_mu_t = torch.tensor(etas, dtype=torch.float32), torch.tensor(mus, dtype=torch.float32)
            for i, (p, _, _) in enumerate(entries):
                self.state[p]["eta"], self.state[p]["mu"] = self._asgd_eta_t[i], self._asgd_mu_t[i]
            index = {id(g): gi for gi, g in enumerate(self.param_groups)}
            self._asgd_entry_group = [index[id(e[1])] for e in entries]
            self._asgd_etas, self._asgd_mu = tuple(etas), mus[0]
            fast_key = fast_key[:1] + ((self._asgd_etas, fast_key[1][1]),) + fast_key[2:]      # the step sizes this table holds
        raw = host.numpy().tobytes()
        if raw != self._uploaded:                      # pointers / lr / weight decay changed since the table on the device was written
            self._dev.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            slot[1] = ev
            self._uploaded = raw
        # the fast path may take over when every gradient was used where it lies (no re-laid-out copy whose address would be stale)
        if mv_key is None:          # first step: the state tensors were created above
            mv = []
            for p, _, _ in entries:
                st = state[p]
                if self.kind == "sgd":
                    m = st.get("momentum_buffer"); mv.append(0 if m is None else m.data_ptr())
                elif not asgd:
                    mv.append(st["exp_avg"].data_ptr()); mv.append(st["exp_avg_sq"].data_ptr())
                if avg_name is not None:
                    mv.append(st[avg_name].data_ptr())
            fast_key = fast_key[:4] + (tuple(mv),)
        self._fast_key, self._fast_steps = fast_key, steps
        self._fast_ok = all(e[2] is e[0].grad for e in entries)
        self._fast_shadowed = [e[0] for i, e in enumerate(entries) if table[i].shadow_bf16]      # only the copies the kernel really rewrites
        return g0, beta1, beta2, step, chunks, self._avg_coef(step)

    def _avg_coef(self, step):
        """the averaging coefficient of step ``step`` (None without averaging).  ASGD: the mu stored after the step before; the eta / mu
        that torch stores after this step are computed here and written into the state (``asgd_coefficients``)."""
        if self._avg_name is None:
            return None
        if self.kind != "asgd":
            return 1.0 if step == 1 else 1.0 - self.ema_decay          # the average starts as a copy (AveragedModel does the same)
        mu = self._asgd_mu
        new = [asgd_coefficients(g["lr"], g["lambd"], g["alpha"], g["t0"], step) for g in self.param_groups]
        self._asgd_etas = tuple([new[gi][0] for gi in self._asgd_entry_group])
        self._asgd_eta_t.copy_(torch.tensor(self._asgd_etas, dtype=torch.float32))
        self._asgd_mu = new[0][1]                      # t0 is the same in every group
        self._asgd_mu_t.fill_(self._asgd_mu)
        return mu

    def _avg_hyper(self, g0, coef):
        if not 0.0 <= coef <= 1.0:
            raise ValueError("FusedOptimizer: averaging coefficient %r outside [0, 1]" % (coef,))
        return L.OptAvgHyper(coef=coef, lambd=float(g0["lambd"]) if self.kind == "asgd" else 0.0, flags=0, reserved=0)

    def start_averaging(self):
        """The NT-ASGD switch: every group's ``t0`` becomes the current step count, so by torch's rule ``mu = 1 / max(1, k - t0)`` the
        average, which has tracked the weights so far, is the running mean of the iterates from the next step on."""
        steps = [float(st["step"]) for st in self.state.values() if "step" in st]
        k = max(steps) if steps else 0.0
        for g in self.param_groups:
            g["t0"] = k
        return k

    @torch.no_grad()
    def swap_averaged(self):
        """Exchange every parameter with its averaged weights (``ax`` / ``ema``) on the device, in one launch; a second call restores every
        bit.  Parameters that were never stepped (a frozen encoder) have no average and are left alone.  The encoder's bf16 filter copies
        are rewritten from the weights that now sit in the parameters and marked current, as ``step`` does: the kernel writes through raw
        pointers, so nothing else would notice.  BatchNorm buffers are not averaged: they stay the live ones
        (``AveragedModel(use_buffers=False)``)."""
        name = self._avg_name
        if name is None:
            raise RuntimeError("FusedOptimizer: no averaged weights are kept (kind='asgd' or ema_decay=)")
        pairs = [(p, self.state[p][name]) for g in self.param_groups for p in g["params"] if name in (self.state.get(p) or {})]
        if not pairs:
            raise RuntimeError("FusedOptimizer.swap_averaged before the first step: there are no averaged weights yet")
        L.require_gpu(*[t for pair in pairs for t in pair])
        dev = pairs[0][0].device
        ce = L.lib().sat_optimizer_chunk_elems()
        table = (L.OptTensor * len(pairs))()
        avg = (C.c_void_p * len(pairs))()
        shadowed = []
        for i, (p, a) in enumerate(pairs):
            if a.dtype != torch.float32 or p.dtype != torch.float32 or a.device != dev or p.device != dev or not _same_layout(a, p):
                raise ValueError("FusedOptimizer.swap_averaged: state[%r] must be fp32 in the layout and on the device of its parameter" % name)
            sh = getattr(p, "_sat_bf16_shadow", None)
            table[i].p, table[i].n = p.data_ptr(), p.numel()
            table[i].shadow_bf16 = sh.data_ptr() if (sh is not None and sh.device == dev and _same_layout(sh, p)) else 0
            avg[i] = a.data_ptr()
            if table[i].shadow_bf16:
                shadowed.append(p)
            elif sh is not None:
                p._sat_shadow_version = -1             # a copy this kernel cannot rewrite in place: the encoder remakes it
        rows = [(ti, 0, s) for ti, (p, _) in enumerate(pairs) for s in range(0, p.numel(), ce)]
        chunks = np.array(rows, dtype=[("tensor", np.int32), ("reserved", np.int32), ("start", np.int64)])
        blocks = [torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to(dev) for b in (table, avg, chunks.tobytes())]
        L.check(L.lib().sat_optimizer_swap(L.ptr(blocks[0]), L.ptr(blocks[1]), L.ptr(blocks[2]), len(rows), L.stream_ptr()), "sat_optimizer_swap")
        self._swap_blocks = blocks                     # read by the launch: alive until the next swap
        for p in shadowed:
            p._sat_shadow_version = p._version
        self._swapped = not self._swapped
        return self._swapped

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with opt.averaged_weights():`` evaluate / save with the averaged weights in the parameters; swapped back on the way out, also on
        an exception.  Stepping inside raises."""
        self.swap_averaged()
        try:
            yield self
        finally:
            self.swap_averaged()

    def _hyper(self, g0, beta1, beta2, step):
        if self.kind == "asgd":
            return L.OptHyper(kind=KINDS["asgd"], first_step=int(step == 1), clip_value=self.clip_value if self.grad_clip == "value" else 0.0)
        return L.OptHyper(kind=KINDS[self.kind], nesterov=int(bool(g0["nesterov"])), first_step=int(step == 1), beta1=beta1, beta2=beta2,
                          eps=g0["eps"], bias_correction1=1.0 - beta1 ** step, bias_correction2_sqrt=math.sqrt(1.0 - beta2 ** step),
                          momentum=float(g0["momentum"]), clip_value=self.clip_value if self.grad_clip == "value" else 0.0)

    def _launch(self, lib, g0, beta1, beta2, step, chunks, loss, avg_coef=None):
        coef = None
        if self.grad_clip == "norm":
            L.check(lib.sat_grad_clip_coef(L.ptr(self._dev), L.ptr(chunks), self._n_chunks, self.clip_value, L.ptr(self._scratch),
                                           L.ptr(self._coef), L.stream_ptr()), "sat_grad_clip_coef")
            coef = self._coef
            self.last_grad_norm = self._coef[1]
        hyper = self._hyper(g0, beta1, beta2, step)
        if avg_coef is not None:                       # the same launch with the average taken in the pass (8 more bytes per element)
            avg = self._avg_hyper(g0, avg_coef)
            L.check(lib.sat_optimizer_step_avg(L.ptr(self._dev), self._dev.data_ptr() + self._avg_off, L.ptr(chunks), self._n_chunks, C.byref(hyper),
                                               C.byref(avg), L.ptr(coef), L.stream_ptr()), "sat_optimizer_step_avg")
            return loss
        L.check(lib.sat_optimizer_step(L.ptr(self._dev), L.ptr(chunks), self._n_chunks, C.byref(hyper), L.ptr(coef), L.stream_ptr()),
                "sat_optimizer_step")
        return loss
