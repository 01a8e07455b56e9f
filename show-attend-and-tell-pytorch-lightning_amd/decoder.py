"""Host side of the decoder hot path: packing plan, workspace and the
``torch.autograd.Function`` wrappers that hand raw device pointers to
``libsat_hip.so``.  Mirrors the decoder half of ``SAT.train_batch``
(reference model.py:487-557) and the loss lines model.py:592-597.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import encoder as E


def _upload(t, dev):
    if dev.type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


class PackPlan:
    """Index maps of ``pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)``
    (model.py:553-554) built once per batch on the host, as the reference does through
    ``lengths.tolist()``: batch order = ``torch.sort(lengths, descending=True)``, rows time-major.
    """

    def __init__(self, lengths, T, device):
        lens = torch.as_tensor(lengths, dtype=torch.int64, device="cpu").reshape(-1)
        self.N, self.T, self.T1 = lens.numel(), int(T), int(T) - 1
        if (lens < 0).any() or (lens > self.T1).any():
            raise ValueError("caption lengths must lie in [0, T-1]")
        _, order = torch.sort(lens, descending=True)          # the call pack_padded_sequence makes
        self.sorted_indices = order
        order_np, lens_np = order.numpy(), lens.numpy()
        self.max_len = int(lens_np.max()) if self.N else 0
        prow = np.full((self.T1, self.N), -1, np.int32)
        offsets = np.zeros(self.T1 + 1, np.int32)
        src, batch_sizes = [], []
        off = 0
        for t in range(self.T1):
            k = int((lens_np > t).sum())
            offsets[t] = off
            if k:
                rows = order_np[:k]
                prow[t, rows] = off + np.arange(k, dtype=np.int32)
                src.append(t * self.N + rows.astype(np.int32))
                batch_sizes.append(k)
            off += k
        offsets[self.T1] = off
        self.P = off
        self.batch_sizes = torch.tensor(batch_sizes, dtype=torch.int64)
        self.src_row_np = np.concatenate(src).astype(np.int32) if src else np.zeros(0, np.int32)
        self.offsets_host = np.ascontiguousarray(offsets)
        self.lengths_cpu = lens
        dev = torch.device(device)
        # pinned staging + asynchronous copies: a copy out of pageable memory blocks the host until the stream has drained, i.e. one
        # host/GPU synchronisation per train step (the host then issues the rest of the step into an empty queue)
        self.prow = _upload(torch.from_numpy(prow), dev)
        self.src_row = _upload(torch.from_numpy(self.src_row_np), dev)
        self.lengths = _upload(lens.to(torch.int32), dev)
        unsorted = torch.empty_like(order); unsorted[order] = torch.arange(self.N)
        self.unsorted_indices = unsorted                     # PackedSequence's index pair (model.py:553-554), host and device
        self.sorted_indices_dev, self.unsorted_indices_dev = _upload(order, dev), _upload(unsorted, dev)

    _cache = collections.OrderedDict()

    @classmethod
    def cached(cls, lengths, T, device):
        """Plans are read-only: batches with the same lengths (bucketed sampling repeats them often) share one."""
        lens = torch.as_tensor(lengths, dtype=torch.int64, device="cpu").reshape(-1)
        key = (int(T), str(torch.device(device)), lens.numpy().tobytes())
        plan = cls._cache.get(key)
        if plan is None:
            plan = cls._cache[key] = cls(lens, T, device)
            if len(cls._cache) > 32:
                cls._cache.popitem(last=False)
        else:
            cls._cache.move_to_end(key)
        return plan

    def pack(self, x_ntx):
        """(N, T-1, ...) padded -> packed rows (P, ...), same order as the library writes."""
        flat = x_ntx.transpose(0, 1).reshape(self.T1 * self.N, *x_ntx.shape[2:])
        return flat.index_select(0, self.src_row.to(torch.int64))

    def teacher_flags(self, epsilon, draw=None):
        """Scheduled sampling decisions (model.py:518): steps 0..2 always feed the caption; later steps
        draw one uniform sample each -- from the CPU generator, like the reference (F7) -- while any
        caption is still running."""
        if draw is None:
            draw = lambda: float(torch.rand(1))
        flags = np.ones(self.T1, np.int32)
        for step in range(min(self.T1, self.max_len)):
            if step <= 2 or draw() <= float(epsilon):
                flags[step] = 1
            else:
                flags[step] = 0
        return flags


def decoder_dims(B, R, T, Lc, D, A, m, n, V, P, deep, padding_idx, precision=0, embed_max_norm=0.0, dropout=0.0,
                 embedding_dropout=0.0, dropout_seed=0, layers=1, weight_drop=0.0, variational_dropout=False):
    if not 1 <= int(layers) <= L.MAX_LSTM_LAYERS:
        raise ValueError("decoder_layers=%d: the library is built for 1..%d stacked LSTM layers" % (layers, L.MAX_LSTM_LAYERS))
    check_weight_drop(weight_drop)
    return L.DecoderDims(B=B, R=R, T=T, L=Lc, D=D, A=A, m=m, n=n, V=V, P=P, deep_output=int(bool(deep)), padding_idx=padding_idx,
                         precision=int(precision), layers=int(layers), embed_max_norm=float(embed_max_norm or 0.0), dropout=float(dropout),
                         embedding_dropout=float(embedding_dropout), dropout_seed=int(dropout_seed), weight_drop=float(weight_drop),
                         variational_dropout=int(bool(variational_dropout)))


def check_weight_drop(p):
    """``weight_drop``: a probability in [0, 1) (0: off)"""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p < 1.0:
        raise ValueError("weight_drop=%r: a probability in [0, 1) (0: off)" % (p,))
    return float(p)


def _params_struct(tensors, layers=1, ln=None):
    """``ln``: the layer-norm group of the normalised cell by name (``_lib.ln_param_names``), or None: those fields stay NULL = the plain cell"""
    s = L.DecoderParams()
    for k in L.PARAM_FIELDS:
        t = tensors.get(k)
        setattr(s, k, None if t is None else t.data_ptr())
    for k in L.UP_FIELDS:
        arr = getattr(s, k)
        for l in range(1, layers):
            arr[l - 1] = tensors["%s_l%d" % (k[3:], l)].data_ptr()
    if ln:
        for k in L.LN_FIELDS:
            arr = getattr(s, k)
            for l in range(layers):
                arr[l] = ln["%s_l%d" % (k, l)].data_ptr()
    return s


def split_ln(params, n_ln):
    """(decoder parameter list, layer-norm group) of the trailing-group form ``*params, *ln`` with ``n_ln`` layer-norm tensors (0: none)"""
    n_ln = int(n_ln)
    if n_ln == 0:
        return list(params), []
    if n_ln < 0 or n_ln % len(L.LN_FIELDS) or n_ln // len(L.LN_FIELDS) != layers_of(len(params) - n_ln):
        raise ValueError("layer-norm group of %d tensors after %d decoder parameters; expected 4 per LSTM layer" % (n_ln, len(params) - n_ln))
    return list(params[:-n_ln]), list(params[-n_ln:])


def layers_of(n_params):
    """number of LSTM layers implied by the length of a decoder parameter list"""
    extra = n_params - len(L.PARAM_FIELDS)
    if extra < 0 or extra % len(L.UP_FIELDS):
        raise ValueError("decoder parameter list has %d entries; expected 18 + 4 per stacked layer" % n_params)
    return 1 + extra // len(L.UP_FIELDS)


def search_desc(stoi, beamk, max_gen_length, temperature, dev, con=None, hist=None, grp=None, req=None, smp=None):
    """The model-independent half of a ``sat_beam_search_desc``: sizes, the HOST temperature and special-id arrays, the checked options of
    ``constraints.SearchOptions.resolve`` as their structs and a ``BeamSampling``.  The caller adds ``d`` / ``w`` / ``ann`` or ``ensemble``;
    what the descriptor points into lives as long as it does (``_keep``)."""
    temps = temperature if isinstance(temperature, list) else [temperature]
    tarr = (C.c_float * len(temps))(*[float(t) for t in temps])
    ids = (C.c_int32 * 4)(*[int(stoi[s]) for s in ("<START>", "<PAD>", "<END>", "<UNK>")])
    desc = L.BeamSearchDesc(beamk=int(beamk), max_gen_length=int(max_gen_length), temperatures_host=tarr, n_temperatures=len(temps), special_ids_host=ids)
    parts = dict(sampling=smp, constraints=con and con.device_struct(dev), history=hist and hist.device_struct(), groups=grp and grp.device_struct(),
                 required=req and req.device_struct(dev))           # a struct, or (struct, the tensors it points into)
    desc._keep = [tarr, ids, parts]
    for field, st in parts.items():
        if st is not None:
            setattr(desc, field, C.pointer(st[0] if isinstance(st, tuple) else st))
    return desc


def beam_search(desc, B, Lc, dev, o=None):
    """``sat_beam_search`` over ``B`` images with ``Lc`` attention locations: allocates the output buffers (``_lib.SEARCH_OUTPUTS``; "req_met"
    with required words only) and the workspace ``sat_beam_search_desc_workspace_bytes`` asks for, enqueues, returns the dict.  ``o``: the
    dict of an earlier call, to enqueue into the same buffers again (graph capture).  A refused descriptor raises the library's message."""
    lib = L.lib()
    if o is None:
        ws_bytes = lib.sat_beam_search_desc_workspace_bytes(C.byref(desc))
        if ws_bytes == 0:
            L.check(1, "sat_beam_search_desc_workspace_bytes")
        K, S = desc.beamk, desc.max_gen_length
        i32 = dict(dtype=torch.int32, device=dev); f32 = dict(dtype=torch.float32, device=dev)
        o = dict(ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), tok_in=torch.empty(S + 2, B, K, **i32), prev_row=torch.empty(S + 2, B, K, **i32),
                 alpha_hist=torch.empty(S + 1, B, K, Lc, **f32), fin_count=torch.empty(B, **i32), fin_step=torch.empty(B, K, **i32),
                 fin_row=torch.empty(B, K, **i32), fin_score=torch.empty(B, K, **f32), fin_mean=torch.empty(B, K, **f32))
        if desc.required:
            o["req_met"] = torch.empty(B, **i32)
    out = L.BeamSearchOut(*[L.ptr(o.get(k)) for k in L.SEARCH_OUTPUTS])
    L.check(lib.sat_beam_search(C.byref(desc), C.byref(out), L.ptr(o["ws"]), o["ws"].numel(), L.stream_ptr()), "sat_beam_search")
    return o


def _check_param(name, t, shape):
    if t is None:
        return
    if tuple(t.shape) != tuple(shape):
        raise ValueError("decoder parameter %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("decoder parameter %s must be contiguous fp32" % name)


_leaf_events = {}          # device index -> (fork event, done event) of the decoder backward's side-stream fork
_leaf_forks = [0]          # how many backward passes forked (tests and tools read it)


def _leaf_side_events(dev, main):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    evs = _leaf_events.get(key)
    if evs is None:
        evs = _leaf_events[key] = (torch.cuda.Event(), torch.cuda.Event())
        evs[0].record(main)          # an event has no handle before its first record
    return evs


def _leaf_side_allowed(tens, n_distinct):
    """what the fork cannot live with: anything that reads a parameter gradient on the main stream before the backward pass ends.  A tied
    weight (autograd adds its two gradients as soon as both exist), a gradient already there (AccumulateGrad adds onto it), the bucket hooks
    of a data-parallel exchange between several ranks, a stream capture (graph.py keeps the fork off by itself)."""
    import torch.distributed as dist
    if not E._DECODER_LEAF_SIDE or n_distinct < sum(t is not None for t in tens.values()):
        return False
    if any(t is not None and t.grad is not None for t in tens.values()):
        return False
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return False
    return not torch.cuda.is_current_stream_capturing()


class DecoderTrainFn(torch.autograd.Function):
    """logits_packed (P,V), alphas (N,T-1,L) = decoder(ann (B,L,D), captions) with BPTT backward.  ``leaf_side``: the caller knows that an
    encoder backward with a side stream follows this Function's backward (``encoder.decoder_leaf_side_for``): the parameter gradients then go
    to that stream and are joined when the backward pass ends, see ``backward``."""

    @staticmethod
    def forward(ctx, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params):
        return DecoderTrainFn._forward(ctx, False, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params)

    @staticmethod
    def backward(ctx, dlogits, dalphas):
        return DecoderTrainFn._backward(ctx, dlogits, dalphas, None)

    @staticmethod
    def _forward(ctx, with_reg, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params, n_ln=0):
        """the body of all four Functions; ``with_reg``: a third output, the (ar, tar) pair of the top-layer states (``DecoderTrainRegFn``);
        ``n_ln``: the last ``n_ln`` tensors of ``params`` are the layer-norm group (``_lib.ln_param_names``) of the normalised cell"""
        lib = L.lib()
        params, ln_params = split_ln(params, n_ln)
        L.require_gpu(ann, caps_i32, *[p for p in params if p is not None], *ln_params)
        layers = layers_of(len(params))
        names = L.param_names(layers)
        tens = dict(zip(names, params))
        ln_tens = dict(zip(L.ln_param_names(layers), ln_params))
        ann = ann.contiguous()
        B, Lc, D = ann.shape
        V, m = tens["embedding"].shape
        n = tens["w_hh"].shape[1]
        A = tens["att_dec"].shape[0]
        N, T = caps_i32.shape
        if N != B * R or plan.N != N or plan.T != T:
            raise ValueError("caption batch (%d,%d) does not match B*R=%d / plan (%d,%d)" % (N, T, B * R, plan.N, plan.T))
        shapes = dict(embedding=(V, m), init_f_w=(m, D), init_f_b=(m,), init_i_w=(2 * n * layers, m), init_i_b=(2 * n * layers,), w_ih=(4 * n, m + D),
                      w_hh=(4 * n, n), b_ih=(4 * n,), b_hh=(4 * n,), att_enc=(A, D), att_dec=(A, n), att_f=(1, A), beta_w=(D, n),
                      beta_b=(D,), out_hidden=(m, n), out_context=(m, D), out_w=(V, m), out_b=(V,))
        for l in range(1, layers):
            shapes.update({"w_ih_l%d" % l: (4 * n, n), "w_hh_l%d" % l: (4 * n, n), "b_ih_l%d" % l: (4 * n,), "b_hh_l%d" % l: (4 * n,)})
        for k in names:
            _check_param(k, tens[k], shapes[k])
            if tens[k] is None and k not in ("out_context", "out_b"):
                raise ValueError("decoder parameter %s is missing" % k)
        for k, t in ln_tens.items():
            if t is None:
                raise ValueError("layer-norm parameter %s is missing" % k)
            _check_param(k, t, (4 * n,) if k.startswith("ln_gate") else (n,))
        # dropout: (p, p_embedding, seed), or with weight-drop / variational dropout (p, p_embedding, seed, weight_drop, variational_dropout)
        p_out, p_emb, seed, *more = dropout
        weight_drop, variational = more if more else (0.0, False)
        dims = decoder_dims(B, R, T, Lc, D, A, m, n, V, plan.P, deep, padding_idx, precision, embed_max_norm, p_out, p_emb, seed, layers=layers,
                            weight_drop=weight_drop, variational_dropout=variational)
        w = _params_struct(tens, layers, ln_tens)
        ws_bytes = lib.sat_decoder_workspace_bytes_ln(C.byref(dims), C.byref(w)) if ln_tens else lib.sat_decoder_workspace_bytes(C.byref(dims))
        if ws_bytes == 0:
            raise L.SatHipError("sat_decoder_workspace_bytes: %s" % lib.sat_last_error().decode())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ann.device)
        logits = torch.empty(max(plan.P, 1), V, dtype=torch.float32, device=ann.device)[:plan.P]
        alphas = torch.empty(N, T - 1, Lc, dtype=torch.float32, device=ann.device)
        teacher = np.ascontiguousarray(teacher, np.int32)
        batch = L.DecoderBatch(ann=ann.data_ptr(), caps=caps_i32.data_ptr(), lengths=plan.lengths.data_ptr(), prow=plan.prow.data_ptr(),
                               src_row=plan.src_row.data_ptr(), step_offsets_host=plan.offsets_host.ctypes.data,
                               teacher_host=teacher.ctypes.data)
        L.check(lib.sat_decoder_train_fwd(C.byref(dims), C.byref(w), C.byref(batch), L.ptr(logits), L.ptr(alphas), L.ptr(ws), ws_bytes,
                                          L.stream_ptr()), "sat_decoder_train_fwd")
        ctx.dims, ctx.plan, ctx.teacher, ctx.ws, ctx.ws_bytes = dims, plan, teacher, ws, ws_bytes
        ctx.caps, ctx.layers, ctx.leaf_side = caps_i32, layers, bool(leaf_side)
        ctx.save_for_backward(ann, alphas, *[p for p in params if p is not None], *ln_params)
        ctx.present = [p is not None for p in params]
        ctx.n_ln = len(ln_params)
        if not with_reg:
            return logits, alphas
        scratch = torch.empty(lib.sat_activation_reg_scratch_bytes(N, T - 1, n), dtype=torch.uint8, device=ann.device)
        reg = torch.empty(2, dtype=torch.float32, device=ann.device)
        L.check(lib.sat_decoder_train_reg_fwd(C.byref(dims), C.byref(batch), L.ptr(ws), ws_bytes, L.ptr(scratch), L.ptr(reg), L.stream_ptr()),
                "sat_decoder_train_reg_fwd")
        return logits, alphas, reg

    @staticmethod
    def _backward(ctx, dlogits, dalphas, dreg):
        """``dreg``: the gradient of the (ar, tar) output, device (2), or None: then the launches of the plain backward and no other"""
        lib = L.lib()
        saved = list(ctx.saved_tensors)
        ann, alphas = saved[0], saved[1]
        it = iter(saved[2:])
        params = [next(it) if present else None for present in ctx.present]
        names = L.param_names(ctx.layers)
        tens = dict(zip(names, params))
        n_ln = getattr(ctx, "n_ln", 0)
        ln_tens = dict(zip(L.ln_param_names(ctx.layers), list(it))) if n_ln else {}
        plan, dims = ctx.plan, ctx.dims
        taken = set()

        def gbuf(t):                  # bucket slice of the data-parallel exchange when there is one; a tied weight appears twice: once only
            if id(t) in taken:
                return torch.empty_like(t)
            taken.add(id(t))
            return L.grad_buffer(t)

        grads = {k: (None if t is None else gbuf(t)) for k, t in tens.items()}
        ln_grads = {k: gbuf(t) for k, t in ln_tens.items()}
        dann = torch.empty_like(ann)
        if dlogits is None:
            dlogits = torch.zeros(plan.P, dims.V, dtype=torch.float32, device=ann.device)
        dlogits = dlogits.contiguous()
        dalphas = None if dalphas is None else dalphas.contiguous()
        batch = L.DecoderBatch(ann=ann.data_ptr(), caps=ctx.caps.data_ptr(), lengths=plan.lengths.data_ptr(), prow=plan.prow.data_ptr(),
                               src_row=plan.src_row.data_ptr(), step_offsets_host=plan.offsets_host.ctypes.data,
                               teacher_host=ctx.teacher.ctypes.data)
        w, g = _params_struct(tens, ctx.layers, ln_tens), _params_struct(grads, ctx.layers, ln_grads)
        side_ptr = ev_ptr = None
        if ctx.leaf_side and ctx.needs_input_grad[0] and _leaf_side_allowed({**tens, **ln_tens}, len(taken)):
            # dann is all the encoder backward waits for: the parameter gradients go to the encoder's side stream, ahead of its weight
            # gradients, and the main stream waits for them when the backward pass ends (nothing may read a .grad before that)
            dev = ann.device
            main, side = torch.cuda.current_stream(dev), E.side_stream(dev)
            fork_ev, done_ev = _leaf_side_events(dev, main)
            side_ptr, ev_ptr = C.c_void_p(side.cuda_stream), C.c_void_p(fork_ev.cuda_event)
        if dreg is None:
            L.check(lib.sat_decoder_train_bwd_fork(C.byref(dims), C.byref(w), C.byref(batch), L.ptr(dlogits), L.ptr(alphas), L.ptr(dalphas),
                                                   C.byref(g), L.ptr(dann), L.ptr(ctx.ws), ctx.ws_bytes, side_ptr, ev_ptr, L.stream_ptr()), "sat_decoder_train_bwd_fork")
        else:
            dreg = dreg.to(torch.float32).contiguous()       # read on the main stream only, in front of the time loop
            L.check(lib.sat_decoder_train_bwd_reg(C.byref(dims), C.byref(w), C.byref(batch), L.ptr(dlogits), L.ptr(alphas), L.ptr(dalphas),
                                                  C.byref(g), L.ptr(dann), L.ptr(ctx.ws), ctx.ws_bytes, side_ptr, ev_ptr, L.stream_ptr(), L.ptr(dreg)),
                    "sat_decoder_train_bwd_reg")
        if side_ptr is not None:
            # what the side stream reads, and what it writes (autograd drops the gradient of a frozen parameter at once): the allocator must
            # not hand these blocks out again before the side stream is done
            for t in (ctx.ws, dlogits, ann, *grads.values(), *ln_grads.values()):
                if t is not None:
                    t.record_stream(side)
            done_ev.record(side)
            _leaf_forks[0] += 1

            def join():
                if E._JOIN_LAG is not None:          # dev (tools/join_lag.py)
                    es, em = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    es.record(side); em.record(main)
                    E._JOIN_LAG.append((em, es))
                main.wait_event(done_ev)
            try:
                torch.autograd.Variable._execution_engine.queue_callback(join)          # runs when this backward pass has finished
            except RuntimeError:                      # not called by the autograd engine
                join()
        if n_ln:          # DecoderTrainLNFn / DecoderTrainLNRegFn: one more leading argument (n_ln), the layer-norm group behind the parameters
            return (dann, None, None, None, None, None, None, None, None, None, None, None, *[grads[k] for k in names], *ln_grads.values())
        return (dann, None, None, None, None, None, None, None, None, None, None, *[grads[k] for k in names])


class DecoderTrainRegFn(torch.autograd.Function):
    """``DecoderTrainFn`` with a third output ``reg`` (2,) on the device: the activation regularisers ``(ar, tar)`` of the top-layer LSTM
    states (include/sat_hip.h, sat_activation_reg_fwd; DESIGN.md 5, "Activation regularisation").  Its gradient travels to
    ``sat_decoder_train_bwd_reg`` as a device pointer: no host read on the way there or back."""

    @staticmethod
    def forward(ctx, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params):
        return DecoderTrainFn._forward(ctx, True, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params)

    @staticmethod
    def backward(ctx, dlogits, dalphas, dreg):
        return DecoderTrainFn._backward(ctx, dlogits, dalphas, dreg)


class DecoderTrainLNFn(torch.autograd.Function):
    """``DecoderTrainFn`` with the layer-normalised LSTM cell ("Layer-normalised LSTM"): ``n_ln`` = 4 * layers, and the
    last ``n_ln`` tensors behind the decoder parameter list are the layer-norm group in ``_lib.ln_param_names`` order.  The parameter
    list itself keeps its meaning (18 + 4 per stacked layer)."""

    @staticmethod
    def forward(ctx, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, n_ln, *params):
        if not n_ln:
            raise ValueError("DecoderTrainLNFn: n_ln = 4 * layers layer-norm tensors (the plain cell: DecoderTrainFn)")
        return DecoderTrainFn._forward(ctx, False, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params, n_ln=n_ln)

    @staticmethod
    def backward(ctx, dlogits, dalphas):
        return DecoderTrainFn._backward(ctx, dlogits, dalphas, None)


class DecoderTrainLNRegFn(torch.autograd.Function):
    """``DecoderTrainLNFn`` with ``DecoderTrainRegFn``'s third output"""

    @staticmethod
    def forward(ctx, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, n_ln, *params):
        if not n_ln:
            raise ValueError("DecoderTrainLNRegFn: n_ln = 4 * layers layer-norm tensors (the plain cell: DecoderTrainRegFn)")
        return DecoderTrainFn._forward(ctx, True, ann, caps_i32, plan, teacher, deep, padding_idx, R, precision, embed_max_norm, dropout, leaf_side, *params, n_ln=n_ln)

    @staticmethod
    def backward(ctx, dlogits, dalphas, dreg):
        return DecoderTrainFn._backward(ctx, dlogits, dalphas, dreg)


class LabelSmoothingFn(torch.autograd.Function):
    """util.py:105-112 on packed rows; returns (loss, accuracy) -- accuracy as in model.py:596-597."""

    @staticmethod
    def forward(ctx, logits, targets_i32, smoothing):
        lib = L.lib()
        L.require_gpu(logits, targets_i32)
        logits = logits.contiguous()
        P, V = logits.shape
        lse = torch.empty(P, dtype=torch.float32, device=logits.device)
        rows = torch.empty(P, dtype=torch.float32, device=logits.device)
        correct = torch.empty(P, dtype=torch.int32, device=logits.device)
        out = torch.empty(2, dtype=torch.float32, device=logits.device)
        L.check(lib.sat_ce_label_smooth_fwd(L.ptr(logits), L.ptr(targets_i32), P, V, float(smoothing), L.ptr(lse), L.ptr(rows),
                                            L.ptr(correct), L.ptr(out), L.stream_ptr()), "sat_ce_label_smooth_fwd")
        ctx.save_for_backward(logits, targets_i32, lse)
        ctx.smoothing = float(smoothing)
        loss, acc = out[0].clone(), out[1].clone()
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, gloss, _gacc):
        lib = L.lib()
        logits, targets, lse = ctx.saved_tensors
        P, V = logits.shape
        dlogits = torch.empty_like(logits)
        g = gloss.reshape(1).to(torch.float32).contiguous()
        L.check(lib.sat_ce_label_smooth_bwd(L.ptr(logits), L.ptr(targets), L.ptr(lse), P, V, ctx.smoothing, L.ptr(g), L.ptr(dlogits),
                                            L.stream_ptr()), "sat_ce_label_smooth_bwd")
        return dlogits, None, None


class TokenLossFn(torch.autograd.Function):
    """The token losses on packed rows (include/sat_hip.h, sat_token_loss_fwd; DESIGN.md 5, "Token losses"):
    ``ce_weight * CE_smoothed + focal_weight * focal(gamma) + ul_alpha * unlikelihood`` with the unlikelihood's negative candidates taken
    from ``caps_i32`` (N, T) through ``src_row`` (``PackPlan.src_row``); both may be None when ``ul_alpha`` is 0.  Returns
    ``(loss, accuracy, terms)`` with ``terms`` the means of (ce, fl, ul, repeat mass), unweighted; differentiable in ``logits`` only, the
    last two are marked non-differentiable."""

    @staticmethod
    def forward(ctx, logits, targets_i32, smoothing, ce_weight, focal_weight, focal_gamma, ul_alpha, caps_i32, src_row, pad_id):
        lib = L.lib()
        L.require_gpu(logits, targets_i32)
        logits = logits.contiguous()
        P, V = logits.shape
        if logits.dtype != torch.float32 or targets_i32.dtype != torch.int32 or targets_i32.numel() != P:
            raise ValueError("TokenLossFn: float32 logits (P, V) and P int32 targets")
        targets_i32 = targets_i32.contiguous()
        N = T = 0
        if float(ul_alpha) != 0.0:
            if caps_i32 is None or src_row is None:
                raise ValueError("TokenLossFn: ul_alpha=%g needs the captions and the packing plan's src_row" % float(ul_alpha))
            L.require_gpu(caps_i32, src_row)
            if caps_i32.dtype != torch.int32 or src_row.dtype != torch.int32 or caps_i32.dim() != 2 or src_row.numel() != P:
                raise ValueError("TokenLossFn: int32 captions (N, T) and %d int32 src_row entries" % P)
            caps_i32, src_row = caps_i32.contiguous(), src_row.contiguous()
            N, T = caps_i32.shape
        else:
            caps_i32 = src_row = None
        f32 = dict(dtype=torch.float32, device=logits.device)
        lse, aux, rows = torch.empty(P, **f32), torch.empty(P, 2, **f32), torch.empty(P, 4, **f32)
        correct = torch.empty(P, dtype=torch.int32, device=logits.device)
        out = torch.empty(6, **f32)
        args = (P, V, float(smoothing), float(ce_weight), float(focal_weight), float(focal_gamma), float(ul_alpha))
        tail = (int(N), int(T), -1 if pad_id is None else int(pad_id))
        L.check(lib.sat_token_loss_fwd(L.ptr(logits), L.ptr(targets_i32), *args, L.ptr(caps_i32), L.ptr(src_row), *tail, L.ptr(lse), L.ptr(aux), L.ptr(rows),
                                       L.ptr(correct), L.ptr(out), L.stream_ptr()), "sat_token_loss_fwd")
        ctx.save_for_backward(logits, targets_i32, lse, aux)
        ctx.args, ctx.tail, ctx.context = args, tail, (caps_i32, src_row)
        loss, acc, terms = out[0].clone(), out[1].clone(), out[2:].clone()
        ctx.mark_non_differentiable(acc, terms)
        return loss, acc, terms

    @staticmethod
    def backward(ctx, gloss, _gacc, _gterms):
        lib = L.lib()
        logits, targets, lse, aux = ctx.saved_tensors
        caps_i32, src_row = ctx.context
        dlogits = torch.empty_like(logits)
        g = gloss.reshape(1).to(torch.float32).contiguous()
        L.check(lib.sat_token_loss_bwd(L.ptr(logits), L.ptr(targets), *ctx.args, L.ptr(caps_i32), L.ptr(src_row), *ctx.tail, L.ptr(lse), L.ptr(aux), L.ptr(g),
                                       L.ptr(dlogits), L.stream_ptr()), "sat_token_loss_bwd")
        return dlogits, None, None, None, None, None, None, None, None, None


class PolicyNLLFn(torch.autograd.Function):
    """The row-weighted policy loss of self-critical training on packed rows (include/sat_hip.h, sat_policy_nll_fwd):
    ``-scale * sum_p row_weight[p] * log q(targets[p])`` with q the softmax of ``logits / temperature`` over the words the search leaves
    unmasked.  ``masked_ids``: device int32 (4) {START, PAD, END, UNK}; the first ``n_first_rows`` packed rows mask all four, the others
    the first two.  Differentiable in ``logits`` only; rows of weight zero get a zero gradient without being read."""

    @staticmethod
    def forward(ctx, logits, targets_i32, row_weight, inv_temperature, masked_ids, n_first_rows, scale):
        lib = L.lib()
        L.require_gpu(logits, targets_i32, row_weight, masked_ids)
        logits = logits.contiguous()
        P, V = logits.shape
        if targets_i32.dtype != torch.int32 or masked_ids.dtype != torch.int32 or row_weight.dtype != torch.float32:
            raise ValueError("PolicyNLLFn: targets and masked_ids are int32, row_weight is float32")
        if targets_i32.numel() != P or row_weight.numel() != P or masked_ids.numel() != 4:
            raise ValueError("PolicyNLLFn: %d targets / %d weights for %d packed rows, %d masked ids (4)"
                             % (targets_i32.numel(), row_weight.numel(), P, masked_ids.numel()))
        targets_i32, row_weight, masked_ids = targets_i32.contiguous(), row_weight.contiguous(), masked_ids.contiguous()
        lse = torch.empty(P, dtype=torch.float32, device=logits.device)
        logq = torch.empty(P, dtype=torch.float32, device=logits.device)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        L.check(lib.sat_policy_nll_fwd(L.ptr(logits), L.ptr(targets_i32), L.ptr(row_weight), P, V, float(inv_temperature), L.ptr(masked_ids),
                                       int(n_first_rows), float(scale), L.ptr(lse), L.ptr(logq), L.ptr(out), L.stream_ptr()), "sat_policy_nll_fwd")
        ctx.save_for_backward(logits, targets_i32, row_weight, lse, masked_ids)
        ctx.args = (float(inv_temperature), int(n_first_rows), float(scale))
        return out[0].clone()

    @staticmethod
    def backward(ctx, gloss):
        lib = L.lib()
        logits, targets, row_weight, lse, masked_ids = ctx.saved_tensors
        inv_temperature, n_first_rows, scale = ctx.args
        P, V = logits.shape
        dlogits = torch.empty_like(logits)
        g = gloss.reshape(1).to(torch.float32).contiguous()
        L.check(lib.sat_policy_nll_bwd(L.ptr(logits), L.ptr(targets), L.ptr(row_weight), L.ptr(lse), P, V, inv_temperature, L.ptr(masked_ids),
                                       n_first_rows, scale, L.ptr(g), L.ptr(dlogits), L.stream_ptr()), "sat_policy_nll_bwd")
        return dlogits, None, None, None, None, None, None


class DistillFn(torch.autograd.Function):
    """The distillation loss on packed rows (include/sat_hip.h, sat_distill_fwd):
    ``(1 - alpha) * CE_smoothed(logits, targets) + alpha * tau^2 * KL(q || softmax(logits / tau))`` with ``q`` the combination of the
    teachers' distributions at ``tau`` (``combine``: "arithmetic" / "geometric", the ensemble search's).  ``teachers``: a list of (P, V)
    float32 tensors, ``weights`` host floats summing to 1.  Returns ``(loss, hard, soft, accuracy)``; differentiable in ``logits`` only,
    the last three are marked non-differentiable.  ``fuse_gradient``: the forward writes the gradient while the rows are in the cache
    and the backward only scales it in place.  Off by default: measured at C2's (P, V) with 1, 2 and 4 teachers it is no faster than the
    backward that rebuilds the gradient from the row scratch ("Distillation"), and it keeps one more (P, V) buffer alive
    between the two."""

    @staticmethod
    def forward(ctx, logits, targets_i32, teachers, weights, combine, inv_tau, alpha, smoothing, fuse_gradient=False):
        lib = L.lib()
        teachers = [t.contiguous() for t in teachers]
        L.require_gpu(logits, targets_i32, *teachers)
        logits = logits.contiguous()
        P, V = logits.shape
        M = len(teachers)
        if combine not in L.ENSEMBLE_COMBINE:
            raise ValueError("DistillFn: combine=%r is none of %r" % (combine, tuple(L.ENSEMBLE_COMBINE)))
        if not 1 <= M <= L.ENSEMBLE_MAX or len(weights) != M:
            raise ValueError("DistillFn: %d teachers (1..%d) with %d weights" % (M, L.ENSEMBLE_MAX, len(weights)))
        if logits.dtype != torch.float32 or targets_i32.dtype != torch.int32 or any(t.dtype != torch.float32 for t in teachers):
            raise ValueError("DistillFn: logits and teachers are float32, targets are int32")
        if targets_i32.numel() != P or any(tuple(t.shape) != (P, V) for t in teachers):
            raise ValueError("DistillFn: %d targets and teachers %s for student logits (%d, %d)" % (targets_i32.numel(), [tuple(t.shape) for t in teachers], P, V))
        targets_i32 = targets_i32.contiguous()
        fused = bool(fuse_gradient) and bool(ctx.needs_input_grad[0])
        f32 = dict(dtype=torch.float32, device=logits.device)
        lse, tlse, cnorm, rows = torch.empty(P, 2, **f32), torch.empty(P, M, **f32), torch.empty(P, **f32), torch.empty(P, 2, **f32)
        correct = torch.empty(P, dtype=torch.int32, device=logits.device)
        out = torch.empty(4, **f32)
        dlogits = torch.empty_like(logits) if fused else None
        tarr = (C.c_void_p * M)(*[t.data_ptr() for t in teachers])
        warr = (C.c_float * M)(*[float(w) for w in weights])
        args = (M, L.ENSEMBLE_COMBINE[combine], P, V, float(inv_tau), float(alpha), float(smoothing))
        L.check(lib.sat_distill_fwd(L.ptr(logits), tarr, warr, args[0], args[1], L.ptr(targets_i32), P, V, args[4], args[5], args[6], L.ptr(lse), L.ptr(tlse),
                                    L.ptr(cnorm), L.ptr(rows), L.ptr(correct), L.ptr(out), L.ptr(dlogits), L.stream_ptr()), "sat_distill_fwd")
        ctx.save_for_backward(logits, targets_i32, lse, tlse, cnorm)
        ctx.teachers, ctx.weights, ctx.args, ctx.dlogits, ctx.fused = teachers, [float(w) for w in weights], args, dlogits, fused
        loss, hard, soft, acc = out[0].clone(), out[1].clone(), out[2].clone(), out[3].clone()
        ctx.mark_non_differentiable(hard, soft, acc)
        return loss, hard, soft, acc

    @staticmethod
    def backward(ctx, gloss, _ghard, _gsoft, _gacc):
        lib = L.lib()
        logits, targets, lse, tlse, cnorm = ctx.saved_tensors
        M, combine, P, V, inv_tau, alpha, smoothing = ctx.args
        fused = ctx.fused
        if fused and ctx.dlogits is None:
            raise RuntimeError("DistillFn: the fused gradient was consumed by an earlier backward")
        dlogits = ctx.dlogits if fused else torch.empty_like(logits)
        ctx.dlogits = None                     # scaled in place: a second backward would scale it twice
        g = gloss.reshape(1).to(torch.float32).contiguous()
        tarr = (C.c_void_p * M)(*[t.data_ptr() for t in ctx.teachers])
        warr = (C.c_float * M)(*ctx.weights)
        L.check(lib.sat_distill_bwd(L.ptr(logits), tarr, warr, M, combine, L.ptr(targets), P, V, inv_tau, alpha, smoothing, L.ptr(lse), L.ptr(tlse), L.ptr(cnorm),
                                    L.ptr(g), int(fused), L.ptr(dlogits), L.stream_ptr()), "sat_distill_bwd")
        return dlogits, None, None, None, None, None, None, None, None


class DoublyStochasticFn(torch.autograd.Function):
    """model.py:594: gamma * ((1 - alphas.sum(dim=1)) ** 2).mean(), fixed-order reduction."""

    @staticmethod
    def forward(ctx, alphas, gamma):
        lib = L.lib()
        L.require_gpu(alphas)
        alphas = alphas.contiguous()
        N, T1, Lc = alphas.shape
        asum = torch.empty(N, Lc, dtype=torch.float32, device=alphas.device)
        part = torch.empty((N * Lc + 255) // 256, dtype=torch.float32, device=alphas.device)
        out = torch.empty(1, dtype=torch.float32, device=alphas.device)
        L.check(lib.sat_doubly_stochastic_fwd(L.ptr(alphas), N, T1, Lc, float(gamma), L.ptr(asum), L.ptr(part), L.ptr(out),
                                              L.stream_ptr()), "sat_doubly_stochastic_fwd")
        ctx.save_for_backward(asum)
        ctx.shape, ctx.gamma = (N, T1, Lc), float(gamma)
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        lib = L.lib()
        (asum,) = ctx.saved_tensors
        N, T1, Lc = ctx.shape
        dal = torch.empty(N, T1, Lc, dtype=torch.float32, device=asum.device)
        gs = g.reshape(1).to(torch.float32).contiguous()
        L.check(lib.sat_doubly_stochastic_bwd(L.ptr(asum), L.ptr(gs), N, T1, Lc, ctx.gamma, L.ptr(dal), L.stream_ptr()),
                "sat_doubly_stochastic_bwd")
        return dal, None


def dropout_scale_reference(seed, stream, idx, p):
    """numpy replica of csrc/decoder_kernels.h:dropout_scale (tests rebuild the masks with it on the host)."""
    M = (1 << 64) - 1
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed & M) + np.uint64((0x9E3779B97F4A7C15 * (stream + 1)) & M) + idx * np.uint64(0xD1342543DE82EF95))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)


def weight_drop_scale_reference(seed, layers, n, p, rows=None, layer0=0):
    """the weight-drop scales of the decoder on the host, built on ``dropout_scale_reference``: (layers, rows, n) float32 with
    ``s[l, r, c] = dropout_scale(seed, 3, ((layer0 + l) * rows + r) * n + c, p)``; ``rows`` defaults to the LSTM's 4n.  ``layer0``: the
    slice of a taller mask that starts at that layer, computed alone."""
    rows = 4 * int(n) if rows is None else int(rows)
    per = rows * int(n)
    idx = np.arange(int(layer0) * per, (int(layer0) + int(layers)) * per, dtype=np.uint64)
    return dropout_scale_reference(seed, 3, idx, p).reshape(int(layers), rows, int(n))


def _weight_drop_args(t, what):
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("%s: a contiguous float32 (layers, rows, cols) or (rows, cols) tensor" % what)
    L.require_gpu(t)
    return t.shape


def weight_drop(w, p, seed, out=None, out_bf16=None):
    """``sat_weight_drop``: (w * s, out_bf16) for w (layers, rows, cols) with the scales of ``weight_drop_scale_reference``; ``out_bf16``,
    when given, receives the bf16 rounding of the same product"""
    layers, rows, cols = _weight_drop_args(w, "weight_drop")
    out = torch.empty_like(w) if out is None else out
    for t, dt in ((out, torch.float32), (out_bf16, torch.bfloat16)):
        if t is not None and (t.dtype != dt or t.numel() != w.numel() or not t.is_contiguous() or not t.is_cuda):
            raise ValueError("weight_drop: outputs are contiguous device tensors of w's size (float32, bfloat16)")
    L.check(L.lib().sat_weight_drop(L.ptr(w), L.ptr(out), L.ptr(out_bf16), layers, rows, cols, float(p), int(seed), L.stream_ptr()), "sat_weight_drop")
    return out, out_bf16


def weight_drop_grad_(g, p, seed):
    """``sat_weight_drop_grad``: g *= s in place (the gradient w.r.t. w from the gradient w.r.t. w * s); returns g"""
    layers, rows, cols = _weight_drop_args(g, "weight_drop_grad_")
    L.check(L.lib().sat_weight_drop_grad(L.ptr(g), layers, rows, cols, float(p), int(seed), L.stream_ptr()), "sat_weight_drop_grad")
    return g


def gemm(A, B, *, amode=0, bmode=0, M=None, N=None, K=None, out=None, accumulate=False, epi=0, bias=None, e0=None, c0=0, c1=0,
         a_rows=None, c_rows=None, out_rows=None, slab=None, bf16_mfma=False, out_dtype=torch.float32):
    """Thin test/driver entry to sat_gemm_f32 (dense modes).  A: (M,K) if amode=0 else (K,M); B: (N,K) if bmode=0 else (K,N)."""
    lib = L.lib()
    L.require_gpu(A, B)
    if M is None:
        M = (a_rows.numel() if a_rows is not None else A.shape[0]) if amode == 0 else A.shape[1]
    if K is None:
        K = A.shape[1] if amode == 0 else A.shape[0]
    if N is None:
        N = B.shape[0] if bmode == 0 else B.shape[1]
    if out is None:
        out = torch.zeros(out_rows if out_rows is not None else M, N, dtype=out_dtype, device=A.device)
    d = L.GemmDesc(A=A.data_ptr(), lda=A.stride(0), a_rows=None if a_rows is None else a_rows.data_ptr(),
                   B=B.data_ptr(), ldb=B.stride(0), C=out.data_ptr(), ldc=out.stride(0),
                   c_rows=None if c_rows is None else c_rows.data_ptr(), M=M, N=N, K=K, amode=amode, bmode=bmode,
                   accumulate=int(accumulate), epi=epi, bias=None if bias is None else bias.data_ptr(),
                   e0=None if e0 is None else e0.data_ptr(), lde0=0 if e0 is None else e0.stride(0), c0=c0, c1=c1,
                   slab=None if slab is None else slab.data_ptr(), slab_elems=0 if slab is None else slab.numel())
    bf = torch.bfloat16
    if bf16_mfma or A.dtype == bf or B.dtype == bf or out.dtype == bf:
        t = L.GemmTypes(a_bf16=int(A.dtype == bf), b_bf16=int(B.dtype == bf), c_bf16=int(out.dtype == bf), bf16_mfma=int(bf16_mfma))
        L.check(lib.sat_gemm_ex(C.byref(d), C.byref(t), L.stream_ptr()), "sat_gemm_ex")
    else:
        L.check(lib.sat_gemm_f32(C.byref(d), L.stream_ptr()), "sat_gemm_f32")
    return out
