"""The decoder backward with its parameter gradients on a side stream (sat_decoder_train_bwd_fork) is the decoder backward: the same kernels
with the same arguments, in the same order per stream.  So every comparison here is BIT for bit (int32 views under torch.equal): the forked
call against the unforked one, the new entry with NULL stream / event against sat_decoder_train_bwd, the eager train step with the fork
against the one without, and the hipGraph replay (which keeps the fork off) against the eager step with it.

Entry-point cases: parameters, annotations, captions, the workspace, dlogits / dalphas, every gradient and dann are views inside buffers
filled with a canary bit pattern (64 elements in front, 64 behind); the frames must be intact afterwards.  Each run gets fresh copies of the
inputs (the forward renormalises the embedding table in place under embed_norm)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemm_ref import CANARY_F32

GUARD = 64          # elements (4 bytes each): 256 bytes, the alignment the workspace needs


def _lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    return L


def framed(t):
    """a copy of ``t`` (4-byte elements) inside a canary-filled buffer; returns (whole as int32, view)"""
    flat = t.contiguous().reshape(-1)
    assert flat.element_size() == 4
    whole = torch.full((2 * GUARD + max(flat.numel(), 1),), CANARY_F32, dtype=torch.int32, device="cuda")
    view = whole[GUARD:GUARD + flat.numel()].view(flat.dtype)
    view.copy_(flat)
    return whole, view.reshape(t.shape)


def frame_intact(whole, n, what):
    assert bool((whole[:GUARD] == CANARY_F32).all()) and bool((whole[GUARD + n:] == CANARY_F32).all()), "%s: canary frame written" % what


BASE = dict(B=2, R=2, T=5, L=4, D=8, A=8, m=8, n=8, V=16, layers=1, deep=True, dropout=0.0, embedding_dropout=0.0, tying=False, embed_norm=0.0,
            lengths=None, teacher=None, precision=0)
CASES = {
    "full": {},
    "ragged": dict(lengths=[3, 2, 3, 1]),                                     # one caption ends early, and ts = 3 < T - 1
    "layers2": dict(layers=2),
    "layers2_ragged": dict(layers=2, lengths=[4, 1, 2, 3]),
    "shallow": dict(deep=False),
    "dropout": dict(dropout=0.3, embedding_dropout=0.2),                      # the per-row InitLSTM path
    "tying": dict(tying=True),                                                # output.output.weight IS the embedding table
    "embed_norm": dict(embed_norm=1.0),
    "tying_embed_norm_sampling": dict(tying=True, embed_norm=1.0, teacher=[1, 1, 1, 0]),
    "sampling": dict(teacher=[1, 1, 0, 0]),                                   # scheduled sampling: argmax of the previous step's logits
    "shallow_layers2_dropout_sampling": dict(deep=False, layers=2, dropout=0.25, teacher=[1, 1, 1, 0], lengths=[4, 4, 2, 3]),
}
# ts * N = 16 * 64 = 1024 rows under the k-major weight-gradient products: split-K in both scratch sets at once
BIG = dict(B=16, R=4, T=17, L=9, D=64, A=32, m=64, n=128, V=128)


def _cfg(over):
    c = dict(BASE); c.update(over)
    return c


def _inputs(c, seed):
    """host tensors of one run: parameters by name, annotations, captions, lengths, dlogits / dalphas generators"""
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    B, R, T, Lc, D, A, m, n, V, NL = (c[k] for k in ("B", "R", "T", "L", "D", "A", "m", "n", "V", "layers"))
    N = B * R

    def rnd(*shape, scale=0.3):
        return (torch.rand(*shape, generator=g) * 2 - 1) * scale
    shapes = dict(embedding=(V, m), init_f_w=(m, D), init_f_b=(m,), init_i_w=(2 * n * NL, m), init_i_b=(2 * n * NL,), w_ih=(4 * n, m + D),
                  w_hh=(4 * n, n), b_ih=(4 * n,), b_hh=(4 * n,), att_enc=(A, D), att_dec=(A, n), att_f=(1, A), beta_w=(D, n),
                  beta_b=(D,), out_hidden=(m, n), out_context=(m, D), out_w=(V, m), out_b=(V,))
    for l in range(1, NL):
        shapes.update({"w_ih_l%d" % l: (4 * n, n), "w_hh_l%d" % l: (4 * n, n), "b_ih_l%d" % l: (4 * n,), "b_hh_l%d" % l: (4 * n,)})
    names = L.param_names(NL)
    params = {k: rnd(*shapes[k], scale=1.5 if k == "embedding" else 0.3) for k in names}          # rows longer than max_norm = 1 exist
    if not c["deep"]:
        params["out_context"] = None
    if c["tying"]:
        params["out_w"] = params["out_b"] = None          # filled in on the device: the same memory as the embedding
    lengths = torch.tensor(c["lengths"] if c["lengths"] is not None else [T - 1] * N, dtype=torch.int64)
    caps = torch.randint(1, V, (N, T), generator=g, dtype=torch.int64).to(torch.int32)
    for r in range(N):
        caps[r, int(lengths[r]) + 1:] = 0          # padding
    teacher = np.ascontiguousarray(c["teacher"] if c["teacher"] is not None else [1] * (T - 1), np.int32)
    return dict(names=names, params=params, ann=rnd(B, Lc, D, scale=1.0), caps=caps, lengths=lengths, teacher=teacher,
                dl_seed=seed + 1000)


def run(c, inp, mode, ws_frame=None):
    """forward + backward of one batch through the C ABI.  mode: "old" = sat_decoder_train_bwd, "null" = the new entry without a side stream,
    "fork" = with one.  Returns ({name: int32 copy of the gradient}, the workspace frame)."""
    L = _lib()
    from sat_amd import decoder as Dk
    lib = L.lib()
    B, R, T, Lc, D, A, m, n, V, NL = (c[k] for k in ("B", "R", "T", "L", "D", "A", "m", "n", "V", "layers"))
    N = B * R
    plan = Dk.PackPlan(inp["lengths"], T, torch.device("cuda"))
    frames = []

    def put(t, what):
        whole, view = framed(t)
        frames.append((whole, view.numel(), what))
        return view
    tens = {k: (None if t is None else put(t, "parameter " + k)) for k, t in inp["params"].items()}
    if c["tying"]:
        tens["out_w"] = tens["embedding"]
    ann, caps = put(inp["ann"], "annotations"), put(inp["caps"], "captions")
    dims = Dk.decoder_dims(B, R, T, Lc, D, A, m, n, V, plan.P, c["deep"], 0, c["precision"], c["embed_norm"], c["dropout"], c["embedding_dropout"],
                           12345, layers=NL)
    ws_bytes = lib.sat_decoder_workspace_bytes(C.byref(dims))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    if ws_frame is None:
        ws_frame = torch.full((2 * GUARD + ws_bytes // 4,), CANARY_F32, dtype=torch.int32, device="cuda")
    ws = ws_frame[GUARD:GUARD + ws_bytes // 4]
    assert ws.data_ptr() % 256 == 0
    logits, alphas = put(torch.zeros(max(plan.P, 1), V), "logits"), put(torch.zeros(N, T - 1, Lc), "alphas")
    batch = L.DecoderBatch(ann=ann.data_ptr(), caps=caps.data_ptr(), lengths=plan.lengths.data_ptr(), prow=plan.prow.data_ptr(),
                           src_row=plan.src_row.data_ptr(), step_offsets_host=plan.offsets_host.ctypes.data, teacher_host=inp["teacher"].ctypes.data)
    w = Dk._params_struct(tens, NL)
    st = L.stream_ptr()
    L.check(lib.sat_decoder_train_fwd(C.byref(dims), C.byref(w), C.byref(batch), L.ptr(logits), L.ptr(alphas), L.ptr(ws), ws_bytes, st), "fwd")
    gd = torch.Generator().manual_seed(inp["dl_seed"])
    dlogits = put((torch.rand(max(plan.P, 1), V, generator=gd) - 0.5) * 0.2, "dlogits")
    dalphas = put((torch.rand(N, T - 1, Lc, generator=gd) - 0.5) * 0.2, "dalphas")
    grads = {k: (None if t is None else put(torch.zeros(t.shape), "gradient of " + k)) for k, t in tens.items()}          # tying: two buffers
    dann = put(torch.zeros(B, Lc, D), "dann")
    g = Dk._params_struct(grads, NL)
    args = (C.byref(dims), C.byref(w), C.byref(batch), L.ptr(dlogits), L.ptr(alphas), L.ptr(dalphas), C.byref(g), L.ptr(dann), L.ptr(ws), ws_bytes)
    if mode == "old":
        L.check(lib.sat_decoder_train_bwd(*args, st), "sat_decoder_train_bwd")
    elif mode == "null":
        L.check(lib.sat_decoder_train_bwd_fork(*args, None, None, st), "sat_decoder_train_bwd_fork")
    else:
        side, ev = torch.cuda.Stream(), torch.cuda.Event()
        ev.record(torch.cuda.current_stream())          # gives the event its handle
        L.check(lib.sat_decoder_train_bwd_fork(*args, C.c_void_p(side.cuda_stream), C.c_void_p(ev.cuda_event), st), "sat_decoder_train_bwd_fork")
        torch.cuda.current_stream().wait_stream(side)   # the join the call leaves to its caller
    torch.cuda.synchronize()
    for whole, nelem, what in frames:
        frame_intact(whole, nelem, "%s (%s)" % (what, mode))
    frame_intact(ws_frame, ws_bytes // 4, "workspace (%s)" % mode)
    out = {k: t.view(torch.int32).clone() for k, t in grads.items() if t is not None}
    out["dann"] = dann.view(torch.int32).clone()
    return out, ws_frame


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs in %d of %d words" % (what, k, int((a[k] != b[k]).sum()), a[k].numel())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_forked_backward_is_the_unforked_backward(name):
    c = _cfg(CASES[name])
    inp = _inputs(c, 7)
    old, _ = run(c, inp, "old")
    assert any(bool((v != 0).any()) for v in old.values())
    null, _ = run(c, inp, "null")
    same(old, null, name + ": NULL stream / event against sat_decoder_train_bwd")
    fork, _ = run(c, inp, "fork")
    same(old, fork, name + ": side stream against sat_decoder_train_bwd")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 1])
def test_split_k_in_both_scratch_sets_over_one_workspace(precision):
    c = _cfg(dict(BIG, precision=precision))
    ws = None
    for seed in (3, 4, 5):          # three batches through ONE workspace: nothing of an earlier backward may leak into a later one
        inp = _inputs(c, seed)
        old, _ = run(c, inp, "old")
        fork, ws = run(c, inp, "fork", ws)
        same(old, fork, "precision %d, batch %d" % (precision, seed))


# ------------------------------------------------------------------ refusals (no GPU needed: every check precedes the first launch)
def _refusal_args(L, shrink=0):
    lib = L.lib()
    dims = L.DecoderDims(B=2, R=2, T=5, L=4, D=8, A=8, m=8, n=8, V=16, P=16, deep_output=1, padding_idx=0, layers=1)
    ws_bytes = lib.sat_decoder_workspace_bytes(C.byref(dims))
    some = 4096          # never dereferenced
    w = L.DecoderParams(**{k: some for k in L.PARAM_FIELDS})
    host = np.zeros(8, np.int32)
    batch = L.DecoderBatch(ann=some, caps=some, lengths=some, prow=some, src_row=some, step_offsets_host=host.ctypes.data, teacher_host=host.ctypes.data)
    return lib, (C.byref(dims), C.byref(w), C.byref(batch), some, some, some, C.byref(w), some, some, ws_bytes - shrink), (dims, w, batch, host)


def test_a_side_stream_needs_its_event_and_an_event_its_stream():
    L = _lib()
    lib, args, _keep = _refusal_args(L)
    assert lib.sat_decoder_train_bwd_fork(*args, C.c_void_p(4096), None, None) != 0
    assert b"side stream and event" in lib.sat_last_error()
    assert lib.sat_decoder_train_bwd_fork(*args, None, C.c_void_p(4096), None) != 0
    assert b"side stream and event" in lib.sat_last_error()
    assert lib.sat_decoder_train_bwd_fork(*args, C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(4096)) != 0
    assert b"caller's stream" in lib.sat_last_error()


def test_a_workspace_without_the_second_scratch_set_is_refused():
    """the workspace of before had one split-K slab; one slab (32 MiB) short of today's size is at least that large"""
    L = _lib()
    lib, args, _keep = _refusal_args(L, shrink=32 << 20)
    assert args[-1] > 32 << 20
    assert lib.sat_decoder_train_bwd_fork(*args, None, None, None) != 0
    assert b"workspace" in lib.sat_last_error()
    assert lib.sat_decoder_train_bwd(*args, None) != 0
    assert b"workspace" in lib.sat_last_error()


# ------------------------------------------------------------------ the train step
def _make(seed=42):
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = O.default_hparams(encoder_arch="resnet18", encoder_dim=64, input_size=64, encoder_size=3, vocab_size=120, embed_dim=24, attention_dim=16,
                           decoder_dim=40, deep_output=True, weight_decay=0.0, decoder_lr=1e-3, embedding_lr=1e-2, encoder_lr=1e-4, opt="adam",
                           adam_b1=0.9, adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None, decoder_tf="always", encoder_finetune_after=0,
                           lr_warmup_steps=4)
    torch.manual_seed(seed)
    model = M.SAT(**vars(hp)).cuda().train()
    model.set_precision("bf16")
    return model, hp


def _batch(hp, seed, B=4, R=3, T=9):
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, hp.input_size, hp.input_size), seed, 0.0, 1.0))
    caps, lengths = prng.captions(B, R, T, hp.vocab_size, seed + 1)
    return img.cuda(), torch.from_numpy(caps).cuda(), torch.from_numpy(lengths)


@pytest.fixture
def side_stream_for_every_batch(monkeypatch):
    """the side stream is for batches of 16 x 256 x 256 pixels and more: let these small ones take it, and put everything back afterwards"""
    from sat_amd import encoder as E
    monkeypatch.setattr(E, "_WGRAD_SIDE_MIN_INPUT_PIXELS", 0)
    monkeypatch.setattr(E, "_WGRAD_STREAM", True)
    monkeypatch.setattr(E, "_DECODER_LEAF_SIDE", True)
    return E


@pytest.mark.gpu
def test_gradients_are_there_when_backward_returns(side_stream_for_every_batch):
    """backward(), then .grad.cpu() with no synchronisation in between: what the fork leaves in .grad is what the unforked step leaves"""
    E = side_stream_for_every_batch
    from sat_amd import decoder as Dk
    got = {}
    for on in (False, True):
        E._DECODER_LEAF_SIDE = on
        model, hp = _make()
        opt = model.configure_optimizers()
        forks = Dk._leaf_forks[0]
        steps = []
        for it in range(3):
            opt.zero_grad(set_to_none=True)
            out = model.training_step(_batch(hp, 11 + it), it)
            out["loss"].backward()
            steps.append([(k, p.grad.cpu().view(torch.int32)) for k, p in model.named_parameters() if p.grad is not None])
            opt.step()
        assert Dk._leaf_forks[0] - forks == (3 if on else 0)
        got[on] = steps
    for it in range(3):
        assert [k for k, _ in got[False][it]] == [k for k, _ in got[True][it]] and len(got[True][it]) > 20
        for (k, a), (_, b) in zip(got[False][it], got[True][it]):
            assert torch.equal(a, b), "step %d: %s.grad differs with the fork" % (it, k)


@pytest.mark.gpu
def test_graph_replay_equals_the_eager_step_with_the_fork(side_stream_for_every_batch):
    """tests/test_gpu_graph.py's configuration with the switch on: the eager steps fork, the captured step keeps the fork off, and both leave
    the same bits in the loss and in every parameter"""
    from sat_amd import decoder as Dk
    from sat_amd.graph import GraphedTrainStep
    eager, hp = _make()
    graphed, _ = _make()
    opt_e, opt_g = eager.configure_optimizers(), graphed.configure_optimizers()
    step = GraphedTrainStep(graphed, opt_g)
    b = _batch(hp, 11)
    forks = Dk._leaf_forks[0]
    for it in range(5):
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(b, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(b, it)
        assert torch.equal(out_e["loss"].detach(), out_g["loss"]), "step %d: loss %r vs %r" % (it, float(out_e["loss"]), float(out_g["loss"]))
        for (k, x), (_, y) in zip(eager.state_dict().items(), graphed.state_dict().items()):
            if torch.is_tensor(x):
                assert torch.equal(x, y), "after step %d: %s differs" % (it, k)
    assert step.stats["captured"] == 1 and step.stats["replayed"] == 4, dict(step.stats)
    assert Dk._leaf_forks[0] - forks == 5 + 1          # every eager step, and the graphed model's first (eager, warming) one
