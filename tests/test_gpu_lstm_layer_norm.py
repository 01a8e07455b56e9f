"""GPU: the layer-normalised LSTM cell ("Layer-normalised LSTM") against tests/lstm_layer_norm_ref.py.

  1. the two cell kernels alone (sat_lstm_ln_cell_fwd / _bwd) in NaN frames with guard bands, against the float64 reference and its
     autograd gradients; the parameter-gradient partials over three steps and their finishing sum;
  2. the train step against the CPU oracle with ``lstm_fn=ln_lstm_step``: logits, alphas, loss and every gradient;
  3. the off path, the side stream, the searches, ensembles, bf16 mode, the captured step and checkpoints."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lstm_layer_norm_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 64
A_OFF, D_OFF = 7, 24                                # embedded gate rows: g_ld = A + D + 4n, the gates behind column A + D


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    itype = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(itype), b.view(itype))


def close_abs(got, ref, what, tol=TOL):
    """within ``tol`` of the reference's largest magnitude"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    print("%-34s max|d|=%.3e  max|ref|=%.3e" % (what, err, scale))
    assert err <= tol * scale, "%s: max|d|=%.3e > %.1e * %.3e" % (what, err, tol, scale)
    return err


def close(a, b, tol=TOL, what=""):
    """the project's comparison (test_gpu_weight_drop.py): within tol * max(1, max|reference|)"""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print("%-60s max|d|=%.3e  scale %.3g" % (what, err, scale))
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol)
    return err


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
class Frame:
    """a device buffer of ``rows`` x ``ld`` floats between two NaN guard bands; ``view`` = its columns [off, off + width).  The whole
    buffer starts as NaN, so everything a kernel must not touch is still NaN afterwards (bit pattern included)."""

    def __init__(self, rows, width, ld=None, off=0, dtype=torch.float32, fill=None):
        self.rows, self.width, self.ld, self.off = rows, width, ld or width, off
        self.buf = torch.full((rows * self.ld + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.body = self.buf[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.view = self.body[:, off:off + width]
        if fill is not None:
            self.view.copy_(fill.to(dtype))

    @property
    def ptr(self):
        return self.buf.data_ptr() + (GUARD + self.off) * self.buf.element_size()

    def intact(self):
        """guards and the columns outside the view are untouched"""
        b = self.buf.float()
        outside = torch.ones(self.rows, self.ld, dtype=torch.bool, device="cuda")
        outside[:, self.off:self.off + self.width] = False
        return bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + self.rows * self.ld:]).all()) and bool(torch.isnan(self.body.float()[outside]).all())


def live_mask(rows):
    """dead rows first, last and in the middle (5 rows and more); 3 rows: the middle one; fewer: all live"""
    live = torch.ones(rows, dtype=torch.int32)
    if rows >= 5:
        live[0] = live[-1] = live[rows // 2] = 0
    elif rows >= 3:
        live[rows // 2] = 0
    return live


@functools.lru_cache(maxsize=None)
def cell_case(rows, n, with_gy, seed=0):
    """inputs of one cell call and the float64 reference with its autograd gradients (computed once, shared, read-only)"""
    from oracle import prng
    u = lambda shape, s, lo=-1.0, hi=1.0: torch.from_numpy(prng.uniform(shape, 1000 * seed + s, lo, hi))
    d = dict(a=u((rows, 4 * n), 1, -2.0, 2.0), gy=u((rows, 4 * n), 2) if with_gy else None, c_prev=u((rows, n), 3), h_prev=u((rows, n), 4),
             dh_out=u((rows, n), 5), dh_carry=u((rows, n), 6), dc_carry=u((rows, n), 7), live=live_mask(rows),
             gw=u((4 * n,), 8, 0.5, 1.5), gb=u((4 * n,), 9, -0.5, 0.5), cw=u((n,), 10, 0.5, 1.5), cb=u((n,), 11, -0.5, 0.5))
    lv = d["live"].bool()
    leaf = {k: d[k].double().clone().requires_grad_() for k in ("a", "c_prev", "gw", "gb", "cw", "cb")}
    pre = leaf["a"] + (d["gy"].double() if with_gy else 0.0)
    out = R.ln_cell(pre[lv], leaf["c_prev"][lv], leaf["gw"], leaf["gb"], leaf["cw"], leaf["cb"])
    dh = (d["dh_out"] + d["dh_carry"]).double()
    loss = (out["h"] * dh[lv]).sum() + (out["c"] * d["dc_carry"].double()[lv]).sum()
    loss.backward()
    full = lambda t, width: torch.zeros(rows, width, dtype=torch.float64).index_put((torch.nonzero(lv).flatten(),), t.detach())
    ref = dict(gates=full(out["gates"], 4 * n), c=d["c_prev"].double().clone(), h=d["h_prev"].double().clone(), xhat=out["xhat"].detach(), rstd=out["rstd"].detach(),
               dgates=leaf["a"].grad * lv.unsqueeze(1), dc_prev=leaf["c_prev"].grad, dgw=leaf["gw"].grad, dgb=leaf["gb"].grad, dcw=leaf["cw"].grad,
               dcb=leaf["cb"].grad)
    ref["c"][lv] = out["c"].detach(); ref["h"][lv] = out["h"].detach()
    return d, ref


def run_cell_fwd(L, d, rows, n, embedded, in_place=False, save=True, bf16=True):
    ld, off = (A_OFF + D_OFF + 4 * n, A_OFF + D_OFF) if embedded else (4 * n, 0)
    dev = lambda t, dt=None: None if t is None else t.cuda().contiguous()
    f = dict(gates=Frame(rows, 4 * n, ld, off, fill=d["a"]), c_prev=Frame(rows, n, fill=d["c_prev"]), h_prev=Frame(rows, n, fill=d["h_prev"]))
    f["c_new"] = f["c_prev"] if in_place else Frame(rows, n)
    f["h_new"] = f["h_prev"] if in_place else Frame(rows, n)
    f["hb"] = Frame(rows, n, dtype=torch.bfloat16) if bf16 else None
    f["xhat"] = Frame(rows, 5 * n) if save else None
    f["rstd"] = Frame(rows, 5) if save else None
    keep = [dev(d[k]) for k in ("gy", "live", "gw", "gb", "cw", "cb")]
    gy, live, gw, gb, cw, cb = keep
    p = lambda fr: None if fr is None else C.c_void_p(fr.ptr)
    L.check(L.lib().sat_lstm_ln_cell_fwd(p(f["gates"]), ld, L.ptr(gy), p(f["c_prev"]), p(f["h_prev"]), p(f["c_new"]), p(f["h_new"]), L.ptr(live), p(f["hb"]),
                                         L.ptr(gw), L.ptr(gb), L.ptr(cw), L.ptr(cb), p(f["xhat"]), p(f["rstd"]), rows, n, L.stream_ptr()), "sat_lstm_ln_cell_fwd")
    torch.cuda.synchronize()
    return f


def run_cell_bwd(L, d, fwd, rows, n, embedded, part=None, bf16=True):
    ld, off = (A_OFF + D_OFF + 4 * n, A_OFF + D_OFF) if embedded else (4 * n, 0)
    f = dict(dh_carry=Frame(rows, n, fill=d["dh_carry"]), dc_carry=Frame(rows, n, fill=d["dc_carry"]), dgates=Frame(rows, 4 * n, ld, off),
             dgb=Frame(rows, 4 * n, ld, off, dtype=torch.bfloat16) if bf16 else None)
    dh_out, c_prev, live, gw, cw, cb = [d[k].cuda().contiguous() for k in ("dh_out", "c_prev", "live", "gw", "cw", "cb")]
    p = lambda fr: None if fr is None else C.c_void_p(fr.ptr)
    L.check(L.lib().sat_lstm_ln_cell_bwd(p(fwd["gates"]), ld, L.ptr(c_prev), p(fwd["xhat"]), p(fwd["rstd"]), L.ptr(dh_out), p(f["dh_carry"]), p(f["dc_carry"]),
                                         p(f["dgates"]), ld, L.ptr(live), p(f["dgb"]), L.ptr(gw), L.ptr(cw), L.ptr(cb), L.ptr(part), rows, n, L.stream_ptr()),
            "sat_lstm_ln_cell_bwd")
    torch.cuda.synchronize()
    return f


def finish_partials(L, part, slots, n):
    outs = [Frame(1, w) for w in (4 * n, 4 * n, n, n)]
    scratch = torch.empty(16 * n, device="cuda")
    L.check(L.lib().sat_lstm_ln_param_grads(L.ptr(part), slots, n, *[C.c_void_p(o.ptr) for o in outs], L.ptr(scratch), L.stream_ptr()), "sat_lstm_ln_param_grads")
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)
    return [o.view.reshape(-1).cpu() for o in outs]


SHAPES = [(1, 1), (1, 3), (5, 20), (33, 64), (7, 65), (3, 260), (1100, 20)]      # the last: more rows than blocks (two rows in some blocks)


@pytest.mark.parametrize("with_gy", [False, True], ids=["nogy", "gy"])
@pytest.mark.parametrize("embedded", [False, True], ids=["dense", "embedded"])
@pytest.mark.parametrize("rows,n", SHAPES)
def test_cell_forward_in_nan_frames(L, rows, n, embedded, with_gy):
    d, ref = cell_case(rows, n, with_gy)
    lv = d["live"].bool()
    f = run_cell_fwd(L, d, rows, n, embedded)
    tag = "fwd %dx%d %s%s " % (rows, n, "embedded" if embedded else "dense", " +gy" if with_gy else "")
    for k in ("gates", "c_new", "h_new", "hb", "xhat", "rstd", "c_prev", "h_prev"):
        assert f[k].intact(), tag + k
    assert bits_equal(f["c_prev"].view, d["c_prev"]) and bits_equal(f["h_prev"].view, d["h_prev"])          # out of place: inputs read only
    close_abs(f["gates"].view, ref["gates"], tag + "gates")
    close_abs(f["c_new"].view, ref["c"], tag + "c")
    close_abs(f["h_new"].view, ref["h"], tag + "h")
    close_abs(f["xhat"].view[lv.cuda()], ref["xhat"], tag + "xhat")
    close_abs(f["rstd"].view[lv.cuda()], ref["rstd"], tag + "rstd")
    # dead rows: state carried bit for bit, zero gates, nothing saved
    dead = ~lv
    assert bits_equal(f["c_new"].view.cpu()[dead], d["c_prev"][dead]) and bits_equal(f["h_new"].view.cpu()[dead], d["h_prev"][dead])
    assert float(f["gates"].view.cpu()[dead].abs().sum()) == 0.0 if bool(dead.any()) else True
    assert bool(torch.isnan(f["xhat"].view.cpu()[dead]).all()) and bool(torch.isnan(f["rstd"].view.cpu()[dead]).all())
    assert bits_equal(f["hb"].view, f["h_new"].view.to(torch.bfloat16))                                   # bf16 copy = the rounded fp32 output
    # in place (c_new == c_prev, h_new == h_prev: the searches' call), without the bf16 copy and the saved values: the same bits
    g = run_cell_fwd(L, d, rows, n, embedded, in_place=True, save=False, bf16=False)
    assert bits_equal(g["c_new"].view, f["c_new"].view) and bits_equal(g["h_new"].view, f["h_new"].view) and bits_equal(g["gates"].view, f["gates"].view)
    assert g["gates"].intact() and g["c_new"].intact() and g["h_new"].intact()


@pytest.mark.parametrize("with_gy", [False, True], ids=["nogy", "gy"])
@pytest.mark.parametrize("embedded", [False, True], ids=["dense", "embedded"])
@pytest.mark.parametrize("rows,n", SHAPES)
def test_cell_backward_in_nan_frames(L, rows, n, embedded, with_gy):
    d, ref = cell_case(rows, n, with_gy)
    lv = d["live"].bool()
    fwd = run_cell_fwd(L, d, rows, n, embedded)
    slots = L.lib().sat_lstm_ln_slots(rows)
    assert slots == min(rows, 1024)
    pf = Frame(slots, 10 * n, fill=torch.zeros(slots, 10 * n))
    part = pf.view
    b = run_cell_bwd(L, d, fwd, rows, n, embedded, part)
    tag = "bwd %dx%d %s%s " % (rows, n, "embedded" if embedded else "dense", " +gy" if with_gy else "")
    for k in ("dh_carry", "dc_carry", "dgates", "dgb"):
        assert b[k].intact(), tag + k
    assert pf.intact() and fwd["gates"].intact() and fwd["xhat"].intact()
    close_abs(b["dgates"].view, ref["dgates"], tag + "dgates")
    dead = ~lv
    if bool(dead.any()):
        assert float(b["dgates"].view.cpu()[dead].abs().sum()) == 0.0 and float(b["dgb"].view.float().cpu()[dead].abs().sum()) == 0.0
        assert bits_equal(b["dc_carry"].view.cpu()[dead], d["dc_carry"][dead]) and bits_equal(b["dh_carry"].view.cpu()[dead], d["dh_carry"][dead])
    close_abs(b["dc_carry"].view.cpu()[lv], ref["dc_prev"][lv], tag + "dc_carry")
    assert float(b["dh_carry"].view.cpu()[lv].abs().sum()) == 0.0                                         # the GEMM after the cell accumulates dh_{t-1}
    assert bits_equal(b["dgb"].view, b["dgates"].view.to(torch.bfloat16))
    dgw, dgb_, dcw, dcb = finish_partials(L, part, slots, n)
    for got, key in ((dgw, "dgw"), (dgb_, "dgb"), (dcw, "dcw"), (dcb, "dcb")):
        close_abs(got, ref[key], tag + key)
    # without the partials and the bf16 copy: the same gate gradients
    b2 = run_cell_bwd(L, d, fwd, rows, n, embedded, None, bf16=False)
    assert bits_equal(b2["dgates"].view, b["dgates"].view) and bits_equal(b2["dc_carry"].view, b["dc_carry"].view)


@pytest.mark.parametrize("rows,n", [(33, 64), (1100, 20), (7, 65)])
def test_parameter_gradient_partials_over_three_steps(L, rows, n):
    """three backward launches with changing live masks add into the same slots; the finishing sum equals the float64 sums; bit-reproducible"""
    slots = L.lib().sat_lstm_ln_slots(rows)
    want = [torch.zeros(w, dtype=torch.float64) for w in (4 * n, 4 * n, n, n)]
    cases = []
    for step in range(3):
        d, _ = cell_case(rows, n, step == 1, seed=step + 1)
        d = dict(d)
        live = torch.ones(rows, dtype=torch.int32)
        live[step::3] = 0                                       # another third of the rows is dead at every step
        d["live"] = live
        lv = live.bool()
        leaf = {k: d[k].double().clone().requires_grad_() for k in ("gw", "gb", "cw", "cb")}
        pre = d["a"].double() + (d["gy"].double() if d["gy"] is not None else 0.0)
        out = R.ln_cell(pre[lv], d["c_prev"].double()[lv], leaf["gw"], leaf["gb"], leaf["cw"], leaf["cb"])
        ((out["h"] * (d["dh_out"] + d["dh_carry"]).double()[lv]).sum() + (out["c"] * d["dc_carry"].double()[lv]).sum()).backward()
        for w, k in zip(want, ("gw", "gb", "cw", "cb")):
            w += leaf[k].grad
        cases.append(d)
    runs = []
    for _ in range(2):
        pf = Frame(slots, 10 * n, fill=torch.zeros(slots, 10 * n))
        for d in cases:
            fwd = run_cell_fwd(L, d, rows, n, False, bf16=False)
            run_cell_bwd(L, d, fwd, rows, n, False, pf.view, bf16=False)
        assert pf.intact()
        runs.append(finish_partials(L, pf.view, slots, n))
    for got, again, ref, key in zip(runs[0], runs[1], want, ("dgw", "dgb", "dcw", "dcb")):
        close_abs(got, ref, "partials %dx%d %s" % (rows, n, key))
        assert bits_equal(got, again), key


# ---------------------------------------------------------------------------------------------- 2. the train step against the oracle
B, NR, T, V, HH, WW = 2, 3, 7, 40, 2, 3                # NR captions per image
SEED = 123456789
DRAWS = [0.9, 0.1, 0.8, 0.2, 0.7, 0.3]
SMALL = dict(A=7, D=24, m=12, n=20)                 # test_gpu_weight_drop.py's shapes
ALIGNED = dict(A=8, D=64, m=12, n=64)               # bf16 mode keeps bf16 operand copies only at n % 64 == D % 64 == 0
LENGTHS = [[1, 6, 3], [6, 2, 4]]                    # ragged: a caption of length 1 and one of full length T - 1


@pytest.fixture(scope="module")
def M():
    import sat_amd  # noqa: F401
    from sat_amd import model
    return model


def make_hp(layers=1, shape="small", **over):
    from oracle import sat_oracle as O
    s = SMALL if shape == "small" else ALIGNED
    return O.default_hparams(**dict(dict(vocab_size=V, encoder_dim=s["D"], embed_dim=s["m"], attention_dim=s["A"], decoder_dim=s["n"], decoder_layers=layers,
                                         lstm_layer_norm=True), **over))


@functools.lru_cache(maxsize=None)
def inputs(layers, shape="small", deep=True):
    """(state dict with random layer-norm gains in [0.5, 1.5] and shifts in [-0.5, 0.5], annotations (B, D, h, w), captions, lengths): read-only"""
    from oracle import prng
    hp = make_hp(layers, shape, deep_output=deep)
    sd = {k: torch.from_numpy(v) for k, v in prng.decoder_state(hp, 71 + layers).items()}
    sd.update(R.ln_state(hp.decoder_dim, layers, 500 + layers))
    ann = torch.from_numpy(prng.uniform((B, hp.encoder_dim, HH, WW), 911))
    caps, _ = prng.captions(B, NR, T, V, 912, ragged=False)
    lengths = torch.tensor(LENGTHS)
    caps = torch.from_numpy(caps)
    for i in range(B):                                          # the wire format: <END> closes every caption, <PAD> follows
        for j in range(NR):
            ln = int(lengths[i, j])
            caps[i, j, ln] = V - 1
            caps[i, j, ln + 1:] = 0
    assert int(lengths.min()) == 1 and int(lengths.max()) == T - 1
    return sd, ann, caps, lengths


def decode(M, hp, sd, layers, shape="small", eps=1.0, precision="fp32", train=True, seed=SEED, reg=False, leaf_side=False, deep=True):
    """one train_decode + backward of a fresh decoder; everything comes back on the host"""
    _, ann, caps, lengths = inputs(layers, shape, deep)
    dec = M.SATDecoder(hp).cuda()
    dec.load_decoder_state(sd)
    dec.train(train)
    dec.sat_precision = precision
    ann_bld = ann.permute(0, 2, 3, 1).reshape(B, HH * WW, hp.encoder_dim).contiguous().cuda().requires_grad_()
    it = iter(DRAWS)
    res = dec.train_decode(ann_bld, caps.cuda(), lengths, eps, draw=lambda: next(it), dropout_seed=seed, leaf_side=leaf_side)
    out = dict(logits=res["logits_packed"].detach().cpu(), alphas=res["alphas"].detach().cpu(), plan=res["plan"])
    loss = res["ce"] + res["ds"]
    if reg:
        loss = dec.add_reg_terms(loss, res["reg"])
        out.update(ar=res["ar"].cpu(), tar=res["tar"].cpu())
    loss.backward()
    torch.cuda.synchronize()
    out.update(loss=loss.detach().cpu(), d_ann=ann_bld.grad.cpu(), grads={k: p.grad.cpu() for k, p in dec.named_parameters()})
    return out


def compare_with_oracle(got, loss_o, out_o, leaves, ann_o, what, layers):
    close(got["logits"], out_o["logits_packed"], what="logits " + what)
    close(got["alphas"], out_o["alphas"], what="alphas " + what)
    close(got["loss"], loss_o, what="loss " + what)
    close(got["d_ann"].reshape(B, HH, WW, -1).permute(0, 3, 1, 2), ann_o.grad, what="d_ann " + what)
    assert set(R.ln_keys(layers)) <= set(got["grads"])
    for k, g in got["grads"].items():
        assert leaves[k].grad is not None, k
        close(g, leaves[k].grad, what=k + " " + what)


@pytest.mark.parametrize("deep", [True, False], ids=["deep", "shallow"])
@pytest.mark.parametrize("eps", [1.0, 0.5])
@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("shape", ["small", "aligned"])
def test_train_step_against_the_oracle(M, shape, layers, eps, deep):
    hp = make_hp(layers, shape, deep_output=deep)
    sd, ann, caps, lengths = inputs(layers, shape, deep)
    got = decode(M, hp, sd, layers, shape, eps, deep=deep)
    leaves = {k: v.clone().requires_grad_() for k, v in sd.items()}
    ann_o = ann.clone().requires_grad_()
    it = iter(DRAWS)
    loss_o, out_o = R.training_loss_ln(leaves, hp, ann_o, caps, lengths, eps, draw=lambda: next(it))
    loss_o.backward()
    compare_with_oracle(got, loss_o, out_o, leaves, ann_o, "%s layers=%d eps=%g %s" % (shape, layers, eps, "deep" if deep else "shallow"), layers)
    # the norm acts: the plain cell on the same weights gives other logits
    with torch.no_grad():
        from oracle import sat_oracle as O
        it = iter(DRAWS)
        _, plain = O.training_loss(sd, hp, ann, caps, lengths, eps, draw=lambda: next(it))
    assert float((plain["logits_packed"] - got["logits"]).abs().max()) > 100 * TOL


def test_with_weight_drop_the_dropouts_and_activation_regularisation_against_the_oracle(M):
    """the flag with everything of the recipe in one step, as test_gpu_weight_drop.py composes it: weight-drop, the per-step dropouts with
    host masks, AR / TAR, two layers, scheduled sampling"""
    import activation_reg_ref as AR
    import test_gpu_weight_drop as W
    from oracle import sat_oracle as O
    layers, p, pe, ar_alpha, tar_beta = 2, 0.3, 0.2, 2.0, 1.0
    sd, ann, caps, lengths = inputs(layers)
    hp = make_hp(layers, weight_drop=0.5, dropout=p, embedding_dropout=pe, ar_alpha=ar_alpha, tar_beta=tar_beta)
    got = decode(M, hp, sd, layers, eps=0.5, reg=True)
    N, lens = B * NR, lengths.reshape(-1)
    from sat_amd import decoder as Dk
    T1 = T - 1
    sc = lambda stream, count, rate: torch.from_numpy(Dk.dropout_scale_reference(SEED, stream, np.arange(count), rate))
    prow = got["plan"].prow.cpu()
    live = prow >= 0
    packed = sc(2, got["plan"].P * hp.embed_dim, p).reshape(got["plan"].P, hp.embed_dim)
    out_mask = torch.zeros(T1, N, hp.embed_dim)
    out_mask[live] = packed[prow[live].long()]
    masks = dict(init=sc(0, N * hp.encoder_dim, p).reshape(N, hp.encoder_dim), emb=sc(1, T1 * N * hp.embed_dim, pe).reshape(T1, N, hp.embed_dim), out=out_mask)
    leaves, sdo = W.oracle_leaves(sd, W.wd_mask(layers, hp.decoder_dim))
    ann_o = ann.clone().requires_grad_()
    hidden = []

    def lstm_fn(sd_, x, h, c, nl):                              # the normalised step; keeps the top-layer state of the live rows
        hn, cn = R.ln_lstm_step(sd_, x, h, c, nl)
        full = torch.zeros(N, hp.decoder_dim)
        full[lens > len(hidden)] = hn[-1]
        hidden.append(full)
        return hn, cn

    it = iter(DRAWS)
    out_o = O.decode_train(sdo, hp, ann_o, caps, lengths, 0.5, lambda: next(it), lstm_fn=lstm_fn, masks=masks)
    while len(hidden) < T1:
        hidden.append(torch.zeros(N, hp.decoder_dim))
    lp, _ = O.pack_time_major(out_o["logits"], out_o["lengths"])
    tp, _ = O.pack_time_major(out_o["targets"], out_o["lengths"])
    ar, tar, _, _ = AR.reg_terms(torch.stack(hidden).double(), lens)
    loss_o = O.label_smoothing_ce(lp, tp, hp.label_smoothing) + O.doubly_stochastic(out_o["alphas"], hp.att_gamma) + (ar_alpha * ar + tar_beta * tar).float()
    loss_o.backward()
    out_o["logits_packed"] = lp
    close(got["ar"], ar, what="ar"); close(got["tar"], tar, what="tar")
    compare_with_oracle(got, loss_o, out_o, leaves, ann_o, "under weight-drop, dropout and AR / TAR", layers)


# ---------------------------------------------------------------------------------------------- 3. off path, side stream, modes
def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _randomise_norm(model, seed=77):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(model.ln_param_list()):
            lo, hi = (0.5, 1.5) if i % 2 == 0 else (-0.5, 0.5)
            p.copy_((lo + (hi - lo) * torch.rand(p.shape, generator=g)).to(p.device))


def test_off_path_is_the_model_without_the_key():
    from test_gpu_graph import _batch, _make
    got = []
    for over in (dict(), dict(lstm_layer_norm=False)):
        model, hp = _make("fp32", over)
        out = model.training_step(_batch(hp, 11), 0)
        out["loss"].backward()
        torch.cuda.synchronize()
        got.append((out["loss"].detach().clone(), out["accuracy"].clone(), _grads(model), list(model.state_dict())))
    (la, aa, ga, ka), (lb, ab, gb, kb) = got
    assert ka == kb and not any(k.startswith("lstm_ln") for k in ka)
    assert torch.equal(la, lb) and torch.equal(aa, ab) and list(ga) == list(gb) and [k for k in ga if not torch.equal(ga[k], gb[k])] == []


def test_side_stream_and_two_eager_runs_leave_the_same_bits(monkeypatch):
    from sat_amd import decoder as Dk, encoder as E
    from test_gpu_graph import _batch, _make
    monkeypatch.setattr(E, "_WGRAD_SIDE_MIN_INPUT_PIXELS", 0)
    monkeypatch.setattr(E, "_WGRAD_STREAM", True)
    runs = []
    for on in (False, True, True):
        monkeypatch.setattr(E, "_DECODER_LEAF_SIDE", on)
        model, hp = _make("bf16", dict(lstm_layer_norm=True, decoder_layers=2, encoder_finetune_after=0))       # the side stream is the bf16 step's
        _randomise_norm(model)
        model.configure_optimizers()                             # ... and wants a trainable trunk
        forks = Dk._leaf_forks[0]
        out = model.training_step(_batch(hp, 11), 0)
        out["loss"].backward()
        g = {k: v.cpu() for k, v in _grads(model).items()}       # no synchronisation in between: the join is the backward's
        assert Dk._leaf_forks[0] - forks == (1 if on else 0)
        runs.append((out["loss"].detach().cpu(), g))
        junk = torch.full((1 << 22,), float("nan"), device="cuda"); del junk
    assert all(k in runs[0][1] for k in ("lstm_ln.gates_l0.weight", "lstm_ln.cell_l1.bias"))
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and [k for k in runs[0][1] if not torch.equal(runs[0][1][k], other[1][k])] == []
    assert float(runs[0][1]["lstm_ln.gates_l0.weight"].abs().max()) > 0


@pytest.mark.parametrize("shape", ["small", "aligned"])
def test_bf16_mode_is_finite_and_reproducible(M, shape):
    """the deviation of loss and logits from fp32 mode is printed (DESIGN.md 5 records it next to the plain cell's), not asserted"""
    layers = 1
    sd = inputs(layers, shape)[0]
    hp = make_hp(layers, shape)
    a = decode(M, hp, sd, layers, shape, precision="bf16")
    b = decode(M, hp, sd, layers, shape, precision="bf16")
    f = decode(M, hp, sd, layers, shape, precision="fp32")
    assert bool(torch.isfinite(a["logits"]).all()) and bool(torch.isfinite(a["loss"])) and all(bool(torch.isfinite(g).all()) for g in a["grads"].values())
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["d_ann"], b["d_ann"])
    assert [k for k in a["grads"] if not torch.equal(a["grads"][k], b["grads"][k])] == []
    plain_sd = {k: v for k, v in sd.items() if not k.startswith("lstm_ln")}
    hp0 = make_hp(layers, shape, lstm_layer_norm=False)
    pb, pf = decode(M, hp0, plain_sd, layers, shape, precision="bf16"), decode(M, hp0, plain_sd, layers, shape, precision="fp32")
    for name, x, y in (("normalised", a, f), ("plain", pb, pf)):
        print("%s %s cell, bf16 against fp32 mode: loss %.3e relative, logits max|d| %.3e (max|logit| %.3g)"
              % (shape, name, abs(float(x["loss"]) - float(y["loss"])) / abs(float(y["loss"])), float((x["logits"] - y["logits"]).abs().max()),
                 float(y["logits"].abs().max())))


def test_graph_replay_equals_the_eager_normalised_step():
    from sat_amd.graph import GraphedTrainStep
    from test_gpu_graph import _batch, _make, _same, _state
    over = dict(lstm_layer_norm=True, decoder_layers=2)
    eager, hp = _make("fp32", over)
    graphed, _ = _make("fp32", over)
    _randomise_norm(eager); _randomise_norm(graphed)
    opt_e, opt_g = eager.configure_optimizers(), graphed.configure_optimizers()
    assert all(any(p is q for g in opt_g.param_groups for q in g["params"]) for p in graphed.ln_param_list())
    step = GraphedTrainStep(graphed, opt_g)
    b = _batch(hp, 11)
    before = [p.detach().clone() for p in graphed.ln_param_list()]
    for it in range(4):          # step 0 warms eagerly, step 1 captures and replays, steps 2 and 3 replay
        opt_e.zero_grad(set_to_none=True)
        out_e = eager.training_step(b, it)
        out_e["loss"].backward()
        opt_e.step()
        out_g = step(b, it)
        assert torch.equal(out_e["loss"].detach(), out_g["loss"]), "step %d: loss %r vs %r" % (it, float(out_e["loss"]), float(out_g["loss"]))
        _same(_state(eager, opt_e), _state(graphed, opt_g), "after step %d" % it)
    assert step.stats["captured"] == 1 and step.stats["replayed"] == 3, dict(step.stats)
    assert all(not torch.equal(a, p) for a, p in zip(before, graphed.ln_param_list()))          # the replayed steps train the norm
    # the flag is part of the key
    assert len(step._graphs) == 1 and all(k[-1] is True for k in step._graphs)
    plain, _ = _make("fp32", dict(decoder_layers=2))
    pstep = GraphedTrainStep(plain, plain.configure_optimizers())
    pstep(b, 0)
    assert len(pstep._graphs) == 1 and all(k[-1] is False for k in pstep._graphs)


def test_checkpoint_round_trip_and_a_plain_checkpoint(M):
    layers = 2
    sd, ann, caps, lengths = inputs(layers)
    hp = make_hp(layers)
    a = M.SATDecoder(hp).cuda().eval()
    a.load_decoder_state(sd)
    b = M.SATDecoder(hp).cuda().eval()
    b.load_state_dict(a.state_dict())
    ann_bld = ann.permute(0, 2, 3, 1).reshape(B, HH * WW, hp.encoder_dim).contiguous().cuda()
    outs = [m.train_decode(ann_bld, caps.cuda(), lengths, 1.0, with_loss=False)["logits_packed"] for m in (a, b)]
    assert torch.equal(outs[0], outs[1])
    plain = {k: v for k, v in sd.items() if not k.startswith("lstm_ln")}
    c = M.SATDecoder(hp).cuda().eval()
    c.load_decoder_state(plain)                                 # raises nothing; the norm keeps its initial values
    for k, v in c.state_dict().items():
        if k.startswith("lstm_ln"):
            assert bool((v == (1.0 if k.endswith("weight") else 0.0)).all()), k
        else:
            assert torch.equal(v.cpu(), plain[k]), k


# ---------------------------------------------------------------------------------------------- 4. the searches
K, S = 3, 6
NOISE = 0.3
#: model seeds chosen on the CPU with the oracle alone so that no selection of O.beam_search(lstm_fn=ln_lstm_step) rests on a near-tie:
#: (layers, noise) -> seed; search_case asserts the margins again
SEARCH_SEEDS = {(1, False): 1, (2, False): 1, (1, True): 6, (2, True): 4}      # measured margins: 5.9e-3, 2.4e-3, 2.5e-3, 2.1e-2
NB = 3
MIXED_SEED = 3                                      # ensemble_ref's margins with it: 3.4e-3 (arithmetic), 7.6e-3 (geometric)


def search_state(layers, seed):
    from oracle import prng
    hp = make_hp(layers)
    sd = {k: torch.from_numpy(v) for k, v in prng.decoder_state(hp, 300 + seed).items()}
    sd.update(R.ln_state(hp.decoder_dim, layers, 700 + seed))
    ann = torch.from_numpy(prng.uniform((NB, hp.encoder_dim, HH, WW), 40 + seed, 0.0, 1.0))
    g = torch.Generator().manual_seed(seed)
    normals = torch.randn(S + 1, layers, NB * K, hp.decoder_dim, generator=g)
    return hp, sd, ann, normals


def oracle_search(layers, noise, seed):
    """O.beam_search(lstm_fn=ln_lstm_step) image by image (the noise hook reads the table by step and row), with the gap between the last
    kept and the first rejected score of every selection: (captions, scores, alphas, perplexities, smallest selection gap, smallest
    gap between two final scores of an image)"""
    import history_ref as HR
    from oracle import sat_oracle as O
    hp, sd, ann, normals = search_state(layers, seed)
    gaps, real_topk = [], torch.topk

    def topk(x, k, *a, **kw):
        if x.dim() == 1:
            gaps.append(HR._boundary_gap(x, k))
        return real_topk(x, k, *a, **kw)

    res = [[], [], [], []]
    final = []
    torch.topk = topk
    try:
        with torch.no_grad():
            for b in range(NB):
                state = {"step": 0}

                def randn(shape, b=b, state=state):
                    s_ = state["step"]; state["step"] += 1
                    return normals[s_, :, b * K:b * K + shape[1], :]

                out = O.beam_search(sd, hp, ann[b:b + 1], beamk=K, max_gen_length=S, return_all=True, lstm_fn=R.ln_lstm_step,
                                    decoder_noise=NOISE if noise else None, randn=randn)
                for r, o in zip(res, out):
                    r.append(o[0])
                s = out[1][0]
                final += [x - y for x, y in zip(s, s[1:])]
    finally:
        torch.topk = real_topk
    return (*res, min(g for g in gaps if g is not None), min(final) if final else float("inf"))


@functools.lru_cache(maxsize=None)
def search_case(layers, noise):
    seed = SEARCH_SEEDS[(layers, noise)]
    want = oracle_search(layers, noise, seed)
    print("search layers=%d noise=%s seed %d: selection margin %.2e, final %.2e" % (layers, noise, seed, want[4], want[5]))
    assert want[4] > 1e-3 and want[5] > 1e-3, "the oracle's own selection rests on a near-tie: choose another seed"
    return want


def check_search(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    for b in range(NB):
        for x, y in zip(got[1][b], want[1][b]):
            assert abs(x - y) <= TOL * max(1.0, abs(y)), (what, b, x, y)
        for x, y in zip(got[2][b], want[2][b]):
            x = x.cpu().reshape(y.shape)
            assert float((x - y).abs().max()) <= TOL, (what, b)


@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noise"])
@pytest.mark.parametrize("layers", [1, 2])
def test_searches_against_the_oracle(M, layers, noise):
    want = search_case(layers, noise)
    hp, sd, ann, normals = search_state(layers, SEARCH_SEEDS[(layers, noise)])
    dec = M.SATDecoder(hp).cuda().eval()
    dec.load_decoder_state(sd)
    ann_bld = ann.permute(0, 2, 3, 1).reshape(NB, HH * WW, hp.encoder_dim).contiguous().cuda()
    kw = dict(beamk=K, max_gen_length=S, return_all=True)
    if noise:
        got_b = dec.beam_decode_batched(ann_bld, (HH, WW), decoder_noise=NOISE, normals=normals.cuda().contiguous(), **kw)
    else:
        got_b = dec.beam_decode_batched(ann_bld, (HH, WW), **kw)
    check_search(got_b, want, "batched")
    loop = [[], [], [], []]
    for b in range(NB):
        state = {"step": 0}

        def randn(shape, b=b, state=state):
            s_ = state["step"]; state["step"] += 1
            return normals[s_, :, b * K:b * K + shape[1], :].cuda()

        one = dec.beam_decode(ann_bld[b:b + 1], (HH, WW), decoder_noise=NOISE if noise else None, randn=randn, **kw)
        for r, o in zip(loop, one):
            r.append(o[0])
    check_search(loop, want, "per-image loop")


def test_ensemble_of_one_normalised_model_is_that_model(M):
    from sat_amd.ensemble import Ensemble
    search_case(1, False)
    hp, sd, ann, _ = search_state(1, SEARCH_SEEDS[(1, False)])
    dec = M.SATDecoder(hp).cuda().eval()
    dec.load_decoder_state(sd)
    ann_bld = ann.permute(0, 2, 3, 1).reshape(NB, HH * WW, hp.encoder_dim).contiguous().cuda()
    kw = dict(beamk=K, max_gen_length=S, return_all=True)
    want = dec.beam_decode_batched(ann_bld, (HH, WW), **kw)
    got = Ensemble([dec], [1.0], "arithmetic").beam_decode_batched([ann_bld], (HH, WW), **kw)
    assert got[0] == want[0]
    for b in range(NB):
        for x, y in zip(got[1][b], want[1][b]):
            assert abs(x - y) <= 1e-5 * max(1.0, abs(y))
        for x, y in zip(got[2][b], want[2][b]):
            assert float((x - y).abs().max()) <= 1e-5


@pytest.mark.parametrize("mode", ["arithmetic", "geometric"])
def test_ensemble_of_a_normalised_and_a_plain_member(M, mode, monkeypatch):
    """the first two steps (max_gen_length = 1) against ensemble_ref with each member's own cell: the host combination of the two oracles'
    per-step distributions, one shared selection"""
    import ensemble_ref as ER
    from oracle import sat_oracle as O
    from sat_amd.ensemble import Ensemble
    hp1, sd1, ann, _ = search_state(1, MIXED_SEED)
    hp0 = make_hp(2, lstm_layer_norm=False)
    from oracle import prng
    sd0 = {k: torch.from_numpy(v) for k, v in prng.decoder_state(hp0, 900 + MIXED_SEED).items()}
    plain_step = O.lstm_step
    monkeypatch.setattr(O, "lstm_step", lambda sd, x, h, c, layers: (R.ln_lstm_step if "lstm_ln.gates_l0.weight" in sd else plain_step)(sd, x, h, c, layers))
    weights = [0.6, 0.4]
    kw = dict(beamk=K, max_gen_length=1, return_all=True)
    m = {}
    with torch.no_grad():
        want = ER.beam_search([(sd1, hp1, ann), (sd0, hp0, ann)], weights, mode, margins=m, **kw)
    boundary = min(x for x in m["boundary"] if x is not None)
    final = min(g for img in m["final"] for g in img)
    print("mixed ensemble %s: selection margin %.2e, final %.2e" % (mode, boundary, final))
    assert boundary > 1e-3 and final > 1e-3
    decs = []
    for hp, sd in ((hp1, sd1), (hp0, sd0)):
        d = M.SATDecoder(hp).cuda().eval()
        d.load_decoder_state(sd)
        decs.append(d)
    assert decs[0].lstm_layer_norm_on() and not decs[1].lstm_layer_norm_on()
    ann_bld = ann.permute(0, 2, 3, 1).reshape(NB, HH * WW, hp1.encoder_dim).contiguous().cuda()
    got = Ensemble(decs, weights, mode).beam_decode_batched([ann_bld, ann_bld], (HH, WW), **kw)
    check_search(got, want, "mixed ensemble " + mode)

