"""GPU: knowledge distillation ("Distillation") against its float64 specification (tests/distill_ref.py) and the CPU oracle:
the loss / gradient kernels (csrc/distill_loss.hip) through the C ABI in both of their forms (the forward writes the gradient and the
backward scales it in place; the backward produces it from the row scratch), ``DistillFn``, ``distill.loss`` and ``SAT.distill_step``.

Tolerances.  The kernels: test_gpu_scst.py::test_policy_kernels_against_the_reference's, 5e-6 of the largest reference entry (floored at
1) for every array, gradient included (gscale is 1.7 P here, so the largest gradient entry is O(1) and the floor does not hide it), and
5e-6 of the sum of the magnitudes of its terms (floored at 1) for each of the three mean losses.  The whole loss: test_gpu_train_step.py's
1e-4 max(1, |loss|) and 1e-3 relative norm for every parameter gradient and for the annotations' gradient (on the damped net, as
test_scst_loss_and_every_gradient_against_the_oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

import distill_ref as R

pytestmark = pytest.mark.gpu

TOL = 5e-6
BAND = 64            # guard elements on either side of every output array
INT_GUARD = -123456789


def rows(P, V, M, seed):
    """student and teacher logits ~ 3 N(0, 1)-like (uniform sums, test_gpu_scst.py::rows), targets anywhere in [0, V), weights > 0 summing to 1"""
    from oracle import prng

    def one(s):
        x = (prng.uniform((P, V), s, -1.0, 1.0) + prng.uniform((P, V), s + 1, -1.0, 1.0) + prng.uniform((P, V), s + 2, -1.0, 1.0)) * 3.0
        return torch.from_numpy(x.astype(np.float32))

    z = one(seed)
    ts = [one(seed + 10 * (i + 1)) for i in range(M)]
    y = torch.from_numpy(prng.integers((P,), seed + 3, 0, V))
    w = prng.uniform((M,), seed + 4, 0.2, 1.0).astype(np.float64)
    w = (w / w.sum()).astype(np.float32)
    return z, ts, [float(x) for x in w], y


def close(a, b, tol=TOL, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    err = float(np.abs(a - b).max()) if b.size else 0.0
    print("%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol))
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, tol)


class Banded:
    """an output array of n elements inside a guard band (NaN, or INT_GUARD for int32), optionally one element off 16-byte alignment"""

    def __init__(self, n, dtype=torch.float32, off=0):
        self.fill = float("nan") if dtype == torch.float32 else INT_GUARD
        self.buf = torch.full((n + 2 * BAND + 4,), self.fill, dtype=dtype, device="cuda")
        self.lo, self.n = BAND + off, n
        self.view = self.buf[self.lo:self.lo + n]

    def intact(self):
        b = self.buf.cpu()
        edge = torch.cat([b[:self.lo], b[self.lo + self.n:]])
        return bool(torch.isnan(edge).all()) if b.dtype == torch.float32 else bool((edge == INT_GUARD).all())


def run_kernels(z, ts, w, combine, y, inv_tau, alpha, smoothing, g, fused, misalign=False):
    """sat_distill_fwd / _bwd through the C ABI, every output inside a guard band.  ``fused``: the forward writes the gradient and the
    backward is the in-place scale; otherwise the backward produces it.  ``misalign`` moves the student's and the teachers' logits and
    dlogits one float off their 16-byte alignment (the 4-byte form)."""
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    lib = L.lib()
    P, V = z.shape
    M = len(ts)
    off = 1 if misalign else 0

    def place(x):
        buf = torch.empty(P * V + 4, dtype=torch.float32, device="cuda")
        v = buf[off:off + P * V].view(P, V)
        v.copy_(x)
        assert (v.data_ptr() % 16 != 0) == misalign
        return v

    zd, td = place(z), [place(t) for t in ts]
    yd = y.to(torch.int32).cuda()
    gd = torch.tensor([g], dtype=torch.float32, device="cuda")
    o = dict(dlogits=Banded(P * V, off=off), out=Banded(4), lse=Banded(2 * P), tlse=Banded(P * M), cnorm=Banded(P), rows=Banded(2 * P),
             correct=Banded(P, torch.int32))
    tarr = (C.c_void_p * M)(*[t.data_ptr() for t in td])
    warr = (C.c_float * M)(*w)
    cmb = L.ENSEMBLE_COMBINE[combine]
    dl = o["dlogits"].view
    L.check(lib.sat_distill_fwd(L.ptr(zd), tarr, warr, M, cmb, L.ptr(yd), P, V, inv_tau, alpha, smoothing, L.ptr(o["lse"].view), L.ptr(o["tlse"].view),
                                L.ptr(o["cnorm"].view), L.ptr(o["rows"].view), L.ptr(o["correct"].view), L.ptr(o["out"].view), L.ptr(dl) if fused else None,
                                L.stream_ptr()), "sat_distill_fwd")
    L.check(lib.sat_distill_bwd(L.ptr(zd), tarr, warr, M, cmb, L.ptr(yd), P, V, inv_tau, alpha, smoothing, L.ptr(o["lse"].view), L.ptr(o["tlse"].view),
                                L.ptr(o["cnorm"].view), L.ptr(gd), int(fused), L.ptr(dl), L.stream_ptr()), "sat_distill_bwd")
    torch.cuda.synchronize()
    got = dict(out=o["out"].view.cpu(), lse=o["lse"].view.cpu().view(P, 2), tlse=o["tlse"].view.cpu().view(P, M), cnorm=o["cnorm"].view.cpu(),
               rows=o["rows"].view.cpu().view(P, 2), correct=o["correct"].view.cpu(), grad=dl.cpu().view(P, V))
    got["intact"] = all(b.intact() for b in o.values())
    return got


def check_against_reference(ref, got, alpha, tau, what):
    assert got["intact"], what + ": a guard band was written"
    close(got["lse"], ref["lse"], what=what + " lse"); close(got["tlse"], ref["tlse"], what=what + " teacher lse")
    close(got["cnorm"], ref["cnorm"], what=what + " c normaliser")
    close(got["rows"][:, 0], ref["hard_rows"], what=what + " hard rows"); close(got["rows"][:, 1], ref["soft_rows"], what=what + " soft rows")
    P = ref["hard_rows"].numel()
    th, ts_ = float(ref["hard_rows"].abs().sum()) / P, float(ref["soft_rows"].abs().sum()) / P
    for i, (name, terms) in enumerate((("loss", (1 - alpha) * th + alpha * tau * tau * ts_), ("hard", th), ("soft", ts_))):
        err = abs(float(got["out"][i]) - float(ref[name]))
        print("%s %s: |d|=%.3e (sum of |terms| %.3g)" % (what, name, err, terms))
        assert err <= TOL * max(1.0, terms), (what, name, float(got["out"][i]), float(ref[name]))
    assert float(got["out"][3]) == float(np.float32(float(ref["accuracy"]))), what + ": accuracy"
    close(got["grad"], ref["grad"], what=what + " dlogits")


A, G = R.ARITHMETIC, R.GEOMETRIC
CASES = [(7, 10000, 2, A, 2.0, 0.3, 0.1), (7, 10000, 8, G, 0.5, 1.0, 0.0), (7, 10000, 1, A, 1.0, 0.0, 0.1), (7, 10000, 3, G, 2.0, 0.3, 0.0),
         (5, 1003, 1, G, 1.0, 0.3, 0.1), (5, 1003, 3, A, 0.5, 1.0, 0.1), (5, 1003, 8, A, 2.0, 0.3, 0.0), (5, 1003, 2, G, 2.0, 0.0, 0.0),
         (3, 8, 2, A, 1.0, 0.3, 0.0), (3, 8, 8, G, 2.0, 1.0, 0.1), (3, 8, 1, A, 0.5, 0.3, 0.1), (3, 8, 3, G, 1.0, 0.0, 0.1),
         (9, 4100, 3, A, 2.0, 0.3, 0.1), (9, 4100, 1, G, 0.5, 1.0, 0.0), (9, 4100, 8, A, 1.0, 0.3, 0.0), (9, 4100, 2, G, 2.0, 0.3, 0.1),
         (2, 7, 8, A, 0.5, 0.3, 0.1), (2, 7, 2, G, 1.0, 1.0, 0.0), (2, 7, 3, A, 2.0, 0.0, 0.0), (2, 7, 1, G, 2.0, 0.3, 0.1)]


@pytest.mark.parametrize("P,V,M,combine,tau,alpha,smoothing", CASES)
def test_distill_kernels_against_the_reference(P, V, M, combine, tau, alpha, smoothing):
    z, ts, w, y = rows(P, V, M, 500 + P + M)
    g = 1.7 * P
    ref = R.distill(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g)
    what = "P=%d V=%d M=%d %s tau=%g alpha=%g" % (P, V, M, combine, tau, alpha)
    fused = run_kernels(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g, fused=True)
    check_against_reference(ref, fused, alpha, tau, what + " fused")
    split = run_kernels(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g, fused=False)
    check_against_reference(ref, split, alpha, tau, what + " split")
    for k in ("out", "lse", "tlse", "cnorm", "rows", "correct"):                  # the forward is the same launch but for the gradient
        assert torch.equal(fused[k], split[k]), k
    again = run_kernels(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g, fused=True)       # two runs, the same bits
    assert all(torch.equal(fused[k], again[k]) for k in ("out", "lse", "tlse", "cnorm", "rows", "correct", "grad"))
    for form in (True, False):                                                   # one float off the alignment: the 4-byte form, the same values
        mis = run_kernels(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g, fused=form, misalign=True)
        check_against_reference(ref, mis, alpha, tau, what + " misaligned")
        close(mis["grad"], fused["grad"], what=what + " misaligned against aligned dlogits")
        close(mis["out"], fused["out"], what=what + " misaligned against aligned out")
        assert torch.equal(mis["correct"], fused["correct"])


@pytest.mark.parametrize("P,V", [(7, 10000), (5, 1003)])
def test_alpha_zero_is_the_label_smoothing_loss(P, V):
    """alpha = 0: LabelSmoothingFn's loss, accuracy and gradient; the teachers are not read (they hold NaN)"""
    import sat_amd  # noqa: F401
    from sat_amd import decoder as Dk
    z, _, _, y = rows(P, V, 1, 300 + P)
    yd = y.to(torch.int32).cuda()
    nan = torch.full((P, V), float("nan"), device="cuda")
    for smoothing in (0.0, 0.1):
        za, zb = z.cuda().requires_grad_(), z.cuda().requires_grad_()
        ce, acc = Dk.LabelSmoothingFn.apply(za, yd, smoothing)
        (ce * (1.7 * P)).backward()
        loss, hard, soft, acc_d = Dk.DistillFn.apply(zb, yd, [nan, nan], [0.5, 0.5], "arithmetic", 0.5, 0.0, smoothing)
        (loss * (1.7 * P)).backward()
        close(loss, ce, what="loss"); close(hard, ce, what="hard"); close(zb.grad, za.grad, what="gradient")
        assert float(soft) == 0.0 and float(acc_d) == float(acc)


def test_distill_fn_returns_the_reference_in_both_gradient_forms():
    import sat_amd  # noqa: F401
    from sat_amd import decoder as Dk
    P, V = 9, 4100
    z, ts, w, y = rows(P, V, 3, 310)
    ref = R.distill(z, ts, w, G, y, 0.5, 0.4, 0.1, 1.7 * P)
    grads = []
    for fuse in (False, True):
        zd = z.cuda().requires_grad_()
        loss, hard, soft, acc = Dk.DistillFn.apply(zd, y.to(torch.int32).cuda(), [t.cuda() for t in ts], w, G, 0.5, 0.4, 0.1, fuse)
        assert loss.requires_grad and not hard.requires_grad and not soft.requires_grad and not acc.requires_grad
        (loss * (1.7 * P)).backward(retain_graph=True)
        close(loss, ref["loss"], what="loss"); close(hard, ref["hard"], what="hard"); close(soft, ref["soft"], what="soft")
        close(zd.grad, ref["grad"], what="gradient (fuse_gradient=%s)" % fuse)
        grads.append(zd.grad.clone())
        if fuse:                                                                 # scaled in place: it serves one backward
            with pytest.raises(RuntimeError, match="consumed"):
                loss.backward()
    close(grads[0], grads[1], what="the two forms")


@pytest.mark.parametrize("combine", [A, G])
def test_the_student_as_its_own_teacher_has_nothing_to_learn(combine):
    for P, V in ((7, 10000), (5, 1003)):
        z, _, _, y = rows(P, V, 1, 320 + P)
        for tau in (0.5, 2.0):
            for fused in (True, False):
                got = run_kernels(z, [z], [1.0], combine, y, 1.0 / tau, 1.0, 0.0, 1.7 * P, fused)
                close(got["rows"][:, 1], torch.zeros(P), what="soft rows"); close(got["grad"], torch.zeros(P, V), what="dlogits")
                assert abs(float(got["out"][0])) <= TOL and abs(float(got["out"][2])) <= TOL and float(got["out"][1]) == 0.0 and got["intact"]


@pytest.mark.parametrize("combine", [A, G])
def test_a_member_of_weight_zero_is_not_read(combine):
    P, V = 5, 1003
    z, ts, _, y = rows(P, V, 2, 340)
    nan = torch.full((P, V), float("nan"))
    for fused in (True, False):
        a = run_kernels(z, [ts[0], nan, ts[1]], [0.25, 0.0, 0.75], combine, y, 0.5, 0.6, 0.1, 3.0, fused)
        b = run_kernels(z, ts, [0.25, 0.75], combine, y, 0.5, 0.6, 0.1, 3.0, fused)
        assert all(torch.equal(a[k], b[k]) for k in ("out", "lse", "cnorm", "rows", "correct", "grad")) and a["intact"]
        assert torch.equal(a["tlse"][:, [0, 2]], b["tlse"]) and bool((a["tlse"][:, 1] == 0).all())
        assert bool(torch.isfinite(a["grad"]).all()) and bool(torch.isfinite(a["out"]).all())


@pytest.mark.parametrize("combine", [A, G])
def test_a_peaked_teacher_gives_a_finite_loss_and_gradient(combine):
    """a logit gap of 300 at tau = 0.5: the teacher's log-probabilities reach -600 and most of q underflows to exactly 0"""
    P, V = 5, 1003
    z, ts, w, y = rows(P, V, 2, 360)
    peaked = ts[0].clone()
    peaked[torch.arange(P), torch.arange(P) * 7 + 1] += 300.0
    for teachers, weights in (([peaked], [1.0]), ([peaked, ts[1]], w)):
        ref = R.distill(z, teachers, weights, combine, y, 2.0, 1.0, 0.0, 1.7 * P)
        for fused in (True, False):
            got = run_kernels(z, teachers, weights, combine, y, 2.0, 1.0, 0.0, 1.7 * P, fused)
            assert bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["grad"]).all()) and bool(torch.isfinite(got["rows"]).all())
            check_against_reference(ref, got, 1.0, 0.5, "peaked M=%d %s" % (len(teachers), combine))


def test_bad_targets_give_a_nan_hard_loss_and_no_fault():
    P, V = 6, 1003
    z, ts, w, y = rows(P, V, 2, 380)
    for bad in (V, -1):
        yb = y.clone(); yb[2] = bad
        ref = R.distill(z, ts, w, A, yb, 0.5, 0.3, 0.1, 1.7 * P)
        for fused in (True, False):
            for misalign in (False, True):
                got = run_kernels(z, ts, w, A, yb, 0.5, 0.3, 0.1, 1.7 * P, fused, misalign)
                assert got["intact"], (bad, fused, misalign)
                assert bool(torch.isnan(got["rows"][2, 0])) and bool(torch.isnan(got["out"][0])) and bool(torch.isnan(got["out"][1]))
                assert bool(torch.isfinite(got["rows"][[0, 1, 3, 4, 5], 0]).all()) and bool(torch.isfinite(got["rows"][:, 1]).all())
                assert bool(torch.isfinite(got["out"][2:]).all()) and bool(torch.isfinite(got["grad"]).all()) and int(got["correct"][2]) == 0
                close(got["grad"], ref["grad"], what="dlogits with target %d" % bad)


# ---------------------------------------------------------------------------------------------------------------- the whole step
OVER = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40,
            deep_output=True, val_beamk=3, val_max_len=7)


def make(seed, damp_residual=None, **over):
    """a tiny SAT model (test_gpu_scst.py::tiny's hyper-parameters unless ``over`` says otherwise) on the GPU and the oracle on its weights;
    ``damp_residual`` as there"""
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    hp = dict(OVER, **over)
    torch.manual_seed(seed)
    model = M.SAT(**vars(O.default_hparams(**hp)))
    if damp_residual is not None:
        with torch.no_grad():
            for blk in [b for li in (5, 6, 7, 8) for b in model.encoder[li]]:
                (blk.bn3 if blk.kind == "bottleneck" else blk.bn2).weight.fill_(damp_residual)
    oracle = O.OracleSAT(O.default_hparams(**hp), {k: v.detach().clone() for k, v in model.state_dict().items()})
    return model.cuda(), oracle


def batch(seed, B=3, Rn=2, T=7):
    from oracle import prng
    img = torch.from_numpy(prng.uniform((B, 3, 64, 64), seed, 0.0, 1.0))
    caps, lengths = prng.captions(B, Rn, T, 60, seed + 1, min_len=3)
    return img, torch.from_numpy(caps), torch.from_numpy(lengths)


def snapshot(models):
    return [({k: v.clone() for k, v in m.state_dict().items()}, [mod.training for mod in m.modules()]) for m in models]


def unchanged(models, snap):
    for m, (state, flags) in zip(models, snap):
        now = m.state_dict()
        if set(now) != set(state) or not all(torch.equal(now[k], state[k]) for k in state):
            return False
        if [mod.training for mod in m.modules()] != flags or any(p.grad is not None for p in m.parameters()):
            return False
    return True


@pytest.mark.parametrize("combine", [A, G])
def test_distill_loss_and_every_gradient_against_the_oracle(combine):
    """B = 3, R = 2, T = 7; two teachers that differ in decoder_dim and deep_output, fp32; every net residual-damped (0.25) for the reason
    test_scst_loss_and_every_gradient_against_the_oracle gives"""
    import sat_amd  # noqa: F401
    from sat_amd import distill
    from oracle import sat_oracle as O
    student, oracle = make(5, 0.25, label_smoothing=0.1)
    t1, o1 = make(6, 0.25, decoder_dim=48)
    t2, o2 = make(7, 0.25, deep_output=False)
    img, caps, lengths = batch(71)
    weights, alpha, tau = [0.25, 0.75], 0.4, 2.0
    t1.train(); t2.eval()                                                          # whichever mode they are left in, they run in eval mode
    snap = snapshot([t1, t2])
    tl = distill.teacher_logits(distill.Ensemble([t1, t2], weights, combine), img.cuda(), caps.cuda(), lengths)
    assert unchanged([t1, t2], snap) and all(not t.requires_grad for t in tl)
    student.train()
    ann_g, _ = student.encode(img.cuda())
    ann_g.retain_grad()
    loss, hard, soft, acc = distill.loss(student, ann_g, caps.cuda(), lengths, tl, weights, combine, alpha, tau, return_parts=True)
    loss.backward()
    # the oracle: the teachers in eval mode without a graph, the student as training_step runs it
    t_logits = []
    for o, got in ((o1, tl[0]), (o2, tl[1])):
        o.encoder.eval()
        with torch.no_grad():
            out = O.decode_train(o.sd, o.hp, o.encoder(img.clone()), caps, lengths, epsilon=1.0)
            lp, _ = O.pack_time_major(out["logits"], out["lengths"])
        close(got, lp, 2e-4, "teacher logits")                                    # the bound the smoke run holds the packed logits to
        t_logits.append(lp)
    ann_o = oracle.encoder(img.clone())
    ann_o.retain_grad()
    out = O.decode_train(oracle.sd, oracle.hp, ann_o, caps, lengths, epsilon=1.0)
    lp, _ = O.pack_time_major(out["logits"], out["lengths"])
    tp, _ = O.pack_time_major(out["targets"], out["lengths"])
    ref = R.distill(lp, t_logits, weights, combine, tp, 1.0 / tau, alpha, 0.1)
    loss_o = ref["loss"].float() + O.doubly_stochastic(out["alphas"], oracle.hp.att_gamma)
    loss_o.backward()
    print("distill loss hip=%.7f oracle=%.7f  hard %.7f / %.7f  soft %.7f / %.7f" % (loss.item(), loss_o.item(), hard.item(), ref["hard"].item(), soft.item(),
                                                                                      ref["soft"].item()))
    assert abs(loss.item() - loss_o.item()) <= 1e-4 * max(1.0, abs(loss_o.item()))
    assert abs(hard.item() - ref["hard"].item()) <= 1e-4 * max(1.0, abs(ref["hard"].item())) and abs(soft.item() - ref["soft"].item()) <= 1e-4
    assert abs(acc.item() - ref["accuracy"].item()) <= 1e-6
    og = oracle.named_grads()
    B, D, h, w = ann_o.shape
    worst = {"annotations": float((ann_g.grad.cpu().double() - ann_o.grad.permute(0, 2, 3, 1).reshape(B, h * w, D).double()).norm())
             / max(1e-9, float(ann_o.grad.double().norm()))}
    for k, p in student.named_parameters():
        assert p.grad is not None, k
        worst[k] = float((p.grad.cpu().double() - og[k].double()).norm()) / max(1e-9, float(og[k].double().norm()))
    for k, e in sorted(worst.items(), key=lambda kv: -kv[1])[:8]:
        print("relative L2 gradient error %-40s %.3e" % (k, e))
    for k, e in worst.items():
        assert e <= 1e-3, "%s: relative L2 gradient error %.3e" % (k, e)
    assert unchanged([t1, t2], snap)


@pytest.mark.parametrize("targets", ["references", "teacher"])
def test_distill_step_end_to_end(targets):
    import sat_amd  # noqa: F401
    from sat_amd.ensemble import Ensemble
    student, _ = make(5, label_smoothing=0.1)
    t1, _ = make(6, decoder_dim=48)
    t2, _ = make(7, deep_output=False)
    teacher = Ensemble([t1, t2], [1.0, 2.0], "geometric")
    t1.train(); t2.eval()
    snap = snapshot([t1, t2])
    b = batch(41, B=4, Rn=3, T=9)
    gb = (b[0].cuda(), b[1].cuda(), b[2])
    student.train()
    opt = torch.optim.SGD(student.parameters(), lr=0.1)
    before = {k: v.detach().clone() for k, v in student.named_parameters()}
    step0 = student.sat_global_step()
    out = student.distill_step(gb, teacher, alpha=0.5, temperature=2.0, targets=targets, beamk=3, max_gen_length=7)
    assert student.training and student.sat_global_step() == step0 + 1           # as training_step counts
    assert set(out) == {"loss", "hard", "soft", "accuracy"} and all(bool(torch.isfinite(v)) for v in out.values())
    assert float(out["soft"]) > 0.0 and float(out["hard"]) > 0.0 and 0.0 <= float(out["accuracy"]) <= 1.0
    out["loss"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in student.parameters())
    opt.step()
    moved = [k for k, v in student.named_parameters() if not torch.equal(v, before[k])]
    assert {"output.output.weight", "embedding.weight", "lstm.weight_hh_l0", "attention.f_att.weight"} <= set(moved), moved
    assert any(k.startswith("encoder.") for k in moved)
    assert unchanged([t1, t2], snap)
    single = student.distill_step(gb, t1, alpha=1.0, temperature=1.0, targets=targets, max_gen_length=7)      # one model as the teacher
    assert bool(torch.isfinite(single["loss"])) and float(single["hard"]) == 0.0 and unchanged([t1, t2], snap)
    student.eval()                                                               # the flag is restored in eval mode as well
    student.distill_step(gb, teacher, targets=targets, max_gen_length=7)
    assert not student.training and student.sat_global_step() == step0 + 3 and unchanged([t1, t2], snap)


def test_teacher_captions_frame_the_teachers_beam_caption():
    import sat_amd  # noqa: F401
    from sat_amd import distill
    t1, _ = make(6, decoder_dim=48)
    img = batch(41, B=4)[0].cuda()
    S = 7
    caps, lengths = distill.teacher_captions(t1, img, 3, S)
    tokens, lens = t1.caption_tokens(img, beamk=3, max_gen_length=S)[:2]
    start, pad, end = 58, 0, 59
    assert tuple(caps.shape) == (4, 1, S + 2) and tuple(lengths.shape) == (4, 1) and not lengths.is_cuda
    for i in range(4):
        n = min(max(int(lens[i]), 1), S)
        assert caps[i, 0].tolist() == [start] + tokens[i, :n].tolist() + [end] + [pad] * (S - n) and int(lengths[i, 0]) == n + 1


def test_distill_step_bf16_is_finite_and_reproducible():
    import sat_amd  # noqa: F401
    student, _ = make(5)
    t1, _ = make(6, decoder_dim=48)
    student.train()
    student.set_precision("bf16")
    b = batch(41, B=4, Rn=3, T=9)
    gb = (b[0].cuda(), b[1].cuda(), b[2])
    state = {k: v.clone() for k, v in student.state_dict().items()}
    runs = []
    for _ in range(2):
        student.load_state_dict(state)                                           # the train-mode pass moves the running statistics
        student.zero_grad(set_to_none=True)
        out = student.distill_step(gb, t1, alpha=0.5, temperature=2.0)
        out["loss"].backward()
        runs.append((out["loss"].detach().clone(), out["hard"].clone(), out["soft"].clone(), student.output.output.weight.grad.clone(),
                     student.embedding.weight.grad.clone()))
    assert all(bool(torch.isfinite(x).all()) for x in runs[0])
    assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))


def test_existing_calls_are_bit_equal_around_a_distill_step():
    import sat_amd  # noqa: F401
    student, _ = make(5)
    t1, _ = make(6, decoder_dim=48)
    student.eval()                                                               # no running statistic moves: what differs would be the step's doing
    for p in student.encoder.parameters():                                       # an eval-mode encoder keeps no batch statistics to back-propagate through
        p.requires_grad = False
    b = batch(41, B=4, Rn=3, T=9)
    gb = (b[0].cuda(), b[1].cuda(), b[2])

    def existing():
        loss = student.training_step(gb, 0)["loss"].detach().clone()
        torch.manual_seed(7)
        caps = student.caption(gb[0], beamk=3, max_gen_length=7, sample_method="multinomial")
        toks = student.caption_tokens(gb[0], beamk=3, max_gen_length=7, sample_method="multinomial", seed=17)
        return loss, caps[0], caps[1], [t.clone() for t in toks]

    before = existing()
    for targets in ("references", "teacher"):
        student.distill_step(gb, t1, targets=targets, max_gen_length=7)["loss"].backward()
        student.zero_grad(set_to_none=True)
    after = existing()
    assert torch.equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2]
    assert all(torch.equal(x, y) for x, y in zip(before[3], after[3]))
