"""CPU: knowledge distillation ("Distillation").  The float64 specification (tests/distill_ref.py) equals torch's own kl_div /
cross_entropy compositions and its gradient is autograd's; the new symbols are declared, exported and bound and the ABI version stays
23; every SAT_EINVAL path answers through the C ABI before anything is launched; ``check_step_args`` raises every ValueError on the host."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "show-attend-and-tell-pytorch-lightning_amd")
NEW_SYMBOLS = ("sat_distill_fwd", "sat_distill_bwd")


def _case(P, V, M, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(P, V, generator=g, dtype=torch.float64) * 2.0
    ts = [torch.randn(P, V, generator=g, dtype=torch.float64) * 3.0 for _ in range(M)]
    w = torch.rand(M, generator=g, dtype=torch.float64) + 0.1
    y = torch.randint(0, V, (P,), generator=g)
    return z, ts, (w / w.sum()).tolist(), y


@pytest.mark.parametrize("combine", [R.ARITHMETIC, R.GEOMETRIC])
@pytest.mark.parametrize("M,tau,alpha,smoothing", [(1, 1.0, 0.5, 0.0), (2, 2.0, 0.3, 0.1), (3, 0.5, 1.0, 0.0), (2, 2.0, 0.0, 0.1), (8, 1.5, 0.7, 0.05)])
def test_reference_is_torchs_kl_div_and_cross_entropy(combine, M, tau, alpha, smoothing):
    P, V = 6, 37
    z, ts, w, y = _case(P, V, M, 10 * M + int(10 * tau))
    ref = R.distill(z, ts, w, combine, y, 1.0 / tau, alpha, smoothing, g=1.7)
    za = z.clone().requires_grad_()
    if combine == R.ARITHMETIC:
        q = sum(wi * torch.softmax(t / tau, -1) for wi, t in zip(w, ts))
    else:
        q = torch.softmax(sum(wi * torch.log_softmax(t / tau, -1) for wi, t in zip(w, ts)), -1)
    hard = F.cross_entropy(za, y, label_smoothing=smoothing)
    soft = F.kl_div(torch.log_softmax(za / tau, -1), q, reduction="batchmean")
    loss = (1.0 - alpha) * hard + alpha * tau * tau * soft
    (loss * 1.7).backward()
    loss, hard, soft = loss.detach(), hard.detach(), soft.detach()
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    if alpha != 1.0:
        assert abs(float(ref["hard"]) - float(hard)) <= 1e-12 * max(1.0, abs(float(hard)))
    else:
        assert float(ref["hard"]) == 0.0 and bool((ref["lse"][:, 0] == 0).all())
    if alpha != 0.0:
        assert abs(float(ref["soft"]) - float(soft)) <= 1e-12 and float(ref["soft"]) > 0.0
    else:
        assert float(ref["soft"]) == 0.0 and bool((ref["tlse"] == 0).all())
    assert float((ref["grad"] - za.grad).abs().max()) <= 1e-13
    assert float(ref["accuracy"]) == float((z.argmax(-1) == y).double().mean())


def test_reference_edges():
    """weight-0 members are skipped whatever they hold; a peaked teacher gives a finite KL; the student as its own teacher gives 0; a bad
    target gives a NaN hard row and no one-hot"""
    P, V = 4, 19
    z, ts, _, y = _case(P, V, 2, 3)
    nan = torch.full((P, V), float("nan"), dtype=torch.float64)
    for combine in (R.ARITHMETIC, R.GEOMETRIC):
        a = R.distill(z, [ts[0], nan, ts[1]], [0.25, 0.0, 0.75], combine, y, 0.5, 0.6, 0.1)
        b = R.distill(z, ts, [0.25, 0.75], combine, y, 0.5, 0.6, 0.1)
        assert torch.equal(a["grad"], b["grad"]) and float(a["loss"]) == float(b["loss"])
        peaked = ts[0].clone(); peaked[:, 3] += 300.0
        o = R.distill(z, [peaked], [1.0], combine, y, 2.0, 1.0, 0.0)
        assert bool(torch.isfinite(o["loss"])) and bool(torch.isfinite(o["grad"]).all())
        o = R.distill(z, [z], [1.0], combine, y, 0.5, 1.0, 0.0)
        assert abs(float(o["soft"])) <= 1e-15 and float(o["grad"].abs().max()) <= 1e-16
    yb = y.clone(); yb[1] = V
    o = R.distill(z, ts, [0.5, 0.5], R.ARITHMETIC, yb, 1.0, 0.3, 0.1)
    assert bool(torch.isnan(o["hard_rows"][1])) and bool(torch.isfinite(o["hard_rows"][[0, 2, 3]]).all()) and bool(torch.isfinite(o["grad"]).all())
    assert bool(torch.isnan(o["loss"]))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(PKG, "libsat_hip.so")):
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-j4"])
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_declared_and_bound(lib):
    from sat_amd import _lib, decoder as Dk, distill, model as M
    raw = C.CDLL(os.path.join(PKG, "libsat_hip.so"))
    header = open(os.path.join(ROOT, "include", "sat_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and ("int %s(" % name) in header, name
    assert "#define SAT_HIP_ABI_VERSION 23" in header and lib.sat_abi_version() == 23       # symbols were added, nothing existing changed
    assert hasattr(Dk, "DistillFn") and hasattr(M.SAT, "distill_step") and distill.TARGETS == ("references", "teacher")


def test_distill_argument_checks(lib):
    """every listed argument fault returns SAT_EINVAL (1) with text from both entry points; every check comes before the launch, so no
    GPU is touched"""
    from sat_amd import _lib
    p = 4096                                                                     # a non-null address: never dereferenced on the host
    fwd_names = ("logits", "teachers", "weights", "M", "combine", "targets", "P", "V", "inv_tau", "alpha", "smoothing", "lse", "tlse", "cnorm", "rows",
                 "correct", "out", "dlogits")
    bwd_names = ("logits", "teachers", "weights", "M", "combine", "targets", "P", "V", "inv_tau", "alpha", "smoothing", "lse", "tlse", "cnorm", "gscale",
                 "from_fwd", "dlogits")

    def ptrs(*a):
        return (C.c_void_p * len(a))(*a)

    def floats(*a):
        return (C.c_float * len(a))(*a)

    default = dict(logits=p, teachers=ptrs(p, p), weights=floats(0.25, 0.75), M=2, combine=0, targets=p, P=6, V=40, inv_tau=0.5, alpha=0.5, smoothing=0.1,
                   lse=p, tlse=p, cnorm=p, rows=p, correct=p, out=p, dlogits=p, gscale=None, from_fwd=0)

    def fwd(**kw):
        return lib.sat_distill_fwd(*[kw.get(n, default[n]) for n in fwd_names], None), lib.sat_last_error().decode()

    def bwd(**kw):
        return lib.sat_distill_bwd(*[kw.get(n, default[n]) for n in bwd_names], None), lib.sat_last_error().decode()

    def bwd_scale(**kw):                                                         # the in-place form checks the same arguments
        return bwd(from_fwd=1, **kw)

    nine = _lib.ENSEMBLE_MAX + 1
    for call, what, nulls in ((fwd, "distill_fwd", ("logits", "teachers", "weights", "targets", "lse", "tlse", "cnorm", "rows", "correct", "out")),
                              (bwd, "distill_bwd", ("logits", "teachers", "weights", "targets", "lse", "tlse", "cnorm", "dlogits")),
                              (bwd_scale, "distill_bwd", ("logits", "teachers", "weights", "targets", "lse", "tlse", "cnorm", "dlogits"))):
        for null in nulls:
            rc, msg = call(**{null: None})
            assert rc == 1 and what in msg and "null pointer" in msg, (null, rc, msg)
        for kw, word in [(dict(teachers=ptrs(p, None)), "teacher 1"), (dict(P=0), "P=0"), (dict(P=-2), "P=-2"), (dict(V=0), "V=0"), (dict(V=-1), "V=-1"),
                         (dict(M=0), "members 0"), (dict(M=-1), "members -1"),
                         (dict(M=nine, teachers=ptrs(*[p] * nine), weights=floats(*[1.0 / nine] * nine)), "members %d" % nine),
                         (dict(weights=floats(-0.25, 1.25)), "weight[0]"), (dict(weights=floats(0.5, float("nan"))), "weight[1]"),
                         (dict(weights=floats(float("inf"), 0.0)), "weight[0]"), (dict(weights=floats(0.5, 0.6)), "sum to"),
                         (dict(weights=floats(0.0, 0.0)), "sum to"), (dict(combine=2), "combine 2"), (dict(combine=-1), "combine -1"),
                         (dict(inv_tau=0.0), "inv_tau"), (dict(inv_tau=-1.0), "inv_tau"), (dict(inv_tau=float("inf")), "inv_tau"),
                         (dict(inv_tau=float("nan")), "inv_tau"), (dict(alpha=-0.1), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
                         (dict(smoothing=-0.1), "smoothing"), (dict(smoothing=1.0), "smoothing"), (dict(smoothing=float("nan")), "smoothing")]:
            rc, msg = call(**kw)
            assert rc == 1 and what in msg and word in msg, (kw, rc, msg)


def _models():
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from oracle import sat_oracle as O
    over = dict(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=24, attention_dim=16, decoder_dim=40)
    torch.manual_seed(5)
    student = M.SAT(**vars(O.default_hparams(**over)))
    a = M.SAT(**vars(O.default_hparams(**dict(over, decoder_dim=48))))
    b = M.SAT(**vars(O.default_hparams(**dict(over, deep_output=True))))
    other = M.SAT(**vars(O.default_hparams(**dict(over, vocab_size=61))))
    return student, a, b, other


def test_check_step_args_raises_every_value_error_on_the_host():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L, distill
    from sat_amd.ensemble import Ensemble
    student, a, b, other = _models()
    ens = Ensemble([a, b], [1.0, 3.0], "geometric")
    assert distill.members(a) == ([a], [1.0], "arithmetic")
    assert distill.members(ens) == ([a, b], [0.25, 0.75], "geometric")
    for teacher in (a, ens):
        distill.check_step_args(student, teacher, 0.5, 2.0, "references")
        distill.check_step_args(student, teacher, 0.0, 0.5, "teacher", 5, 12)
        distill.check_step_args(student, teacher, 1.0, 1.0, "teacher", 1, L.CAPTION_MAX_LEN - 1)
    ok = dict(teacher=ens, alpha=0.5, temperature=2.0, targets="references")
    for kw, word in [(dict(teacher=None), "SAT model or an Ensemble"), (dict(teacher=[a, b]), "SAT model or an Ensemble"), (dict(alpha=-0.1), "alpha"),
                     (dict(alpha=1.1), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=[0.5]), "alpha"), (dict(temperature=0.0), "temperature"),
                     (dict(temperature=-1.0), "temperature"), (dict(temperature=float("inf")), "temperature"), (dict(temperature=float("nan")), "temperature"),
                     (dict(temperature=[1.0, 2.0]), "temperature"), (dict(targets="both"), "targets"), (dict(targets=None), "targets"),
                     (dict(beamk=0), "beamk"), (dict(max_gen_length=0), "max_gen_length"), (dict(max_gen_length=L.CAPTION_MAX_LEN), "max_gen_length"),
                     (dict(teacher=student), "distil itself"), (dict(teacher=Ensemble([a, student])), "distil itself"),
                     (dict(teacher=other), "vocabulary"), (dict(teacher=Ensemble([other])), "vocabulary")]:
        args = dict(ok); args.update(kw)
        with pytest.raises(ValueError, match=word):
            distill.check_step_args(student, **args)
    stoi = dict(b.hp.vocab_stoi)                                                  # the same size, <END> and <UNK> the other way round
    stoi["<END>"], stoi["<UNK>"] = stoi["<UNK>"], stoi["<END>"]
    b.hp["vocab_stoi"] = stoi
    with pytest.raises(ValueError, match="START, PAD, END, UNK"):
        distill.check_step_args(student, b, 0.5, 2.0, "references")
    # SAT.distill_step refuses in front of its host half: the step count does not move, and no check reached a device
    img = torch.zeros(2, 3, 64, 64)
    batch = (img, torch.zeros(2, 3, 9, dtype=torch.int64), torch.full((2, 3), 4))
    step0 = student.sat_global_step()
    for kw, word in [(dict(alpha=2.0), "alpha"), (dict(temperature=0.0), "temperature"), (dict(targets="beam"), "targets")]:
        with pytest.raises(ValueError, match=word):
            student.distill_step(batch, a, **kw)
    with pytest.raises(ValueError, match="distil itself"):
        student.distill_step(batch, student)
    assert student.sat_global_step() == step0
    with pytest.raises(L.SatHipError):                                            # past the checks a CPU model reaches the library's "no GPU" error
        student.distill_step(batch, a)
