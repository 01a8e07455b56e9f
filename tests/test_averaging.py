"""CPU: the host side of the averaged weights ("Averaged weights"): the eta / mu bookkeeping of ``kind="asgd"`` against
``torch.optim.ASGD``'s own state, the non-monotonic trigger of NT-ASGD on hand-worked sequences, the constructor's errors, the
reference-optimizer branch of ``configure_optimizers`` and the argument validation of the new C entry points (no launch: no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

import averaging_ref as R


@pytest.mark.parametrize("lambd", [0.0, 1e-3])
def test_asgd_coefficients_are_torchs_bit_for_bit(lambd):
    import sat_amd  # noqa: F401
    from sat_amd.optim import asgd_coefficients
    g = torch.Generator().manual_seed(1)
    ps = [torch.randn(n, generator=g).requires_grad_() for n in (3, 4, 5, 6, 7)]
    opt = torch.optim.ASGD(R.groups(ps), lr=1e-2, lambd=lambd, alpha=0.75, t0=2)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.7)
    for k in range(1, 9):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        lrs = [gr["lr"] for gr in opt.param_groups]                 # the rates the step sees: the scheduler acts one step late on eta
        opt.step()
        for gr, lr in zip(opt.param_groups, lrs):
            eta, mu = asgd_coefficients(lr, gr["lambd"], gr["alpha"], gr["t0"], k)
            for p in gr["params"]:
                st = opt.state[p]
                assert np.float32(eta) == np.float32(float(st["eta"])) and float(st["eta"]) == eta, (k, lr, eta, float(st["eta"]))
                assert float(st["mu"]) == mu, (k, mu, float(st["mu"]))
        sched.step()
        if k == 4:              # what start_averaging() does
            for gr in opt.param_groups:
                gr["t0"] = k
    assert float(opt.state[ps[0]]["mu"]) == float(np.float32(1 / 4))        # 1 / max(1, 8 - 4)


def test_non_monotonic_trigger_on_hand_worked_sequences():
    import sat_amd  # noqa: F401
    from sat_amd.optim import NonMonotonicTrigger
    # mode="max", n=2: check i fires when len(log) > 2 and v < max(log[:-3])
    #   v:            1     2     3     2.5   2.5   1.5                  3.5    0
    #   log[:-3]:     []    []    []    [1]   [1,2] [1,2,3]              ...
    #   fires:        no    no    no    no    no    yes (1.5 < 3)        never again
    t = NonMonotonicTrigger(n=2, mode="max")
    assert [t.update(v) for v in (1, 2, 3, 2.5, 2.5, 1.5, 3.5, 0)] == [False, False, False, False, False, True, False, False]
    assert t.fired and len(t.log) == 8
    # within the first n + 1 checks nothing can fire, however bad the values are
    t = NonMonotonicTrigger(n=3, mode="max")
    assert [t.update(v) for v in (9, 1, 0, -1)] == [False] * 4 and not t.fired
    assert t.update(-2) is True                                     # the fifth check: -2 < max([9])
    # a monotonically improving sequence never fires, in either mode
    t = NonMonotonicTrigger(n=1, mode="max")
    assert not any(t.update(v) for v in range(12)) and not t.fired
    t = NonMonotonicTrigger(n=1, mode="min")
    assert not any(t.update(-v) for v in range(12)) and not t.fired
    # mode="min" (a loss), n=1: fires when v > min(log[:-2])
    #   v:         5    4    4.5          3      3.5   4.5
    #   log[:-2]:  []   []   [5]          [5,4]  [5,4,4.5]  [5,4,4.5,3]
    #   fires:     no   no   no (4.5<5)   no     no (3.5 < 4)   yes (4.5 > 3)
    t = NonMonotonicTrigger(n=1, mode="min")
    assert [t.update(v) for v in (5, 4, 4.5, 3, 3.5, 4.5, 9)] == [False, False, False, False, False, True, False]
    # Merity et al.'s default n=5 is the default here, and an equal value is not "worse"
    t = NonMonotonicTrigger()
    assert t.n == 5 and t.mode == "max"
    assert not any(t.update(1.0) for _ in range(10))
    with pytest.raises(ValueError):
        NonMonotonicTrigger(mode="best")


def test_constructor_errors_and_the_reference_optimizer_branch():
    import sat_amd  # noqa: F401
    from sat_amd import model as M
    from sat_amd.optim import FusedOptimizer
    from oracle import sat_oracle as O
    ps = [torch.zeros(4, requires_grad=True)]
    with pytest.raises(ValueError):
        FusedOptimizer(ps, kind="asgd", ema_decay=0.9)
    for d in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            FusedOptimizer(ps, kind="adam", ema_decay=d)
    with pytest.raises(ValueError):
        FusedOptimizer(ps, kind="asgd", lambd=-1e-4)
    opt = FusedOptimizer(ps, kind="asgd")                           # torch's defaults
    assert {k: opt.param_groups[0][k] for k in ("lambd", "alpha", "t0")} == dict(lambd=1e-4, alpha=0.75, t0=1e6)
    assert FusedOptimizer(ps, kind="adam").ema_decay == 0.0         # off by default
    with pytest.raises(RuntimeError):
        FusedOptimizer(ps, kind="adam", ema_decay=0.9).swap_averaged()          # before any step
    with pytest.raises(RuntimeError):
        FusedOptimizer(ps, kind="adam").swap_averaged()                         # no averaging at all
    hp = O.default_hparams(encoder_arch="resnet18", encoder_dim=32, input_size=64, encoder_size=3, vocab_size=60, embed_dim=8, attention_dim=8,
                           decoder_dim=12, weight_decay=0.0, decoder_lr=2e-3, embedding_lr=1e-2, encoder_lr=1e-4, opt="asgd", adam_b1=0.9,
                           adam_b2=0.999, momentum=0.9, nesterov=False, scheduler=None, fused_optimizer=False, asgd_lambd=0.0, asgd_alpha=0.5,
                           asgd_t0=7)
    model = M.SAT(**vars(hp))
    opt = model.configure_optimizers()
    assert type(opt) is torch.optim.ASGD
    for g in opt.param_groups:
        assert (g["lambd"], g["alpha"], g["t0"]) == (0.0, 0.5, 7)
    assert opt.param_groups[0]["lr"] == 2e-3
    hp.fused_optimizer, hp.ema_decay, hp.opt = True, 0.99, "adam"
    opt = M.SAT(**vars(hp)).configure_optimizers()
    assert isinstance(opt, FusedOptimizer) and opt.ema_decay == 0.99 and opt.kind == "adam"


def test_new_entry_points_validate_before_they_launch():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    lib = _lib.lib()
    assert lib.sat_abi_version() == 23
    one = ctypes.create_string_buffer(64)                          # stands for a table: nothing is read with n_chunks = 0 / a failed check
    tab = ctypes.cast(one, ctypes.c_void_p)
    hyper = _lib.OptHyper(kind=1, beta1=0.9, beta2=0.999, eps=1e-8, bias_correction1=0.1, bias_correction2_sqrt=0.03)
    ok, bad = _lib.OptAvgHyper(coef=0.1), _lib.OptAvgHyper(coef=1.5)

    def failed(rc):
        return rc == 1 and len(lib.sat_last_error()) > 0

    # null tables
    assert failed(lib.sat_optimizer_step_avg(None, tab, tab, 1, ctypes.byref(hyper), ctypes.byref(ok), None, None)) and b"null" in lib.sat_last_error()
    assert failed(lib.sat_optimizer_step_avg(tab, None, tab, 1, ctypes.byref(hyper), ctypes.byref(ok), None, None))
    assert failed(lib.sat_optimizer_step_avg_dev(None, tab, tab, 1, tab, tab, None, None)) and b"null" in lib.sat_last_error()
    assert failed(lib.sat_optimizer_step_avg_dev(tab, tab, tab, 1, tab, None, None, None))
    assert failed(lib.sat_optimizer_swap(None, tab, tab, 1, None)) and b"null" in lib.sat_last_error()
    assert failed(lib.sat_optimizer_swap(tab, None, tab, 1, None))
    # a coefficient of 1.5, a negative lambd, an unknown kind (the host can read them only where they arrive in host memory)
    assert failed(lib.sat_optimizer_step_avg(tab, tab, tab, 1, ctypes.byref(hyper), ctypes.byref(bad), None, None)) and b"coefficient" in lib.sat_last_error()
    assert failed(lib.sat_optimizer_step_avg(tab, tab, tab, 1, ctypes.byref(hyper), ctypes.byref(_lib.OptAvgHyper(coef=0.5, lambd=-1.0)), None, None))
    assert b"lambd" in lib.sat_last_error()
    assert failed(lib.sat_optimizer_step_avg(tab, tab, tab, 1, ctypes.byref(_lib.OptHyper(kind=4)), ctypes.byref(ok), None, None))
    assert b"kind" in lib.sat_last_error()
    # nothing to do is not an error; ASGD is a kind of the averaging entry points only
    asgd = _lib.OptHyper(kind=3)
    assert lib.sat_optimizer_step_avg(tab, tab, tab, 0, ctypes.byref(asgd), ctypes.byref(ok), None, None) == 0
    assert lib.sat_optimizer_step_avg_dev(tab, tab, tab, 0, tab, tab, None, None) == 0
    assert lib.sat_optimizer_swap(tab, tab, tab, 0, None) == 0
    assert lib.sat_optimizer_step(tab, tab, 1, ctypes.byref(asgd), None, None) == 1 and b"kind" in lib.sat_last_error()
