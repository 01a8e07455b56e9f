"""CPU: the launch plan of the attention step (sat_attention_step_plan: host arithmetic only, no device is touched), the float64 reference
of tests/attention_ref.py, and the inputs of tests/attention_cases.py.

launch_attention_fwd, launch_attention_bwd and attention_context_bwd (csrc/decoder.hip) take their form, rows per pass, vector width,
chunk and LDS sizes from the function this query returns, so what is asserted here is what runs: every case of the table lands on the
plan written next to it -- a retuned rule fails here until the table is derived again -- and test_gpu_attention_forms.py then runs it.

Sensitivity.  A comparison against a reference proves something only if the reference itself would notice the mistake.  For every case
the reference is evaluated again without the last location, the last attention unit, the last feature and the last caption row of each
image (the result padded back with zeros, which is what a kernel that skips the element leaves), and every compared output that depends
on the removed element must move by at least 100 times the tolerance of the GPU comparison, 1e-4 max(1, max|ref|).  Independent by the
formula, and therefore exempt: alphas of the features; DZ = dZ + dXZ beta of locations and units; dalpha = DZ . ann + its external
gradient of the units."""
import ctypes

import pytest
import torch

import attention_cases as C
import attention_ref as R

TOL = 1e-4          # the bound of test_gpu_attention_forms.py


@pytest.fixture(scope="module")
def lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


STEP = [pytest.param(i, c, id=C.step_id(c)) for i, c in enumerate(C.STEP_CASES)]
CTX = [pytest.param(i, c, id=C.ctx_id(c)) for i, c in enumerate(C.CTX_CASES)]


@pytest.mark.parametrize("i,c", STEP)
def test_step_case_lands_on_the_plan_it_was_written_for(lib, i, c):
    T1, _ = C.steps(i)
    rc, got = C.query(lib, c, T1)
    assert rc == 0, lib.sat_last_error()
    assert got == c["plan"], "%s (%s)" % (C.step_id(c), c["why"])
    assert 0 < got[5] <= 160 * 1024 and 0 <= got[6] <= 160 * 1024
    assert got[2] == -(-c["R"] // got[1])
    rc, got_b = C.query(lib, c, T1, bf16=True)
    if C.runs_bf16(c):          # the bf16 operands change no launch shape
        assert rc == 0 and got_b == c["plan"]
    else:                       # and the single launch has none
        assert rc != 0 and got_b == (0,) * 7 and b"bf16" in lib.sat_last_error()


@pytest.mark.parametrize("i,c", CTX)
def test_context_case_lands_on_the_plan_it_was_written_for(lib, i, c):
    rc, got = C.query(lib, c)
    assert rc == 0, lib.sat_last_error()
    assert got == c["plan"], "%s (%s)" % (C.ctx_id(c), c["why"])
    assert 0 < got[2] <= 160 * 1024 and got[1] % got[0] == 0 and got[1] * 4 >= c["L"]


def test_case_table_reaches_every_form():
    seen = set()
    for c in C.STEP_CASES:
        form, rn, passes, vw = c["plan"][:4]
        seen.add((c["op"], form, vw, min(passes, 3)))
        seen.add((c["op"], form, "RN", rn))
        if c["op"] == "bwd":
            seen.add(("bwd", form, "dalphas", c["dalphas"]))
    for passes in (1, 2, 3):
        assert ("fwd", C.SPLIT, 4, passes) in seen and ("bwd", C.SPLIT, 4, passes) in seen
    for passes in (1, 2):
        assert ("fwd", C.SINGLE, 4, passes) in seen and ("bwd", C.SINGLE, 1, passes) in seen
    assert ("fwd", C.SINGLE, 1, 1) in seen
    for form in (C.SPLIT, C.SINGLE):
        assert ("bwd", form, "dalphas", True) in seen and ("bwd", form, "dalphas", False) in seen
    for rn in (1, 5, 8):
        assert ("fwd", C.SPLIT, "RN", rn) in seen and ("bwd", C.SPLIT, "RN", rn) in seen
    assert {c["plan"][0] for c in C.CTX_CASES} == {13, 16} and {c["plan"][1] for c in C.CTX_CASES} == {13, 16, 32, 64}
    # every multi-row case has a live row, a dead row and a dead image; every multi-pass case a pass that is dead as a whole
    for i, c in enumerate(C.STEP_CASES):
        T1, step = C.steps(i)
        live = (C.lengths_for(c["R"], T1, step) > step).reshape(C.B, c["R"])
        assert bool(live.any()) and bool((~live).any()) and bool((~live).all(1).any()) and bool(live[-1, -1])
        if c["R"] > 1:
            assert bool((live.any(1) & (~live).any(1)).any())
        if c["R"] > 8:
            passes = [live[:, p:p + 8] for p in range(0, c["R"], 8)]
            assert any(bool((~p).all(1)[b]) and bool(live[b].any()) for p in passes for b in range(C.B))


def test_plan_and_entry_point_validation(lib):
    out = (ctypes.c_int32 * 9)(*([7] * 9))
    ok = dict(op=0, B=2, R=3, L=5, D=8, A=4, hc_ld=12, T1=2, flags=7)
    assert lib.sat_attention_step_plan(*ok.values(), out) == 0 and list(out)[:5] == [0, 3, 1, 4, 64]
    bad = [dict(op=3), dict(op=-1), dict(B=0), dict(R=0), dict(L=0), dict(D=0), dict(A=0), dict(T1=0), dict(hc_ld=11), dict(flags=16), dict(flags=-1),
           dict(op=1, A=0), dict(op=1, hc_ld=11), dict(op=2, L=-3), dict(op=2, T1=0),
           dict(flags=15, D=10, hc_ld=20), dict(flags=15, A=6, hc_ld=20), dict(op=1, flags=11, D=10, hc_ld=20), dict(op=1, flags=9),          # bf16 operands outside the split pair
           dict(L=20000), dict(op=1, D=6000, hc_ld=6004, flags=0), dict(op=2, T1=200, L=196)]          # more than 160 KiB of LDS
    for over in bad:
        a = dict(ok); a.update(over)
        out[:] = [7] * 9
        assert lib.sat_attention_step_plan(*a.values(), out) == 1, over          # SAT_EINVAL
        assert list(out) == [0] * 9 and lib.sat_last_error()
    assert lib.sat_attention_step_plan(*ok.values(), None) == 1 and b"null" in lib.sat_last_error()
    # the step entry points refuse a bad shape before anything is launched (the pointers are never followed)
    p = ctypes.c_void_p(256)
    fwd = lambda B=2, R=3, L=5, D=8, A=4, hc_ld=12, T1=2, step=1: lib.sat_attention_step_fwd(p, p, p, hc_ld, p, p, step, p, T1, p, p, B, R, L, D, A, None)
    fwd_ex = lambda B=2, R=3, L=5, D=8, A=4, hc_ld=12, T1=2, step=1: lib.sat_attention_step_fwd_ex(p, p, p, hc_ld, p, p, step, p, T1, p, p, B, R, L, D, A,
                                                                                                 p, None, None, None)
    bwd_ex = lambda B=2, R=3, L=5, D=8, A=4, hc_ld=12, T1=2, step=1: lib.sat_attention_step_bwd_ex(p, p, p, hc_ld, p, p, step, p, None, T1, p, p, p, p, p, hc_ld, p,
                                                                                                 p, p, B, R, L, D, A, None, None, None)
    for f in (fwd, fwd_ex, bwd_ex):
        for over in (dict(B=0), dict(R=0), dict(L=0), dict(D=0), dict(A=0), dict(T1=0), dict(step=-1), dict(step=2), dict(hc_ld=11)):
            assert f(**over) == 1, over
            assert lib.sat_last_error()
    assert lib.sat_attention_step_fwd(None, p, p, 12, p, p, 0, p, 1, p, p, 2, 3, 5, 8, 4, None) == 1


def test_reference_agrees_with_the_oracle_attention():
    """attention_ref.forward / backward against oracle.sat_oracle.soft_attention (the reference's SoftAttention) and autograd through it"""
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(5)
    N, D, A, n, Hh, Ww = 4, 6, 5, 7, 2, 3
    L = Hh * Ww
    sd = {"attention.encoder_att.weight": torch.randn(A, D, generator=g, dtype=torch.float64),
          "attention.decoder_att.weight": torch.randn(A, n, generator=g, dtype=torch.float64),
          "attention.f_att.weight": torch.randn(1, A, generator=g, dtype=torch.float64)}
    ann = torch.randn(N, D, Hh, Ww, generator=g, dtype=torch.float64).requires_grad_()
    h = torch.randn(N, n, generator=g, dtype=torch.float64)
    gz, ga = torch.randn(N, D, generator=g, dtype=torch.float64), torch.randn(N, L, generator=g, dtype=torch.float64)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    z, alpha = O.soft_attention(sdo, ann, h)
    ((z * gz).sum() + (alpha.reshape(N, L) * ga).sum()).backward()
    a = ann.detach().reshape(N, D, L).permute(0, 2, 1)
    U, q = a @ sd["attention.encoder_att.weight"].t(), h @ sd["attention.decoder_att.weight"].t()
    ones, wf = torch.ones(N, D, dtype=torch.float64), sd["attention.f_att.weight"][0]
    lengths = torch.ones(N, dtype=torch.int32)
    f = R.forward(U, q, ones, wf, a, lengths, 0, 1)
    assert torch.allclose(f["Z"], z.detach(), rtol=0, atol=1e-12) and torch.allclose(f["alphas"], alpha.detach().reshape(N, L), rtol=0, atol=1e-12)
    assert torch.equal(f["XZ"], f["Z"])
    b = R.backward(U, q, ones, wf, a, lengths, 0, 1, gz, torch.zeros(N, D), ga)
    assert torch.allclose(b["dwf_part"].sum(0), sdo["attention.f_att.weight"].grad[0], rtol=0, atol=1e-12)
    assert torch.allclose(b["dU"].reshape(N * L, A).t() @ a.reshape(N * L, D), sdo["attention.encoder_att.weight"].grad, rtol=0, atol=1e-11)
    assert torch.allclose(b["dq"].t() @ h, sdo["attention.decoder_att.weight"].grad, rtol=0, atol=1e-11)
    dann = b["dann_context"] + R.dann_scores(b["dU"], sd["attention.encoder_att.weight"])
    assert torch.allclose(dann, ann.grad.reshape(N, D, L).permute(0, 2, 1), rtol=0, atol=1e-11)
    assert torch.equal(b["DZ"], gz)
    # dead rows give zeros, and the context term is the plain triple sum
    lengths[1] = 0
    f = R.forward(U, q, ones, wf, a, lengths, 0, 1)
    assert not f["Z"][1].any() and not f["alphas"][1].any() and f["Z"][0].any()
    b = R.backward(U, q, ones, wf, a, lengths, 0, 1, gz, gz, ga)
    assert not b["dq"][1].any() and not b["DZ"][1].any() and not b["da"][1].any() and not b["dU"][1].any()
    want = torch.einsum("nl,nd->nld", f["alphas"], b["DZ"])
    assert torch.allclose(b["dann_context"], want, rtol=0, atol=1e-13)


# ------------------------------------------------------------------ sensitivity of the reference on the table's inputs
def _pad(t, shape):
    out = torch.zeros(shape, dtype=t.dtype)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out


def _step_outputs(c, d, R_rows, cut):
    """the reference's compared outputs with `cut` = (rows, locations, features, units) kept; rows are cut per image"""
    Rk, Lk, Dk, Ak = cut
    rows = torch.arange(C.B * R_rows).reshape(C.B, R_rows)[:, :Rk].reshape(-1)
    if min(cut) == 0:
        return None
    U, q, beta, wf, ann = d["U"][:, :Lk, :Ak], d["q"][rows][:, :Ak], d["beta"][rows][:, :Dk], d["wf"][:Ak], d["ann"][:, :Lk, :Dk]
    lengths = d["lengths"][rows]
    if c["op"] == "fwd":
        return R.forward(U, q, beta, wf, ann, lengths, d["step"], Rk)
    out = R.backward(U, q, beta, wf, ann, lengths, d["step"], Rk, d["dZ"][rows][:, :Dk], d["dXZ"][rows][:, :Dk],
                     None if d["dalpha"] is None else d["dalpha"][rows][:, :Lk])
    return out


EXEMPT = {("alphas", "feature"), ("DZ", "location"), ("DZ", "unit"), ("da", "unit")}


@pytest.mark.parametrize("i,c", STEP)
def test_step_reference_notices_every_last_element(i, c):
    Rr, L, D, A = c["R"], c["L"], c["D"], c["A"]
    for bf in ((False, True) if C.runs_bf16(c) else (False,)):
        d = C.step_inputs(c, i, "real", bf)
        full = _step_outputs(c, d, Rr, (Rr, L, D, A))
        for what, cut in (("row", (Rr - 1, L, D, A)), ("location", (Rr, L - 1, D, A)), ("feature", (Rr, L, D - 1, A)), ("unit", (Rr, L, D, A - 1))):
            less = _step_outputs(c, d, Rr, cut)
            rows = torch.arange(C.B * Rr).reshape(C.B, Rr)[:, :cut[0]].reshape(-1)
            for k, ref in full.items():
                if (k, what) in EXEMPT:
                    continue
                if less is None:
                    moved = ref.abs().max()
                elif ref.shape[0] == C.B * Rr and k not in ("dU", "dwf_part", "dann_context"):          # row outputs: the cut rows back in place
                    back = torch.zeros_like(ref)
                    back[rows] = _pad(less[k], (len(rows),) + ref.shape[1:])
                    moved = (ref - back).abs().max()
                else:
                    moved = (ref - _pad(less[k], ref.shape)).abs().max()
                bound = 100 * TOL * max(1.0, float(ref.abs().max()))
                assert float(moved) >= bound, "%s without the last %s: %s moves by %.3g < %.3g" % (C.step_id(c), what, k, float(moved), bound)


@pytest.mark.parametrize("i,c", CTX)
def test_context_reference_notices_every_last_element(i, c):
    d = C.ctx_inputs(c, i, "real")
    Rr, L, D, T1 = c["R"], c["L"], c["D"], c["T1"]
    full = R.context_bwd(d["alphas"], d["DZ"], d["lengths"], Rr)
    bound = 100 * TOL * max(1.0, float(full.abs().max()))
    rows = torch.arange(C.B * Rr).reshape(C.B, Rr)[:, :Rr - 1].reshape(-1)
    cuts = {"location": R.context_bwd(d["alphas"][:, :, :L - 1], d["DZ"], d["lengths"], Rr) if L > 1 else None,
            "feature": R.context_bwd(d["alphas"], d["DZ"][:, :, :D - 1], d["lengths"], Rr) if D > 1 else None,
            "row": R.context_bwd(d["alphas"][rows], d["DZ"][:, rows], d["lengths"][rows], Rr - 1) if Rr > 1 else None}
    for what, less in cuts.items():
        moved = full.abs().max() if less is None else (full - _pad(less, full.shape)).abs().max()
        assert float(moved) >= bound, "%s without the last %s: dann moves by %.3g < %.3g" % (C.ctx_id(c), what, float(moved), bound)
    lens = set(int(v) for v in d["lengths"])
    assert {0, T1, T1 + 3} <= lens
