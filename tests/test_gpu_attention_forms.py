"""GPU: every launch form of the attention step (csrc/decoder_kernels.h: the split pairs attention_scores + attention_context and
attention_bwd_dalpha + attention_bwd_tanh, the single launches attention_fwd_kernel<VW> and attention_bwd_kernel, dann_from_context<NQ>)
against the float64 reference of tests/attention_ref.py.  The shapes and the plans they were written for are in tests/attention_cases.py;
test_attention_plan.py proves without a GPU that each shape lands on its form and that the reference notices a dropped last element.

The C ABI is called directly (sat_attention_step_fwd_ex / _bwd_ex reach the score scratch and the bf16 operands), so every allocation is
the test's own:
  inputs   views inside NaN-filled buffers.  NaN also fills the hc columns past A + D, every other step of alphas / dalphas, and the rows
           of hc, alphas, dalphas, Z, dZ, dXZ that belong to finished captions: a kernel that lets them into a result shows.  In the bf16
           stream the fp32 ann is NaN as a whole: only the bf16 copy may be streamed.
  outputs  views inside canary buffers (gemm_ref.CANARY_F32 / CANARY_BF16), canaries themselves at the start.  What must still be a canary
           afterwards: the frames, the other steps of alphas, the dhc columns past A + D (fp32 and bf16), the dalpha scratch in the
           single-launch form, the score scratch in the single-launch form and past B R L always.  dU and dwf_part start from known
           values and must come back as value + gradient.  Dead rows give exact zeros.
(a) reals: within 1e-4 max(1, max|ref|) of the float64 reference -- close() of test_gpu_modules.py, which compares the same entry points.
    A host fp32 emulation of the forward sits near 3e-7, so the bound has some 300x margin; the worst error per form is printed.
(b) small integers (backward: ann, Z, dZ, dXZ, dalpha in -2 .. 2, beta in {0, 1/2, 1}; context backward: alphas in eighths, DZ and the
    dann accumulated onto integers): DZ, the gate columns of dhc, the split form's dalpha scratch and dann are exact in fp32 whatever the
    order of the additions, and must equal the reference bit for bit.
(c) bf16 side outputs: xz_bf16 == XZ.to(bfloat16), dhc_bf16[:, :A+D] == dhc[:, :A+D].to(bfloat16), bit for bit.
(e) the path: the plan query's form, and the profiler scopes of the split kernels ran, or did not."""
import pytest
import torch

import attention_cases as C
import attention_ref as R
from gemm_ref import CANARY_BF16, CANARY_F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-4
GUARD = 64          # elements on either side of every view; a multiple of 8, so a view starts on a 16-byte boundary in either type


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)


def nan_framed(t, off=0, dtype=torch.float32):
    """host tensor t as a contiguous view inside a NaN-filled device buffer, `off` elements past a 16-byte boundary"""
    n = t.numel()
    whole = torch.full((GUARD + off + n + GUARD,), NAN, dtype=dtype, device="cuda")
    view = whole[GUARD + off:GUARD + off + n]
    view.copy_(t.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == (off * whole.element_size()) % 16
    return whole, view.view(t.shape)


def canary_framed(shape, dtype=torch.float32, inside=None):
    n = 1
    for s in shape:
        n *= s
    bits, canary = (torch.int16, CANARY_BF16) if dtype == torch.bfloat16 else (torch.int32, CANARY_F32)
    whole = torch.empty(GUARD + n + GUARD, dtype=dtype, device="cuda")
    whole.view(bits).fill_(canary)
    view = whole[GUARD:GUARD + n].view(shape)
    if inside is not None:
        view.copy_(inside.to(dtype))
    assert view.data_ptr() % 16 == 0
    return whole, view


def canaries(t):
    bits, canary = (torch.int16, CANARY_BF16) if t.dtype == torch.bfloat16 else (torch.int32, CANARY_F32)
    return int((t.contiguous().view(bits) == canary).sum())


def frame_intact(whole, what):
    assert canaries(whole[:GUARD]) == GUARD and canaries(whole[-GUARD:]) == GUARD, "%s: the frame around it changed" % what


def all_canary(t, what):
    assert canaries(t) == t.numel(), "%s: %d element(s) were written" % (what, t.numel() - canaries(t))


WORST = {}


def close(got, ref, what, form):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    WORST[form] = max(WORST.get(form, 0.0), err / scale)
    print("%s: max|d| = %.3e (scale %.3g); worst of form '%s' so far %.3e" % (what, err, scale, form, WORST[form]))
    assert err <= TOL * scale, "%s: max|d|=%.3e (scale %.3g, tol %.1e)" % (what, err, scale, TOL)


def exact(got, ref, what):
    got = got.detach().float().cpu()
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    assert torch.equal(got, ref.float()), "%s: %d element(s) differ from the exact result" % (what, int((got != ref.float()).sum()))


def form_name(c, bf):
    p = c["plan"]
    return "%s %s%s" % (c["op"], "split" if p[0] == C.SPLIT else "single VW=%d" % p[3], " bf16 stream" if bf else "")


def hc_buffer(d, c, live):
    """(N, hc_ld): [q | beta | NaN] on live rows, NaN on finished ones"""
    N, A, D = d["q"].shape[0], c["A"], c["D"]
    hc = torch.full((N, c["hc_ld"]), NAN)
    hc[live, :A] = d["q"][live]
    hc[live, A:A + D] = d["beta"][live]
    return hc


def live_rows_only(t, live):
    out = torch.full_like(t, NAN)
    out[live] = t[live]
    return out


def one_step_of(t, T1, step, live):
    """(N, X) -> (N, T1, X): the step's slice on live rows, NaN everywhere else"""
    out = torch.full((t.shape[0], T1, t.shape[1]), NAN)
    out[live, step] = t[live]
    return out


def scopes_ran(L, names, c, kernels):
    split = c["plan"][0] == C.SPLIT
    for k in kernels:
        assert (k in names) == split, "%s: the scopes that ran are %s" % (c["why"], names)


STEP = [pytest.param(i, c, bf, id=C.step_id(c) + ("-bf16" if bf else "")) for i, c in enumerate(C.STEP_CASES)
        for bf in ((False, True) if C.runs_bf16(c) else (False,))]


@pytest.mark.parametrize("i,c,bf", [p for p in STEP if p.values[1]["op"] == "fwd"])
def test_attention_forward_form(L, i, c, bf):
    lib = L.lib()
    Rr, Lc, D, A = c["R"], c["L"], c["D"], c["A"]
    N = C.B * Rr
    d = C.step_inputs(c, i, "real", bf)
    T1, step, lengths = d["T1"], d["step"], d["lengths"]
    live = lengths > step
    rc, plan = C.query(lib, c, T1, bf)
    assert rc == 0 and plan == c["plan"], plan
    split = plan[0] == C.SPLIT
    ref = R.forward(d["U"], d["q"], d["beta"], d["wf"], d["ann"], lengths, step, Rr)
    tag, form = C.step_id(c) + (" bf16" if bf else ""), form_name(c, bf)

    annw, ann = nan_framed(torch.full_like(d["ann"], NAN) if bf else d["ann"], c["ann_off"])
    annbw, annb = nan_framed(d["ann"], 0, torch.bfloat16) if bf else (None, None)
    Uw, U = nan_framed(d["U"])
    hcw, hc = nan_framed(hc_buffer(d, c, live))
    wfw, wf = nan_framed(d["wf"])
    lens = lengths.cuda()
    alw, alphas = canary_framed((N, T1, Lc))
    Zw, Z = canary_framed((N, D))
    XZw, XZ = canary_framed((N, D))
    scw, sc = canary_framed((N * Lc,)) if c["scratch"] else (None, None)
    xbw, xzb = canary_framed((N, D), torch.bfloat16) if bf else (None, None)

    L.profile_start()
    rc = lib.sat_attention_step_fwd_ex(L.ptr(ann), L.ptr(U), L.ptr(hc), c["hc_ld"], L.ptr(wf), L.ptr(lens), step, L.ptr(alphas), T1, L.ptr(Z), L.ptr(XZ),
                                       C.B, Rr, Lc, D, A, L.ptr(sc) if c["scratch"] else None, L.ptr(annb) if bf else None, L.ptr(xzb) if bf else None,
                                       L.stream_ptr())
    torch.cuda.synchronize()
    names = [e["name"] for e in L.profile_stop()]
    L.check(rc, "sat_attention_step_fwd_ex")
    scopes_ran(L, names, c, ("attention_scores", "attention_context"))

    for whole, what in ((alw, "alphas"), (Zw, "Z"), (XZw, "XZ")) + (((scw, "score scratch"),) if c["scratch"] else ()) + (((xbw, "xz_bf16"),) if bf else ()):
        frame_intact(whole, tag + " " + what)
    for t in range(T1):
        if t != step:
            all_canary(alphas[:, t], tag + " alphas of step %d" % t)
    if c["scratch"] and not split:
        all_canary(sc, tag + " score scratch (single launch)")
    close(alphas[:, step], ref["alphas"], tag + " alphas", form)
    close(Z, ref["Z"], tag + " Z", form)
    close(XZ, ref["XZ"], tag + " XZ", form)
    dead = ~live
    assert not bool(alphas[:, step].cpu()[dead].any()) and not bool(Z.cpu()[dead].any()) and not bool(XZ.cpu()[dead].any()), tag + ": a dead row is not zero"
    s = alphas[:, step].cpu()[live].double().sum(1)
    assert bool(((s - 1).abs() < 1e-5).all()), tag + ": a live row of alphas does not sum to 1"
    if bf:
        assert torch.equal(xzb.view(torch.int16), XZ.to(torch.bfloat16).view(torch.int16)), tag + ": xz_bf16 is not XZ rounded to bf16"
    # the inputs were only read
    for whole, view, what in ((Uw, U, "U"), (hcw, hc, "hc"), (wfw, wf, "wf")):
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), what


def int_reference(d, c, live):
    """exact DZ, gate gradient and dalpha of the integer data set (every product and sum is a multiple of 1/8 far below 2^24)"""
    Rr = c["R"]
    m = live.double()[:, None]
    beta, dZ, dXZ, Zin, ann = (d[k].double() for k in ("beta", "dZ", "dXZ", "Z_in", "ann"))
    DZ = (dZ + dXZ * beta) * m
    gate = dXZ * Zin * beta * (1 - beta) * m
    img = torch.arange(DZ.shape[0]) // Rr
    da = torch.einsum("nd,nld->nl", DZ, ann[img])
    if d["dalpha"] is not None:
        da = da + d["dalpha"].double()
    return DZ, gate, da * m


@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c,bf", [p for p in STEP if p.values[1]["op"] == "bwd"])
def test_attention_backward_form(L, i, c, bf, dataset):
    lib = L.lib()
    Rr, Lc, D, A = c["R"], c["L"], c["D"], c["A"]
    N, dhc_ld = C.B * Rr, c["hc_ld"] + c["dhc_pad"]
    d = C.step_inputs(c, i, dataset, bf)
    T1, step, lengths = d["T1"], d["step"], d["lengths"]
    live = lengths > step
    rc, plan = C.query(lib, c, T1, bf)
    assert rc == 0 and plan == c["plan"], plan
    split = plan[0] == C.SPLIT
    fwd = R.forward(d["U"], d["q"], d["beta"], d["wf"], d["ann"], lengths, step, Rr)
    Z_in = d["Z_in"] if dataset == "int" else fwd["Z"].float()
    tag, form = "%s %s%s" % (C.step_id(c), dataset, " bf16" if bf else ""), form_name(c, bf)
    g = torch.Generator().manual_seed(8000 + i)
    dU0 = torch.randint(-4, 5, (C.B, Lc, A), generator=g).float() / 2
    dwf0 = torch.randint(-4, 5, (C.B, A), generator=g).float() / 2

    annw, ann = nan_framed(torch.full_like(d["ann"], NAN) if bf else d["ann"], c["ann_off"])
    annbw, annb = nan_framed(d["ann"], 0, torch.bfloat16) if bf else (None, None)
    Uw, U = nan_framed(d["U"])
    hcw, hc = nan_framed(hc_buffer(d, c, live))
    wfw, wf = nan_framed(d["wf"])
    lens = lengths.cuda()
    _, alphas = nan_framed(one_step_of(fwd["alphas"].float(), T1, step, live))
    _, dalphas = nan_framed(one_step_of(d["dalpha"], T1, step, live)) if d["dalpha"] is not None else (None, None)
    _, Zs = nan_framed(live_rows_only(Z_in, live))
    _, dZ = nan_framed(live_rows_only(d["dZ"], live))
    _, dXZ = nan_framed(live_rows_only(d["dXZ"], live))
    DZw, DZ = canary_framed((N, D))
    dhcw, dhc = canary_framed((N, dhc_ld))
    dUw, dU = canary_framed((C.B, Lc, A), inside=dU0)
    dwfw, dwf = canary_framed((C.B, A), inside=dwf0)
    daw, da = canary_framed((N, Lc))
    dhbw, dhcb = canary_framed((N, dhc_ld), torch.bfloat16) if bf else (None, None)

    L.profile_start()
    rc = lib.sat_attention_step_bwd_ex(L.ptr(ann), L.ptr(U), L.ptr(hc), c["hc_ld"], L.ptr(wf), L.ptr(lens), step, L.ptr(alphas),
                                       L.ptr(dalphas) if dalphas is not None else None, T1, L.ptr(Zs), L.ptr(dZ), L.ptr(dXZ), L.ptr(DZ), L.ptr(dhc), dhc_ld,
                                       L.ptr(dU), L.ptr(dwf), L.ptr(da), C.B, Rr, Lc, D, A, L.ptr(annb) if bf else None, L.ptr(dhcb) if bf else None,
                                       L.stream_ptr())
    torch.cuda.synchronize()
    names = [e["name"] for e in L.profile_stop()]
    L.check(rc, "sat_attention_step_bwd_ex")
    scopes_ran(L, names, c, ("attention_bwd_dalpha", "attention_bwd_tanh"))

    for whole, what in ((DZw, "DZ"), (dhcw, "dhc"), (dUw, "dU"), (dwfw, "dwf_part"), (daw, "dalpha scratch")) + (((dhbw, "dhc_bf16"),) if bf else ()):
        frame_intact(whole, tag + " " + what)
    if dhc_ld > A + D:
        all_canary(dhc[:, A + D:], tag + " dhc past A + D")
        if bf:
            all_canary(dhcb[:, A + D:], tag + " dhc_bf16 past A + D")
    if not split:
        all_canary(da, tag + " dalpha scratch (single launch)")
    for t, what in ((DZ, "DZ"), (dhc[:, :A + D], "dhc"), (dU, "dU"), (dwf, "dwf_part")):
        assert not bool(torch.isnan(t).any()), "%s %s: NaN in the result" % (tag, what)
    dead = ~live
    assert not bool(DZ.cpu()[dead].any()) and not bool(dhc[:, :A + D].cpu()[dead].any()), tag + ": a dead row is not zero"
    if dataset == "int":
        DZr, gater, dar = int_reference(d, c, live)
        exact(DZ, DZr, tag + " DZ")
        exact(dhc[:, A:A + D], gater, tag + " gate columns of dhc")
        if split:
            exact(da, dar, tag + " dalpha scratch")
    else:
        ref = R.backward(d["U"], d["q"], d["beta"], d["wf"], d["ann"], lengths, step, Rr, d["dZ"], d["dXZ"], d["dalpha"])
        close(DZ, ref["DZ"], tag + " DZ", form)
        close(dhc[:, :A], ref["dq"], tag + " dhc[:, :A]", form)
        close(dhc[:, A:A + D], ref["dbeta_pre"], tag + " dhc[:, A:A+D]", form)
        close(dU, dU0.double() + ref["dU"], tag + " dU", form)
        close(dwf, dwf0.double() + ref["dwf_part"], tag + " dwf_part", form)
        if split:
            close(da, ref["da"], tag + " dalpha scratch", form)
        # the context term of the annotation gradient, from this step's alphas and the DZ just written
        a1 = torch.zeros(N, 1, Lc); a1[live, 0] = fwd["alphas"].float()[live]
        _, a1d = nan_framed(a1)
        dannw, dann = canary_framed((C.B, Lc, D))
        flags = live.to(torch.int32).cuda()
        L.check(lib.sat_attention_context_bwd(L.ptr(a1d), L.ptr(DZ), L.ptr(flags), L.ptr(dann), 0, C.B, Rr, 1, Lc, D, L.stream_ptr()), "sat_attention_context_bwd")
        torch.cuda.synchronize()
        frame_intact(dannw, tag + " dann")
        close(dann, ref["dann_context"], tag + " dann (context term)", form)
    if bf:
        assert torch.equal(dhcb[:, :A + D].contiguous().view(torch.int16), dhc[:, :A + D].to(torch.bfloat16).contiguous().view(torch.int16)), \
            tag + ": dhc_bf16 is not dhc rounded to bf16"


CTX = [pytest.param(i, c, id=C.ctx_id(c)) for i, c in enumerate(C.CTX_CASES)]


@pytest.mark.parametrize("dataset", ["real", "int"])
@pytest.mark.parametrize("i,c", CTX)
def test_attention_context_backward_form(L, i, c, dataset):
    lib = L.lib()
    Rr, Lc, D, T1, acc = c["R"], c["L"], c["D"], c["T1"], c["accumulate"]
    rc, plan = C.query(lib, c)
    assert rc == 0 and plan == c["plan"], plan
    d = C.ctx_inputs(c, i, dataset)
    ref = R.context_bwd(d["alphas"], d["DZ"], d["lengths"], Rr, d["dann0"] if acc else None)
    tag = "%s %s" % (C.ctx_id(c), dataset)
    aw, alphas = nan_framed(d["alphas"])
    gw, DZ = nan_framed(d["DZ"])
    lens = d["lengths"].cuda()
    dannw, dann = canary_framed((C.B, Lc, D), inside=d["dann0"] if acc else None)
    L.check(lib.sat_attention_context_bwd(L.ptr(alphas), L.ptr(DZ), L.ptr(lens), L.ptr(dann), acc, C.B, Rr, T1, Lc, D, L.stream_ptr()), "sat_attention_context_bwd")
    torch.cuda.synchronize()
    frame_intact(dannw, tag + " dann")
    if dataset == "int":
        exact(dann, ref, tag + " dann")
    else:
        close(dann, ref, tag + " dann", "context bwd NQ=%d" % plan[0])
    assert bool(torch.isnan(aw[:GUARD]).all()) and bool(torch.isnan(gw[-GUARD:]).all())
