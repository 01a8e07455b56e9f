"""Every launch form of the fused optimizer step (csrc/optimizer.hip) at the C ABI, against the float64 reference of tests/optimizer_ref.py,
every stream in a frame of canaries.  The launches are the table of tests/optimizer_cases.py (test_optimizer_cases.py shows on the CPU that
it reaches every form); each builds its own device tables and calls sat_optimizer_step / _dev / _avg / _avg_dev / _swap / sat_grad_clip_coef
directly.  Each case asserts the alignment of every pointer it passes, so it runs the form it was written for.

The bound on p, m, v and the average, per element:  k * 2^-24 * (sum of the magnitudes of the terms of the element's expression), both from
optimizer_ref: k is the number of fp32 roundings on the longest path of the expression, operands' counts adding up through products and
quotients (the rules are in optimizer_ref's docstring).  The count was taken from opt_update / asgd_update / avg_elem as built for gfx950:
  * contraction is on for the file and the compiler fuses some a * b + c and not others (the 16-byte loop of optimizer_step_kernel forms
    beta2 * v and ((1 - beta2) g) g with one packed multiply and adds them; lr * update is multiplied, then subtracted), and the 4-byte
    loop need not agree with the 16-byte loop.  Every C operator therefore counts as one rounding, the explicit fmaf()s as one: a
    contraction only removes a rounding.
  * fp32 `/` is v_div_scale / v_rcp / fma refinement / v_div_fmas / v_div_fixup and sqrtf is v_sqrt_f32 with the two fma residual tests
    that move the result by an ulp: the correctly rounded sequences, one rounding each.
With weight decay, norm and value clipping, nesterov momentum and an averaging coefficient below 1 (optimizer_ref.K_TABLE):
    SGD  p 6, m 3, average 9      Adam  p 21, m 6, v 8, average 24      AdamW  p 18, m 5, v 6, average 21      ASGD  p 3, average 6
and less where a setting is off (plain SGD: 2).  Nothing here is tuned to what the kernel returns; the tests print the worst
err / bound per kernel, kind and stream.

Exact outputs: plain SGD with lr = 2^-6 (lr g is exact, so p - lr g rounds once however the compiler contracts) equals the once-rounded
reference bit for bit; with an averaging coefficient of 1 the average has the bits of p, with 0 it keeps its own; the bf16 copy is the
round-to-nearest-even bf16 of the p the kernel left; g, and the m / v a kind does not use, keep their bits; every frame keeps its canaries.

Non-finite gradients follow torch.nn.utils: clip_grad_value_ keeps a NaN and clamps +-inf, clip_grad_norm_ hands on a NaN coefficient for a
NaN norm (every element of every tensor becomes NaN) and coefficient 0 for an infinite norm.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import averaging_ref as A
import optimizer_cases as O
import optimizer_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                # elements of canary on either side of every stream
CANARY = {torch.float32: (torch.int32, 0x7FC12345), torch.bfloat16: (torch.int16, 0x7FC1), torch.float64: (torch.int64, 0x7FF8123456789ABC)}
SHADOW_ELEMS = {0: 0, 2: 1, 8: 4}         # offset of the bf16 copy in elements
WORST = {}                                # (kernel, kind, stream) -> worst err / bound seen


def f32(x):
    return float(np.float32(x))


def bits(t):
    return t.view(CANARY[t.dtype][0])


def frame(n, dtype=torch.float32, off=0, data=None):
    """n elements at element GUARD + off of an allocation of canaries -> (whole, window)"""
    whole = torch.empty(GUARD + off + n + GUARD, dtype=dtype, device="cuda")
    bits(whole).fill_(CANARY[dtype][1])
    assert whole.data_ptr() % 16 == 0
    win = whole[GUARD + off:GUARD + off + n]
    if data is not None:
        win.copy_(data)
    return whole, win


def frame_intact(whole, win, what):
    lo = (win.data_ptr() - whole.data_ptr()) // whole.element_size()
    b, c = bits(whole), CANARY[whole.dtype][1]
    assert lo >= GUARD and whole.numel() - lo - win.numel() >= GUARD
    assert bool((b[:lo] == c).all()) and bool((b[lo + win.numel():] == c).all()), "%s: a store outside the tensor" % (what,)


def all_canary(win):
    return bool((bits(win) == CANARY[win.dtype][1]).all())


def to_device(raw):
    return torch.from_numpy(np.frombuffer(bytes(raw), dtype=np.uint8).copy()).cuda()


class Launch:
    """the device state of one case: per tensor the framed streams and their initial values, the tables, the hyper-parameters"""

    def __init__(self, case, poison=None, coef_dev=None):
        from sat_amd import _lib
        self.L, self.case = _lib, case
        kernel, kind = case["kernel"], case["kind"]
        code, h = O.KINDS[kind]
        self.hyper = dict(kind=code, nesterov=int(h.get("nesterov", 0)), first_step=int(h.get("first_step", 0)), clip_value=f32(case["clip_value"]))
        for key in ("beta1", "beta2", "eps", "bias_correction1", "bias_correction2_sqrt", "momentum"):
            self.hyper[key] = f32(h.get(key, 0.0))
        self.avg = None if case["avg_coef"] is None else dict(coef=f32(case["avg_coef"]), lambd=f32(O.LAMBD) if code == O.ASGD else 0.0)
        self.tensors = []
        table = (_lib.OptTensor * len(case["tensors"]))()
        avg_table = (C.c_void_p * len(case["tensors"]))()
        for ti, t in enumerate(case["tensors"]):
            n, off = t["n"], O.offsets(kernel, kind, t)
            gen = torch.Generator().manual_seed(1000 * ti + n % 997)          # the values depend on the row, not on its alignment
            init = dict(p=torch.randn(n, generator=gen), g=torch.randn(n, generator=gen), m=0.3 * torch.randn(n, generator=gen),
                        v=torch.randn(n, generator=gen) ** 2, a=torch.randn(n, generator=gen))
            if case["exact"]:
                init["g"] = torch.round(init["g"] * 2.0 ** 20) / 2.0 ** 20          # lr g and p - lr g are exact in float64
                init["p"] = torch.where(init["p"].abs() < 2.0 ** -20, torch.ones(n), init["p"])
            if poison is not None:
                poison(ti, init["g"])
            st = dict(row=t, off=off, init=init, wide=O.is_wide(kernel, kind, off), fr={})
            for s in ("p", "g", "m", "v", "a"):
                # streams the launch passes hold values; m / v the kind must not read, and everything the launch does not pass, hold canaries
                unread = (s in ("m", "v") and s not in O.reads(kernel, kind)) or (kernel == O.SWAP and s in ("g", "m", "v"))
                if kind == "sgd_first" and s == "m":
                    unread = True          # first step: the buffer is written, never read
                eo = (off.get(s) or 0) // 4
                st["fr"][s] = frame(n, torch.float32, eo, None if unread else init[s])
                if unread:
                    init[s] = None
                if s in off and off[s] is not None:
                    assert st["fr"][s][1].data_ptr() % 16 == off[s], (case["name"], ti, s)
            if off["shadow"] is not None:
                st["fr"]["shadow"] = frame(n, torch.bfloat16, SHADOW_ELEMS[off["shadow"]], init["p"].to(torch.bfloat16))
                ptr = st["fr"]["shadow"][1].data_ptr()
                assert ptr % 16 == off["shadow"] and ptr % 8 == off["shadow"] % 8 and ptr % 2 == 0, (case["name"], ti)
            e = table[ti]
            e.p, e.g, e.n, e.lr, e.weight_decay = st["fr"]["p"][1].data_ptr(), st["fr"]["g"][1].data_ptr(), n, t["lr"], t["wd"]
            e.m = 0 if off.get("m") is None else st["fr"]["m"][1].data_ptr()
            e.v = 0 if off.get("v") is None else st["fr"]["v"][1].data_ptr()
            e.shadow_bf16 = 0 if off["shadow"] is None else st["fr"]["shadow"][1].data_ptr()
            avg_table[ti] = None if off.get("a") is None else st["fr"]["a"][1].data_ptr()
            self.tensors.append(st)
        rows = O.chunk_rows(case["tensors"])
        if case["shuffle"]:
            rows = [rows[i] for i in np.random.default_rng(5).permutation(len(rows))]
            assert rows != O.chunk_rows(case["tensors"])
        arr = np.array([(ti, 0, s) for ti, s in rows], dtype=[("tensor", np.int32), ("reserved", np.int32), ("start", np.int64)])
        self.n_chunks = len(rows)
        self.table, self.avg_table, self.chunks = to_device(table), to_device(avg_table), to_device(arr.tobytes())
        self.coef_value = None if case["clip_coef"] is None else f32(case["clip_coef"])          # what the kernel reads from clip_coef[0]
        self.coef = coef_dev if coef_dev is not None else (None if case["clip_coef"] is None else torch.tensor([case["clip_coef"], 0.0], device="cuda"))
        torch.cuda.synchronize()
        self.before = self.snapshot()

    def snapshot(self):
        return [{s: bits(w).cpu().clone() for s, (w, _) in st["fr"].items()} for st in self.tensors]

    def c_hyper(self, **over):
        return self.L.OptHyper(**dict(self.hyper, **over))

    def c_avg(self, **over):
        return self.L.OptAvgHyper(**dict(dict(self.avg, flags=0, reserved=0), **over))

    def run(self, entry):
        L, lib = self.L, self.L.lib()
        p = L.ptr
        if entry == "sat_optimizer_step":
            rc = lib.sat_optimizer_step(p(self.table), p(self.chunks), self.n_chunks, C.byref(self.c_hyper()), p(self.coef), L.stream_ptr())
        elif entry == "sat_optimizer_step_dev":
            self.hyper_dev = to_device(self.c_hyper())
            rc = lib.sat_optimizer_step_dev(p(self.table), p(self.chunks), self.n_chunks, p(self.hyper_dev), p(self.coef), L.stream_ptr())
        elif entry == "sat_optimizer_step_avg":
            rc = lib.sat_optimizer_step_avg(p(self.table), p(self.avg_table), p(self.chunks), self.n_chunks, C.byref(self.c_hyper()),
                                            C.byref(self.c_avg()), p(self.coef), L.stream_ptr())
        elif entry == "sat_optimizer_step_avg_dev":
            self.hyper_dev, self.avg_dev = to_device(self.c_hyper()), to_device(self.c_avg())
            rc = lib.sat_optimizer_step_avg_dev(p(self.table), p(self.avg_table), p(self.chunks), self.n_chunks, p(self.hyper_dev), p(self.avg_dev),
                                                p(self.coef), L.stream_ptr())
        else:
            assert entry == "sat_optimizer_swap"
            rc = lib.sat_optimizer_swap(p(self.table), p(self.avg_table), p(self.chunks), self.n_chunks, L.stream_ptr())
        L.check(rc, entry)
        torch.cuda.synchronize()
        return self

    def frames_intact(self):
        for ti, st in enumerate(self.tensors):
            for s, (whole, win) in st["fr"].items():
                frame_intact(whole, win, (self.case["name"], ti, s))

    def unchanged(self, ti, streams=None):
        """the whole allocation of these streams of tensor ti, frame and window, has the bits it had before the launch"""
        now = {s: bits(w).cpu() for s, (w, _) in self.tensors[ti]["fr"].items()}
        for s in (streams or now):
            assert torch.equal(now[s], self.before[ti][s]), "%s: tensor %d: %s was written" % (self.case["name"], ti, s)


def judge(launch, what, got, ref, key):
    """(a): got (fp32 tensor on the device) against a T of the reference, element by element; NaN where and only where the reference has one"""
    got = got.cpu().numpy().astype(np.float64)
    want_nan = np.isnan(ref.v)
    assert (np.isnan(got) == want_nan).all(), "%s: NaN at %d element(s) where the reference has none, or the other way round" % (what, int((np.isnan(got) != want_nan).sum()))
    ok = ~want_nan
    if ok.any():
        err, bound = np.abs(got[ok] - ref.v[ok]), ref.bound()[ok]
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        worst = float(ratio.max())
        WORST[key] = max(WORST.get(key, 0.0), worst)
        assert worst <= 1.0, "%s: err / bound = %.3f at element %d (err %.3e, k = %d)" % (what, worst, int(np.argmax(ratio)), float(err[np.argmax(ratio)]), ref.k)


def same_bits(a, b):
    return torch.equal(bits(a.contiguous()).cpu(), bits(b.contiguous()).cpu())


def copy_follows(st, what):
    """(b): the bf16 copy is the round-to-nearest-even bf16 of the fp32 p that is in memory now"""
    if "shadow" not in st["fr"]:
        return
    p, sh = st["fr"]["p"][1].cpu(), st["fr"]["shadow"][1].cpu()
    want = p.to(torch.bfloat16)
    nan = torch.isnan(p)
    assert bool((torch.isnan(sh.float()) == nan).all()), what
    assert torch.equal(bits(sh)[~nan], bits(want)[~nan]), "%s: the bf16 copy is not the rounded p" % (what,)


def check_step(launch):
    """(a), (b), (c) after one step"""
    case = launch.case
    kernel, kind = case["kernel"], case["kind"]
    f64 = lambda t: None if t is None else t.numpy().astype(np.float64)          # noqa: E731
    for ti, st in enumerate(launch.tensors):
        t, init, fr = st["row"], st["init"], st["fr"]
        what = "%s tensor %d (n = %d, %s)" % (case["name"], ti, t["n"], "wide" if st["wide"] else "narrow")
        if t["omit"]:
            launch.unchanged(ti)
            continue
        passed_a = kernel == O.AVG and st["off"]["a"] is not None
        ref = R.step(launch.hyper, f32(t["lr"]), f32(t["wd"]), f64(init["p"]), f64(init["g"]), f64(init["m"]) if st["off"]["m"] is not None else None,
                     f64(init["v"]), f64(init["a"]) if passed_a else None, avg=launch.avg, coef=launch.coef_value)
        for s in ("p", "m", "v", "a"):
            if ref[s] is not None and (s != "m" or st["off"]["m"] is not None):
                judge(launch, "%s: %s" % (what, s), fr[s][1], ref[s], (kernel, kind, s))
            else:
                launch.unchanged(ti, [s])                     # not written: ASGD's m and v, SGD's v, a NULL average, m without momentum
                if init[s] is None:
                    assert all_canary(fr[s][1])
        launch.unchanged(ti, ["g"])
        copy_follows(st, what)
        if case["exact"]:
            want = torch.from_numpy(ref["p"].v.astype(np.float32))
            assert same_bits(fr["p"][1], want), "%s: plain SGD is not the once-rounded p - lr g" % (what,)
        if passed_a and launch.avg["coef"] == 1.0:
            assert same_bits(fr["a"][1], fr["p"][1]), "%s: coefficient 1 stores p itself" % (what,)
        if passed_a and launch.avg["coef"] == 0.0:
            launch.unchanged(ti, ["a"])
    launch.frames_intact()


def report(kernel, kind):
    for key in sorted(k for k in WORST if k[:2] == (kernel, kind)):
        print("worst err / bound  %-8s %-12s %s: %.3f" % (key + (WORST[key],)))


STEP_CASES = [c for c in O.CASES if c["kernel"] in (O.STEP, O.AVG)]
SWAP_CASES = [c for c in O.CASES if c["kernel"] == O.SWAP]


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: c["name"])
def test_step_forms(case):
    """(a) values, (b) the bf16 copy, (c) frames and untouched streams, (d) _dev bit-equal to its host-hyper twin"""
    import sat_amd  # noqa: F401
    host_entry, dev_entry = O.ENTRIES[case["kernel"]]
    host = Launch(case).run(host_entry)
    check_step(host)
    dev = Launch(case).run(dev_entry)
    for ti, (a, b) in enumerate(zip(host.snapshot(), dev.snapshot())):
        for s in a:
            assert torch.equal(a[s], b[s]), "%s: tensor %d: %s differs between %s and %s" % (case["name"], ti, s, host_entry, dev_entry)
    report(case["kernel"], case["kind"])


@pytest.mark.parametrize("case", SWAP_CASES, ids=lambda c: c["name"])
def test_swap_forms(case):
    """(d): one swap exchanges the bits of p and the average and the copy follows p; a second one restores every bit"""
    import sat_amd  # noqa: F401
    launch = Launch(case)
    launch.run("sat_optimizer_swap")
    for ti, st in enumerate(launch.tensors):
        t, init, fr = st["row"], st["init"], st["fr"]
        if t["omit"] or not t["avg"]:
            launch.unchanged(ti)
            continue
        assert same_bits(fr["p"][1], init["a"]) and same_bits(fr["a"][1], init["p"]), (case["name"], ti)
        copy_follows(st, (case["name"], ti))
        launch.unchanged(ti, ["g", "m", "v"])
    launch.frames_intact()
    launch.run("sat_optimizer_swap")
    for ti in range(len(launch.tensors)):
        launch.unchanged(ti)          # p, the average and the copy (which started as the rounded p)


@pytest.mark.parametrize("kernel,kind", [(O.STEP, "adam"), (O.AVG, "adam"), (O.AVG, "asgd"), (O.STEP, "sgd_nesterov")])
def test_wide_and_narrow_runs_of_the_same_values(kernel, kind):
    """(e): both meet the bound; bit equality between them is not required (the compiler may contract the two loops differently) and only
    reported"""
    import sat_amd  # noqa: F401
    kw = dict(avg_coef=0.25) if kernel == O.AVG else {}
    runs = []
    for mis in (None, "p"):
        tensors = [O.tensor(n, 3e-3, 0.05, mis=mis, shadow=0) for n in O.NARROW_EXTENTS]
        case = O.case("%s-%s-%s" % (kernel, kind, "narrow" if mis else "wide"), kernel, kind, tensors, "", clip_coef=0.37, clip_value=0.4, **kw)
        launch = Launch(case).run(O.ENTRIES[kernel][0])
        assert all(st["wide"] == (mis is None) for st in launch.tensors)
        check_step(launch)
        runs.append(launch)
    for s in ("p", "a") + O.reads(kernel, kind) if kernel == O.AVG else ("p",) + O.reads(kernel, kind):
        eq = all(same_bits(x["fr"][s][1], y["fr"][s][1]) for x, y in zip(runs[0].tensors, runs[1].tensors))
        print("%s %s: %s of the wide and the narrow run %s" % (kernel, kind, s, "bit-equal" if eq else "differ in bits (both within the bound)"))
    report(kernel, kind)


# ---------------------------------------------------------------------------------------------------------------- sat_grad_clip_coef
def _norm_launch(sizes, mis, fill):
    from sat_amd import _lib
    table = (_lib.OptTensor * len(sizes))()
    frames, grads = [], []
    for ti, n in enumerate(sizes):
        gen = torch.Generator().manual_seed(77 + ti)
        g = torch.randn(n, generator=gen)
        if fill == "zeros":
            g.zero_()
        elif fill == "1e20":
            g.fill_(1e20)
        elif fill in ("nan", "inf") and ti == len(sizes) - 2:
            g[n // 2] = float(fill)          # one element of one tensor
        fr = frame(n, torch.float32, 1 if ti == mis else 0, g)
        assert fr[1].data_ptr() % 16 == (4 if ti == mis else 0)
        table[ti].g, table[ti].n = fr[1].data_ptr(), n
        frames.append(fr); grads.append(g)
    rows = O.chunk_rows([O.tensor(n) for n in sizes])
    arr = np.array([(ti, 0, s) for ti, s in rows], dtype=[("tensor", np.int32), ("reserved", np.int32), ("start", np.int64)])
    scratch, coef = frame(len(rows), torch.float64), frame(2)
    dev = (to_device(table), to_device(arr.tobytes()))
    rc = _lib.lib().sat_grad_clip_coef(_lib.ptr(dev[0]), _lib.ptr(dev[1]), len(rows), 0.5, _lib.ptr(scratch[1]), _lib.ptr(coef[1]), _lib.stream_ptr())
    _lib.check(rc, "sat_grad_clip_coef")
    torch.cuda.synchronize()
    for ti, (fr, g) in enumerate(zip(frames, grads)):
        frame_intact(fr[0], fr[1], ("norm g", ti))
        assert same_bits(fr[1], g), "g was written"
    frame_intact(scratch[0], scratch[1], "norm scratch")
    frame_intact(coef[0], coef[1], "norm coef")
    return grads, coef[1], scratch[1]


@pytest.mark.parametrize("name,sizes,mis,fill", O.NORM_CASES, ids=[c[0] for c in O.NORM_CASES])
def test_grad_clip_coef(name, sizes, mis, fill):
    """(f), and the norm half of (g)"""
    import sat_amd  # noqa: F401
    grads, coef, scratch = _norm_launch(sizes, mis, fill)
    got0, got1 = (float(x) for x in coef.cpu())
    want0, want1 = R.norm_coef([g.numpy() for g in grads], 0.5)
    if fill == "nan":
        assert math.isnan(got0) and math.isnan(got1) and math.isnan(want0)
        return
    if fill == "inf":
        assert got0 == 0.0 and got1 == float("inf") and want0 == 0.0
        return
    # one rounding of the float64 sqrt, one of its cast to float (the fixed-order float64 sum of up to 2e5 squares is exact to ~1e-13)
    assert abs(got1 - want1) <= 2.0 ** -23 * want1, (got1, want1)
    assert math.isfinite(got1)
    # coef[0] follows from coef[1] in fp32: the addition and the division are correctly rounded
    c = np.float32(0.5) / (np.float32(got1) + np.float32(1e-6))
    assert np.float32(got0) == (np.float32(1.0) if c > 1 else c), (got0, c)
    assert abs(got0 - want0) <= 2.0 ** -22 * want0
    if fill == "zeros":
        assert got1 == 0.0 and got0 == 1.0
    if fill == "1e20":
        assert got1 > 1e22          # the squares overflow fp32, not the float64 partial sums
    print("grad norm %s: %.9g (float64 %.17g), coefficient %.9g" % (name, got1, want1, got0))


# ---------------------------------------------------------------------------------------------------------------- non-finite gradients
def _poison(ti, g):
    """n = 11: NaN in lane 1 of the second float4 and in the scalar tail (elements 8..10), +-inf beside them"""
    g[5], g[10], g[2], g[9] = float("nan"), float("nan"), float("inf"), float("-inf")


@pytest.mark.parametrize("kernel,kind", [(O.STEP, "adam"), (O.STEP, "adamw"), (O.STEP, "sgd_nesterov"), (O.AVG, "adam"), (O.AVG, "asgd")])
def test_value_clip_keeps_nan_and_clamps_inf(kernel, kind):
    """(g): torch.nn.utils.clip_grad_value_ keeps NaN and clamps +-inf to +-clip_value; the neighbours of a NaN meet the bound"""
    import sat_amd  # noqa: F401
    kw = dict(avg_coef=0.25) if kernel == O.AVG else {}
    case = O.case("%s-%s-nonfinite" % (kernel, kind), kernel, kind, [O.tensor(11, 3e-3, 0.05, shadow=0), O.tensor(11, 1e-2, 0.0, mis="p"), O.tensor(11, 1e-2, 0.0)],
                  "", clip_value=0.4, **kw)
    for entry in O.ENTRIES[kernel]:
        launch = Launch(case, poison=_poison).run(entry)
        assert [st["wide"] for st in launch.tensors] == [True, False, True]
        check_step(launch)          # the reference clips as torch does: NaN where and only where it has one, everything else within the bound
        for st in launch.tensors:
            p = st["fr"]["p"][1].cpu()
            assert torch.isnan(p).nonzero().reshape(-1).tolist() == [5, 10]
            for s in O.reads(kernel, kind):
                assert torch.isnan(st["fr"][s][1].cpu()).nonzero().reshape(-1).tolist() == [5, 10], s
            if kernel == O.AVG:
                assert torch.isnan(st["fr"]["a"][1].cpu()).nonzero().reshape(-1).tolist() == [5, 10]
        if O.KINDS[kind][0] in (O.ADAM, O.ADAMW):          # +-inf arrive as +-clip_value: m of those elements, in float64
            st = launch.tensors[2]
            m0, b1 = st["init"]["m"].double(), launch.hyper["beta1"]
            m = st["fr"]["m"][1].cpu().double()
            for i, gc in ((2, f32(0.4)), (9, -f32(0.4))):
                want = float(m0[i]) + (gc - float(m0[i])) * (1.0 - b1)
                assert abs(float(m[i]) - want) <= 6 * R.U * (abs(float(m0[i])) + (abs(gc) + abs(float(m0[i]))) * (1.0 - b1))


@pytest.mark.parametrize("kernel,kind", [(O.STEP, "adam"), (O.STEP, "sgd"), (O.AVG, "asgd"), (O.AVG, "adamw")])
def test_nan_norm_makes_every_element_nan(kernel, kind):
    """(g): a NaN in one tensor's gradient makes the norm and the coefficient NaN (clip_grad_norm_), and the step that reads that coefficient
    leaves every element of every tensor NaN"""
    import sat_amd  # noqa: F401
    _, coef, _ = _norm_launch((5, 65537, 1023), 1, "nan")
    assert bool(torch.isnan(coef).all())
    kw = dict(avg_coef=0.25) if kernel == O.AVG else {}
    case = O.case("%s-%s-nan-norm" % (kernel, kind), kernel, kind, [O.tensor(5, 3e-3, 0.05, shadow=0), O.tensor(65537, 1e-2, 0.0, mis="g"), O.tensor(1023, 1e-2, 0.0)],
                  "", clip_coef=float("nan"), **kw)
    launch = Launch(case, coef_dev=coef).run(O.ENTRIES[kernel][0])
    check_step(launch)
    for st in launch.tensors:
        assert bool(torch.isnan(st["fr"]["p"][1]).all())
        for s in O.reads(kernel, kind):
            assert bool(torch.isnan(st["fr"][s][1]).all())
        if kernel == O.AVG:
            assert bool(torch.isnan(st["fr"]["a"][1]).all())
        if "shadow" in st["fr"]:
            assert bool(torch.isnan(st["fr"]["shadow"][1].float()).all())


@pytest.mark.parametrize("kind,how", [("adam", ("value", 0.02)), ("adam", ("norm", 0.5)), ("sgd", ("norm", 1.0)), ("asgd", ("value", 0.02))])
def test_fused_optimizer_keeps_nan_as_torch_does(kind, how):
    """(g) end to end: FusedOptimizer beside torch.optim on the CPU (the harness of test_gpu_optimizer.py) with a NaN in one gradient element
    of the second step.  Clipped by value, that element of p is NaN from then on and nothing else; clipped by norm, everything is."""
    import sat_amd  # noqa: F401
    from sat_amd.optim import FusedOptimizer
    gen = torch.Generator().manual_seed(7)
    shapes = [(5,), (70001,), (33, 17), (20, 30), (64, 3, 3, 8), (1,)]
    ref = [torch.randn(s, generator=gen).requires_grad_() for s in shapes]
    dev = [p.detach().clone().cuda().requires_grad_() for p in ref]
    topt = A.torch_optimizer(kind, A.groups(ref))
    fopt = FusedOptimizer(A.groups(dev), kind=kind, lr=1e-2, betas=(0.8, 0.95), momentum=0.9 if kind == "sgd" else 0.0, nesterov=kind == "sgd",
                          grad_clip=how[0], clip_value=how[1])
    for step in range(3):
        for i, (p, q) in enumerate(zip(ref, dev)):
            gr = torch.randn(p.shape, generator=gen)
            if step == 1 and i == 1:
                gr[65537] = float("nan")          # second chunk of the second tensor
            p.grad = gr.clone(); q.grad = gr.cuda()
        norm = A.clip(ref, how)
        topt.step(); fopt.step()
        if how[0] == "norm":
            assert math.isnan(float(fopt.last_grad_norm)) == math.isnan(float(norm))
        for i, (p, q) in enumerate(zip(ref, dev)):
            want, got = p.detach(), q.detach().cpu()
            assert torch.equal(torch.isnan(want), torch.isnan(got)), (kind, how, step, i)
            ok = ~torch.isnan(want)
            expect_nan = 0 if step == 0 else (want.numel() if how[0] == "norm" else int(i == 1))
            assert int((~ok).sum()) == expect_nan, (kind, how, step, i)
            if ok.any():
                err = float((got[ok] - want[ok]).abs().max())
                assert err <= A.BOUND * max(1.0, float(want[ok].abs().max())), (kind, how, step, i, err)


# ---------------------------------------------------------------------------------------------------------------- host validation
def test_host_validation_leaves_everything_untouched():
    """(h)"""
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    lib, p, sp = _lib.lib(), _lib.ptr, _lib.stream_ptr
    tensors = [O.tensor(5, shadow=0), O.tensor(1025, 3e-3, 0.05)]
    plain = Launch(O.case("validation-step", O.STEP, "adam", tensors, "", clip_value=0.4))
    avg = Launch(O.case("validation-avg", O.AVG, "adam", tensors, "", avg_coef=0.25))
    asgd = Launch(O.case("validation-asgd", O.AVG, "asgd", tensors, "", avg_coef=0.25))
    T, Ch, n = p(plain.table), p(plain.chunks), plain.n_chunks
    hy = C.byref(plain.c_hyper())
    hyper_dev = to_device(plain.c_hyper())
    scratch, coef = frame(n, torch.float64), frame(2)
    bad = [
        # null tables
        lambda: lib.sat_optimizer_step(None, Ch, n, hy, None, sp()), lambda: lib.sat_optimizer_step(T, None, n, hy, None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, None, None, sp()),
        lambda: lib.sat_optimizer_step_dev(None, Ch, n, p(hyper_dev), None, sp()), lambda: lib.sat_optimizer_step_dev(T, None, n, p(hyper_dev), None, sp()),
        lambda: lib.sat_optimizer_step_dev(T, Ch, n, None, None, sp()),
        lambda: lib.sat_grad_clip_coef(None, Ch, n, 0.5, p(scratch[1]), p(coef[1]), sp()), lambda: lib.sat_grad_clip_coef(T, None, n, 0.5, p(scratch[1]), p(coef[1]), sp()),
        lambda: lib.sat_grad_clip_coef(T, Ch, n, 0.5, None, p(coef[1]), sp()), lambda: lib.sat_grad_clip_coef(T, Ch, n, 0.5, p(scratch[1]), None, sp()),
        lambda: lib.sat_grad_clip_coef(T, Ch, 0, 0.5, p(scratch[1]), p(coef[1]), sp()), lambda: lib.sat_grad_clip_coef(T, Ch, n, 0.0, p(scratch[1]), p(coef[1]), sp()),
        # an unknown kind; ASGD on the plain step; bias corrections
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(kind=7)), None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(kind=-1)), None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(kind=O.ASGD)), None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(bias_correction1=0.0)), None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(bias_correction2_sqrt=-1.0)), None, sp()),
        lambda: lib.sat_optimizer_step(T, Ch, n, C.byref(plain.c_hyper(kind=O.ADAMW, bias_correction1=-0.5)), None, sp()),
    ]
    for launch in (avg, asgd):
        Ta, Av, Cha, na = p(launch.table), p(launch.avg_table), p(launch.chunks), launch.n_chunks
        h, ah = launch.c_hyper, launch.c_avg
        hd, ad = to_device(h()), to_device(ah())
        keep = (hd, ad)
        bad += [
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(None, Av, Cha, na, C.byref(h()), C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, None, Cha, na, C.byref(h()), C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, None, na, C.byref(h()), C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, None, C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h()), None, None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, hd=hd, ad=ad: lib.sat_optimizer_step_avg_dev(None, Av, Cha, na, p(hd), p(ad), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, hd=hd, ad=ad: lib.sat_optimizer_step_avg_dev(Ta, None, Cha, na, p(hd), p(ad), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, hd=hd, ad=ad: lib.sat_optimizer_step_avg_dev(Ta, Av, None, na, p(hd), p(ad), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, hd=hd, ad=ad: lib.sat_optimizer_step_avg_dev(Ta, Av, Cha, na, None, p(ad), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, hd=hd, ad=ad: lib.sat_optimizer_step_avg_dev(Ta, Av, Cha, na, p(hd), None, None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha: lib.sat_optimizer_swap(None, Av, Cha, 1, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha: lib.sat_optimizer_swap(Ta, None, Cha, 1, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha: lib.sat_optimizer_swap(Ta, Av, None, 1, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h(kind=4)), C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h(kind=-1)), C.byref(ah()), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h()), C.byref(ah(coef=-0.1)), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h()), C.byref(ah(coef=1.5)), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h()), C.byref(ah(coef=float("nan"))), None, sp()),
            lambda Ta=Ta, Av=Av, Cha=Cha, na=na, h=h, ah=ah: lib.sat_optimizer_step_avg(Ta, Av, Cha, na, C.byref(h()), C.byref(ah(lambd=-1e-3)), None, sp()),
        ]
    bad.append(lambda: lib.sat_optimizer_step_avg(p(avg.table), p(avg.avg_table), p(avg.chunks), avg.n_chunks, C.byref(avg.c_hyper(bias_correction1=0.0)),
                                                  C.byref(avg.c_avg()), None, sp()))
    for i, call in enumerate(bad):
        assert call() != 0, "call %d was accepted" % i
        assert lib.sat_last_error()
    # n_chunks == 0 is not an error and writes nothing
    ok = [lambda: lib.sat_optimizer_step(T, Ch, 0, hy, None, sp()), lambda: lib.sat_optimizer_step_dev(T, Ch, 0, p(hyper_dev), None, sp()),
          lambda: lib.sat_optimizer_step_avg(p(avg.table), p(avg.avg_table), p(avg.chunks), 0, C.byref(avg.c_hyper()), C.byref(avg.c_avg()), None, sp()),
          lambda: lib.sat_optimizer_step_avg_dev(p(avg.table), p(avg.avg_table), p(avg.chunks), 0, p(hyper_dev), p(to_device(avg.c_avg())), None, sp()),
          lambda: lib.sat_optimizer_swap(p(avg.table), p(avg.avg_table), p(avg.chunks), 0, sp())]
    for i, call in enumerate(ok):
        assert call() == 0, "n_chunks == 0, call %d" % i
    torch.cuda.synchronize()
    for launch in (plain, avg, asgd):
        for ti in range(len(launch.tensors)):
            launch.unchanged(ti)
    assert all_canary(scratch[0]) and all_canary(coef[0])
