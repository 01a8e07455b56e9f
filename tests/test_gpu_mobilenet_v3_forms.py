"""GPU: every launch form of the kernels mobilenet_v3_small added - the depthwise 5x5 convolution (csrc/depthwise5x5.hip), BatchNorm +
hard-swish and squeeze-and-excitation (csrc/mobilenet_v3.hip) - against the float64 specifications of tests/mobilenet_v3_kernel_ref.py.
The shapes and the plans they were written for are in tests/mobilenet_v3_kernel_cases.py; test_mobilenet_v3_plan.py holds without a GPU
that each shape lands on its form (restated from the launchers: the library has no plan query for these kernels),
test_mobilenet_v3_kernel_ref.py that the specifications are torch's and the data sets what is said here.

The C ABI is called directly, so every allocation is the test's own:
  inputs    views inside buffers that are NaN on both sides: at least (W + 4) C elements for the 5x5 (more than two rows of taps), 4096
            elements elsewhere (more than a row of the widest case); view starts are 16-byte aligned; the frames are still NaN afterwards;
  outputs   y, dx, the filter gradient, the saved statistics and SE vectors, the running statistics and every parameter gradient are views
            inside canary buffers: after the call every element outside the view still has the canary's bits;
  scratch   a view of exactly sat_dwconv5x5_wgrad_scratch_bytes / sat_bn_scratch_bytes / sat_se_bwd_scratch_bytes, NaN inside (a partial
            that is summed without having been written shows), canaries around it.  The BatchNorm statistics pass needs no state in its
            scratch: it starts from the all-NaN words as in test_gpu_batchnorm_forms.py.
No output may hold a NaN.  The 5x5 filter gradient, dgamma / dbeta and the four SE parameter gradients repeat themselves bit for bit on a
second call with a fresh NaN scratch.

Data sets
  "int" (5x5)   x, dy, w from {-2 .. 2}: every partial sum is an integer below 2^24, outputs are at most 100 in magnitude (bf16 holds them):
                forward, data gradient and filter gradient equal the reference bit for bit in both storage types.
  "real"        oracle.prng.uniform values, rounded to bf16 first for bf16 storage (see the generators in the case file).
  "exact"       (BN + hard-swish backward and eval forward) mean, beta integers, invstd, |gamma| powers of two and x such that v is exact in
                fp32: 12.5 % of the elements sit exactly at v = 3, 12.5 % at v = -3, the rest inside the three regions.  Every branch
                decision is the same in both precisions, so the bounds below hold with dv = 0 and no element is excused.

Bounds, each against the float64 reference and per element (u = 2^-24; "bf16" = the output is stored in bf16: + 2^-8 |ref|):
  5x5 forward, data gradient   1e-5 max(1, max|ref|) (at most 25 fused multiply-adds of values below 1) [+ bf16]
  5x5 filter gradient          L u S_abs + u |ref|, S_abs = sum |dy x| of the tap and channel, L = ceil(min(chunk, pixels) / lanes) + lanes: the
                               longest fp32 chain of a partial (a thread's pixels, then the lanes); the partials are added in double.
  BN statistics                as test_gpu_batchnorm_forms.py: from a pass |mean - ref| <= 2 u |ref| + 4 u A (A = mean |x - x[0]|),
                               |invstd - ref| <= ref (2 u + 4 u (1 + (mean - x[0])^2 / (var + eps))); from tiles 1 fp32 ulp of the float64 formula
                               on the float tile values; running statistics 4 u max(|old|, |new|) of the update on the stored mean.
  v = t + beta, t = (x - mean) invstd gamma
                               dv = n u (|t| + |beta|) + |invstd gamma| dmean + |(x - mean) gamma| dinvstd with n = 4 roundings (train) or
                               8 (eval: 1 / sqrt(var + eps) adds three) and dmean, dinvstd the statistics bounds above (0 where they are given)
  y = hardswish(v)             2 (1.5 dv + 4 u |y|) [+ bf16]   (|hardswish'| <= 1.5; v + 3, the product and the division round once each)
  backward g' = dy slope(v)    dg = |dy| (dv / 3 + 2 u |slope|) + u |g'| (+ 0.5 |dy| where the float64 v lies within dv of a kink: either branch is a
                               correct fp32 result; at most 0.1 % of a case, asserted on the reference)
  dbeta, dgamma (double sums)  2 (sum dg + u |ref|),  2 (sum (dg |xhat| + 2 u |g' xhat|) + u |ref|)
  BN dx = fa (g' - fb - (x - mean) fc)
                               2 |fa| (dg + dfb + |x - mean| dfc + 4 u (|g'| + |fb| + |(x - mean) fc|)) + 4 u |ref| [+ bf16] with
                               dfb = (tol(dbeta) + 3 u |dbeta|) / M, dfc = invstd (tol(dgamma) + 4 u |dgamma|) / M
  SE pool (double sum)         3 u mean_hw |x|
  SE h                         2 (C + 1) u (sum_c |w1 pool| + |b1|) + |w1| tol(pool)       (a chain of C fused multiply-adds and the bias)
  SE z2                        2 (S + 1) u (sum_j |w2 h| + |b2|) + |w2| tol(h)
  SE s, y                      tol(z2) / 6 + 3 u;   |x| tol(s) + 2 u |y| [+ bf16]
  SE backward                  ds: 2 u (sum_hw |dy x| + |ds|);  dz2: tol(ds) / 6 + u |dz2| where -3 < z2 < 3, else exactly 0;
                               dz1: 2 C u sum_c |w2 dz2| + |w2|^T tol(dz2) where h > 0, else exactly 0;  dpool: 2 S u sum_j |w1 dz1| + |w1|^T tol(dz1);
                               dx: tol(dpool) / HW + 4 u (|dy s| + |dpool| / HW) [+ bf16];
                               dw1, db1, dw2, db2 (double sums over the images of the kernel's own float dz1 / dz2): the propagated
                               tol(dz1) |pool|, tol(dz1), tol(dz2) |h|, tol(dz2) summed over the images + 2 u |ref|.
Every test prints "worst err / bound" per output; the largest measured on the MI355X over all cases:
(fp32 / bf16; a bf16-stored output sits at 0.99: the rounding of the stored value itself, half an ulp = 2^-8 |ref|)
  5x5 real: forward 0.022 / 0.99, data gradient 0.019 / 0.99, filter gradient 0.15 / 0.054; the int set is exact.
  BN + hard-swish: pass mean 0.31 / 0.35, pass invstd 0.19 / 0.25, tile mean and invstd - / 0.50, running statistics 0.38 / 0.00,
  y 0.11 / 0.99, eval y 0.13 / 0.99 (exact set 0.073 / 0.58), dbeta 0.12 / 0.14, dgamma 0.10 / 0.20, dx 0.13 / 0.99.
  SE: pool 0.57 / 0.47, h 0.028 / 0.026, z2 0.044 / 0.013, s 0.022 / 0.035, y 0.038 / 0.99, dz2 0.37 / 0.29, dz1 0.020 / 0.019,
  dpool 0.014 / 0.026, dx 0.21 / 0.99, dw1 0.014 / 0.020, db1 0.013 / 0.016, dw2 0.39 / 0.34, db2 0.32 / 0.21.
"""
import math

import pytest
import torch

import batchnorm_ref as BR
import mobilenet_v3_kernel_cases as K
import mobilenet_v3_kernel_ref as R
from gemm_ref import CANARY_BF16, CANARY_F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64, F32 = torch.float64, torch.float32
U = K.U
DEV = "cuda"
GUARD = 4096          # elements on either side of every view outside the 5x5 tests (a multiple of 16)


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)
    for k in sorted(WORST):
        print("WORST %s %s %.4f" % (k[0], k[1], WORST[k]))


WORST = {}


# ------------------------------------------------------------------ frames
class Frames:
    """the allocations of one call: NaN-framed inputs, canary-framed outputs; check() after the call"""

    def __init__(self, guard=GUARD):
        self.guard, self.ins, self.outs = guard, [], {}

    def inp(self, t, dtype):
        n, g = t.numel(), self.guard
        whole = torch.full((g + n + g,), NAN, dtype=dtype, device=DEV)
        view = whole[g:g + n]
        view.copy_(t.reshape(-1).to(dtype))
        assert view.data_ptr() % 16 == 0
        self.ins.append((whole, n))
        return view

    def out(self, name, n, dtype, inside=None):
        bits, canary = (torch.int16, CANARY_BF16) if dtype == torch.bfloat16 else (torch.int32, CANARY_F32)
        g = self.guard
        whole = torch.empty(g + n + g, dtype=dtype, device=DEV)
        whole.view(bits).fill_(canary)
        view = whole[g:g + n]
        if inside is not None:
            view.copy_(inside.reshape(-1).to(dtype)) if torch.is_tensor(inside) else view.fill_(inside)
        assert view.data_ptr() % 16 == 0
        self.outs[name] = (whole, view, bits, canary, n)
        return view

    def scratch(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return self.out("scratch", nbytes // 4, F32, inside=NAN)

    def check(self, what):
        torch.cuda.synchronize()
        g = self.guard
        for name, (whole, view, bits, canary, n) in self.outs.items():
            b = whole.view(bits)
            bad = int((b[:g] != canary).sum()) + int((b[g + n:] != canary).sum())
            assert bad == 0, "%s %s: %d element(s) outside the output changed" % (what, name, bad)
        for whole, n in self.ins:
            assert bool(torch.isnan(whole[:g]).all()) and bool(torch.isnan(whole[g + n:]).all()), what + ": an input's frame was written"

    def result(self, *names):
        return {k: self.outs[k][1] for k in names}


def same_bits(a, b):
    v = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.view(v), b.view(v))


def check(got, ref, tol, what, label, dtype):
    """|got - ref| <= tol per element (tol = 0: equal), no NaN; prints and records worst err / bound"""
    got = got.double().cpu().reshape(ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    err = (got - ref).abs()
    tol = tol.expand_as(ref) if torch.is_tensor(tol) else torch.full_like(ref, tol)
    pos = tol > 0
    worst = float((err[pos] / tol[pos]).max()) if bool(pos.any()) else 0.0
    WORST[(label, dtype)] = max(WORST.get((label, dtype), 0.0), worst)
    print("%s: worst err / bound %.3f" % (what, worst))
    bad = err > tol
    assert not bool(bad.any()), "%s: %d element(s) beyond the bound (worst err / bound %.3g, worst err %.3g)" % (what, int(bad.sum()), worst, float(err.max()))


def bf_term(ref, bf):
    return 2.0 ** -8 * ref.abs() if bf else torch.zeros_like(ref)


# ------------------------------------------------------------------ depthwise 5x5
_DW5 = {}


def dw5_reference(shape, dataset, bf):
    key = (shape, dataset, bf and dataset == "real")
    if key not in _DW5:
        _DW5.clear()
        N, H, W, C, stride = shape
        d = K.dw5_data(shape, dataset, bf)
        dw, s_abs = R.dw5_wgrad(d["dy"], d["x"], stride)
        d.update(y=R.dw5_forward(d["x"], d["w"], stride), dx=R.dw5_dgrad(d["dy"], d["w"], H, W, stride), dw=dw, s_abs=s_abs)
        _DW5[key] = d
    return _DW5[key]


@pytest.mark.parametrize("c,dataset,dtype", [pytest.param(c, ds, dt, id="%s-%s-%s" % ("x".join(map(str, c["shape"])), ds, dt))
                                             for c in K.DW5_CASES for ds in ("int", "real") for dt in c["run"]])
def test_dw5_form(L, c, dataset, dtype):
    shape = c["shape"]
    N, H, W, C, stride = shape
    bf = dtype == K.BF16
    adt = torch.bfloat16 if bf else F32
    lib, dt = L.lib(), int(bf)
    plan = K.dw5_plan(shape)
    assert plan == c["plan"]          # (test_mobilenet_v3_plan.py asserts the same without a GPU; the scratch size below holds the partial count)
    chunk, parts, cvb, lanes = plan
    d = dw5_reference(shape, dataset, bf)
    P, Q = K.dw5_out(H, stride), K.dw5_out(W, stride)
    guard = max(64, -(-((W + 4) * C) // 16) * 16)
    tag = "dw5 %s %s %s" % (shape, dataset, dtype)
    flat = lambda ref: 0.0 if dataset == "int" else 1e-5 * max(1.0, float(ref.abs().max())) + bf_term(ref, bf)

    fr = Frames(guard)
    x, dy, w = fr.inp(d["x"], adt), fr.inp(d["dy"], adt), fr.inp(d["w"], F32)
    y = fr.out("y", N * P * Q * C, adt)
    L.check(lib.sat_dwconv5x5_fwd_t(dt, L.ptr(x), L.ptr(w), L.ptr(y), N, H, W, C, stride, L.stream_ptr()), "sat_dwconv5x5_fwd_t")
    fr.check(tag + " forward")
    check(y, d["y"], flat(d["y"]), tag + " forward", "dw5 forward " + dataset, dtype)

    dx = fr.out("dx", N * H * W * C, adt)
    L.check(lib.sat_dwconv5x5_dgrad_t(dt, L.ptr(dy), L.ptr(w), L.ptr(dx), N, H, W, C, stride, L.stream_ptr()), "sat_dwconv5x5_dgrad_t")
    fr.check(tag + " data gradient")
    check(dx, d["dx"], flat(d["dx"]), tag + " data gradient", "dw5 data gradient " + dataset, dtype)

    need = lib.sat_dwconv5x5_wgrad_scratch_bytes(N, H, W, C, stride)
    assert need == parts * 25 * C * 4
    runs = []
    for _ in range(2):
        fw = Frames(guard)
        sc, dw = fw.scratch(need), fw.out("dw", C * 25, F32)
        L.check(lib.sat_dwconv5x5_wgrad_t(dt, L.ptr(dy), L.ptr(x), L.ptr(dw), N, H, W, C, stride, L.ptr(sc), L.stream_ptr()), "sat_dwconv5x5_wgrad_t")
        fw.check(tag + " filter gradient")
        fr.check(tag + " filter gradient (inputs)")
        runs.append(dw.clone())
    assert same_bits(runs[0], runs[1]), tag + ": the filter gradient does not repeat itself bit for bit"
    if dataset == "int":
        tol = 0.0
    else:
        chain = math.ceil(min(chunk, N * P * Q) / lanes) + lanes
        tol = chain * U * d["s_abs"] + U * d["dw"].abs()          # (a tap that only ever meets the padding has S_abs = 0: exactly 0 is expected)
    check(runs[0], d["dw"], tol, tag + " filter gradient", "dw5 filter gradient " + dataset, dtype)


# ------------------------------------------------------------------ BatchNorm + hard-swish
def _hs_params(datasets):
    return [pytest.param(c, ds, dt, id="%s-%s-%s" % (c["name"], ds, dt)) for c in K.HS_CASES for ds in datasets for dt in c["run"]]


def hs_y_tol(f, x, mean, invstd, gamma, beta, roundings, dmean, dinvstd, bf):
    dv = roundings * U * (f["t"].abs() + beta.abs()) + (invstd * gamma).abs() * dmean + ((x - mean) * gamma).abs() * dinvstd
    return 2 * (1.5 * dv + 4 * U * f["y"].abs()) + bf_term(f["y"], bf)


@pytest.mark.parametrize("c,dtype", [pytest.param(c, dt, id="%s-%s" % (c["name"], dt)) for c in K.HS_CASES for dt in c["run"]])
def test_bn_hswish_forward_form(L, c, dtype):
    bf = dtype == K.BF16
    adt = torch.bfloat16 if bf else F32
    lib, rows, C = L.lib(), c["rows"], c["C"]
    assert K.hs_plan(lib, dtype, rows, C) == c["plans"][dtype]
    d = K.hs_data(c, "real", bf)
    x, gamma, beta = d["x"], d["gamma"], d["beta"]
    tag = "bn_hswish %s %s" % (c["name"], dtype)

    fr = Frames()
    xv, gv, bv = fr.inp(x, adt), fr.inp(gamma, F32), fr.inp(beta, F32)
    tiles = BR.tile_sums(x, c["tile_rows"]) if c["tile_rows"] else None          # (ntiles, C, 2) float (sum, sum of squares): the layout of the convolution epilogue
    tv = fr.inp(tiles, F32) if tiles is not None else None
    y, mean, invstd = fr.out("y", rows * C, adt), fr.out("mean", C, F32), fr.out("invstd", C, F32)
    rm, rv = fr.out("run_mean", C, F32, d["run_mean"]), fr.out("run_var", C, F32, d["run_var"])
    sc = fr.scratch(lib.sat_bn_scratch_bytes(rows, C))
    L.check(lib.sat_bn_hswish_train_fwd_t(int(bf), L.ptr(xv), rows, C, L.ptr(tv), c["tile_rows"], L.ptr(gv), L.ptr(bv), K.HS_EPS, K.HS_MOMENTUM, L.ptr(rm), L.ptr(rv),
                                          L.ptr(mean), L.ptr(invstd), L.ptr(y), L.ptr(sc), L.stream_ptr()), "sat_bn_hswish_train_fwd_t")
    fr.check(tag + " train forward")

    if tiles is None:
        m, var, istd, unb = R.bn_train_stats(x, K.HS_EPS)
        dmean = 2 * U * m.abs() + 4 * U * (x - x[0]).abs().mean(0)
        dinvstd = istd * (2 * U + 4 * U * (1 + (m - x[0]) ** 2 / (var + K.HS_EPS)))
        label = "pass"
    else:
        m, var, istd, unb = BR.stats_from_tiles(tiles, rows, K.HS_EPS)
        dmean, dinvstd = BR.ulp32(m), BR.ulp32(istd)
        label = "tile"
    check(mean, m, dmean, tag + " save_mean", "bn_hswish %s mean" % label, dtype)
    check(invstd, istd, dinvstd, tag + " save_invstd", "bn_hswish %s invstd" % label, dtype)
    for k, got, new in (("run_mean", rm, mean.double().cpu()), ("run_var", rv, unb)):
        want = R.running_update(d[k], new, K.HS_MOMENTUM)
        check(got, want, 4 * U * torch.maximum(d[k].to(F64).abs(), want.abs()), tag + " " + k, "bn_hswish running statistics", dtype)
    f = R.bn_hs_forward(x, m, istd, gamma, beta)
    check(y, f["y"], hs_y_tol(f, x, m, istd, gamma, beta, 4, dmean, dinvstd, bf), tag + " y", "bn_hswish y", dtype)

    # eval mode on the same data, then on the exact set (eps = 0, run_var = 1 / invstd^2: v is exact, dv = 0)
    for dataset, dd, eps, roundings in (("real", d, K.HS_EPS, 8), ("exact", K.hs_data(c, "exact", bf), 0.0, 0)):
        fe = Frames()
        ins = [fe.inp(dd["x"], adt)] + [fe.inp(dd[k], F32) for k in ("run_mean", "run_var", "gamma", "beta")]
        ye = fe.out("y", rows * C, adt)
        L.check(lib.sat_bn_hswish_eval_fwd_t(int(bf), L.ptr(ins[0]), rows, C, L.ptr(ins[1]), L.ptr(ins[2]), eps, L.ptr(ins[3]), L.ptr(ins[4]), L.ptr(ye), L.stream_ptr()),
                "sat_bn_hswish_eval_fwd_t")
        fe.check(tag + " eval forward " + dataset)
        rmean, rvar = dd["run_mean"].to(F64), dd["run_var"].to(F64)
        fe_ref = R.bn_hs_eval_forward(dd["x"], rmean, rvar, eps, dd["gamma"], dd["beta"])
        if dataset == "exact":
            assert torch.equal(fe_ref["v"], dd["v"])
        tol = hs_y_tol(fe_ref, dd["x"], rmean, 1.0 / torch.sqrt(rvar + eps), dd["gamma"], dd["beta"], roundings, 0.0, 0.0, bf)
        check(ye, fe_ref["y"], tol, tag + " eval y " + dataset, "bn_hswish eval y " + dataset, dtype)


@pytest.mark.parametrize("c,dataset,dtype", _hs_params(("real", "exact")))
def test_bn_hswish_backward_form(L, c, dataset, dtype):
    bf = dtype == K.BF16
    adt = torch.bfloat16 if bf else F32
    lib, rows, C = L.lib(), c["rows"], c["C"]
    assert K.hs_plan(lib, dtype, rows, C) == c["plans"][dtype]
    d = K.hs_data(c, dataset, bf)
    x, dy, gamma, beta = d["x"], d["dy"], d["gamma"], d["beta"]
    if dataset == "exact":
        mean, invstd = d["mean"], d["invstd"]
    else:          # the forward reference's statistics as the floats the forward would have saved; the reference's backward uses exactly those
        m, var, istd, unb = R.bn_train_stats(x, K.HS_EPS)
        mean, invstd = m.float().to(F64), istd.float().to(F64)
    b = R.bn_hs_backward(x, dy, mean, invstd, gamma, beta)
    tag = "bn_hswish %s %s %s backward" % (c["name"], dataset, dtype)
    if dataset == "exact":
        assert torch.equal(b["v"], d["v"])
        dv, near = torch.zeros_like(b["v"]), torch.zeros_like(b["v"], dtype=torch.bool)
    else:
        dv, near = K.hs_kink_delta(b["t"], beta), K.hs_near_kink(b["v"], b["t"], beta)
        print("%s: %d element(s) within the fp32 error of a kink" % (tag, int(near.sum())))
        assert float(near.sum()) <= 0.001 * near.numel()

    runs = []
    for _ in range(2):
        fr = Frames()
        ins = [fr.inp(dy, adt), fr.inp(x, adt)] + [fr.inp(t, F32) for t in (mean, invstd, gamma, beta)]
        dx, dgamma, dbeta = fr.out("dx", rows * C, adt), fr.out("dgamma", C, F32), fr.out("dbeta", C, F32)
        sc = fr.scratch(lib.sat_bn_scratch_bytes(rows, C))
        L.check(lib.sat_bn_hswish_train_bwd_t(int(bf), *[L.ptr(t) for t in ins[:2]], rows, C, *[L.ptr(t) for t in ins[2:]], L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta),
                                              L.ptr(sc), L.stream_ptr()), "sat_bn_hswish_train_bwd_t")
        fr.check(tag)
        runs.append(fr.result("dx", "dgamma", "dbeta"))
    for k in ("dx", "dgamma", "dbeta"):
        assert same_bits(runs[0][k], runs[1][k]), "%s: %s does not repeat itself bit for bit" % (tag, k)
    got = runs[0]

    g, xhat, M = b["g"], b["xhat"], rows
    dg = dy.abs() * (dv / 3 + 2 * U * b["slope"].abs()) + U * g.abs() + torch.where(near, 0.5 * dy.abs(), torch.zeros_like(dy))
    tol_dbeta = 2 * (dg.sum(0) + U * b["dbeta"].abs())
    tol_dgamma = 2 * ((dg * xhat.abs() + 2 * U * (g * xhat).abs()).sum(0) + U * b["dgamma"].abs())
    check(got["dbeta"], b["dbeta"], tol_dbeta, tag + " dbeta", "bn_hswish dbeta " + dataset, dtype)
    check(got["dgamma"], b["dgamma"], tol_dgamma, tag + " dgamma", "bn_hswish dgamma " + dataset, dtype)
    fa, fb, fc = gamma * invstd, b["dbeta"] / M, invstd * b["dgamma"] / M
    dfb, dfc = (tol_dbeta + 3 * U * b["dbeta"].abs()) / M, invstd * (tol_dgamma + 4 * U * b["dgamma"].abs()) / M
    xc = (x - mean).abs()
    tol_dx = 2 * fa.abs() * (dg + dfb + xc * dfc + 4 * U * (g.abs() + fb.abs() + xc * fc.abs())) + 4 * U * b["dx"].abs() + bf_term(b["dx"], bf)
    check(got["dx"], b["dx"], tol_dx, tag + " dx", "bn_hswish dx " + dataset, dtype)


# ------------------------------------------------------------------ squeeze-and-excitation
def _se_params():
    return [pytest.param(c, dt, id="%s-%s" % ("x".join(map(str, c["shape"])), dt)) for c in K.SE_CASES for dt in c["run"]]


@pytest.mark.parametrize("c,dtype", _se_params())
def test_se_forward_form(L, c, dtype):
    bf = dtype == K.BF16
    adt = torch.bfloat16 if bf else F32
    lib = L.lib()
    N, HW, C, S = c["shape"]
    assert K.se_passes(C) == c["passes"]
    d = K.se_data(c, bf)
    f = R.se_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"])
    tag = "se %s %s forward" % (c["shape"], dtype)

    fr = Frames()
    ins = [fr.inp(d["x"], adt)] + [fr.inp(d[k], F32) for k in ("w1", "b1", "w2", "b2")]
    pool, h, z2, s = fr.out("pool", N * C, F32), fr.out("h", N * S, F32), fr.out("z2", N * C, F32), fr.out("s", N * C, F32)
    y = fr.out("y", N * HW * C, adt)
    L.check(lib.sat_se_fwd_t(int(bf), L.ptr(ins[0]), N, HW, C, S, *[L.ptr(t) for t in ins[1:]], L.ptr(pool), L.ptr(h), L.ptr(z2), L.ptr(s), L.ptr(y), L.stream_ptr()),
            "sat_se_fwd_t")
    fr.check(tag)

    w1a, w2a = d["w1"].abs(), d["w2"].abs()
    tol_pool = 3 * U * f["a_pool"]
    tol_h = 2 * (C + 1) * U * f["a_h"] + tol_pool @ w1a.t()
    tol_z2 = 2 * (S + 1) * U * f["a_z2"] + tol_h @ w2a.t()
    tol_s = tol_z2 / 6 + 3 * U
    tol_y = d["x"].abs() * tol_s[:, None, :] + 2 * U * f["y"].abs() + bf_term(f["y"], bf)
    for k, got, tol in (("pool", pool, tol_pool), ("h", h, tol_h), ("z2", z2, tol_z2), ("s", s, tol_s), ("y", y, tol_y)):
        check(got, f[k], tol, "%s %s" % (tag, k), "se " + k, dtype)


@pytest.mark.parametrize("c,dtype", _se_params())
def test_se_backward_form(L, c, dtype):
    bf = dtype == K.BF16
    adt = torch.bfloat16 if bf else F32
    lib = L.lib()
    N, HW, C, S = c["shape"]
    d = K.se_data(c, bf)
    sv = K.se_saved(d, R.se_forward(d["x"], d["w1"], d["b1"], d["w2"], d["b2"]))          # exactly +-3 in two channels of z2, exact zeros in h
    b = R.se_backward(d["dy"], d["x"], d["w1"], d["w2"], **sv)
    tag = "se %s %s backward" % (c["shape"], dtype)
    need = lib.sat_se_bwd_scratch_bytes(N, C, S)
    assert need == 4 * K.se_scratch_floats(N, C, S)

    runs = []
    for _ in range(2):
        fr = Frames()
        ins = [fr.inp(d["dy"], adt), fr.inp(d["x"], adt)] + [fr.inp(t, F32) for t in (d["w1"], d["w2"], sv["pool"], sv["h"], sv["z2"], sv["s"])]
        dx = fr.out("dx", N * HW * C, adt)
        grads = [fr.out(k, n, F32) for k, n in (("dw1", S * C), ("db1", S), ("dw2", C * S), ("db2", C))]
        sc = fr.scratch(need)
        L.check(lib.sat_se_bwd_t(int(bf), L.ptr(ins[0]), L.ptr(ins[1]), N, HW, C, S, *[L.ptr(t) for t in ins[2:]], L.ptr(dx), *[L.ptr(t) for t in grads], L.ptr(sc),
                                 L.stream_ptr()), "sat_se_bwd_t")
        fr.check(tag)
        runs.append(fr.result("dx", "dw1", "db1", "dw2", "db2", "scratch"))
    for k in ("dx", "dw1", "db1", "dw2", "db2"):
        assert same_bits(runs[0][k], runs[1][k]), "%s: %s does not repeat itself bit for bit" % (tag, k)
    got = runs[0]
    sc = got["scratch"]
    assert not bool(torch.isnan(sc).any()), tag + ": a scratch word was left unwritten"
    got.update(dz2=sc[:N * C], dpool=sc[N * C:2 * N * C], dz1=sc[2 * N * C:])          # sat_se_bwd_t's layout of its scratch

    w1a, w2a = d["w1"].abs(), d["w2"].abs()
    zero = torch.zeros_like
    tol_ds = 2 * U * (b["a_ds"] + b["ds"].abs())
    inside = (sv["z2"] > -3.0) & (sv["z2"] < 3.0)
    tol_dz2 = torch.where(inside, tol_ds / 6 + U * b["dz2"].abs(), zero(tol_ds))
    tol_dz1 = torch.where(sv["h"] > 0.0, 2 * C * U * b["a_dz1"] + tol_dz2 @ w2a, zero(sv["h"]))
    tol_dpool = 2 * S * U * b["a_dpool"] + tol_dz1 @ w1a
    tol_dx = tol_dpool[:, None, :] / HW + 4 * U * ((d["dy"] * sv["s"][:, None, :]).abs() + b["dpool"].abs()[:, None, :] / HW) + bf_term(b["dx"], bf)
    tols = dict(dz2=tol_dz2, dz1=tol_dz1, dpool=tol_dpool, dx=tol_dx,
                dw1=tol_dz1.t() @ sv["pool"].abs() + 2 * U * b["dw1"].abs(), db1=tol_dz1.sum(0) + 2 * U * b["db1"].abs(),
                dw2=tol_dz2.t() @ sv["h"].abs() + 2 * U * b["dw2"].abs(), db2=tol_dz2.sum(0) + 2 * U * b["db2"].abs())
    for k in ("dz2", "dz1", "dpool", "dx", "dw1", "db1", "dw2", "db2"):
        check(got[k], b[k], tols[k], "%s %s" % (tag, k), "se " + k, dtype)
    # the decisions are read from the saved vectors: exactly 0 at z2 = +-3 and at h = 0
    dz2, dz1 = got["dz2"].cpu().reshape(N, C), got["dz1"].cpu().reshape(N, S)
    assert bool((dz2[:, 0] == 0).all()) and bool((dz2[:, -1] == 0).all()), tag + ": dz2 at z2 = +-3"
    assert bool((dz1[sv["h"] == 0.0] == 0).all()), tag + ": dz1 at h = 0"
