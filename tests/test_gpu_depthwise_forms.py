"""GPU: every launch form of the depthwise 3x3 kernels (csrc/depthwise.hip: the rolling-window kernels, several rows per thread with a
short last row block, the capped grid of the rolling filter gradient, blocks with idle lanes) against the float64 reference of
tests/depthwise_ref.py.  The shapes and the plans they were written for are in tests/depthwise_cases.py; test_depthwise_plan.py proves
without a GPU that each shape lands on its form.

The C ABI is called directly, so every allocation is the test's own:
  x, dy, w     views into larger buffers that are NaN on both sides, each guard at least (W + 2) * C elements (more than a row of pixels: a
               tap that is fetched from beyond the map poisons the result); view starts are 16-byte aligned;
  y, dx, dw, the filter gradient's scratch
               views into canary buffers: after the call every element outside the view still has the canary's bits; the scratch itself
               starts as NaN, so a partial slice that is added without having been written shows.

Data set "int": x, dy, w drawn from {-2 .. 2}.  Every product and partial sum is an integer below 2^24 (the largest possible magnitude is
4 * N P Q <= 4 * 100352 for the filter gradient, 36 for an output element, which bf16 holds exactly): whatever the order of the
additions the result is the reference's, bit for bit, in both storage types.  This run finds a misplaced tap, a dropped or repeated row
or column.
Data set "real": oracle.prng.uniform values (rounded to bf16 first for bf16 storage).  fp32 outputs within 1e-5 * max(1, max|ref|); bf16
outputs within 2^-8 |ref| (one rounding of the stored value) plus that; the filter gradient per element within
L 2^-24 S_abs + 2^-24 |ref|, where S_abs = sum |dy x| of the tap and channel and L = ceil(pixels / partial slices) + 256 bounds the longest
fp32 addition chain of one partial (the worst-case bound of recursive summation; the partials are then added in double).
The filter gradient runs twice per data set and must repeat itself bit for bit."""
import ctypes
import math

import pytest
import torch

import depthwise_cases as D
import depthwise_ref as R
from gemm_ref import CANARY_BF16, CANARY_F32

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)
    _CACHE.clear()


def _guard(W, C):
    return -(-((W + 2) * C) // 16) * 16          # a multiple of 16 elements: the view starts on a 16-byte boundary in either type


def framed_input(t, dtype, guard):
    """t (host, fp32) as a view inside a NaN-filled device buffer"""
    n = t.numel()
    whole = torch.full((guard + n + guard,), NAN, dtype=dtype, device="cuda")
    view = whole[guard:guard + n]
    view.copy_(t.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == 0
    return whole, view


def framed_output(n, dtype, guard, inside=None):
    """n elements inside a canary-filled device buffer (the view itself = the canary too, or `inside`)"""
    bits, canary = (torch.int16, CANARY_BF16) if dtype == torch.bfloat16 else (torch.int32, CANARY_F32)
    whole = torch.empty(guard + n + guard, dtype=dtype, device="cuda")
    whole.view(bits).fill_(canary)
    view = whole[guard:guard + n]
    if inside is not None:
        view.fill_(inside)
    assert view.data_ptr() % 16 == 0
    return whole, view, (bits, canary, guard, n)


def assert_guards_intact(whole, frame, what):
    bits, canary, guard, n = frame
    b = whole.view(bits)
    bad = int((b[:guard] != canary).sum()) + int((b[guard + n:] != canary).sum())
    assert bad == 0, "%s: %d element(s) outside the output changed" % (what, bad)


_CACHE = {}


def data_and_reference(shape, dataset, bf):
    """inputs (host fp32, exactly representable in the storage type) and the float64 results; the last set is kept for the next case"""
    from oracle import prng
    key = (shape, dataset, bf and dataset == "real")
    if key in _CACHE:
        return _CACHE[key]
    _CACHE.clear()
    N, H, W, C, stride = shape
    P, Q = R.out_size(H, stride), R.out_size(W, stride)
    seed = 1000 * H + 10 * W + C
    if dataset == "int":
        draw = lambda shp, s: torch.from_numpy(prng.integers(shp, seed + s, 0, 5) - 2).float()
    else:
        rnd = (lambda t: t.to(torch.bfloat16).float()) if bf else (lambda t: t)
        draw = lambda shp, s: rnd(torch.from_numpy(prng.uniform(shp, seed + s)))
    x, dy = draw((N, H, W, C), 1), draw((N, P, Q, C), 2)
    w = torch.from_numpy(prng.integers((C, 9), seed + 3, 0, 5) - 2).float() if dataset == "int" else torch.from_numpy(prng.uniform((C, 9), seed + 3))
    dw, s_abs = R.wgrad(dy, x, stride)
    out = dict(x=x, dy=dy, w=w, P=P, Q=Q, y=R.forward(x, w, stride), dx=R.dgrad(dy, w, H, W, stride), dw=dw, s_abs=s_abs)
    _CACHE[key] = out
    return out


def compare(got, ref, dataset, bf, what):
    got = got.float().cpu()
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    if dataset == "int":
        assert torch.equal(got, ref.reshape(-1).float()), "%s: %d element(s) differ from the exact result" % (what, int((got != ref.reshape(-1).float()).sum()))
        return
    ref = ref.reshape(-1)
    tol = torch.full_like(ref, 1e-5 * max(1.0, float(ref.abs().max())))
    if bf:
        tol += 2.0 ** -8 * ref.abs()
    worst = float(((got.double() - ref).abs() / tol).max())
    print("%s: worst err / tol %.3f" % (what, worst))
    assert worst <= 1.0, what


PARAMS = [pytest.param(c, dataset, dtype, id="%s-%s-%s" % ("x".join(map(str, c["shape"])), dataset, dtype))
          for c in D.CASES for dataset in ("int", "real") for dtype in c["run"]]


@pytest.mark.parametrize("c,dataset,dtype", PARAMS)
def test_depthwise_form(L, c, dataset, dtype):
    shape = c["shape"]
    N, H, W, C, stride = shape
    bf = dtype == D.BF16
    adt = torch.bfloat16 if bf else torch.float32
    lib, dt = L.lib(), int(bf)
    # the plan the shape was written for is the plan the library takes (test_depthwise_plan.py asserts the same without a GPU)
    for op in D.OPS:
        rc, got = D.query(lib, op, dtype, shape)
        assert rc == 0 and D.as_written(op, shape, got) == c["plans"][dtype][op], (op, got)
    parts = c["plans"][dtype]["wgrad"][4]
    d = data_and_reference(shape, dataset, bf)
    P, Q = d["P"], d["Q"]
    guard = _guard(W, C)
    tag = "%s %s %s" % (shape, dataset, dtype)

    xw, xv = framed_input(d["x"], adt, guard)
    gw, gv = framed_input(d["dy"], adt, guard)
    ww, wv = framed_input(d["w"], torch.float32, guard)

    yw, yv, yf = framed_output(N * P * Q * C, adt, guard)
    L.check(lib.sat_dwconv3x3_fwd_t(dt, L.ptr(xv), L.ptr(wv), L.ptr(yv), N, H, W, C, stride, L.stream_ptr()), "sat_dwconv3x3_fwd_t")
    torch.cuda.synchronize()
    assert_guards_intact(yw, yf, tag + " forward")
    compare(yv, d["y"], dataset, bf, tag + " forward")
    del yw, yv

    dxw, dxv, dxf = framed_output(N * H * W * C, adt, guard)
    L.check(lib.sat_dwconv3x3_dgrad_t(dt, L.ptr(gv), L.ptr(wv), L.ptr(dxv), N, H, W, C, stride, L.stream_ptr()), "sat_dwconv3x3_dgrad_t")
    torch.cuda.synchronize()
    assert_guards_intact(dxw, dxf, tag + " data gradient")
    compare(dxv, d["dx"], dataset, bf, tag + " data gradient")
    del dxw, dxv

    need = lib.sat_dwconv3x3_wgrad_scratch_bytes(N, H, W, C, stride)
    assert need >= parts * 9 * C * 4 and need % 4 == 0
    runs = []
    for _ in range(2):
        sw, sv, sf = framed_output(need // 4, torch.float32, guard, inside=NAN)
        dww, dwv, dwf = framed_output(C * 9, torch.float32, guard)
        L.check(lib.sat_dwconv3x3_wgrad_t(dt, L.ptr(gv), L.ptr(xv), L.ptr(dwv), N, H, W, C, stride, L.ptr(sv), L.stream_ptr()), "sat_dwconv3x3_wgrad_t")
        torch.cuda.synchronize()
        assert_guards_intact(sw, sf, tag + " filter gradient scratch")
        assert_guards_intact(dww, dwf, tag + " filter gradient")
        runs.append(dwv.clone())
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32)), tag + ": the filter gradient does not repeat itself bit for bit"
    got = runs[0].cpu()
    assert not bool(torch.isnan(got).any()), tag + " filter gradient: NaN in the result"
    if dataset == "int":
        assert torch.equal(got, d["dw"].reshape(-1).float()), tag + " filter gradient: %d element(s) differ from the exact result" % int((got != d["dw"].reshape(-1).float()).sum())
    else:
        chain = math.ceil(N * P * Q / parts) + 256
        tol = chain * 2.0 ** -24 * d["s_abs"].reshape(-1) + 2.0 ** -24 * d["dw"].reshape(-1).abs()
        err = (got.double() - d["dw"].reshape(-1)).abs()          # (a tap that only ever meets the padding has S_abs = 0: exactly 0 is expected)
        print("%s filter gradient: worst err / tol %.3f (chain bound %d)" % (tag, float((err / tol.clamp(min=1e-300)).max()), chain))
        assert bool((err <= tol).all()), tag + " filter gradient"
    # the inputs were only read
    for whole, view, what in ((xw, xv, "x"), (gw, gv, "dy"), (ww, wv, "w")):
        assert bool(torch.isnan(whole[:guard]).all()) and bool(torch.isnan(whole[guard + view.numel():]).all()), what
