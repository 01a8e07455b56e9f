"""GPU: every gather form of the dense convolutions ("Convolution gather forms": G1 - G18) against the float64 tap-loop
reference conv_ref, inside NaN frames.  The cases and the kernel each must reach are in conv_cases.py.

Each case calls the C ABI directly (sat_conv2d_fwd / _dgrad / _wgrad and their _bf16 forms) with nothing forced: the shipped dispatch
picks the kernel.  The activation, the output gradient and the filter each live as a dense (rows, channels) window of a NaN-filled
allocation with max(R, S) * (max(W, Q) + 1) guard pixels before and after (2 guard rows for the filter), so a gather that is a filter
height off the map lands inside the allocation and in NaN; the bias sits in a NaN frame; the result lives in a frame of canary bit
patterns with guard rows of the same depth; the split-K slab is NaN-filled and exactly sat_conv2d_wgrad_slab_bytes long (where that is
0 the case runs once more with a generous slab).  Then
  (a) the values agree with conv_ref (inputs rounded to bf16 first for bf16 storage) per element: gemm_ref.tol_f32(ref, Kr) for the fp32
      accumulation, + 2^-8 |ref| for a bf16 result, + 2^-8 |prod| more for a bf16 accumulate (the staged write-out rounds the tile
      before it adds the old value: the two_roundings rule of test_gpu_gemm_store_paths.py);
  (b) nothing outside the result window changed (raw bits); the parity classes without taps hold +0.0, or the old bits under accumulate;
  (c) the result is non-finite exactly where the reference is: nowhere, unless the case is a poison case.  Forward and filter gradient:
      a NaN in one activation channel and an Inf in one filter tap / one output-gradient element; the zero padding times the Inf is NaN
      in the reference as in every kernel.  Data gradient: both go into the output gradient - an Inf FILTER tap would meet the zeros that
      stand for "no output pixel under this tap", and how many of those a pixel has is the kernel's business (the parity classes have
      none), so the operation does not define the result there;
  (d) the sorted profiler scope names, one per launch, equal the case's list.  A mismatch FAILS: re-derive the case;
  (e) a filter gradient is bit-identical when the call is repeated.
"""
import ctypes
import os
import zlib

import pytest
import torch

import conv_cases as T
import conv_ref as R
import gemm_ref as G

pytestmark = pytest.mark.gpu

# nothing may be forced: the table pins what the SHIPPED rules launch
_FORCED = sorted(k for k in os.environ if k.startswith(("SAT_GLDS_", "SAT_SPLIT_")) or k in ("SAT_NO_GLDS", "SAT_TILES128_MIN", "SAT_TILE_ORDER",
                                                                                             "SAT_NO_WGRAD3X3", "SAT_WIDE_TILES", "SAT_W3_TARGET",
                                                                                             "SAT_PROFILE_SHAPES"))
assert not _FORCED, "dispatch overrides are set: %s" % _FORCED

F32, BF = torch.float32, torch.bfloat16
NAN = float("nan")
GENEROUS_SLAB = 1 << 22          # floats


@pytest.fixture(scope="module")
def env():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)


def _frame(t2d, dtype, guard, fill):
    whole, view = G.framed(t2d.shape[0], t2d.shape[1], dtype, pad_cols=0, guard_rows=guard, fill=fill, device="cuda", aligned=True)
    return whole, view


def _launch(L, c, geom, ptrs, slab):
    lib = L.lib()
    sfx = "_bf16" if c["dt"] == "bf16" else ""
    st = L.stream_ptr()
    L.profile_start()
    try:
        if c["op"] == "fwd":
            rc = getattr(lib, "sat_conv2d_fwd" + sfx)(ptrs["x"], ptrs["w"], ptrs["bias"], ptrs["out"], ctypes.byref(geom), st)
        elif c["op"] == "dgrad":
            rc = getattr(lib, "sat_conv2d_dgrad" + sfx)(ptrs["dy"], ptrs["w"], ptrs["out"], ctypes.byref(geom), 1 if c["accumulate"] else 0, st)
        else:
            rc = getattr(lib, "sat_conv2d_wgrad" + sfx)(ptrs["dy"], ptrs["x"], ptrs["out"], ctypes.byref(geom), L.ptr(slab), 0 if slab is None else slab.numel(), st)
        L.check(rc, c["id"])
        torch.cuda.synchronize()
    finally:
        entries = L.profile_stop()
    return sorted(e["name"] for e in entries for _ in range(int(e["launches"])))


def _tapless_class_mask(c):
    """(H, W) bool: pixels of the stride-2 parity classes that no filter tap reaches (conv_dgrad_any: rc * sc == 0)"""
    g = c["g"]
    m = torch.zeros(g["H"], g["W"], dtype=torch.bool)
    if not (c["op"] == "dgrad" and c["dt"] == "bf16" and g["stride"] == 2):
        return m
    for ph in range(2):
        for pw in range(2):
            r0, s0 = (ph + g["pad"]) & 1, (pw + g["pad"]) & 1
            if r0 >= g["R"] or s0 >= g["S"]:
                m[ph::2, pw::2] = True
    return m


def run_case(L, c):
    g = c["g"]
    bf = c["dt"] == "bf16"
    dt = BF if bf else F32
    P, Q = R.out_hw(g)
    M, N, Kr = T.gemm_dims(c)
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    x = torch.randn(g["N"], g["H"], g["W"], g["C"], generator=gen)
    w = torch.randn(g["K"], g["R"], g["S"], g["C"], generator=gen)
    dy = torch.randn(g["N"], P, Q, g["K"], generator=gen)
    bias = torch.randn(g["K"], generator=gen) if c["bias"] else None
    old = torch.randn(g["N"], g["H"], g["W"], g["C"], generator=gen).to(dt).float() if c["accumulate"] else None
    if c["poison"]:
        if c["op"] == "fwd":
            x[g["N"] - 1, g["H"] // 2, 0, 3] = NAN; w[g["K"] - 2, g["R"] - 1, 0, 5 % g["C"]] = float("inf")
        elif c["op"] == "dgrad":
            dy[g["N"] - 1, P // 2, 0, 3] = NAN; dy[0, 0, Q - 1, 5] = float("-inf")
        else:
            x[g["N"] - 1, g["H"] // 2, 0, 3] = NAN; dy[0, 0, Q - 1, 5] = float("inf")

    guard = max(g["R"], g["S"]) * (max(g["W"], Q) + 1)
    geom = L.ConvGeom(**g)
    _, vx = _frame(x.reshape(-1, g["C"]), dt, guard, NAN)
    _, vdy = _frame(dy.reshape(-1, g["K"]), dt, guard, NAN)
    _, vw = _frame(w.reshape(g["K"], -1), dt, 2, NAN)
    ptrs = dict(x=L.ptr(vx), dy=L.ptr(vdy), w=L.ptr(vw), bias=None)
    if c["op"] != "dgrad":
        vx.copy_(x.reshape(-1, g["C"]))
    if c["op"] != "fwd":
        vdy.copy_(dy.reshape(-1, g["K"]))
    if c["op"] != "wgrad":
        vw.copy_(w.reshape(g["K"], -1))
    if bias is not None:
        vbias = G.framed(1, g["K"], F32, pad_cols=3, guard_rows=1, fill=NAN, device="cuda")[1][0]
        vbias.copy_(bias)
        ptrs["bias"] = L.ptr(vbias)

    out_dt = F32 if c["op"] == "wgrad" else dt
    canary = G.CANARY_BF16 if out_dt == BF else G.CANARY_F32
    if c["op"] == "fwd":
        shape, rows, ref, prod = (g["N"], P, Q, g["K"]), (M, N), R.forward(g, x, w, bias, round_inputs_to_bf16=bf), None
    elif c["op"] == "dgrad":
        shape, rows = (g["N"], g["H"], g["W"], g["C"]), (M, N)
        ref, prod = R.dgrad(g, dy, w, dx_old=old, accumulate=c["accumulate"], round_inputs_to_bf16=bf)
    else:
        shape, rows, ref, prod = (g["K"], g["R"], g["S"], g["C"]), (M, N), R.wgrad(g, dy, x, round_inputs_to_bf16=bf), None
    out_guard = 2 if c["op"] == "wgrad" else guard

    def one_run(slab, want_names):
        whole, vo = G.framed(rows[0], rows[1], out_dt, pad_cols=0, guard_rows=out_guard, fill=canary, device="cuda", aligned=True)
        if c["accumulate"]:
            vo.copy_(old.reshape(rows))
        ptrs["out"] = L.ptr(vo)
        names = _launch(L, c, geom, ptrs, slab)
        assert names == want_names, "the dispatch took %s, the case was written for %s" % (names, want_names)          # (d)
        G.assert_frame_untouched(whole, vo, canary)          # (b)
        return vo

    def check_values(vo, what):
        got = vo.float().cpu().double().reshape(shape)
        nan_got, nan_ref = torch.isnan(got), torch.isnan(ref)
        assert torch.equal(nan_got, nan_ref), "%s: NaN at %d elements, the reference has %d" % (what, int(nan_got.sum()), int(nan_ref.sum()))   # (c)
        inf = torch.isinf(ref)
        assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), what
        assert c["poison"] or not (nan_ref.any() or inf.any())
        tol = torch.full_like(ref, G.tol_f32(ref, Kr))
        if out_dt == BF:
            tol += 2.0 ** -8 * ref.abs().nan_to_num(0.0, 0.0, 0.0)
            if c["accumulate"]:
                tol += 2.0 ** -8 * prod.abs().nan_to_num(0.0, 0.0, 0.0)          # two roundings
        fin = torch.isfinite(ref)
        err = (got - ref).abs()[fin]
        worst = (err / tol[fin]).max().item() if err.numel() else 0.0
        print("%s [%s %s]%s: max |err| %.3e, worst err / tol %.3f" % (c["id"], c["form"], c["dt"], what, err.max().item() if err.numel() else 0.0, worst))
        assert worst <= 1.0          # (a)
        tapless = _tapless_class_mask(c)
        if tapless.any():
            bits = vo.view(torch.int16).cpu().reshape(shape)[:, tapless]
            want = old.to(BF).view(torch.int16).reshape(shape)[:, tapless] if c["accumulate"] else torch.zeros_like(bits)          # +0.0
            assert torch.equal(bits, want), "%s: the parity classes without taps" % what

    if c["op"] != "wgrad":
        check_values(one_run(None, c["names"]), "")
        return
    nbytes = L.lib().sat_conv2d_wgrad_slab_bytes(ctypes.byref(geom))
    assert nbytes % 4 == 0
    slab = torch.full((nbytes // 4,), NAN, device="cuda") if nbytes else None          # a partial that is read without having been written shows
    first = one_run(slab, c["names"])
    check_values(first, "")
    again = one_run(slab, c["names"])
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), "the repeated filter gradient differs"          # (e)
    if not nbytes:
        check_values(one_run(torch.full((GENEROUS_SLAB,), NAN, device="cuda"), c.get("names_slab", c["names"])), " (slab offered)")


@pytest.mark.parametrize("c", T.TABLE, ids=lambda c: c["id"])
def test_conv_gather_form(env, c):
    run_case(env, c)
