"""GPU: the LDS ring of the kernels that transpose an operand out of LDS (csrc/gemm_glds_kernel.h forms (0,1), (1,1), (1,2), (3,3) and
csrc/wgrad3x3.hip), whose fragment reads are inline asm with hand-counted waits (csrc/lds_frag.h).  A fragment read that overtakes the
LDS-DMA write of its tile, or a k-tile issued into a stage that is still being read, gives wrong products with no fault, so every form
runs at every ring depth sat_debug_option("glds_stages", n) can force and at reductions of
    1 k-tile (64), 2 (fewer tiles than stages), 5 and 9 (steady state plus drain); the split-K form at 19 and 33 tiles (10 + 9, 9 + 9 + 9 + 6)
and asserts
  (1) result - and tile statistics - at depths 1, 2, 3 and 4 are bit-identical to each other (the arithmetic, the order of the k-tiles and
      of the additions do not depend on the depth).  wgrad3x3 has no one-stage form: depth 1 runs as depth 2 there;
  (2) a repeated call is bit-identical;
  (3) the values agree with the float64 references of gemm_ref.py / conv_ref.py within the bounds those files already use: gemm_ref.tol_f32
      for the fp32 results, + 2^-8 |ref| for a bf16 result, + 2^-8 |product| for a joined one (conv_epilogue_cases.element_tol), the
      statistics within conv_epilogue_cases.stats_ref's fp32 summation bound;
  (4) no NaN anywhere in a result.
Framing: operands sit in NaN frames (conv_epilogue_cases / gemm_ref.framed), results in canary frames, split-K slabs start as NaN, and before
every call poison_lds() fills the LDS of the chip with NaN - 256 workgroups of the 128x128 form at depth 4 (128 KiB each, one per CU) multiply
NaN operands - so a fragment read ahead of its tile's arrival reads NaN, not the previous call's (identical) tile.
The smallest shapes that reach the ring: M = 128, N = 64 for the dense forms (two 64x64 tiles, or one 128x64 tile; the data gradients on the
128x128 tile have 128 channels), one 8 x 8 image for the 3x3 forms; the gemm_glds forms run on all three tile forms ("glds_tile"), each of
which is its own instantiation of the kernel.
"""
import ctypes

import pytest
import torch

import conv_epilogue_cases as T
import conv_ref as R
import gemm_ref as G
import test_gpu_conv_epilogues as E

pytestmark = pytest.mark.gpu

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64
NAN = float("nan")
DEPTHS = (1, 2, 3, 4)
KS = (64, 128, 320, 576)          # 1, 2, 5, 9 k-tiles
TILES = {"64x64": 0, "128x128": 1, "128x64": 2}          # csrc/gemm_glds.hip


@pytest.fixture(scope="module")
def env():
    import sat_amd  # noqa: F401
    from sat_amd import _lib, decoder
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield decoder, _lib
    for name, value in (("glds_stages", 0), ("glds_tile", -1), ("wgrad3x3", 1)):
        _lib.lib().sat_debug_option(name.encode(), value)
    torch.set_num_threads(threads)


def option(L, name, value):
    L.check(L.lib().sat_debug_option(name.encode(), value), "sat_debug_option(%s, %d)" % (name, value))


_POISON = {}


def poison_lds(dk, L):
    """NaN into every stage of every CU's LDS: 16 x 16 tiles of 128x128, four k-tiles, four stages"""
    if not _POISON:
        _POISON["a"] = torch.full((2048, 256), NAN, dtype=BF, device="cuda")
        _POISON["b"] = torch.full((256, 2048), NAN, dtype=BF, device="cuda")
        _POISON["c"] = torch.empty(2048, 2048, dtype=F32, device="cuda")
    option(L, "glds_stages", 4)
    option(L, "glds_tile", TILES["128x128"])
    L.profile_start()
    dk.gemm(_POISON["a"], _POISON["b"], amode=0, bmode=1, out=_POISON["c"], bf16_mfma=True)
    torch.cuda.synchronize()
    names = [e["name"] for e in L.profile_stop()]
    assert names == ["gemm_glds_nn_128x128"], names
    option(L, "glds_tile", -1)


def at_every_depth(dk, L, call, tile=-1):
    """call() -> (scope names, {name: tensor}) at depths 1 .. 4 and once more at the last depth; asserts (1), (2), (4); returns the first outcome"""
    runs = []
    for depth in DEPTHS + (DEPTHS[-1],):
        poison_lds(dk, L)
        option(L, "glds_stages", depth)
        option(L, "glds_tile", tile)
        try:
            runs.append(call())
        finally:
            option(L, "glds_stages", 0)
            option(L, "glds_tile", -1)
    names, first = runs[0]
    for t in first.values():
        assert not bool(torch.isnan(t.float()).any()), "NaN in a result at depth 1"          # (4)
    for depth, (n, out) in zip(DEPTHS[1:] + ("%d, repeated" % DEPTHS[-1],), runs[1:]):
        assert n == names, "depth %s launched %s, depth 1 %s" % (depth, n, names)
        for key, t in first.items():
            diff = int((t.view(torch.uint8) != out[key].view(torch.uint8)).sum())
            assert diff == 0, "%s at depth %s differs from depth 1 in %d bytes" % (key, depth, diff)          # (1), (2)
    return names, first


def profiled(L, fn):
    L.profile_start()
    try:
        rc = fn(L.stream_ptr())
        torch.cuda.synchronize()
    finally:
        names = sorted(e["name"] for e in L.profile_stop() for _ in range(int(e["launches"])))
    return rc, names


# ============================================================================= (0,1) bf16: the 1x1 data gradients, plain and joined with statistics
def _dgrad_case(kind, g):
    fused = kind == "fused"
    return dict(id="ring-%s-K%d" % (kind, g["R"] * g["S"] * g["K"]), kind=kind, op="dgrad", dt="bf16", g=g, relu_mask=fused, accumulate=False, add_mask=fused, stats=fused)


def _run_dgrad(dk, L, c, tile, want_name):
    s = T.inputs(c)
    ops = E.Operands(L, c, s)
    lib, p = L.lib(), L.ptr
    nbytes = lib.sat_conv2d_dgrad_stats_bytes(ctypes.byref(ops.geom))
    tile_rows = []

    def call():
        whole, vo = E._result_frame(ops.M, ops.N, ops.guard)
        swhole, sview = E._stats_frame(nbytes)
        tr = ctypes.c_int32(E.UNSET)
        if c["kind"] == "fused":
            fn = E._call_epilogue(L, c, ops, vo, sview[0], ctypes.byref(tr))
        else:
            fn = lambda st: lib.sat_conv2d_dgrad_bf16(p(ops.src), p(ops.w), p(vo), ctypes.byref(ops.geom), 0, st)          # noqa: E731
        rc, names = profiled(L, fn)
        L.check(rc, c["id"])
        G.assert_frame_untouched(whole, vo, G.CANARY_BF16)
        out = dict(dx=vo.clone())
        if c["kind"] == "fused":
            tile_rows.append(tr.value)
            nt = -(-ops.M // tr.value)
            G.assert_frame_untouched(swhole, sview[:, :nt * ops.N * 2], G.CANARY_F32)
            out["statistics"] = sview[0, :nt * ops.N * 2].clone()
        return names, out

    names, out = at_every_depth(dk, L, call, tile)
    assert names == [want_name], "the dispatch took %s, the case was written for %s" % (names, want_name)
    ref, prod = T.expected(c, s)
    got = out["dx"].float().cpu().to(F64)
    worst = float(((got - ref).abs() / T.element_tol(c, s, ref, prod)).max())
    worst_s = 0.0
    if c["kind"] == "fused":
        assert len(set(tile_rows)) == 1
        cs = dict(c, tile_rows=tile_rows[0])
        gst = out["statistics"].cpu().to(F64).reshape(-1, ops.N, 2)
        assert bool(torch.isfinite(gst).all())
        sref, stol = T.stats_ref(cs, s, got, tile_rows[0])
        err = (gst - sref).abs()
        worst_s = float(torch.where(stol > 0, err / stol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
    print("RING %s [%s]: result worst err / tol %.3f, statistics worst err / tol %.3f" % (c["id"], want_name, worst, worst_s))
    assert worst <= 1.0 and worst_s <= 1.0          # (3)
    ops.assert_inputs_unchanged()


def _channels(tile):
    """result columns of a data gradient: the 128-wide tile gets the 128 columns the shipped rules ask of it (M, N >= 128)"""
    return 128 if tile == "128x128" else 64


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", ["plain", "fused"])
def test_nn_bf16_data_gradient(env, kind, K, tile):
    dk, L = env
    _run_dgrad(dk, L, _dgrad_case(kind, R.geom(2, 8, 8, _channels(tile), K, 1, 1, 1, 0)), TILES[tile], "gemm_glds_nn_" + tile)


# ============================================================================= (3,3): the gathered data gradients.  One 8 x 8 image, 64 channels and filters;
# the taps set the reduction: 1x1 with pad 1 (one k-tile; only the 1x1 / pad 0 form is a plain GEMM), 1x2, 1x5, 3x3 pad 1
DGRAD_TAPS = {64: (1, 1, 1), 128: (1, 2, 0), 320: (1, 5, 0), 576: (3, 3, 1)}


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K", KS)
def test_conv_dgrad_bf16(env, K, tile):
    dk, L = env
    r, s, pad = DGRAD_TAPS[K]
    _run_dgrad(dk, L, _dgrad_case("plain", R.geom(1, 8, 8, _channels(tile), 64, r, s, 1, pad)), TILES[tile], "gemm_glds_conv_dgrad_" + tile)


# ============================================================================= (0,1) float and (1,1) float: sat_gemm_ex, fp32 result of bf16 operands
def _run_gemm(dk, L, mode, M, N, K, tile, want_names, slab_elems=0):
    amode, bmode = {"nn": (0, 1), "tn": (1, 1)}[mode]
    gen = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    A = torch.randn(M, K, generator=gen)
    B = torch.randn(K, N, generator=gen)
    A_st = A if amode == 0 else A.t()
    _, va = G.framed(A_st.shape[0], A_st.shape[1], BF, pad_cols=8, guard_rows=1, fill=NAN, device="cuda", aligned=True)
    _, vb = G.framed(K, N, BF, pad_cols=8, guard_rows=1, fill=NAN, device="cuda", aligned=True)
    va.copy_(A_st)
    vb.copy_(B)

    def call():
        whole, vc = G.framed(M, N, F32, pad_cols=4, guard_rows=2, fill=G.CANARY_F32, device="cuda", aligned=True)
        slab = torch.full((slab_elems,), NAN, device="cuda") if slab_elems else None          # a partial read before it is written shows
        L.profile_start()
        try:
            dk.gemm(va, vb, amode=amode, bmode=bmode, M=M, N=N, K=K, out=vc, slab=slab, bf16_mfma=True)
            torch.cuda.synchronize()
        finally:
            names = sorted(e["name"] for e in L.profile_stop() for _ in range(int(e["launches"])))
        G.assert_frame_untouched(whole, vc, G.CANARY_F32)
        if slab is not None:          # exactly `splits` partials: each of them written in full (the reduce shares the GEMM's profiler scope)
            assert not bool(torch.isnan(slab).any()), "%d floats of the slab were not written" % int(torch.isnan(slab).sum())
        return names, dict(C=vc.clone())

    names, out = at_every_depth(dk, L, call, tile)
    assert names == sorted(want_names), "the dispatch took %s, the case was written for %s" % (names, sorted(want_names))
    ref, _, _ = G.reference(A_st, B, amode=amode, bmode=bmode, round_inputs_to_bf16=True)
    err = float((out["C"].cpu().to(F64) - ref).abs().max())
    tol = G.tol_f32(ref, K)
    print("RING %s %dx%dx%d [%s]: max |err| %.3e, bound %.3e" % (mode, M, N, K, names[0], err, tol))
    assert err <= tol          # (3)


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K", KS)
def test_nn_float(env, K, tile):
    dk, L = env
    _run_gemm(dk, L, "nn", 128, 64, K, TILES[tile], ["gemm_glds_nn_" + tile])


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K", KS)
def test_tn_float(env, K, tile):
    dk, L = env
    _run_gemm(dk, L, "tn", 128, 64, K, TILES[tile], ["gemm_glds_tn_" + tile])


# split-K (launch_gemm_bf16_tile: a slab, fewer than 256 tiles, K >= 1024): ns = min(768 / 2 tiles, K / 512, 4 at least by the byte rule) ->
# K = 1216: two splits of 10 and 9 k-tiles; K = 2112: four of 9, 9, 9 and 6.  The partials go through the fixed-order reduce kernel.
@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("K,splits", [(1024 + 192, 2), (2048 + 64, 4)])
def test_tn_float_split_k(env, K, splits, tile):
    dk, L = env
    _run_gemm(dk, L, "tn", 128, 64, K, TILES[tile], ["gemm_glds_tn_" + tile], slab_elems=splits * 128 * 64)


# ============================================================================= (1,2) and wgrad3x3: the 3x3 weight gradients over n images of 8 x 8 pixels (n k-tiles)
def _run_wgrad(dk, L, n, own, tile, want_names):
    g = R.geom(n, 8, 8, 64, 64, 3, 3, 1, 1)
    gen = torch.Generator().manual_seed(77 + n)
    x = R.bf16_round(torch.randn(n, 8, 8, 64, generator=gen))
    dy = R.bf16_round(torch.randn(n, 8, 8, 64, generator=gen))
    guard = 10 * 64
    keep = []

    def nan_framed(t):
        whole = torch.full((guard + t.numel() + guard,), NAN, dtype=BF, device="cuda")
        view = whole[guard:guard + t.numel()]
        view.copy_(t.reshape(-1))
        keep.append((whole, whole.clone()))
        return view

    xv, gv = nan_framed(x), nan_framed(dy)
    geom = L.ConvGeom(**g)
    out_elems = 64 * 9 * 64

    def call():
        whole, vw = G.framed(1, out_elems, F32, guard_rows=1, fill=G.CANARY_F32, device="cuda")
        fn = lambda st: L.lib().sat_conv2d_wgrad_bf16(L.ptr(gv), L.ptr(xv), L.ptr(vw[0]), ctypes.byref(geom), None, 0, st)          # noqa: E731
        option(L, "wgrad3x3", 1 if own else 0)
        try:
            rc, names = profiled(L, fn)
        finally:
            option(L, "wgrad3x3", 1)
        L.check(rc, "sat_conv2d_wgrad_bf16")
        G.assert_frame_untouched(whole, vw, G.CANARY_F32)
        return names, dict(dW=vw[0].clone())

    names, out = at_every_depth(dk, L, call, tile)
    assert names == want_names, "the dispatch took %s, the case was written for %s" % (names, want_names)
    ref = R.wgrad(g, dy, x).reshape(-1)
    err = float((out["dW"].cpu().to(F64) - ref).abs().max())
    tol = G.tol_f32(ref, n * 64)
    print("RING wgrad %d images [%s]: max |err| %.3e, bound %.3e" % (n, names[0], err, tol))
    assert err <= tol          # (3)
    for whole, before in keep:
        assert torch.equal(whole.view(torch.int16), before.view(torch.int16))


@pytest.mark.parametrize("tile", sorted(TILES))
@pytest.mark.parametrize("n", [k // 64 for k in KS])
def test_conv_wgrad_implicit_gemm(env, n, tile):
    dk, L = env
    _run_wgrad(dk, L, n, False, TILES[tile], ["gemm_glds_conv_wgrad_" + tile])


@pytest.mark.parametrize("n", [k // 64 for k in KS])
def test_wgrad3x3_nine_waves(env, n):
    """the W = 8 geometry of test_gpu_wgrad3x3_forms.py: 21 LDS-DMA pieces per k-tile, waves that issue two and wait on vmcnt(2) / vmcnt(4)"""
    dk, L = env
    _run_wgrad(dk, L, n, True, -1, ["gemm_wgrad3x3"])
