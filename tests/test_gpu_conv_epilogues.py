"""GPU: the three epilogues of the dense bf16 convolution launches ("Convolution statistics epilogues") - forward tile statistics,
BatchNorm-backward tile statistics, the joined gradient - on every launch form that can carry one, against float64 references inside NaN
frames.  The cases, the kernel each must reach and the *tile_rows it must report are in conv_epilogue_cases.py.

Each case calls the C ABI directly (sat_conv2d_fwd_bf16_stats / sat_conv2d_dgrad_bf16_bnstats / sat_conv2d_dgrad_bf16_fused) with nothing
forced.  Activations, gradients and filters are dense windows of NaN-filled allocations with guard pixels as in test_gpu_conv_forms.py; bn_x
and add_src are framed the same way; both masks lie between 0xFF bytes; bn_mean / bn_invstd sit in NaN frames; the result lives in a frame of
canary bit patterns and, for a joined launch, starts as canary NaN itself (a finite result proves the old contents were never read); the
statistics buffer is exactly sat_conv2d_{fwd,dgrad}_stats_bytes long inside a canary frame.  Then
  (1) the stored y / dx agree with conv_ref per element under the rule of test_gpu_conv_forms.py (two roundings for accumulating and joined
      launches);
  (2) they are bit-identical to the same call without the epilogue: sat_conv2d_fwd_bf16 / sat_conv2d_dgrad_bf16, and for a joined launch the
      two-step path (add_src gated by the mask written into dx, then sat_conv2d_dgrad_bf16 with accumulate = 1);
  (3) add_src, bn_x and the masks are unchanged (raw bits of their whole allocations);
  (4) *tile_rows equals the table's value;
  (5) EVERY tile and channel of the statistics agrees with the float64 sums over the kernel's own stored values in rows
      [t * tile_rows, min(M, (t + 1) * tile_rows)) - "of the stored values" is the contract - within the fp32 summation bound
      (tile_rows + 2) * 2^-24 * sum |terms| (conv_epilogue_cases.stats_ref: derived, not measured); the worst err / tol is printed;
  (6) nothing outside the result window changed, and nothing outside the first ntiles * N * 2 floats of the statistics buffer (the sizes assume
      64-row tiles: with 128-row tiles the upper part keeps its canary);
  (7) no NaN in the result or the statistics, although every operand sits in NaN;
  (8) the sorted profiler scope names equal the case's list.  A mismatch FAILS: re-derive the case;
  (9) a repeated call gives bit-identical results and statistics (the reduction order is fixed).
The declined and refused requests follow the table's cases.
"""
import ctypes
import os

import pytest
import torch

import batchnorm_ref as B
import conv_epilogue_cases as T
import conv_ref as R
import gemm_ref as G

pytestmark = pytest.mark.gpu

# nothing may be forced: the table pins what the SHIPPED rules launch
_FORCED = sorted(k for k in os.environ if k.startswith(("SAT_GLDS_", "SAT_SPLIT_")) or k in ("SAT_NO_GLDS", "SAT_TILES128_MIN", "SAT_TILE_ORDER",
                                                                                             "SAT_NO_WGRAD3X3", "SAT_WIDE_TILES", "SAT_W3_TARGET",
                                                                                             "SAT_PROFILE_SHAPES"))
assert not _FORCED, "dispatch overrides are set: %s" % _FORCED

F32, BF, U8, F64 = torch.float32, torch.bfloat16, torch.uint8, torch.float64
NAN = float("nan")
SAT_EINVAL = 1                    # csrc/common.h
UNSET = -7                        # what *tile_rows holds before a call
MASK_GUARD = 64                   # bytes of 0xFF in front of and behind a mask


@pytest.fixture(scope="module")
def env():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)


def _framed(t2d, guard, offset_elems=0):
    """t2d (rows, cols) as a dense bf16 window of a NaN allocation with `guard` rows around it, offset_elems * 2 bytes off a 16-byte boundary"""
    whole, view = G.framed(t2d.shape[0], t2d.shape[1], BF, pad_cols=0, guard_rows=guard, fill=NAN, offset_elems=offset_elems, device="cuda",
                           aligned=offset_elems % 8 == 0)
    view.copy_(t2d)
    return whole, view


def _framed_vec(v):
    whole, view = G.framed(1, v.numel(), F32, pad_cols=3, guard_rows=1, fill=NAN, device="cuda")
    view[0].copy_(v)
    return whole, view[0]


def _framed_mask(bits):
    packed = B.pack_mask(bits)
    whole = torch.full((2 * MASK_GUARD + packed.numel(),), 0xFF, dtype=U8, device="cuda")
    view = whole[MASK_GUARD:MASK_GUARD + packed.numel()]
    view.copy_(packed)
    return whole, view


def _result_frame(M, N, guard, offset_elems=0):
    return G.framed(M, N, BF, pad_cols=0, guard_rows=guard, fill=G.CANARY_BF16, offset_elems=offset_elems, device="cuda", aligned=offset_elems % 8 == 0)


def _stats_frame(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0
    whole, view = G.framed(1, nbytes // 4, F32, guard_rows=1, fill=G.CANARY_F32, device="cuda")
    return whole, view          # view: (1, floats)


def _profiled(L, call):
    """(return code, sorted scope names, one per launch) of call(stream)"""
    L.profile_start()
    try:
        rc = call(L.stream_ptr())
        torch.cuda.synchronize()
    finally:
        entries = L.profile_stop()
    return rc, sorted(e["name"] for e in entries for _ in range(int(e["launches"])))


def _bits16(t):
    return t.view(torch.int16)


class Operands:
    """the device side of one case's inputs; `keep` = (name, whole allocation, its bits before any call) of everything a call must not write"""

    def __init__(self, L, c, s, bn_off=0, add_off=0):
        g = c["g"]
        P, Q = R.out_hw(g)
        self.M, self.N = s["M"], s["N"]
        self.guard = max(g["R"], g["S"]) * (max(g["W"], Q) + 1)
        self.geom = L.ConvGeom(**g)
        self.keep = []
        src_cols = g["C"] if c["op"] == "fwd" else g["K"]
        self.src = self._add("src", *_framed(s["src"].reshape(-1, src_cols), self.guard))
        self.w = self._add("w", *_framed(s["w"].reshape(g["K"], -1), 2))
        self.bn_x = self.add_src = self.relu_mask = self.add_mask = self.mean = self.invstd = self.old = None
        if c["op"] == "fwd":
            return
        self.bn_x = self._add("bn_x", *_framed(s["bn_x"], self.guard, bn_off))
        self.add_src = self._add("add_src", *_framed(s["add_src"], self.guard, add_off))
        self.relu_mask = self._add("bn_relu_mask", *_framed_mask(s["relu_bits"]))
        self.add_mask = self._add("add_mask", *_framed_mask(s["add_bits"]))
        self.mean = self._add("bn_mean", *_framed_vec(s["mean"]))
        self.invstd = self._add("bn_invstd", *_framed_vec(s["invstd"]))
        self.old = s["old"].to(BF).cuda()
        self.add_bits = s["add_bits"].cuda()

    def _add(self, name, whole, view):
        self.keep.append((name, whole, whole.clone()))
        return view

    def assert_inputs_unchanged(self):
        for name, whole, before in self.keep:
            assert torch.equal(whole.view(U8), before.view(U8)), "%s (or its frame) was written to" % name          # (3)


def _call_epilogue(L, c, ops, out, stats, tr):
    lib, p = L.lib(), L.ptr
    if c["kind"] == "fwd":
        return lambda st: lib.sat_conv2d_fwd_bf16_stats(p(ops.src), p(ops.w), p(out), ctypes.byref(ops.geom), p(stats), tr, st)
    relu = p(ops.relu_mask) if c["relu_mask"] else None
    if c["kind"] == "bnstats":
        return lambda st: lib.sat_conv2d_dgrad_bf16_bnstats(p(ops.src), p(ops.w), p(out), ctypes.byref(ops.geom), 1 if c["accumulate"] else 0, p(ops.bn_x), relu,
                                                            p(ops.mean), p(ops.invstd), p(stats), tr, st)
    am = p(ops.add_mask) if c["add_mask"] else None
    if not c["stats"]:
        return lambda st: lib.sat_conv2d_dgrad_bf16_fused(p(ops.src), p(ops.w), p(out), ctypes.byref(ops.geom), p(ops.add_src), am, None, None, None, None, None, None, st)
    return lambda st: lib.sat_conv2d_dgrad_bf16_fused(p(ops.src), p(ops.w), p(out), ctypes.byref(ops.geom), p(ops.add_src), am, p(ops.bn_x), relu, p(ops.mean),
                                                      p(ops.invstd), p(stats), tr, st)


def _plain(L, c, ops, out_off=0):
    """the same result without the epilogue: (frame, window).  A joined launch: add_src gated by the mask written out, then an accumulating call"""
    lib, p = L.lib(), L.ptr
    whole, vo = _result_frame(ops.M, ops.N, ops.guard, out_off)
    if c["kind"] == "fwd":
        rc = lib.sat_conv2d_fwd_bf16(p(ops.src), p(ops.w), None, p(vo), ctypes.byref(ops.geom), L.stream_ptr())
    else:
        acc = c["accumulate"]
        if c["kind"] == "fused":
            vo.copy_(torch.where(ops.add_bits, ops.add_src, torch.zeros((), dtype=BF, device="cuda")) if c["add_mask"] else ops.add_src)
            acc = True
        elif acc:
            vo.copy_(ops.old)
        rc = lib.sat_conv2d_dgrad_bf16(p(ops.src), p(ops.w), p(vo), ctypes.byref(ops.geom), 1 if acc else 0, L.stream_ptr())
    L.check(rc, c["id"] + " (plain)")
    torch.cuda.synchronize()
    G.assert_frame_untouched(whole, vo, G.CANARY_BF16)
    return whole, vo


def run_case(L, c):
    s = T.inputs(c)
    ops = Operands(L, c, s)
    M, N = ops.M, ops.N
    lib = L.lib()
    nbytes = (lib.sat_conv2d_fwd_stats_bytes if c["kind"] == "fwd" else lib.sat_conv2d_dgrad_stats_bytes)(ctypes.byref(ops.geom))
    assert nbytes == -(-M // 64) * N * 2 * 4          # sized for 64-row tiles

    def one_run():
        whole, vo = _result_frame(M, N, ops.guard)
        if c["accumulate"]:
            vo.copy_(ops.old)          # (a joined launch keeps the canary NaN: it must not read dx)
        swhole, sview = _stats_frame(nbytes) if c["stats"] else (None, None)
        tr = ctypes.c_int32(UNSET)
        rc, names = _profiled(L, _call_epilogue(L, c, ops, vo, None if sview is None else sview[0], ctypes.byref(tr) if c["stats"] else None))
        L.check(rc, c["id"])
        assert names == c["names"], "the dispatch took %s, the case was written for %s" % (names, c["names"])          # (8)
        G.assert_frame_untouched(whole, vo, G.CANARY_BF16)          # (6)
        if c["stats"]:
            assert tr.value == c["tile_rows"], "*tile_rows = %d, the case was written for %d" % (tr.value, c["tile_rows"])          # (4)
            nt = -(-M // tr.value)
            G.assert_frame_untouched(swhole, sview[:, :nt * N * 2], G.CANARY_F32)          # (6)
            return vo, sview[0, :nt * N * 2].reshape(nt, N, 2)
        return vo, None

    vo, st = one_run()
    ref, prod = T.expected(c, s)
    got = vo.float().cpu().to(F64)
    assert bool(torch.isfinite(got).all()), "%d non-finite results" % int((~torch.isfinite(got)).sum())          # (7)
    worst_v = float(((got - ref).abs() / T.element_tol(c, s, ref, prod)).max())
    worst_s, where = 0.0, ""
    if c["stats"]:
        gst = st.cpu().to(F64)
        assert bool(torch.isfinite(gst).all()), "%d non-finite statistics" % int((~torch.isfinite(gst)).sum())          # (7)
        sref, stol = T.stats_ref(c, s, got, c["tile_rows"])
        err = (gst - sref).abs()
        ratio = torch.where(stol > 0, err / stol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst_s = float(ratio.max())
        t, ch, k = [int(i) for i in torch.nonzero(ratio == ratio.max())[0]]
        where = "tile %d of %d, channel %d, value %d: got %.9g, reference %.9g, tol %.3g" % (t, gst.shape[0], ch, k, gst[t, ch, k], sref[t, ch, k], stol[t, ch, k])
    print("EPILOGUE %s [%s]: result worst err / tol %.3f, statistics worst err / tol %.3f" % (c["id"], c["form"], worst_v, worst_s))
    assert worst_v <= 1.0          # (1)
    assert worst_s <= 1.0, where          # (5)

    _, plain = _plain(L, c, ops)
    assert torch.equal(_bits16(vo), _bits16(plain)), "the result differs from the call without the epilogue at %d elements" % int((_bits16(vo) != _bits16(plain)).sum())   # (2)
    vo2, st2 = one_run()
    assert torch.equal(_bits16(vo), _bits16(vo2)), "the repeated result differs"          # (9)
    if c["stats"]:
        assert torch.equal(st.view(torch.int32), st2.view(torch.int32)), "the repeated statistics differ"          # (9)
    ops.assert_inputs_unchanged()          # (3)


@pytest.mark.parametrize("c", T.TABLE, ids=lambda c: c["id"])
def test_conv_epilogue(env, c):
    run_case(env, c)


# ============================================================================= declined requests: OK, *tile_rows == 0, statistics untouched, the result as plain
def _declined(L, c, ops, out_off=0):
    lib = L.lib()
    nbytes = (lib.sat_conv2d_fwd_stats_bytes if c["kind"] == "fwd" else lib.sat_conv2d_dgrad_stats_bytes)(ctypes.byref(ops.geom))
    whole, vo = _result_frame(ops.M, ops.N, ops.guard, out_off)
    if c["accumulate"]:
        vo.copy_(ops.old)
    swhole, sview = _stats_frame(nbytes)
    tr = ctypes.c_int32(UNSET)
    rc, names = _profiled(L, _call_epilogue(L, c, ops, vo, sview[0], ctypes.byref(tr)))
    L.check(rc, c["id"])
    assert tr.value == 0
    assert bool((swhole.view(torch.int32) == G.CANARY_F32).all()), "a declined request wrote statistics"
    G.assert_frame_untouched(whole, vo, G.CANARY_BF16)
    _, plain = _plain(L, c, ops, out_off)
    assert torch.equal(_bits16(vo), _bits16(plain))
    got = vo.float().cpu().to(F64)
    s = T.inputs(c)
    ref, prod = T.expected(c, s)
    assert float(((got - ref).abs() / T.element_tol(c, s, ref, prod)).max()) <= 1.0
    ops.assert_inputs_unchanged()
    return names


def _loose(kind, g, **kw):
    c = dict(id="declined-%s" % kind, kind=kind, op="fwd" if kind == "fwd" else "dgrad", dt="bf16", g=g, relu_mask=False, accumulate=False, add_mask=False, stats=True)
    c.update(kw)
    return c


@pytest.mark.parametrize("accumulate", [False, True])
def test_bnstats_with_stride_2_is_declined(env, accumulate):
    """parity classes write interleaved rows: no tile statistics; four launches as sat_conv2d_dgrad_bf16 makes them"""
    c = _loose("bnstats", T.S2_GEOM, relu_mask=True, accumulate=accumulate)
    assert _declined(env, c, Operands(env, c, T.inputs(c))) == T.S2_NAMES


def test_bnstats_with_bn_x_8_bytes_off_is_declined(env):
    c = _loose("bnstats", T.OFF_GEOM_DGRAD, relu_mask=True)
    ops = Operands(env, c, T.inputs(c), bn_off=4)
    assert ops.bn_x.data_ptr() % 16 == 8
    assert _declined(env, c, ops) == [T.GL_DG]


def test_forward_with_y_8_bytes_off_is_declined(env):
    c = _loose("fwd", T.OFF_GEOM_FWD)
    assert _declined(env, c, Operands(env, c, T.inputs(c)), out_off=4) == [T.GL_FWD]


# ============================================================================= refused requests: an error code, no launch, no byte of dx or the statistics changed
def _refused(L, c, ops, call, code=SAT_EINVAL):
    rc, names = _profiled(L, call)
    assert rc != 0 and (code is None or rc == code), "return code %d" % rc
    assert names == [], "a refused request launched %s" % names
    ops.assert_inputs_unchanged()


def _fused_args(L, c, ops, out, stats_buf, tr_ref, **over):
    p = L.ptr
    a = dict(add_src=p(ops.add_src), add_mask=p(ops.add_mask), bn_x=p(ops.bn_x), relu=p(ops.relu_mask), mean=p(ops.mean), invstd=p(ops.invstd), stats=p(stats_buf),
             tr=tr_ref)
    a.update(over)
    return lambda st: L.lib().sat_conv2d_dgrad_bf16_fused(p(ops.src), p(ops.w), p(out), ctypes.byref(ops.geom), a["add_src"], a["add_mask"], a["bn_x"], a["relu"], a["mean"],
                                                          a["invstd"], a["stats"], a["tr"], st)


def _refusal_setup(L, g, add_off=0):
    c = _loose("fused", g, add_mask=True, relu_mask=True)
    ops = Operands(L, c, T.inputs(c), add_off=add_off)
    whole, vo = _result_frame(ops.M, ops.N, ops.guard)
    nbytes = L.lib().sat_conv2d_dgrad_stats_bytes(ctypes.byref(ops.geom))
    swhole, sview = _stats_frame(nbytes)
    tr = ctypes.c_int32(UNSET)

    def untouched():
        assert bool((whole.view(torch.int16) == torch.tensor(G.CANARY_BF16, dtype=torch.int16)).all()), "a refused request wrote dx"
        assert bool((swhole.view(torch.int32) == G.CANARY_F32).all()), "a refused request wrote statistics"
        assert tr.value in (UNSET, 0), "a refused request reports tile statistics (*tile_rows = %d)" % tr.value
    return c, ops, vo, sview[0], tr, untouched


@pytest.mark.parametrize("with_stats", [False, True])
def test_fused_with_stride_2_is_refused(env, with_stats):
    c, ops, vo, stats, tr, untouched = _refusal_setup(env, T.S2_GEOM)
    over = {} if with_stats else dict(bn_x=None, relu=None, mean=None, invstd=None, stats=None, tr=None)
    _refused(env, c, ops, _fused_args(env, c, ops, vo, stats, ctypes.byref(tr), **over))
    untouched()


@pytest.mark.parametrize("with_stats", [False, True])
def test_fused_with_null_add_src_is_refused(env, with_stats):
    c, ops, vo, stats, tr, untouched = _refusal_setup(env, T.OFF_GEOM_DGRAD)
    over = {} if with_stats else dict(bn_x=None, relu=None, mean=None, invstd=None, stats=None, tr=None)
    _refused(env, c, ops, _fused_args(env, c, ops, vo, stats, ctypes.byref(tr), add_src=None, **over))
    untouched()


@pytest.mark.parametrize("with_stats", [False, True])
def test_fused_with_add_src_8_bytes_off_is_refused(env, with_stats):
    c, ops, vo, stats, tr, untouched = _refusal_setup(env, T.OFF_GEOM_DGRAD, add_off=4)
    assert ops.add_src.data_ptr() % 16 == 8
    over = {} if with_stats else dict(bn_x=None, relu=None, mean=None, invstd=None, stats=None, tr=None)
    _refused(env, c, ops, _fused_args(env, c, ops, vo, stats, ctypes.byref(tr), **over), code=None)          # an error code, whichever
    untouched()


@pytest.mark.parametrize("missing", ["mean", "invstd", "stats", "tr"])
def test_fused_with_bn_x_but_a_null_statistics_pointer_is_refused(env, missing):
    c, ops, vo, stats, tr, untouched = _refusal_setup(env, T.OFF_GEOM_DGRAD)
    _refused(env, c, ops, _fused_args(env, c, ops, vo, stats, ctypes.byref(tr), **{missing: None}))
    untouched()


@pytest.mark.parametrize("missing", ["stats", "tr"])
def test_forward_stats_with_a_null_statistics_pointer_is_refused(env, missing):
    L = env
    c = _loose("fwd", T.OFF_GEOM_FWD)
    ops = Operands(L, c, T.inputs(c))
    whole, vo = _result_frame(ops.M, ops.N, ops.guard)
    swhole, sview = _stats_frame(L.lib().sat_conv2d_fwd_stats_bytes(ctypes.byref(ops.geom)))
    tr = ctypes.c_int32(UNSET)
    a = dict(stats=L.ptr(sview[0]), tr=ctypes.byref(tr))
    a[missing] = None
    _refused(L, c, ops, lambda st: L.lib().sat_conv2d_fwd_bf16_stats(L.ptr(ops.src), L.ptr(ops.w), L.ptr(vo), ctypes.byref(ops.geom), a["stats"], a["tr"], st))
    assert bool((whole.view(torch.int16) == torch.tensor(G.CANARY_BF16, dtype=torch.int16)).all()) and bool((swhole.view(torch.int32) == G.CANARY_F32).all())
    assert tr.value in (UNSET, 0)


@pytest.mark.parametrize("missing", ["bn_x", "mean", "invstd", "stats", "tr"])
def test_bnstats_with_a_null_statistics_pointer_is_refused(env, missing):
    L = env
    c = _loose("bnstats", T.OFF_GEOM_DGRAD, relu_mask=True)
    ops = Operands(L, c, T.inputs(c))
    whole, vo = _result_frame(ops.M, ops.N, ops.guard)
    swhole, sview = _stats_frame(L.lib().sat_conv2d_dgrad_stats_bytes(ctypes.byref(ops.geom)))
    tr = ctypes.c_int32(UNSET)
    p = L.ptr
    a = dict(bn_x=p(ops.bn_x), mean=p(ops.mean), invstd=p(ops.invstd), stats=p(sview[0]), tr=ctypes.byref(tr))
    a[missing] = None
    _refused(L, c, ops, lambda st: L.lib().sat_conv2d_dgrad_bf16_bnstats(p(ops.src), p(ops.w), p(vo), ctypes.byref(ops.geom), 0, a["bn_x"], p(ops.relu_mask), a["mean"],
                                                                        a["invstd"], a["stats"], a["tr"], st))
    assert bool((whole.view(torch.int16) == torch.tensor(G.CANARY_BF16, dtype=torch.int16)).all()) and bool((swhole.view(torch.int32) == G.CANARY_F32).all())
    assert tr.value in (UNSET, 0)


# ============================================================================= the Python wrappers on the three declined shapes
def test_encoder_wrappers_return_no_tiles_for_the_declined_shapes(env, monkeypatch):
    from sat_amd import encoder as E

    def nchw_filter(s, g):          # (K, C, R, S) in KRSC memory
        return s["w"].to(BF).cuda().reshape(g["K"], g["R"], g["S"], g["C"]).permute(0, 3, 1, 2)

    # stride 2
    g = T.S2_GEOM
    c = _loose("bnstats", g, relu_mask=True)
    s = T.inputs(c)
    P, Q = R.out_hw(g)
    shape = (g["N"], g["H"], g["W"], g["C"])
    dy = s["src"].to(BF).cuda().reshape(g["N"], P, Q, g["K"])
    bn = (s["bn_x"].to(BF).cuda().reshape(shape), (s["mean"].cuda(), s["invstd"].cuda(), B.pack_mask(s["relu_bits"]).cuda()))
    dx, tiles = E.conv_dgrad(dy, nchw_filter(s, g), shape, 2, g["pad"], bn=bn)
    assert tiles is None
    plain = E.conv_dgrad(dy, nchw_filter(s, g), shape, 2, g["pad"])
    assert torch.equal(_bits16(dx), _bits16(plain))

    # bn_x 8 bytes off a 16-byte boundary (contiguous all the same)
    g = T.OFF_GEOM_DGRAD
    c = _loose("bnstats", g, relu_mask=True)
    s = T.inputs(c)
    P, Q = R.out_hw(g)
    shape = (g["N"], g["H"], g["W"], g["C"])
    dy = s["src"].to(BF).cuda().reshape(g["N"], P, Q, g["K"])
    room = torch.empty(s["bn_x"].numel() + 8, dtype=BF, device="cuda")
    bx = room[4:4 + s["bn_x"].numel()].view(shape)
    bx.copy_(s["bn_x"].reshape(shape))
    assert bx.data_ptr() % 16 == 8 and bx.is_contiguous()
    stats = (s["mean"].cuda(), s["invstd"].cuda(), B.pack_mask(s["relu_bits"]).cuda())
    dx, tiles = E.conv_dgrad(dy, nchw_filter(s, g), shape, 1, g["pad"], bn=(bx, stats))
    assert tiles is None
    _, tiles_aligned = E.conv_dgrad(dy, nchw_filter(s, g), shape, 1, g["pad"], bn=(bx.clone(), stats))
    assert tiles_aligned is not None and tiles_aligned[1] == 64          # the same call on an aligned bn_x does produce them

    # forward with y 8 bytes off: the wrapper allocates y itself, so hand it such an allocation for that one shape
    g = T.OFF_GEOM_FWD
    c = _loose("fwd", g)
    s = T.inputs(c)
    P, Q = R.out_hw(g)
    x = s["src"].to(BF).cuda().reshape(g["N"], g["H"], g["W"], g["C"])
    y, tiles = E.conv_fwd_stats(x, nchw_filter(s, g), 1, g["pad"])
    assert tiles is not None and tiles[1] == 64 and y.data_ptr() % 16 == 0
    real_empty = torch.empty

    def empty_off(*size, **kw):
        if tuple(size) == (g["N"], P, Q, g["K"]) and kw.get("dtype") == BF:
            return real_empty(y.numel() + 8, **kw)[4:4 + y.numel()].view(*size)
        return real_empty(*size, **kw)

    monkeypatch.setattr(torch, "empty", empty_off)
    y_off, tiles = E.conv_fwd_stats(x, nchw_filter(s, g), 1, g["pad"])
    monkeypatch.undo()
    assert y_off.data_ptr() % 16 == 8 and tiles is None
    assert torch.equal(_bits16(y_off), _bits16(y))
