"""The case table of the convolution gather forms ("Convolution gather forms": G1 - G18), shared by test_conv_cases.py (CPU: the
table itself) and test_gpu_conv_forms.py (GPU: every case against conv_ref inside NaN frames).

A case names the geometry (the fields of sat_conv_geom), the storage type ("f32": sat_conv2d_*, "bf16": sat_conv2d_*_bf16), the
operation ("fwd", "dgrad", "wgrad"), accumulate (dgrad), bias (fwd) and the profiler scope names the shipped dispatch must produce, one
per launch, sorted.  The names are derived by hand from conv_*_any (csrc/encoder.hip), launch_gemm / pick_tile (csrc/gemm.hip),
launch_gemm_bf16_tile (csrc/gemm_bf16.hip) and launch_gemm_glds (csrc/gemm_glds.hip); the comment in front of each group says which rule
sends it there.  When a dispatch rule changes, the GPU test fails and the group is to be re-derived, not skipped.

The rules, in the order they apply (M x N x Kr is the implicit GEMM: forward N*P*Q x K x R*S*C, data gradient N*H*W x C x R*S*K, filter
gradient K x R*S*C x N*P*Q):
  f32   always the exact fp32 kernel; 128x128 tiles when cdiv(M,128) * cdiv(N,128) >= 384 and M, N >= 128, else 64x64.
  bf16  the 128-wide request when that product is >= 192 (M, N >= 128), unless it is < 512 with Kr <= 256 and no slab; also with a slab,
        M, N >= 128 and Kr >= 4096.  Then the direct-to-LDS kernel ("glds") unless it declines: stride_w set, Kr % 64, channels of the
        gathered operand % 64 (forward C, data gradient K), R*S > 32, a data gradient with stride != 1 outside a parity class.  Its tile:
        64x64 -> 128x64 when N <= 64 and M >= 8192 (never for a filter gradient); 128x128 -> 128x64 for a forward / data gradient without
        split-K when Kr <= 1152 or the 128-tile product is < 512.  What glds declines runs on the register-staged kernel ("bf16 ... _b")
        at the requested width.
  bf16 data gradient with stride 2: one launch per (h % 2, w % 2) class that has pixels; with accumulate the classes without taps
        (Kr == 0) are skipped.  1x1 / stride 1 / pad 0: a plain GEMM ("nn" data gradient), not a gather.
  bf16 filter gradient 3x3 / stride 1 / pad 1 with C, K % 64 == 0, W in {8, 16, 32, 64}, H % (64 / W) == 0: wgrad3x3 ("gemm_wgrad3x3").

COST CAP.  2 * M * N * Kr <= 3e10 and the largest tensor of a case (in its storage type) <= 64 MiB.  The costliest case is
fwd-glds128x128 (2 * 8100 * 1024 * 1728 = 2.87e10); its float64 reference (conv_ref.forward) was measured at 0.42 s (first call; 0.30 s repeated) on
16 CPU threads (REF_SECONDS_LARGEST; the limit is 5 s).
"""
import conv_ref as R

COST_CAP = 3e10
BYTES_CAP = 64 << 20
REF_SECONDS_LARGEST = 0.42          # measured, see the header

FORMS = {
    "G1": "fp32 kernel, forward gather (a_row_setup / a_row_fetch), 64x64",
    "G2": "fp32 kernel, forward gather, 128x128",
    "G3": "fp32 kernel, data-gradient gather (stride predicate) with the k-major filter read (b_k_fetch)",
    "G4": "fp32 kernel, filter-gradient pixel gather (b_k_fetch)",
    "G5": "register-staged bf16 kernel, forward (row_setup / k_decode / row_fetch)",
    "G6": "register-staged bf16 kernel, data gradient over the whole map (stride 1 and 3)",
    "G7": "register-staged bf16 kernel, data gradient by parity class (stride 2)",
    "G8": "register-staged bf16 kernel, filter gradient (k_decode / bk_fetch)",
    "G9": "direct-to-LDS kernel, forward 64x64 (a_off0 / tap_mask / set_tap / advance_tile)",
    "G10": "direct-to-LDS kernel, forward 128x64",
    "G11": "direct-to-LDS kernel, forward 128x128",
    "G12": "direct-to-LDS kernel, data gradient stride 1, 64x64",
    "G13": "direct-to-LDS kernel, data gradient stride 1, 128x64",
    "G14": "direct-to-LDS kernel, data gradient by parity class (stride 2)",
    "G15": "direct-to-LDS kernel, filter gradient 64x64 without split-K (fill_tab)",
    "G16": "direct-to-LDS kernel, filter gradient 128x128 with split-K",
    "G17": "hand-off of an eligible 3x3 filter gradient to wgrad3x3",
    "G18": "hand-off of a 1x1 / stride 1 / pad 0 data gradient to the plain GEMM",
}

F32_FWD, F32_FWD128 = "gemm_f32_conv_fwd_64x64", "gemm_f32_conv_fwd_128x128"
F32_DG, F32_WG, F32_NN = "gemm_f32_conv_dgrad_64x64", "gemm_f32_conv_wgrad_64x64", "gemm_f32_nn_64x64"
REG_FWD, REG_DG, REG_WG, REG_NN = "gemm_bf16_conv_fwd_64x64_b", "gemm_bf16_conv_dgrad_64x64_b", "gemm_bf16_conv_wgrad_64x64_b", "gemm_bf16_nn_64x64_b"
GL_FWD, GL_FWD_TALL, GL_FWD128 = "gemm_glds_conv_fwd_64x64", "gemm_glds_conv_fwd_128x64", "gemm_glds_conv_fwd_128x128"
GL_DG, GL_DG_TALL = "gemm_glds_conv_dgrad_64x64", "gemm_glds_conv_dgrad_128x64"
GL_WG, GL_WG128, GL_NN_TALL = "gemm_glds_conv_wgrad_64x64", "gemm_glds_conv_wgrad_128x128", "gemm_glds_nn_128x64"
W3 = "gemm_wgrad3x3"

TABLE = []


def case(cid, form, op, dt, g, names, **kw):
    c = dict(id=cid, form=form, op=op, dt=dt, g=g, names=sorted(names if isinstance(names, (list, tuple)) else [names]), accumulate=False, bias=False,
             poison=False)
    c.update(kw)
    TABLE.append(c)
    return c


def gemm_dims(c):
    """(M, N, Kr) of the implicit GEMM"""
    g = c["g"]
    P, Q = R.out_hw(g)
    if c["op"] == "fwd":
        return g["N"] * P * Q, g["K"], g["R"] * g["S"] * g["C"]
    if c["op"] == "dgrad":
        return g["N"] * g["H"] * g["W"], g["C"], g["R"] * g["S"] * g["K"]
    return g["K"], g["R"] * g["S"] * g["C"], g["N"] * P * Q


def largest_tensor_bytes(c):
    g = c["g"]
    P, Q = R.out_hw(g)
    item = 4 if c["dt"] == "f32" else 2
    x, y, w = g["N"] * g["H"] * g["W"] * g["C"] * item, g["N"] * P * Q * g["K"] * item, g["K"] * g["R"] * g["S"] * g["C"] * (4 if c["op"] == "wgrad" else item)
    return max(x, y, w)


G = R.geom

# ============================================================================= forward
# The geometries every kernel family gathers: (tag, N, H, W, R, S, stride, pad).  The channel counts choose the family - fp32 storage: the
# fp32 kernel; bf16 with C = 8 / 24 / 40 (C % 64 != 0): glds declines, register-staged; bf16 with C = 64: glds.  All are small
# (cdiv(M,128) * cdiv(N,128) < 192), so every one runs on 64x64 tiles.
FWD_GEOMS = [
    ("3x3", 2, 9, 9, 3, 3, 1, 1),                  # 162 pixels: 2.5 row tiles
    ("onetile", 1, 8, 8, 3, 3, 1, 1),              # exactly one tile of 64 pixels
    ("pad2", 2, 7, 6, 3, 3, 1, 2),                 # pad > R // 2: the output is larger than the map
    ("pad0", 2, 7, 9, 3, 3, 1, 0),
    ("h1", 3, 1, 9, 3, 3, 1, 1),                   # one image row: the taps above and below are always outside
    ("w1", 3, 9, 1, 3, 3, 1, 1),
    ("w2", 3, 5, 2, 3, 3, 1, 1),                   # W = 2 < S
    ("s2odd", 2, 9, 11, 3, 3, 2, 1),
    ("s2even", 2, 10, 12, 3, 3, 2, 1),
    ("s2mixed", 2, 10, 11, 3, 3, 2, 1),
    ("s3", 2, 11, 10, 3, 3, 3, 1),
    ("1x1s2", 2, 9, 10, 1, 1, 2, 0),               # the shortest reduction that is still a gather
    ("1x7", 2, 5, 9, 1, 7, 1, 3),                  # rectangular, one pad: P = H + 6, Q = W
    ("7x1", 2, 9, 5, 7, 1, 1, 3),
    ("5x5", 1, 9, 10, 5, 5, 1, 2),                 # 25 taps: under the 32-bit tap mask of glds
    ("7x7", 1, 9, 9, 7, 7, 1, 3),                  # 49 taps: glds declines (R*S > 32) whatever C is
    ("7x7s2", 1, 13, 12, 7, 7, 2, 3),
]
for i, (tag, n, h, w, r, s, st, pd) in enumerate(FWD_GEOMS):
    bias = i % 2 == 0
    # fp32 storage -> launch_gemm's own kernel (bf16_mfma = 0); M * N tiny -> pick_tile gives 64x64
    case("fwd-f32-" + tag, "G1", "fwd", "f32", G(n, h, w, 4, 12, r, s, st, pd), F32_FWD, bias=bias)
    # C = 8: launch_gemm_glds returns -1 at `g.C % 64` -> register-staged
    case("fwd-reg-" + tag, "G5", "fwd", "bf16", G(n, h, w, 8, 16, r, s, st, pd), REG_FWD, bias=not bias)
    # C = 64: glds takes it unless R*S > 32 (7x7: register-staged although C % 64 == 0)
    case("fwd-glds-" + tag, "G5" if r * s > 32 else "G9", "fwd", "bf16", G(n, h, w, 64, 72 if i % 3 == 0 else 64, r, s, st, pd),
         REG_FWD if r * s > 32 else GL_FWD, bias=bias)
# fp32 128x128: 2209 pixels x 3072 filters = 18 x 24 = 432 >= 384 tiles of 128, both ragged
case("fwd-f32-128x128", "G2", "fwd", "f32", G(1, 47, 47, 4, 3076, 3, 3, 1, 1), F32_FWD128, bias=True)
# register-staged, the other channel counts below 64 (k-tile of 64 spans 2.67 / 1.6 taps) and one above (C = 72: 0.89 taps)
case("fwd-reg-c24", "G5", "fwd", "bf16", G(2, 10, 11, 24, 24, 3, 3, 2, 1), REG_FWD)
case("fwd-reg-c40", "G5", "fwd", "bf16", G(2, 9, 7, 40, 16, 3, 3, 1, 1), REG_FWD, bias=True)
case("fwd-reg-c72", "G5", "fwd", "bf16", G(2, 9, 7, 72, 16, 3, 3, 1, 1), REG_FWD)
# stride_w: the stem's tap-pair view (R = 7, S = 4, C = 8, stride 2 down and 1 across, no padding); glds declines any stride_w
case("fwd-reg-stem-sw1", "G5", "fwd", "bf16", G(2, 21, 14, 8, 64, 7, 4, 2, 0, 1), REG_FWD)
case("fwd-reg-sw1-c64", "G5", "fwd", "bf16", G(2, 9, 8, 64, 64, 3, 3, 2, 1, 1), REG_FWD, bias=True)
# glds 64x64, several k-tiles per tap (advance_tile wraps c0 inside a tap): C = 128 (2), 192 (3); 3 x 2 workgroups, so the rotation
# start (bx * 5 + by * 3 + bz) % T differs between them.  T: 1x1 stride 2 with C = 64 / 128 -> 1 / 2 k-tiles (in FWD_GEOMS: 1), 3x3 -> 9 - 27
case("fwd-glds-c128", "G9", "fwd", "bf16", G(2, 9, 9, 128, 72, 3, 3, 1, 1), GL_FWD)
case("fwd-glds-c192", "G9", "fwd", "bf16", G(2, 7, 9, 192, 72, 3, 3, 1, 1), GL_FWD, bias=True)
case("fwd-glds-1x1s2-c128", "G9", "fwd", "bf16", G(2, 9, 10, 128, 64, 1, 1, 2, 0), GL_FWD)
case("fwd-glds-c128-s2", "G9", "fwd", "bf16", G(2, 10, 11, 128, 64, 3, 3, 2, 1), GL_FWD)
# glds 128x64 from the 64-wide request: N = 64 filters and M = 2 * 63 * 66 = 8316 >= 8192 pixels (64.97 row tiles)
case("fwd-glds-128x64-tall", "G10", "fwd", "bf16", G(2, 63, 66, 64, 64, 3, 3, 1, 1), GL_FWD_TALL, bias=True)
# glds 128x64 from the 128-wide request: 65 x 3 = 195 >= 192 tiles, Kr = 576 > 256 keeps the 128-wide request, Kr <= 1152 narrows it
case("fwd-glds-128x64-narrowed", "G10", "fwd", "bf16", G(2, 64, 65, 64, 384, 3, 3, 1, 1), GL_FWD_TALL)
# glds 128x128: 64 x 8 = 512 tiles (not < 512) and Kr = 9 * 192 = 1728 > 1152; 8100 pixels = 63.3 row tiles
case("fwd-glds128x128", "G11", "fwd", "bf16", G(1, 90, 90, 192, 1024, 3, 3, 1, 1), GL_FWD128)
# NaN in one activation channel, Inf in one filter tap: one case per kernel family
case("fwd-f32-poison", "G1", "fwd", "f32", G(2, 9, 9, 4, 12, 3, 3, 1, 1), F32_FWD, poison=True)
case("fwd-reg-poison", "G5", "fwd", "bf16", G(2, 9, 9, 8, 16, 3, 3, 1, 1), REG_FWD, poison=True)
case("fwd-glds-poison", "G9", "fwd", "bf16", G(2, 9, 9, 64, 64, 3, 3, 1, 1), GL_FWD, poison=True)

# ============================================================================= data gradient
for acc in (False, True):
    a = "-acc" if acc else ""
    # fp32: the generic gather with the stride predicate, stride 1, 2, 3 (fp32 never splits a stride-2 gradient into classes)
    for tag, geo in (("s1", G(2, 9, 9, 8, 12, 3, 3, 1, 1)), ("s2", G(2, 10, 11, 8, 12, 3, 3, 2, 1)), ("s3", G(2, 11, 10, 8, 12, 3, 3, 3, 1)),
                     ("7x7s2", G(1, 13, 12, 4, 8, 7, 7, 2, 3)), ("1x1s2", G(2, 9, 10, 8, 12, 1, 1, 2, 0)), ("pad2", G(2, 7, 6, 8, 12, 3, 3, 1, 2)),
                     ("1x7", G(2, 5, 9, 8, 12, 1, 7, 1, 3))):
        case("dgrad-f32-%s%s" % (tag, a), "G3", "dgrad", "f32", geo, F32_DG, accumulate=acc)
    # 1x1 / stride 1 / pad 0: conv_dgrad_any hands a row-major x k-major GEMM over: fp32; bf16 with K = 8 filters (Kr % 64 != 0:
    # register-staged); bf16 with K = 64 and C = 64 <= 64 columns over 8316 >= 8192 pixels: glds 128x64
    case("dgrad-f32-1x1" + a, "G18", "dgrad", "f32", G(3, 8, 9, 16, 8, 1, 1, 1, 0), F32_NN, accumulate=acc)
    case("dgrad-reg-1x1" + a, "G18", "dgrad", "bf16", G(3, 8, 9, 16, 8, 1, 1, 1, 0), REG_NN, accumulate=acc)
    case("dgrad-glds-1x1-128x64" + a, "G18", "dgrad", "bf16", G(2, 63, 66, 64, 64, 1, 1, 1, 0), GL_NN_TALL, accumulate=acc)
    # bf16 stride 1: K = 16 filters -> glds declines at `g.K % 64`; K = 64 -> glds 64x64; 8316 pixels x C = 64 -> glds 128x64
    case("dgrad-reg-s1" + a, "G6", "dgrad", "bf16", G(2, 9, 9, 8, 16, 3, 3, 1, 1), REG_DG, accumulate=acc)
    case("dgrad-reg-s1-pad2" + a, "G6", "dgrad", "bf16", G(2, 7, 6, 8, 16, 3, 3, 1, 2), REG_DG, accumulate=acc)
    case("dgrad-glds-s1" + a, "G12", "dgrad", "bf16", G(2, 9, 9, 72, 64, 3, 3, 1, 1), GL_DG, accumulate=acc)
    case("dgrad-glds-s1-k128" + a, "G12", "dgrad", "bf16", G(2, 9, 7, 64, 128, 3, 3, 1, 1), GL_DG, accumulate=acc)
    case("dgrad-glds-s1-pad2" + a, "G12", "dgrad", "bf16", G(2, 7, 6, 64, 64, 3, 3, 1, 2), GL_DG, accumulate=acc)
    case("dgrad-glds-s1-5x5" + a, "G12", "dgrad", "bf16", G(1, 9, 10, 64, 64, 5, 5, 1, 2), GL_DG, accumulate=acc)
    case("dgrad-glds-s1-1x7" + a, "G12", "dgrad", "bf16", G(2, 5, 9, 64, 64, 1, 7, 1, 3), GL_DG, accumulate=acc)
    case("dgrad-glds-s1-128x64" + a, "G13", "dgrad", "bf16", G(2, 63, 66, 64, 64, 3, 3, 1, 1), GL_DG_TALL, accumulate=acc)
    # bf16 stride 2: four parity classes, each a small launch on 64x64; K = 16 / 8 filters -> register-staged, K = 64 -> glds (the class
    # flag lifts its stride != 1 refusal).  7x7 has R*S = 49 > 32: register-staged whatever K is.
    for fam, form, k, c, nm in (("reg", "G7", 16, 8, REG_DG), ("glds", "G14", 64, 64, GL_DG)):
        for tag, geo in (("3x3", G(2, 10, 12, c, k, 3, 3, 2, 1)), ("oddh", G(2, 9, 12, c, k, 3, 3, 2, 1)), ("oddw", G(2, 10, 11, c, k, 3, 3, 2, 1)),
                         ("5x5", G(1, 10, 11, c, k, 5, 5, 2, 2)), ("pad0", G(2, 9, 11, c, k, 3, 3, 2, 0))):
            case("dgrad-%s-s2-%s%s" % (fam, tag, a), form, "dgrad", "bf16", geo, [nm] * 4, accumulate=acc)
        # H = 1: the ph = 1 classes have no pixels (Hc = 0) and are not launched
        case("dgrad-%s-s2-h1%s" % (fam, a), form, "dgrad", "bf16", G(3, 1, 12, c, k, 3, 3, 2, 1), [nm] * 2, accumulate=acc)
        # 1x1 / pad 0: only the (0, 0) class has a tap; the other three are launched with Kr = 0 to store zeros - and not at all when accumulating
        case("dgrad-%s-s2-1x1%s" % (fam, a), form, "dgrad", "bf16", G(2, 9, 10, c, k, 1, 1, 2, 0), [nm] * (1 if acc else 4), accumulate=acc)
    case("dgrad-reg-s2-7x7-k8" + a, "G7", "dgrad", "bf16", G(1, 13, 12, 8, 8, 7, 7, 2, 3), [REG_DG] * 4, accumulate=acc)
    case("dgrad-reg-s2-7x7-k64" + a, "G7", "dgrad", "bf16", G(1, 13, 12, 64, 64, 7, 7, 2, 3), [REG_DG] * 4, accumulate=acc)
    # bf16 stride 3: no parity classes, and glds refuses stride != 1 without them although K % 64 == 0
    case("dgrad-reg-s3-k64" + a, "G6", "dgrad", "bf16", G(2, 11, 10, 64, 64, 3, 3, 3, 1), REG_DG, accumulate=acc)
    case("dgrad-reg-s3-k16" + a, "G6", "dgrad", "bf16", G(2, 11, 10, 8, 16, 3, 3, 3, 1), REG_DG, accumulate=acc)
case("dgrad-f32-poison", "G3", "dgrad", "f32", G(2, 9, 9, 8, 12, 3, 3, 1, 1), F32_DG, poison=True)
case("dgrad-reg-s2-poison", "G7", "dgrad", "bf16", G(2, 10, 12, 8, 16, 3, 3, 2, 1), [REG_DG] * 4, poison=True)
case("dgrad-glds-s2-poison", "G14", "dgrad", "bf16", G(2, 10, 12, 64, 64, 3, 3, 2, 1), [GL_DG] * 4, poison=True)

# ============================================================================= filter gradient
# (every case runs with a slab of exactly sat_conv2d_wgrad_slab_bytes and, where that is 0, once more with a generous one; none of the
# "slab offered" rules moves one of these cases to another kernel, except where names_slab says so)
# fp32: always the fp32 kernel (with its own split-K under one scope)
for tag, geo in (("3x3", G(2, 9, 9, 8, 12, 3, 3, 1, 1)), ("s2", G(2, 10, 11, 8, 12, 3, 3, 2, 1)), ("5x5", G(1, 9, 10, 4, 8, 5, 5, 1, 2)),
                 ("long", G(4, 16, 16, 8, 12, 3, 3, 1, 1)), ("pad2", G(2, 7, 6, 8, 12, 3, 3, 1, 2)), ("1x7", G(2, 5, 9, 8, 12, 1, 7, 1, 3))):
    case("wgrad-f32-" + tag, "G4", "wgrad", "f32", geo, F32_WG)
# register-staged: the pixel count N*P*Q % 64 != 0 (glds declines at `k.K % 64`), whatever the channels are; stride_w; 7x7 (R*S > 32)
case("wgrad-reg-3x3", "G8", "wgrad", "bf16", G(2, 9, 9, 8, 16, 3, 3, 1, 1), REG_WG)
case("wgrad-reg-c64", "G8", "wgrad", "bf16", G(2, 9, 9, 64, 64, 3, 3, 1, 1), REG_WG)
case("wgrad-reg-s2", "G8", "wgrad", "bf16", G(2, 10, 11, 24, 24, 3, 3, 2, 1), REG_WG)
case("wgrad-reg-5x5", "G8", "wgrad", "bf16", G(1, 9, 10, 8, 16, 5, 5, 1, 2), REG_WG)
case("wgrad-reg-stem-sw1", "G8", "wgrad", "bf16", G(2, 21, 14, 8, 64, 7, 4, 2, 0, 1), REG_WG)          # 2 * 8 * 11 = 176 pixels
case("wgrad-reg-sw1-64px", "G8", "wgrad", "bf16", G(1, 21, 11, 64, 64, 7, 4, 2, 0, 1), REG_WG)         # 8 * 8 = 64 pixels, C = 64: only stride_w keeps glds off
case("wgrad-reg-7x7-64px", "G8", "wgrad", "bf16", G(1, 8, 8, 8, 16, 7, 7, 1, 3), REG_WG)               # 64 pixels, R*S = 49
case("wgrad-reg-long", "G8", "wgrad", "bf16", G(3, 21, 21, 8, 16, 3, 3, 1, 1), REG_WG)                 # 1323 pixels: split-K when a slab is offered
# wgrad3x3's nearest neighbours that it refuses, all with N*P*Q % 64 == 0 and C = K = 64 -> glds 64x64, no split (N*P*Q < 1024):
# W = 12; H % (64 / W) != 0 (W = 16, H = 6, two images); pad 0 (10 x 10 -> 8 x 8)
case("wgrad-glds-w12", "G15", "wgrad", "bf16", G(1, 16, 12, 64, 64, 3, 3, 1, 1), GL_WG)
case("wgrad-glds-h6w16", "G15", "wgrad", "bf16", G(2, 6, 16, 64, 64, 3, 3, 1, 1), GL_WG)
case("wgrad-glds-pad0", "G15", "wgrad", "bf16", G(1, 10, 10, 64, 64, 3, 3, 1, 0), GL_WG)
# glds 64x64: channels need not be multiples of 64 (the pixel table carries the gather); one k-tile, several, stride 2, 5x5, rectangular
case("wgrad-glds-c8", "G15", "wgrad", "bf16", G(1, 16, 12, 8, 16, 3, 3, 1, 1), GL_WG)
case("wgrad-glds-s2", "G15", "wgrad", "bf16", G(2, 16, 15, 64, 72, 3, 3, 2, 1), GL_WG)                 # 2 * 8 * 8 = 128 pixels
case("wgrad-glds-1x1s2", "G15", "wgrad", "bf16", G(1, 16, 15, 64, 64, 1, 1, 2, 0), GL_WG)              # one k-tile
case("wgrad-glds-5x5", "G15", "wgrad", "bf16", G(2, 8, 12, 64, 64, 5, 5, 1, 2), GL_WG)                 # bit 24 of the tap mask
case("wgrad-glds-1x7", "G15", "wgrad", "bf16", G(2, 2, 8, 64, 64, 1, 7, 1, 3), GL_WG)                  # P = 8: 2 * 8 * 8 = 128 pixels
case("wgrad-glds-pad2", "G15", "wgrad", "bf16", G(1, 6, 6, 64, 64, 3, 3, 1, 2), GL_WG)                 # 8 x 8 outputs
# glds 128x128 with split-K: a slab, M = K = 128 filters, N = C = 128, N*P*Q = 4096 >= 64 * 64.  1 tile, want 512, K / 512 = 8 splits of 8
# k-tiles.  Without the generous slab it is the same: sat_conv2d_wgrad_slab_bytes (the fp32 kernel's 32 splits) is not 0.
case("wgrad-glds-128x128-splitk", "G16", "wgrad", "bf16", G(4, 64, 64, 128, 128, 1, 1, 2, 0), GL_WG128)
# ... and 4160 pixels = 65 k-tiles over 8 splits: 9 each, the last split has 2
case("wgrad-glds-128x128-short-last", "G16", "wgrad", "bf16", G(5, 64, 52, 128, 128, 1, 1, 2, 0), GL_WG128)
# 64x64 with split-K: 2 x 9 tiles, N*P*Q = 1024 = 16 k-tiles: want 42, K / 512 = 2 splits
case("wgrad-glds-64x64-splitk", "G15", "wgrad", "bf16", G(4, 16, 16, 64, 72, 3, 3, 1, 1), GL_WG)       # (K = 72: not wgrad3x3's)
# the eligible 3x3 itself and with another width
case("wgrad-w3-8x8", "G17", "wgrad", "bf16", G(1, 8, 8, 64, 64, 3, 3, 1, 1), W3)
case("wgrad-w3-16x16", "G17", "wgrad", "bf16", G(2, 16, 16, 64, 128, 3, 3, 1, 1), W3)
case("wgrad-f32-poison", "G4", "wgrad", "f32", G(2, 9, 9, 8, 12, 3, 3, 1, 1), F32_WG, poison=True)
case("wgrad-reg-poison", "G8", "wgrad", "bf16", G(2, 9, 9, 8, 16, 3, 3, 1, 1), REG_WG, poison=True)
case("wgrad-glds-poison", "G15", "wgrad", "bf16", G(1, 16, 12, 64, 64, 3, 3, 1, 1), GL_WG, poison=True)

BY_ID = {c["id"]: c for c in TABLE}
