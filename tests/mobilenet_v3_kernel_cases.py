"""The shapes that pin every launch form of the kernels mobilenet_v3_small added (csrc/depthwise5x5.hip, csrc/mobilenet_v3.hip), with the
plan each was written for.

The library has no plan query for these kernels (none could be added with this table), so dw5_plan and
hs_plan below restate dw5_chunk / dw5_cvb and hs_grid.  test_mobilenet_v3_plan.py (no GPU) asserts that the restatements give exactly
these plans and holds them against what the library does answer: sat_dwconv5x5_wgrad_scratch_bytes equals the restated partial count
times 25 C floats for every shape (a retuned dw5_chunk fails it), and the restated hard-swish partials fit sat_bn_scratch_bytes.
test_gpu_mobilenet_v3_forms.py runs the shapes.  Where a form is no longer reached the shape is changed until it is again: a mismatch
fails, nothing is skipped.  Each shape is the smallest that reaches its form.

Plans:
  depthwise 5x5 filter gradient   (chunk = output pixels per partial, partials, cvb = channel vectors per block, pixel lanes = 256 // cvb);
                                  the forward and the data gradient have one form: a thread per output pixel and four channels.
  BN + hard-swish backward        (CV = vector columns per block, row lanes = 256 // CV, column blocks, rows per part, parts), per storage type
                                  (a vector is 4 channels in fp32, 8 in bf16).
  squeeze-and-excitation          no host plan: the pass structure of image_colsum is a function of C alone (se_passes below).
"""

F32, BF16 = "fp32", "bf16"
VEC = {F32: 4, BF16: 8}          # channels per 16-byte vector (BN + hard-swish, SE); the 5x5 kernels take 4 channels per thread in both types


# ------------------------------------------------------------------ depthwise 5x5
def dw5(shape, run, plan, why):
    """shape (N, H, W, C, stride); plan: the filter gradient's, the same in both storage types"""
    return dict(shape=shape, run=run, plan=plan, why=why)


DW5_CASES = [
    dw5((1, 1, 1, 4, 1), (F32, BF16), (64, 1, 1, 256), "the smallest legal call: only the centre tap lies inside the map; one pixel for 256 pixel lanes"),
    dw5((1, 2, 3, 12, 1), (F32, BF16), (64, 1, 3, 85), "H < 3 and W < 5: every pixel misses taps on both sides; cvb = 3: 255 live threads; bf16 with "
        "C % 8 != 0 (8-byte loads off 16-byte boundaries)"),
    dw5((2, 7, 5, 24, 2), (F32, BF16), (64, 1, 6, 42), "cvb = 6: 252 live threads; stride 2 with odd H and W (the last output row / column reads the last "
        "input row / column as its centre)"),
    dw5((2, 9, 11, 132, 2), (F32, BF16), (64, 1, 11, 23), "C / 4 = 33: cvb = 11, 253 live threads, three channel groups; odd map sizes at stride 2"),
    dw5((2, 10, 12, 8, 2), (F32, BF16), (64, 1, 2, 128), "even map sizes at stride 2: the last output row / column lies one short of the map's edge, "
        "the data gradient's last row / column takes the odd taps only"),
    dw5((1, 6, 6, 148, 1), (F32, BF16), (64, 1, 1, 256), "C / 4 = 37 (prime): cvb = 1, 256 pixel lanes for 36 pixels, 37 channel groups"),
    dw5((1, 5, 5, 160, 1), (F32, BF16), (64, 1, 20, 12), "C / 4 = 40: cvb = 20 and two channel groups (grid.y = 2), 240 live threads"),
    dw5((3, 40, 37, 8, 1), (F32, BF16), (64, 70, 2, 128), "4440 pixels: 70 partials, more than the 64 lanes of the finish kernel (lanes 0 - 5 add two); "
        "the last chunk is ragged (24 pixels for 128 lanes); more than one block of the forward / data gradient"),
    dw5((1, 260, 257, 4, 1), (F32, BF16), (128, 523, 1, 256), "66820 pixels: the only shape above the 64-pixel floor of the chunk (128); the finish kernel's "
        "lanes take nine partials each; ragged last chunk (4 pixels)"),
]


def dw5_out(n, stride):
    return (n + 4 - 5) // stride + 1


def dw5_plan(shape):
    """(chunk, partials, cvb, pixel lanes) as dw5_chunk / dw5_cvb of csrc/depthwise5x5.hip decide them.  The library has no query for this
    plan; what it does answer, sat_dwconv5x5_wgrad_scratch_bytes = partials * 25 * C * 4, is held against this count by the plan test."""
    N, H, W, C, stride = shape
    npix = N * dw5_out(H, stride) * dw5_out(W, stride)
    chunk = min(max((-(-npix // 1024) + 63) // 64 * 64, 64), 2048)
    cv = C // 4
    cvb = min(cv, 32)
    while cv % cvb:
        cvb -= 1
    return chunk, -(-npix // chunk), cvb, 256 // cvb


# ------------------------------------------------------------------ BatchNorm + hard-swish
def hs(name, rows, C, why, tile_rows=0, **plans):
    """plans: one per storage type the case runs in"""
    return dict(name=name, rows=rows, C=C, why=why, tile_rows=tile_rows, run=tuple(t for t in (F32, BF16) if t in plans), plans=plans)


HS_CASES = [
    hs("5x4", 5, 4, "CV = 1, 256 row lanes for 5 rows; C = 4: the one width where the 64 bytes of ticket words are as large as a part's partials, so "
       "hs_grid's cap counts them as room for one more part", fp32=(1, 256, 1, 2048, 1)),
    hs("300x40", 300, 40, "C / 4 = 10: CV = 8, two column blocks, six idle columns in the second; two parts, the second ragged (44 rows for 32 row "
       "lanes); 3000 vectors: the apply kernels' last block is partly idle", fp32=(8, 32, 2, 256, 2)),
    hs("50x24", 50, 24, "bf16 with C / 8 = 3: CV = 2, two column blocks with one live column in the second; fewer rows than the 128 row lanes",
       bf16=(2, 128, 2, 1024, 1)),
    hs("20x1028", 20, 1028, "C / 4 = 257: CV = 256, a single row lane, a second column block with one live column, three parts (8, 8, 4 rows)",
       fp32=(256, 1, 2, 8, 3)),
    hs("1300x16", 1300, 16, "several parts with a ragged last one in both types (fp32: 512, 512, 276 rows; bf16: 1024, 276); 5200 / 2600 vectors for the "
       "apply kernels", fp32=(4, 64, 1, 512, 3), bf16=(2, 128, 1, 1024, 2)),
    hs("1x8", 1, 8, "one row in bf16: one live thread in the statistics block, variance 0, one vector for the apply kernels", bf16=(1, 256, 1, 2048, 1)),
    hs("9x2056", 9, 2056, "the single row lane in bf16 (C / 8 = 257): both LDS passes (h = 0, 4) with RL = 1; two parts (8, 1 rows)",
       bf16=(256, 1, 2, 8, 2)),
    hs("200x32-tiles", 200, 32, "bf16 through tile_stats: the statistics of sat_bn_hswish_train_fwd_t come from four row tiles of 64 (the last one "
       "8 rows), not from a pass over x", tile_rows=64, bf16=(4, 64, 1, 512, 1)),
]


def hs_plan(lib, dtype, rows, C):
    """(CV, row lanes, column blocks, rows per part, parts) as hs_grid of csrc/mobilenet_v3.hip decides them, its cap taken from the
    library's sat_bn_scratch_bytes.  The library has no query for this plan."""
    cvt = C // VEC[dtype]
    CV = min(cvt, 256)
    while 256 % CV:
        CV -= 1
    RL, colblocks = 256 // CV, -(-cvt // CV)
    cap = (lib.sat_bn_scratch_bytes(rows, C) - 64) // (C * 2 * 8)
    want = max(min(max(512 // colblocks, 1), cap), 1)
    rows_per = max(-(-rows // want), RL * 8)
    return CV, RL, colblocks, rows_per, -(-rows // rows_per)


# ------------------------------------------------------------------ squeeze-and-excitation
def se_passes(C):
    """image_colsum walks the channels 64 at a time: (passes, channels of the last pass CB, its pixel lanes 256 // CB)"""
    passes = -(-C // 64)
    cb = C - 64 * (passes - 1)
    return passes, cb, 256 // cb


def se(shape, run, passes, why):
    """shape (N, HW, C, S); passes: what se_passes(C) must give"""
    return dict(shape=shape, run=run, passes=passes, why=why)


SE_CASES = [
    se((1, 1, 4, 1), (F32,), (1, 4, 64), "the smallest legal call: one pixel for 64 pixel lanes, one image, S = 1, C + S + 2 S C = 13 parameter "
       "gradients in one block"),
    se((3, 49, 24, 8), (F32, BF16), (1, 24, 10), "CB = 24: 10 lanes, 240 live threads; 2 S C + S + C = 416: all four segments of se_wgrad_kernel change "
       "inside a block (192, 200 in the first, 392, 416 in the second)"),
    se((2, 15, 72, 24), (F32, BF16), (2, 8, 32), "two passes, the second with CB = 8 and 32 lanes, more than the 15 pixels"),
    se((2, 7, 576, 144), (F32, BF16), (9, 64, 4), "nine full passes; the channel loops of the FC layers take three trips (576 > 2 x 256)"),
    se((1, 3, 1024, 256), (F32, BF16), (16, 64, 4), "the limits C = 1024 and S = 256: the LDS vectors are full, fewer pixels than lanes"),
    se((2, 3136, 16, 8), (F32,), (1, 16, 16), "a long pixel loop: 196 pixels per lane, many blocks of the scale kernels"),
    se((5, 196, 16, 8), (F32, BF16), (1, 16, 16), "five images: the image-ordered parameter-gradient sums; the first SE of the network in bf16"),
    se((2, 9, 40, 16), (F32, BF16), (1, 40, 6), "CB = 40: 6 lanes, 240 live threads, in both types"),
    se((2, 10, 32, 3), (F32, BF16), (1, 32, 8), "S = 3: a squeeze width below the 8 torchvision ever builds, odd: the rows of w2 lie off 16-byte boundaries"),
]


def se_scratch_floats(N, C, S):
    """what sat_se_bwd_scratch_bytes documents: dz2 [N][C], dpool [N][C], dz1 [N][S]"""
    return N * (2 * C + S)


# ------------------------------------------------------------------ the inputs of a case (float64, exactly representable in the storage type)
U = 2.0 ** -24
HS_EPS, HS_MOMENTUM = 1e-3, 0.01          # torchvision's BatchNorm2d(eps = 0.001, momentum = 0.01)
#: the pre-activations of the "exact v" data set: multiples of 1 / 2; 2 / 16 exactly at 3, 2 / 16 exactly at -3, 7 / 16 strictly inside
#: (-3, 3), 2 / 16 below -3, 3 / 16 above 3
EXACT_V = (3.0, -3.0, 0.0, 1.5, -2.5, 4.0, -4.5, 3.0, -3.0, 2.5, -0.5, 5.0, -3.5, 3.5, -1.0, 0.5)


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


def _draw(seed, bf):
    import torch
    from oracle import prng
    import mobilenet_v3_kernel_ref as R
    uni = lambda shp, k: torch.from_numpy(prng.uniform(shp, seed + k)).to(torch.float64)
    ints = lambda shp, k, lo, hi: torch.from_numpy(prng.integers(shp, seed + k, 0, hi - lo) + lo).to(torch.float64)          # (prng.integers takes lo >= 0)
    return uni, ints, (lambda t: R.to_storage(t, bf)), (lambda t: t.float().to(torch.float64))


def dw5_data(shape, dataset, bf):
    """x, dy in the storage type, w fp32: "int" draws all three from {-2 .. 2}, "real" from oracle.prng.uniform"""
    N, H, W, C, stride = shape
    P, Q = dw5_out(H, stride), dw5_out(W, stride)
    uni, ints, rnd, f32 = _draw(1000 * H + 10 * W + C + stride, bf)
    if dataset == "int":
        return dict(x=ints((N, H, W, C), 1, -2, 3), dy=ints((N, P, Q, C), 2, -2, 3), w=ints((C, 25), 3, -2, 3))
    return dict(x=rnd(uni((N, H, W, C), 1)), dy=rnd(uni((N, P, Q, C), 2)), w=uni((C, 25), 3))


def hs_data(c, dataset, bf):
    """"real": per-channel mean and spread, gamma of either sign, beta up to 2: v reaches all three regions of the hard-swish.
    "exact": mean and beta integers, invstd and |gamma| powers of two, x = mean + (v - beta) / (invstd gamma) with v from EXACT_V: every
    operation of v = (x - mean) invstd gamma + beta is exact in fp32 (and x, a multiple of 1 / 4 below 16, is exact in bf16), so the branch
    decision is the same in both precisions.  Element e = r C + c takes EXACT_V[(e + e // 16) % 16]: the smallest case meets every value, and from row to row a vector lane meets both kinks.
    run_var of the exact set = 1 / invstd^2, to be used with eps = 0."""
    import torch
    rows, C = c["rows"], c["C"]
    uni, ints, rnd, f32 = _draw(_seed(c["name"]), bf)
    d = dict(rows=rows, C=C, dy=rnd(uni((rows, C), 3)))
    if dataset == "exact":
        d["mean"], d["beta"] = ints((C,), 1, -2, 3), ints((C,), 2, -1, 2)
        d["invstd"] = 2.0 ** ints((C,), 4, -1, 1)          # 1 / 2, 1
        scale = 2.0 ** ints((C,), 5, 0, 2)                 # invstd |gamma| = 1, 2
        d["gamma"] = torch.where(ints((C,), 6, 0, 2) > 0, scale, -scale) / d["invstd"]
        e = torch.arange(rows * C).reshape(rows, C)
        idx = (e + e // 16) % 16
        d["v"] = torch.tensor(EXACT_V, dtype=torch.float64)[idx]
        d["x"] = d["mean"] + (d["v"] - d["beta"]) / (d["invstd"] * d["gamma"])
        assert torch.equal(rnd(d["x"]), d["x"])
        d["run_mean"], d["run_var"] = d["mean"].float(), (1.0 / d["invstd"] ** 2).float()
        return d
    chan_mean, chan_std = 2.0 * uni((C,), 1), 0.5 + uni((C,), 4).abs()
    d["x"] = rnd(chan_mean + chan_std * uni((rows, C), 2))
    g = 0.5 + 1.5 * uni((C,), 6).abs()
    d["gamma"], d["beta"] = f32(torch.where(uni((C,), 7) > -0.3, g, -g)), f32(2.0 * uni((C,), 8))
    d["run_mean"], d["run_var"] = uni((C,), 15).float(), (0.5 + uni((C,), 16).abs()).float()
    return d


def hs_kink_delta(t, beta):
    """the fp32 error bound of v = (x - mean) invstd gamma + beta: four roundings (the subtraction, two products, the sum)"""
    return 4 * U * (t.abs() + beta.abs())


def hs_near_kink(v, t, beta):
    """elements whose float64 v lies within the fp32 error of v of a kink: either branch is a correct fp32 result"""
    delta = hs_kink_delta(t, beta)
    return ((v - 3.0).abs() <= delta) | ((v + 3.0).abs() <= delta)


def se_data(c, bf):
    """x with a per-channel offset (pooled means of O(1)), FC weights scaled by fan-in, b2 up to 4: z2 reaches all three regions of the hard-sigmoid"""
    N, HW, C, S = c["shape"]
    uni, ints, rnd, f32 = _draw(1000 * HW + 10 * C + S, bf)
    return dict(x=rnd(uni((C,), 1) + uni((N, HW, C), 2)), dy=rnd(uni((N, HW, C), 3)),
                w1=f32(2.0 * uni((S, C), 4) / C ** 0.5), b1=f32(0.2 * uni((S,), 5)), w2=f32(3.0 * uni((C, S), 6) / S ** 0.5), b2=f32(4.0 * uni((C,), 7)))


def se_saved(d, ref):
    """the saved vectors the backward call is handed: the forward reference's, as floats, with z2 exactly 3 in channel 0 and exactly -3 in
    the last channel (s there 1 and 0), and h exactly 0 in squeeze channel 0 when S > 1 (next to the zeros the ReLU leaves)"""
    f32 = lambda t: t.float().to(t.dtype)
    pool, h, z2, s = f32(ref["pool"]).clone(), f32(ref["h"]).clone(), f32(ref["z2"]).clone(), f32(ref["s"]).clone()
    z2[:, 0], s[:, 0] = 3.0, 1.0
    z2[:, -1], s[:, -1] = -3.0, 0.0
    if h.shape[1] > 1:
        h[:, 0] = 0.0
    return dict(pool=pool, h=h, z2=z2, s=s)
