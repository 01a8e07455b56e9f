"""GPU: every write-out of the GEMM family ("GEMM store paths": S1 - S6) against a float64 reference, inside guard bands.

Each case goes through sat_amd.decoder.gemm (sat_gemm_f32 / sat_gemm_ex) with nothing forced: the shipped dispatch rules pick the
kernel, and the case then asserts
  (a) the values against gemm_ref.reference (C = f(C_old + A.B), inputs rounded to bf16 first for the bf16 MFMA kernels),
  (b) that every byte of the C allocation outside C[0:M, 0:N] - row padding, guard rows, the elements in front of a shifted window,
      rows a scatter does not reach - still holds the canary bit pattern,
  (c) that the result is NaN exactly where the reference is (nowhere, unless the case puts one into an operand): A, B, bias and e0 live
      in NaN-filled frames, so an unmasked read beyond their logical extent poisons the result,
  (d) that the kernel family and tile the case was written for ran (profiler scope names).  A mismatch FAILS: when the dispatch
      heuristics change, the cases are to be re-derived, not skipped.

Tolerances.  fp32 result: _tol of test_gpu_gemm.py (3e-6 * max(1, max|ref|) * max(1, sqrt(K))).  bf16 result: one rounding of the exact
value, 2^-8 * |ref| + _tol (half an ulp of bf16 is at most 2^-8 of the value); the staged bf16 write-out S1 with accumulate rounds the
tile before it adds the old value: 2^-8 * (|A.B| + |ref|) + _tol.  Elements that went through fast_sigmoid / fast_tanh: 3e-5
absolute, as in test_gpu_gemm.py.
"""
import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
MODES = {"nt": (0, 0), "nn": (0, 1), "tn": (1, 1)}
C0, C1 = 5, 21          # sigmoid range: starts inside the first 16-byte segment of a row, ends inside a later one


@pytest.fixture(scope="module")
def env():
    import sat_amd  # noqa: F401
    from sat_amd import _lib, decoder
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield decoder, _lib
    torch.set_num_threads(threads)


def kernel_name(family, mode, tile, types):
    if family == "f32":
        return "gemm_f32_%s_%s" % (mode, tile)
    if family == "reg":
        return "gemm_bf16_%s_%s_%s" % (mode, tile, types[0])
    return "gemm_glds_%s_%s" % (mode, tile)


def case(family, mode, M, N, K, types="f32", tile="64x64", **kw):
    """types: "f32" = the exact fp32 kernel; otherwise element types of A, B, C ("f" fp32, "b" bf16) of a bf16-MFMA request."""
    c = dict(family=family, mode=mode, M=M, N=N, K=K, types=types, tile=tile)
    c.update(kw)
    return c


def case_id(c):
    parts = [c["family"], c["tile"], c["mode"], "%dx%dx%d" % (c["M"], c["N"], c["K"]), c["types"]]
    for k in ("epi", "accumulate", "pad_ab", "pad_c", "c_off", "gather", "scatter", "slab", "poison"):
        if c.get(k):
            parts.append("%s%s" % (k, "" if c[k] is True else c[k]))
    return "-".join(parts)


def run_case(env, c):
    dk, L = env
    dev = "cuda"
    amode, bmode = MODES[c["mode"]]
    M, N, K, types = c["M"], c["N"], c["K"], c["types"]
    mfma = types != "f32"
    ta, tb, tc = (F32, F32, F32) if not mfma else tuple(BF if ch == "b" else F32 for ch in types)
    epi, accumulate = c.get("epi", 0), bool(c.get("accumulate"))
    gather, scatter = bool(c.get("gather")), bool(c.get("scatter"))
    g = torch.Generator().manual_seed(c.get("seed", 1000 * M + 10 * N + K))
    R = M + 20 if gather else M          # rows of the gather source
    A = torch.randn(R, K, generator=g); B = torch.randn(K, N, generator=g)
    if c.get("poison") == "nan_a":
        A[3, 5] = float("nan")
    if c.get("poison") == "inf_b":
        B[7, 11] = float("inf")
    a_rows = c_rows = None
    out_rows = M
    if gather:
        a_rows = torch.randint(0, R, (M,), generator=g).to(torch.int32)
        if epi != G.EPI_ADD_TANH:
            a_rows[3] = -1          # (epilogue 3 reads e0 by the gathered row: no row -1 there)
    if scatter:
        out_rows = M + 5
        c_rows = torch.randperm(out_rows, generator=g)[:M].to(torch.int32); c_rows[7] = -1
    bias = torch.randn(N, generator=g) if epi in (1, 2, 5) else None
    e0 = None
    if epi == G.EPI_ADD_TANH:
        e0 = torch.randn(R, N, generator=g)
    if epi == G.EPI_MUL_DTANH:
        e0 = torch.tanh(torch.randn(M, N, generator=g))
    C_old = torch.randn(out_rows, N, generator=g).to(tc).float() if accumulate else None

    A_st = A if amode == 0 else A.t()
    B_st = B.t() if bmode == 0 else B
    # K = 0: an empty tensor has no address to hand over; the operands are then four columns of NaN that must never be read
    fa, fb = (A_st, B_st) if K > 0 else (torch.full((A_st.shape[0], 4), float("nan")), torch.full((B_st.shape[0], 4), float("nan")))
    pad_ab = c.get("pad_ab", 8 if mfma else 3)          # the bf16 kernels need 16-byte gatherable rows; the fp32 kernel also takes odd ones
    nan = float("nan")
    _, va = G.framed(fa.shape[0], fa.shape[1], ta, pad_cols=pad_ab, guard_rows=1, fill=nan, device=dev, aligned=True if mfma else None)
    _, vb = G.framed(fb.shape[0], fb.shape[1], tb, pad_cols=pad_ab, guard_rows=1, fill=nan, device=dev, aligned=True if mfma else None)
    va.copy_(fa); vb.copy_(fb)
    vbias = ve0 = None
    if bias is not None:
        vbias = G.framed(1, N, F32, pad_cols=3, guard_rows=1, fill=nan, device=dev)[1][0]
        vbias.copy_(bias)
    if e0 is not None:
        _, ve0 = G.framed(e0.shape[0], N, F32, pad_cols=5, guard_rows=1, fill=nan, device=dev)          # lde0 = N + 5
        ve0.copy_(e0)
    canary = G.CANARY_BF16 if tc == BF else G.CANARY_F32
    whole_c, vc = G.framed(out_rows, N, tc, pad_cols=c.get("pad_c", 8), guard_rows=2, fill=canary, offset_elems=c.get("c_off", 0), device=dev,
                           aligned=c.get("c_aligned"))
    if accumulate:
        vc.copy_(C_old)
    slab = None
    if c.get("slab"):
        slab = torch.full((c["slab"],), nan, device=dev)          # a partial that is read without having been written shows

    L.profile_start()
    dk.gemm(va, vb, amode=amode, bmode=bmode, M=M, N=N, K=K, out=vc, accumulate=accumulate, epi=epi, bias=vbias, e0=ve0, c0=C0, c1=C1,
            a_rows=None if a_rows is None else a_rows.to(dev), c_rows=None if c_rows is None else c_rows.to(dev), slab=slab, bf16_mfma=mfma)
    torch.cuda.synchronize()
    names = sorted(e["name"] for e in L.profile_stop())
    want_name = kernel_name(c["family"], c["mode"], c["tile"], types)
    assert names == [want_name], "the dispatch took %s, the case was written for %s" % (names, want_name)          # (d)

    ref, written, acc = G.reference(A_st, B_st, amode=amode, bmode=bmode, C_old=C_old, accumulate=accumulate, epi=epi, bias=bias, e0=e0, c0=C0, c1=C1,
                                    a_rows=a_rows, c_rows=c_rows, out_rows=out_rows, round_inputs_to_bf16=mfma)
    G.assert_frame_untouched(whole_c, vc, canary, untouched_rows=~written if scatter else None)          # (b)
    got = vc.float().cpu().double()[written]
    ref = ref[written]
    nan_got, nan_ref = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(nan_got, nan_ref), "NaN at %d elements, the reference has %d" % (int(nan_got.sum()), int(nan_ref.sum()))   # (c)
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf])
    tol = torch.full_like(ref, G.tol_f32(ref, K))
    if epi == G.EPI_BIAS_SIGMOID_RANGE:
        tol[:, C0:C1] = 3e-5
    if epi == G.EPI_ADD_TANH:
        tol[:] = 3e-5
    if tc == BF:
        tol += 2.0 ** -8 * ref.abs().nan_to_num(0.0, 0.0, 0.0)
        if c.get("two_roundings"):
            dest = torch.arange(M) if c_rows is None else c_rows.long()
            accw = torch.zeros(out_rows, N, dtype=torch.float64); accw[dest[dest >= 0]] = acc[dest >= 0].abs()
            tol += 2.0 ** -8 * accw[written].nan_to_num(0.0, 0.0, 0.0)
    fin = torch.isfinite(ref)
    err = (got - ref).abs()[fin]
    worst = (err / tol[fin]).max().item() if err.numel() else 0.0
    print("%s: max |err| %.3e, worst err / tol %.3f" % (case_id(c), err.max().item() if err.numel() else 0.0, worst))
    assert worst <= 1.0          # (a)


def bf16_wide(c):
    """the request is eligible for the staged bf16 write-out S1 as far as shape and epilogue go (the frame decides the rest)"""
    return c["types"].endswith("b") and c["types"] != "f32" and c["N"] % 8 == 0


# ----------------------------------------------------------------------------- the shape table
SLAB = 1 << 20
TABLE = []
# exact fp32 kernel: its own scalar store, k tail (K = 40 = 2.5 k-tiles of 16), odd ldc (37 + 4); odd lda / ldb take the scalar
# loads, + 4 the float4 ones
for mode in MODES:
    for pad_ab in (3, 4):
        TABLE.append(case("f32", mode, 70, 37, 40, pad_ab=pad_ab, pad_c=4))
# K = 0: nothing to multiply, the result is f(C_old) or f(0)
for acc in (False, True):
    for epi in (0, 1):
        TABLE.append(case("f32", "nt", 33, 20, 0, accumulate=acc, epi=epi, pad_ab=4, pad_c=3))
# 128 x 128 tile of the fp32 kernel: 17 x 25 = 425 >= 384 tiles, ragged last row and column tiles
TABLE.append(case("f32", "nt", 2053, 3075, 24, tile="128x128", pad_c=1))
# fp32 split-K (2 tiles, K / 128 = 64 splits) with the ragged-N reduce, accumulating
TABLE.append(case("f32", "tn", 96, 41, 8192, accumulate=True, slab=SLAB, pad_c=2))
# register-staged bf16 kernel, fp32 operands rounded on the way into LDS: K = 40 ends inside the 64-wide k-tile
TABLE.append(case("reg", "nt", 70, 36, 40, "fff", pad_c=4, c_aligned=True))          # S2
TABLE.append(case("reg", "nt", 70, 37, 40, "fff", pad_c=4))          # S3
TABLE.append(case("reg", "nn", 72, 40, 40, "fff", pad_c=4, c_aligned=True))
TABLE.append(case("reg", "tn", 72, 40, 40, "fff", pad_c=4, c_aligned=True))
TABLE.append(case("reg", "nn", 72, 40, 40, "fff", pad_c=3))          # odd ldc: S3
# register-staged, bf16 operands (K % 64 != 0: the direct-to-LDS kernel declines)
for mode in ("nt", "nn"):
    TABLE.append(case("reg", mode, 136, 72, 40, "bbb", pad_c=8, c_aligned=True))          # S1
    TABLE.append(case("reg", mode, 136, 72, 40, "bbf", pad_c=4, c_aligned=True))          # S2
TABLE.append(case("reg", "nt", 136, 70, 40, "bbb", pad_c=8))          # ragged N: S3, bf16 result
TABLE.append(case("reg", "nt", 136, 70, 40, "bbf", pad_c=4))          # ragged N: S3, fp32 result
# S1-shaped requests that the frame sends to S3: ldc % 8 != 0, C two elements off a 16-byte boundary, both
TABLE.append(case("reg", "nt", 136, 72, 40, "bbb", pad_c=3))
TABLE.append(case("reg", "nt", 136, 72, 40, "bbb", pad_c=8, c_off=2, c_aligned=False))
TABLE.append(case("reg", "nt", 136, 72, 40, "bbb", pad_c=3, c_off=4, c_aligned=False))          # (2 rows of 75 + 2 would be aligned again)
TABLE.append(case("reg", "nt", 136, 72, 40, "bbf", pad_c=4, c_off=2, c_aligned=False))          # the same for S2
# direct-to-LDS kernel, 64 x 64: one k-tile (one stage); three k-tiles (two stages for an fp32 result, one for a bf16 result)
for K in (64, 192):
    for mode in ("nt", "nn"):
        TABLE.append(case("glds", mode, 70, 72, K, "bbb", pad_c=8, c_aligned=True))
        TABLE.append(case("glds", mode, 70, 72, K, "bbf", pad_c=4, c_aligned=True))
    TABLE.append(case("glds", "nt", 70, 70, K, "bbb", pad_c=8))          # ragged N: S3
    TABLE.append(case("glds", "nt", 70, 70, K, "bbf", pad_c=4))
TABLE.append(case("glds", "tn", 72, 72, 192, "bbf", pad_c=4, c_aligned=True))
# 128 x 64 reached from the 64-wide request: N <= 64 with a k-major A of >= 128 rows, or with >= 8192 rows
TABLE.append(case("glds", "tn", 136, 64, 128, "bbf", tile="128x64", pad_c=4, c_aligned=True))
TABLE.append(case("glds", "nt", 8200, 56, 64, "bbf", tile="128x64", pad_c=4, c_aligned=True))
TABLE.append(case("glds", "nt", 8200, 56, 64, "bbb", tile="128x64", pad_c=8, c_aligned=True))
# 128 x 64 reached from the 128-wide request: 13 x 16 = 208 >= 192 tiles of 128 and K > 256, row-major A, no split
for N in (2048, 2043):
    TABLE.append(case("glds", "nt", 1541, N, 320, "bbf", tile="128x64", pad_c=4, c_aligned=True if N % 4 == 0 else None))
    TABLE.append(case("glds", "nt", 1541, N, 320, "bbb", tile="128x64", pad_c=8, c_aligned=True if N % 8 == 0 else None))
# 128 x 128 with split-K (slab, M, N >= 128, K >= 4096: 4 tiles, 8 splits).  S4: N % 4 == 0; S5: ragged N, which only a row-major B
# allows (a k-major bf16 B needs N % 8 == 0 to be gathered 16 bytes at a time)
TABLE.append(case("glds", "tn", 136, 136, 4096, "bbf", tile="128x128", slab=SLAB, pad_c=4, c_aligned=True))
TABLE.append(case("glds", "nn", 136, 136, 4096, "bbf", tile="128x128", slab=SLAB, pad_c=4, c_aligned=True))
TABLE.append(case("glds", "nt", 136, 140, 4096, "bbf", tile="128x128", slab=SLAB, pad_c=4, c_aligned=True))
TABLE.append(case("glds", "nt", 136, 138, 4096, "bbf", tile="128x128", slab=SLAB, pad_c=4))          # S5
TABLE.append(case("glds", "nt", 136, 138, 4096, "bbf", tile="128x128", slab=SLAB, pad_c=4, accumulate=True, epi=5))
# register-staged split-K (2 tiles, 8 splits): S4, and S5 through the row-major B
TABLE.append(case("reg", "tn", 96, 40, 4096, "fff", slab=SLAB, pad_c=4, c_aligned=True))
TABLE.append(case("reg", "tn", 96, 44, 4096, "fff", slab=SLAB, pad_c=4, c_aligned=True))
TABLE.append(case("reg", "tn", 96, 44, 4096, "fff", slab=SLAB, pad_c=3, accumulate=True, epi=1))          # S4 partials, put() in the reduce
TABLE.append(case("reg", "nt", 96, 41, 4096, "fff", slab=SLAB, pad_c=4))          # S5
# S6, the many-split reduce.  launch_gemm_bf16_tile for 64 x 64 x 16384 with a slab: one 64-wide tile (blocks = 1 < 256), K >= 16 * 64, so
# want = 768 / 1 = 768, maxs = K / (8 * 64) = 32, lim = (M + N) * K * 2 / (8 * M * N) = 128 -> ns = 32; 256 k-tiles / 32 = 8 per split,
# nsplit = 32 >= 32, N % 4 == 0 -> wide slab, M * N / 4 / 256 = 4 < 256 -> splitk_reduce_z16_kernel.  The slab holds 32 * M * N floats.
TABLE.append(case("reg", "tn", 64, 64, 16384, "fff", slab=32 * 64 * 64, pad_c=4, c_aligned=True))
TABLE.append(case("glds", "tn", 64, 64, 16384, "bbf", slab=32 * 64 * 64, pad_c=4, c_aligned=True))
TABLE.append(case("glds", "tn", 64, 64, 16384, "bbf", slab=32 * 64 * 64, pad_c=3, accumulate=True, epi=2))          # put() from the many-split reduce


@pytest.mark.parametrize("c", TABLE, ids=case_id)
def test_shape_table(env, c):
    run_case(env, c)


# ----------------------------------------------------------------------------- epilogues x accumulate on one case per kernel and store path
REPS = [
    case("f32", "nt", 70, 37, 40, pad_c=4),
    case("reg", "nt", 70, 36, 40, "fff", pad_c=4, c_aligned=True),          # S2
    case("reg", "nt", 70, 37, 40, "fff", pad_c=4),                          # S3
    case("reg", "nt", 136, 72, 40, "bbb", pad_c=8, c_aligned=True),         # S1
    case("reg", "nt", 136, 72, 40, "bbf", pad_c=4, c_aligned=True),         # S2
    case("reg", "nt", 136, 70, 40, "bbb", pad_c=8),                         # S3
    case("reg", "nt", 136, 70, 40, "bbf", pad_c=4),                         # S3
    case("glds", "nt", 70, 72, 64, "bbb", pad_c=8, c_aligned=True),         # S1
    case("glds", "nt", 70, 72, 64, "bbf", pad_c=4, c_aligned=True),         # S2
    case("glds", "nt", 70, 70, 64, "bbb", pad_c=8),                         # S3
    case("glds", "nt", 70, 70, 64, "bbf", pad_c=4),                         # S3
    case("glds", "nn", 200, 72, 128, "bbb", pad_c=8, c_aligned=True),       # S1, two row tiles
]
CROSS = []
for rep in REPS:
    for epi in range(6):
        for acc in (False, True):
            if epi == 0 and not acc:
                continue          # in the table
            c = dict(rep, epi=epi, accumulate=acc)
            # S1 with accumulate adds the old value to the ROUNDED tile; only epilogue 0 reaches S1 with accumulate, every other
            # accumulating bf16 request takes put(): one rounding
            c["two_roundings"] = acc and bf16_wide(rep) and bool(rep.get("c_aligned")) and epi == 0
            CROSS.append(c)


@pytest.mark.parametrize("c", CROSS, ids=case_id)
def test_epilogues_and_accumulate(env, c):
    """bias and e0 sit in NaN frames (lde0 = N + 5); the sigmoid range [5, 21) straddles 16-byte segments.  With accumulate and epilogue 5
    the result is relu(C_old + A.B + bias), whichever write-out the request takes - not relu(A.B + bias) + C_old."""
    run_case(env, c)


# ----------------------------------------------------------------------------- row gather and scatter
ROWMAPS = []
# K % 64 == 0 too: the direct-to-LDS kernel must decline a_rows
for types, K, pad_c in (("fff", 40, 4), ("bbf", 40, 4), ("bbb", 40, 8), ("bbf", 64, 4), ("bbb", 128, 8)):
    ROWMAPS.append(case("reg", "nt", 70, 72, K, types, pad_c=pad_c, gather=True))
    ROWMAPS.append(case("reg", "nt", 70, 72, K, types, pad_c=pad_c, gather=True, epi=3))          # e0 indexed by the gathered row
    ROWMAPS.append(case("reg", "nn", 70, 72, K, types, pad_c=pad_c, gather=True, epi=1, accumulate=True))
for types, pad_c in (("fff", 4), ("bbf", 4), ("bbb", 8)):
    ROWMAPS.append(case("reg", "nt", 70, 72, 40, types, pad_c=pad_c, scatter=True))
    ROWMAPS.append(case("reg", "nt", 70, 72, 40, types, pad_c=pad_c, scatter=True, gather=True, epi=5))
ROWMAPS.append(case("f32", "nt", 70, 37, 40, pad_c=4, gather=True, scatter=True, epi=1))
# the scatter alone does not keep a request off the direct-to-LDS kernel
ROWMAPS.append(case("glds", "nt", 70, 72, 64, "bbb", pad_c=8, scatter=True))


@pytest.mark.parametrize("c", ROWMAPS, ids=case_id)
def test_row_gather_and_scatter(env, c):
    """a_rows[3] = -1 is a zero row, c_rows[7] = -1 drops the row; the five rows of C that no GEMM row maps to keep the canary."""
    run_case(env, c)


# ----------------------------------------------------------------------------- NaN / Inf in the logical operands
SPECIALS = [
    case("reg", "nt", 136, 72, 40, "bbb", pad_c=8, c_aligned=True, poison="nan_a", epi=5),          # S1: row 3 is NaN and stays NaN under the ReLU
    case("glds", "nt", 70, 72, 64, "bbf", pad_c=4, c_aligned=True, poison="nan_a", epi=5),          # S2
    case("reg", "nt", 70, 37, 40, "fff", pad_c=4, poison="nan_a", epi=5),                           # S3
    case("f32", "nt", 70, 37, 40, pad_c=4, poison="nan_a"),
    case("f32", "nn", 70, 37, 40, pad_c=4, poison="inf_b"),          # column 11 is +-Inf by the sign of A[:, 7]
    case("glds", "nn", 70, 72, 64, "bbb", pad_c=8, c_aligned=True, poison="inf_b"),
    case("reg", "nt", 136, 72, 40, "bbf", pad_c=4, c_aligned=True, poison="inf_b", epi=5),          # -Inf becomes 0 under the ReLU
]


@pytest.mark.parametrize("c", SPECIALS, ids=case_id)
def test_nan_and_inf_propagate_to_their_row_or_column_only(env, c):
    run_case(env, c)
