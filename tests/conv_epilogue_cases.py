"""The case table of the convolution epilogues ("Convolution statistics epilogues"), shared by test_conv_epilogue_cases.py (CPU:
the table, and that its inputs would show the faults it is there for) and test_gpu_conv_epilogues.py (GPU: every case through the C ABI).

The three epilogues sit in the write phase of the dense bf16 convolution launches (store_tile / store_tile_w and BnAcc in
csrc/gemm_bf16_common.h):
  "fwd"      sat_conv2d_fwd_bf16_stats      per row tile and output channel (sum v, sum v^2) of the stored values
  "bnstats"  sat_conv2d_dgrad_bf16_bnstats  per row tile and channel (sum g, sum g xhat): g = stored value where the bn_relu_mask bit is set
                                            (everywhere without a mask), xhat = (bn_x - mean) * invstd; the launch may accumulate
  "fused"    sat_conv2d_dgrad_bf16_fused    dx = data gradient + (add_mask bit ? add_src : 0), the statistics above optional

A case names the geometry (the fields of sat_conv_geom), what is handed in (relu_mask, accumulate, add_mask, stats), the sorted profiler
scope names the shipped dispatch must produce and the *tile_rows it must report.  Names and tile heights are derived by hand from
conv_fwd_any / conv_dgrad_any (csrc/encoder.hip), launch_gemm_bf16_tile (csrc/gemm_bf16.hip) and launch_gemm_glds (csrc/gemm_glds.hip); the
comment in front of each group says which rule sends it there.  A mismatch on the GPU FAILS the case: re-derive it, do not skip it.

The rules (M x N x Kr is the implicit GEMM: forward N*P*Q x K x R*S*C, data gradient N*H*W x C x R*S*K; conv_cases.py states them in full):
  request   128-wide when cdiv(M,128) * cdiv(N,128) >= 192 and M, N >= 128, unless that product is < 512 with Kr <= 256; else 64-wide
  glds      the direct-to-LDS kernel takes the launch unless Kr % 64, the gathered channels % 64 (forward C, data gradient K) or R*S > 32;
            64x64 -> 128x64 when N <= 64 and M >= 8192; 128x128 -> 128x64 when Kr <= 1152 or the 128-tile product is < 512, and always for
            a plain GEMM (1x1 / stride 1 / pad 0: "nt" forward, "nn" data gradient)
  reg       what glds declines runs on the register-staged kernel ("gemm_bf16_..._b") at the requested width
  *tile_rows is the tile HEIGHT of the kernel that ran (the BM of its scope name), 0 when the epilogue was declined: a data gradient by
  parity classes (stride 2), bn_x or the result off a 16-byte boundary.

COST CAP (conv_cases.py's): 2 * M * N * Kr <= 3e10, the largest tensor of a case <= 64 MiB.  The costliest geometry is that of conv_cases.py's
fwd-glds128x128 (8100 x 1024 x 1728, 2.87e10) and its data-gradient mirror; the float64 references are computed once per geometry.
"""
import functools
import re
import zlib

import torch

import batchnorm_ref as B
import conv_cases as CC
import conv_ref as R

COST_CAP, BYTES_CAP = CC.COST_CAP, CC.BYTES_CAP
F64 = torch.float64
U32 = 2.0 ** -24          # unit roundoff of fp32

FORMS = {
    "F1": "forward statistics, register-staged 64x64 (store_tile)",
    "F2": "forward statistics, register-staged 128x128",
    "F3": "forward statistics, direct-to-LDS 64x64",
    "F4": "forward statistics, direct-to-LDS 128x64 (tall rule and narrowed from the 128-wide request)",
    "F5": "forward statistics, direct-to-LDS 128x128",
    "F6": "forward statistics, plain GEMM (1x1 / stride 1 / pad 0: A_ROW / B_ROW) on all three tile forms it reaches",
    "B1": "backward statistics (BnAcc), register-staged 64x64",
    "B2": "backward statistics, register-staged 128x128 (eight segments per thread)",
    "B3": "backward statistics, direct-to-LDS 64x64",
    "B4": "backward statistics, direct-to-LDS 128x64 (tall rule and narrowed)",
    "B5": "backward statistics, direct-to-LDS 128x128 (eight segments per thread)",
    "B6": "backward statistics, plain GEMM (1x1 / stride 1 / pad 0: the nn kernels) at 64x64 and 128x64",
    "J1": "joined gradient, register-staged 64x64",
    "J2": "joined gradient, direct-to-LDS 64x64",
    "J3": "joined gradient, nn 64x64",
    "J4": "joined gradient, direct-to-LDS 128x64",
    "J5": "joined gradient, direct-to-LDS 128x128",
}

REG_FWD, REG_FWD128, REG_NT = CC.REG_FWD, "gemm_bf16_conv_fwd_128x128_b", "gemm_bf16_nt_64x64_b"
GL_FWD, GL_FWD_TALL, GL_FWD128 = CC.GL_FWD, CC.GL_FWD_TALL, CC.GL_FWD128
GL_NT, GL_NT_TALL = "gemm_glds_nt_64x64", "gemm_glds_nt_128x64"
REG_DG, REG_DG128, REG_NN = CC.REG_DG, "gemm_bf16_conv_dgrad_128x128_b", CC.REG_NN
GL_DG, GL_DG_TALL, GL_DG128 = CC.GL_DG, CC.GL_DG_TALL, "gemm_glds_conv_dgrad_128x128"
GL_NN, GL_NN_TALL = "gemm_glds_nn_64x64", CC.GL_NN_TALL

TABLE = []


def case(cid, form, kind, g, names, tile_rows, **kw):
    c = dict(id=cid, form=form, kind=kind, op="fwd" if kind == "fwd" else "dgrad", dt="bf16", g=g,
             names=sorted(names if isinstance(names, (list, tuple)) else [names]), tile_rows=tile_rows,
             relu_mask=False, accumulate=False, add_mask=False, stats=kind != "fused")
    c.update(kw)
    TABLE.append(c)
    return c


gemm_dims = CC.gemm_dims


def largest_tensor_bytes(c):
    """activations, gradients, filters, bn_x, add_src are all bf16; the float statistics are smaller than the result they describe"""
    return CC.largest_tensor_bytes(c)


def tile_rows_of(name):
    """the tile height a scope name states: gemm_glds_conv_fwd_128x64 -> 128"""
    return int(re.search(r"_(\d+)x(\d+)(_b)?$", name).group(1))


G = R.geom

# ============================================================================= forward statistics
# (M = N*P*Q pixels, N = K filters, Kr = R*S*C)
# C = 8: glds declines at `g.C % 64` (and Kr = 72 % 64) -> register-staged at the 64-wide request.  162 rows = 2.5 tiles; 72 filters: the second
# column tile has one live 8-column group
case("fwd-reg64", "F1", "fwd", G(2, 9, 9, 8, 72, 3, 3, 1, 1), REG_FWD, 64)
# C = 64: glds 64x64.  1 x 5 x 13 = 65 rows: a second tile of ONE row; K = 136: a third column tile of one 8-column group
case("fwd-glds64-k64", "F3", "fwd", G(1, 5, 13, 64, 64, 3, 3, 1, 1), GL_FWD, 64)
case("fwd-glds64-k136", "F3", "fwd", G(1, 5, 13, 64, 136, 3, 3, 1, 1), GL_FWD, 64)
# exactly one tile; the smallest N (one live column group of the only column tile)
case("fwd-glds64-onetile", "F3", "fwd", G(1, 8, 8, 64, 64, 3, 3, 1, 1), GL_FWD, 64)
case("fwd-glds64-k8", "F3", "fwd", G(2, 9, 9, 64, 8, 3, 3, 1, 1), GL_FWD, 64)
# tall rule: N = 64 <= 64 filters over 91 * 91 = 8281 >= 8192 pixels: 64 tiles of 128 and a ragged one of 89 rows
case("fwd-glds128x64-tall", "F4", "fwd", G(1, 91, 91, 64, 64, 3, 3, 1, 1), GL_FWD_TALL, 128)
# 3 * 8281 = 24843 pixels x 128 filters: 195 x 1 >= 192 tiles of 128, Kr = 576 > 256 keeps the 128-wide request, Kr <= 1152 narrows it; 11 rows ragged
case("fwd-glds128x64-narrowed", "F4", "fwd", G(3, 91, 91, 64, 128, 3, 3, 1, 1), GL_FWD_TALL, 128)
# conv_cases.py's fwd-glds128x128: 64 x 8 = 512 tiles (not < 512), Kr = 1728 > 1152; 8100 rows = 63 tiles and 36 rows
case("fwd-glds128x128", "F5", "fwd", G(1, 90, 90, 192, 1024, 3, 3, 1, 1), GL_FWD128, 128)
# C = 8, 7x7 stride 2 (R*S = 49 > 32 as well): 2 * 111 * 111 = 24642 pixels x 128 filters = 193 tiles of 128 (66 rows ragged), Kr = 392 > 256 -> the
# 128-wide request on the register-staged kernel
case("fwd-reg128x128", "F2", "fwd", G(2, 222, 222, 8, 128, 7, 7, 2, 3), REG_FWD128, 128)
# 1x1 / stride 1 / pad 0: conv_fwd_any hands a plain A_ROW x B_ROW GEMM over ("nt").  C = 64: glds 64x64; C = 8 (K % 64): register-staged;
# 8281 pixels x 64 filters: glds 128x64 by the tall rule.  The two glds cases are the ones where the `row < M` of the forward sums matters: the plain
# row-major load of the direct-to-LDS kernel clamps a row past M to row M - 1, so the accumulator holds a copy of the last row there, while the
# gathers (and the register-staged kernel) feed zeros for such rows
case("fwd-nt-glds64", "F6", "fwd", G(2, 9, 9, 64, 72, 1, 1, 1, 0), GL_NT, 64)
case("fwd-nt-reg64", "F6", "fwd", G(2, 9, 9, 8, 72, 1, 1, 1, 0), REG_NT, 64)
case("fwd-nt-glds128x64", "F6", "fwd", G(1, 91, 91, 64, 64, 1, 1, 1, 0), GL_NT_TALL, 128)

# ============================================================================= backward statistics
# (M = N*H*W pixels, N = C channels, Kr = R*S*K: the forward geometries with "C" and "K" exchanged where the gather needs it - the gathered
# operand is the OUTPUT gradient, so K % 64 != 0 sends a launch to the register-staged kernel.)  Every form with bn_relu_mask NULL and given;
# the small ones also accumulating onto finite old values.
BN_GEOMS = [
    # (tag, form, geometry, name, tile rows, small)
    ("reg64", "B1", G(2, 9, 9, 72, 8, 3, 3, 1, 1), REG_DG, 64, True),                       # K = 8: glds declines at `g.K % 64`
    ("glds64-c64", "B3", G(1, 5, 13, 64, 64, 3, 3, 1, 1), GL_DG, 64, True),                 # 65 rows
    ("glds64-c136", "B3", G(1, 5, 13, 136, 64, 3, 3, 1, 1), GL_DG, 64, True),               # third column tile of one group
    ("glds64-onetile", "B3", G(1, 8, 8, 64, 64, 3, 3, 1, 1), GL_DG, 64, True),
    ("glds64-c8", "B3", G(2, 9, 9, 8, 64, 3, 3, 1, 1), GL_DG, 64, True),                    # N = 8: one live column group (glds wants N >= 8)
    ("glds128x64-tall", "B4", G(1, 91, 91, 64, 64, 3, 3, 1, 1), GL_DG_TALL, 128, False),    # N <= 64, M = 8281 >= 8192
    ("glds128x64-narrowed", "B4", G(3, 91, 91, 128, 64, 3, 3, 1, 1), GL_DG_TALL, 128, False),   # 195 tiles of 128, 256 < Kr = 576 <= 1152
    # M = 8100, C = 1024, Kr = 9 * 192 = 1728: 512 tiles, Kr > 1152 keeps 128x128; BnAcc holds 128 * 16 / 256 = 8 segments per thread
    ("glds128x128", "B5", G(1, 90, 90, 1024, 192, 3, 3, 1, 1), GL_DG128, 128, False),
    # K = 8, 7x7 stride 1: 24642 pixels x 128 channels = 193 tiles of 128, Kr = 392 > 256 -> register-staged 128x128
    ("reg128x128", "B2", G(2, 111, 111, 128, 8, 7, 7, 1, 3), REG_DG128, 128, False),
    # 1x1 / stride 1 / pad 0: the plain row-major x k-major GEMM ("nn"); K = 8: register-staged; 8281 x 64: glds 128x64 by the tall rule
    ("nn-glds64", "B6", G(2, 9, 9, 72, 64, 1, 1, 1, 0), GL_NN, 64, True),
    ("nn-reg64", "B6", G(2, 9, 9, 72, 8, 1, 1, 1, 0), REG_NN, 64, True),
    ("nn-glds128x64", "B6", G(1, 91, 91, 64, 64, 1, 1, 1, 0), GL_NN_TALL, 128, False),
]
for tag, form, geo, name, tr, small in BN_GEOMS:
    for relu in (False, True):
        for acc in ((False, True) if small else (False,)):
            case("bn-%s%s%s" % (tag, "-relu" if relu else "", "-acc" if acc else ""), form, "bnstats", geo, name, tr, relu_mask=relu, accumulate=acc)

# ============================================================================= joined gradient
# an accumulating launch of the same kernels (conv_dgrad_any sets accumulate = 1), so the names are those of the group above.  add_mask NULL
# and given; without statistics, and with them - once with no mask at all, once with both masks (independent bits)
for tag, form, geo, name, tr in (("reg64", "J1", G(2, 9, 9, 72, 8, 3, 3, 1, 1), REG_DG, 64), ("glds64", "J2", G(1, 5, 13, 136, 64, 3, 3, 1, 1), GL_DG, 64),
                                 ("nn64", "J3", G(2, 9, 9, 72, 64, 1, 1, 1, 0), GL_NN, 64), ("glds128x64", "J4", G(1, 91, 91, 64, 64, 3, 3, 1, 1), GL_DG_TALL, 128),
                                 ("glds128x128", "J5", G(1, 90, 90, 1024, 192, 3, 3, 1, 1), GL_DG128, 128)):
    for am in (False, True):
        case("join-%s%s" % (tag, "-mask" if am else ""), form, "fused", geo, name, 0, add_mask=am, stats=False)
        case("join-%s%s-stats" % (tag, "-mask" if am else ""), form, "fused", geo, name, tr, add_mask=am, stats=True, relu_mask=am)

BY_ID = {c["id"]: c for c in TABLE}

# ============================================================================= declined and refused requests
# declined: the call succeeds on the plain kernels and reports *tile_rows == 0; refused: an error code and no launch
S2_GEOM = G(2, 10, 12, 64, 64, 3, 3, 2, 1)          # stride 2: four parity-class launches on glds 64x64 (conv_cases.py's dgrad-glds-s2-3x3)
S2_NAMES = [GL_DG] * 4
OFF_GEOM_DGRAD = G(1, 5, 13, 136, 64, 3, 3, 1, 1)   # bn_x / add_src 8 bytes off a 16-byte boundary
OFF_GEOM_FWD = G(1, 5, 13, 64, 136, 3, 3, 1, 1)     # y 8 bytes off: no 16-byte store path, so no statistics (the 2-byte stores of put())


# ============================================================================= inputs and float64 references
def last_rows(M):
    """bool (M): the last row of every 64-row tile (so of every 128-row tile too) and the last row of all"""
    r = torch.arange(M)
    return ((r + 1) % 64 == 0) | (r == M - 1)


@functools.lru_cache(maxsize=2)
def _shared(op, gkey):
    g = dict(gkey)
    gen = torch.Generator().manual_seed(zlib.crc32(repr((op, gkey)).encode()))
    P, Q = R.out_hw(g)
    fwd = op == "fwd"
    M, N, Kr = (g["N"] * P * Q, g["K"], g["R"] * g["S"] * g["C"]) if fwd else (g["N"] * g["H"] * g["W"], g["C"], g["R"] * g["S"] * g["K"])
    src = R.bf16_round(torch.randn(*((g["N"], g["H"], g["W"], g["C"]) if fwd else (g["N"], P, Q, g["K"])), generator=gen))
    w = R.bf16_round(torch.randn(g["K"], g["R"], g["S"], g["C"], generator=gen) / Kr ** 0.5)          # results of magnitude 1
    s = dict(g=g, M=M, N=N, Kr=Kr, src=src, w=w)
    if fwd:
        s["prod"] = R.forward(g, src, w).reshape(M, N)
        return s
    s["prod"] = R.dgrad(g, src, w)[0].reshape(M, N)
    last = last_rows(M)

    def boosted():
        """randn; the last row of every tile and the last channel at least 1.5 in magnitude (|x - mean| >= 1)"""
        t = torch.randn(M, N, generator=gen)
        big = torch.where(t < 0, -1.5 + t, 1.5 + t)
        t[last] = big[last]
        t[:, -1] = big[:, -1]
        return R.bf16_round(t)

    def bits():
        """Bernoulli(1/2); every bit of the last row of every tile set"""
        b = torch.rand(M, N, generator=gen) < 0.5
        b[last] = True
        return b

    s["old"] = R.bf16_round(torch.randn(M, N, generator=gen))
    s["add_src"], s["bn_x"] = boosted(), boosted()
    # deliberately NOT the statistics of bn_x: distinct per channel, so a column mix-up shows
    s["mean"] = ((torch.randperm(N, generator=gen).double() + 0.5) / N - 0.5).float()
    s["invstd"] = (0.5 + 1.5 * (torch.randperm(N, generator=gen).double() + 0.5) / N).float()
    s["relu_bits"], s["add_bits"] = bits(), bits()
    return s


def inputs(c):
    """everything a case reads, on the CPU, as float32 tensors that hold bf16 values (mean / invstd: the floats themselves) and bool bit maps;
    shared - and not to be written to - between the cases of one geometry.  prod (M, N) float64 is the convolution alone."""
    return _shared(c["op"], tuple(sorted(c["g"].items())))


def expected(c, s, relu_bits=None, add_bits=None):
    """(ref, prod) float64 (M, N): the result the call must store, and the convolution's own part of it"""
    prod = s["prod"]
    if c["kind"] == "fused":
        ab = (s["add_bits"] if add_bits is None else add_bits) if c["add_mask"] else torch.ones_like(s["add_bits"])
        return prod + torch.where(ab, s["add_src"].to(F64), torch.zeros((), dtype=F64)), prod
    if c["accumulate"]:
        return prod + s["old"].to(F64), prod
    return prod, prod


def element_tol(c, s, ref, prod):
    """the per-element rule of test_gpu_conv_forms.py: fp32 accumulation + one bf16 rounding, + a second one for accumulating / joined launches"""
    import gemm_ref
    tol = torch.full_like(ref, gemm_ref.tol_f32(ref, s["Kr"])) + 2.0 ** -8 * ref.abs()
    if c["accumulate"] or c["kind"] == "fused":
        tol += 2.0 ** -8 * prod.abs()
    return tol


def tile_of_rows(M, tile_rows, shift=0):
    """tile index of every row; shift = 1 moves every tile boundary one row down (row t * tile_rows - 1 falls into tile t)"""
    return (torch.arange(M) + shift) // tile_rows


def _tile_sum(terms, tiles, nt):
    out = torch.zeros(nt + 1, terms.shape[1], dtype=F64)          # (a shifted boundary pushes the last row into a tile that does not exist)
    out.index_add_(0, tiles, terms)
    return out[:nt]


def stats_ref(c, s, v, tile_rows, *, relu_bits=None, drop_rows=None, shift=0):
    """The statistics "of the stored values" v (M, N) float64, per tile of tile_rows rows and per channel: (ref, tol), both (ntiles, N, 2).
    Forward: sum v, sum v^2.  Backward: sum g, invstd * sum g (x - mean), g = v where the relu bit is set (everywhere without a mask); mean
    and invstd are the floats the call is given.  tol = (tile_rows + 2) * 2^-24 * sum |terms| (* invstd): fp32 summation of at most
    tile_rows terms in any order, one rounding of the term and one of the final scale.
    drop_rows (bool (M)): rows left out; shift: see tile_of_rows; relu_bits: other mask bits than the case's."""
    M, N = v.shape
    nt = -(-M // tile_rows)
    tiles = tile_of_rows(M, tile_rows, shift)
    if c["kind"] == "fwd":
        t0, t1, scale = v, v * v, torch.ones(N, dtype=F64)
    else:
        bits = (s["relu_bits"] if relu_bits is None else relu_bits) if c["relu_mask"] else None
        gv = v if bits is None else torch.where(bits, v, torch.zeros((), dtype=F64))
        t0, t1, scale = gv, gv * (s["bn_x"].to(F64) - s["mean"].to(F64)), s["invstd"].to(F64)
    if drop_rows is not None:
        keep = (~drop_rows).to(F64)[:, None]
        t0, t1 = t0 * keep, t1 * keep
    ref = torch.stack([_tile_sum(t0, tiles, nt), _tile_sum(t1, tiles, nt) * scale], dim=2)
    tol = (tile_rows + 2) * U32 * torch.stack([_tile_sum(t0.abs(), tiles, nt), _tile_sum(t1.abs(), tiles, nt) * scale], dim=2)
    return ref, tol


def shifted_bits(bits):
    """the bits a kernel sees that reads every mask byte one byte too far; beyond the mask lies 0xFF"""
    packed = B.pack_mask(bits)
    moved = torch.cat([packed[1:], torch.full((1,), 0xFF, dtype=torch.uint8)])
    return B.unpack_mask(moved, bits.numel()).reshape(bits.shape)
