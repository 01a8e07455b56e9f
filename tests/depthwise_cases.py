"""The shapes that pin every launch form of the depthwise 3x3 kernels (csrc/depthwise.hip), with the plan each was written for.

test_depthwise_plan.py (no GPU) asserts that sat_dwconv3x3_plan returns exactly these plans; test_gpu_depthwise_forms.py runs the
shapes.  When dw_rows / dw_chunk or the block shapes are retuned the plans here are re-derived and, where a form is no longer reached,
the shape is changed until it is again: a mismatch fails, nothing is skipped.

A plan: forward and data gradient (form, R, tail); filter gradient (form, R, tail, cvb, partial slices).  form 0 = generic kernel,
1 = rolling window; R = rows per thread; tail = rows of the last row block when R does not divide the rows the kernel walks (P for the
forward, H for both gradients), else 0.
"""

F32, BF16 = "fp32", "bf16"


def case(shape, run, why, **plans):
    """shape (N, H, W, C, stride); run: the storage types the GPU test runs; plans: one per storage type the shape is valid for"""
    return dict(shape=shape, run=run, why=why, plans=plans)


def plan(fwd, dgrad, wgrad):
    return dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad)


CASES = [
    case((2, 63, 66, 256, 1), (F32, BF16), "rolling fwd / dgrad R = 2 with an odd H; wgrad rolling R = 8 (fp32), R = 4 tail 3 (bf16)",
         fp32=plan((1, 2, 1), (1, 2, 1), (1, 8, 7, 32, 132)), bf16=plan((0, 1, 0), (0, 1, 0), (1, 4, 3, 32, 264))),
    case((2, 127, 130, 256, 1), (F32, BF16), "rolling R = 8 tail 7 (fp32); the only bf16 rolling fwd / dgrad shape with a tail (R = 4, tail 3)",
         fp32=plan((1, 8, 7), (1, 8, 7), (1, 8, 7, 32, 520)), bf16=plan((1, 4, 3), (1, 4, 3), (1, 8, 7, 32, 520))),
    case((8, 5, 820, 256, 1), (F32, BF16), "H < R: one thread covers a whole column, both halo rows lie outside the map",
         fp32=plan((1, 8, 5), (1, 8, 5), (1, 8, 5, 32, 820)), bf16=plan((1, 4, 1), (1, 4, 1), (1, 8, 5, 32, 820))),
    case((2, 4096, 1, 256, 1), (F32, BF16), "W = 1: both side columns are masked in every row",
         fp32=plan((1, 2, 0), (1, 2, 0), (1, 8, 0, 32, 128)), bf16=plan((0, 1, 0), (0, 1, 0), (1, 4, 0, 32, 256))),
    case((8, 112, 112, 32, 1), (F32, BF16), "the first mobilenet_v2 depthwise layer at 8 images: R = 3 tail 1 (fp32); bf16 wgrad R = 6 tail 4",
         fp32=plan((1, 3, 1), (1, 3, 1), (1, 8, 0, 8, 392)), bf16=plan((0, 1, 0), (0, 1, 0), (1, 6, 4, 4, 266))),
    case((2, 181, 182, 128, 1), (F32, BF16), "fp32 wgrad wants 1047 blocks, capped at 1024: blocks take several columns",
         fp32=plan((1, 8, 5), (1, 8, 5), (1, 8, 5, 32, 1024)), bf16=plan((1, 4, 1), (1, 4, 1), (1, 8, 5, 16, 524))),
    case((3, 45, 47, 132, 1), (F32,), "wgrad rolling with cv = 33: cvb = 11, 253 live threads",
         fp32=plan((0, 1, 0), (0, 1, 0), (1, 3, 0, 11, 92))),
    case((1, 96, 99, 264, 1), (BF16,), "the same cvb = 11 block in bf16 (cv = 33)",
         fp32=plan((1, 2, 0), (1, 2, 0), (1, 8, 0, 22, 108)), bf16=plan((0, 1, 0), (0, 1, 0), (1, 4, 0, 11, 104))),
    case((2, 61, 60, 148, 1), (F32,), "cv = 37 (prime): cvb = 1, 256 pixel lanes",
         fp32=plan((0, 1, 0), (0, 1, 0), (1, 4, 1, 1, 8))),
    case((4, 90, 93, 256, 2), (F32, BF16), "stride 2: fwd R = 2 with P = 45 (tail 1, fp32); dgrad R = 8 tail 2 (fp32), R = 4 tail 2 (bf16)",
         fp32=plan((0, 2, 1), (0, 8, 2), (0, 1, 0, 32, 133)), bf16=plan((0, 1, 0), (0, 4, 2), (0, 1, 0, 32, 133))),
    case((2, 131, 130, 512, 2), (F32, BF16), "stride 2: fwd R = 4 with P = 66 (tail 2, fp32), R = 2 (bf16); dgrad R = 8 tail 3",
         fp32=plan((0, 4, 2), (0, 8, 3), (0, 1, 0, 32, 135)), bf16=plan((0, 2, 0), (0, 8, 3), (0, 1, 0, 32, 135))),
]

# the shapes of test_gpu_shufflenet.py::test_depthwise3x3_fwd_dgrad_wgrad (all of them one row per thread; C % 8 == 0)
EXISTING = [(2, 9, 9, 8, 1), (2, 10, 11, 24, 2), (3, 7, 5, 48, 1), (2, 8, 8, 96, 2), (1, 1, 1, 8, 1), (2, 2, 3, 16, 2), (4, 28, 28, 24, 2),
            (2, 14, 14, 352, 1), (16, 56, 56, 24, 2)]

OPS = {"fwd": 0, "dgrad": 1, "wgrad": 2}
VEC = {F32: 4, BF16: 8}          # channels per 16-byte vector


def out_size(n, stride):
    return (n + 2 - 3) // stride + 1


def query(lib, op, dtype, shape):
    """(status, [form, R, cvb, partial slices]) of sat_dwconv3x3_plan"""
    import ctypes
    out = (ctypes.c_int32 * 4)()
    rc = lib.sat_dwconv3x3_plan(OPS[op], int(dtype == BF16), *shape, out)
    return rc, list(out)


def as_written(op, shape, got):
    """the query's answer in the layout of the table: (form, R, tail) or (form, R, tail, cvb, slices)"""
    N, H, W, C, stride = shape
    form, R, cvb, parts = got
    rows = out_size(H, stride) if op == "fwd" else H
    tail = rows % R
    return (form, R, tail) if op != "wgrad" else (form, R, tail, cvb, parts)
