"""Host reference and memory frames for the GEMM store-path tests (test_gpu_gemm_store_paths.py; checked by test_gemm_ref.py).

reference()               float64 restatement of one launch of the GEMM family: C = f(C_old + A.B), epilogues as csrc/gemm_bf16_common.h ep_value
framed()                  a logical rows x cols window inside one larger allocation: row padding (leading dimension > cols), guard rows
                          above and below, every element outside (and, until the caller fills it, inside) the window = `fill`
assert_frame_untouched()  everything outside the window still holds the fill, compared as raw bits (the fills are NaN payloads)
"""
import torch

EPI_NONE, EPI_BIAS, EPI_BIAS_SIGMOID_RANGE, EPI_ADD_TANH, EPI_MUL_DTANH, EPI_BIAS_RELU = range(6)

CANARY_BF16 = 0x7FC1          # quiet NaNs with a payload: no finite result, and no NaN the arithmetic produces, has these bits
CANARY_F32 = 0x7FC12345

_INT_OF = {torch.bfloat16: torch.int16, torch.float32: torch.int32}


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def tol_f32(ref, K):
    """fp32 accumulation in another order than the reference: the bound of tests/test_gpu_gemm.py"""
    finite = ref[torch.isfinite(ref)]
    top = float(finite.abs().max()) if finite.numel() else 0.0
    return 3e-6 * max(1.0, top) * max(1.0, K ** 0.5)


def reference(A, B, *, amode=0, bmode=0, C_old=None, accumulate=False, epi=EPI_NONE, bias=None, e0=None, c0=0, c1=0, a_rows=None,
              c_rows=None, out_rows=None, round_inputs_to_bf16=False):
    """A, B as stored: A (M, K) for amode 0 - the gather SOURCE when a_rows is given - else (K, M); B (N, K) for bmode 0, else (K, N).
    Returns (C, written, acc): C float64 (out_rows, N) with rows that no GEMM row lands on left as C_old (NaN without one), `written`
    the bool mask of the rows that were stored, acc = A.B per GEMM row (before accumulate and epilogue)."""
    f64 = torch.float64
    if round_inputs_to_bf16:
        A, B = bf16_round(A.float()), bf16_round(B.float())
    A, B = A.to(f64), B.to(f64)
    if a_rows is not None:
        if amode != 0:
            raise ValueError("a_rows gathers rows of a row-major A")
        r = torch.as_tensor(a_rows).long()
        A = A[r.clamp(min=0)]
        A = torch.where((r >= 0)[:, None], A, torch.zeros_like(A))          # a negative entry is a zero row: nothing is read for it
    Am = A if amode == 0 else A.t()
    Bm = B.t() if bmode == 0 else B
    M, N = Am.shape[0], Bm.shape[1]
    acc = Am @ Bm if Am.shape[1] > 0 else torch.zeros(M, N, dtype=f64)
    dest = torch.arange(M) if c_rows is None else torch.as_tensor(c_rows).long()
    if out_rows is None:
        out_rows = M if c_rows is None else int(dest.max()) + 1
    C = torch.full((out_rows, N), float("nan"), dtype=f64) if C_old is None else C_old.to(f64).clone()
    written = torch.zeros(out_rows, dtype=torch.bool)
    cols = torch.arange(N)
    for row in range(M):
        o = int(dest[row])
        if o < 0:
            continue          # a negative c_rows entry drops the row
        v = acc[row].clone()
        if accumulate:
            v = v + C_old[o].to(f64)          # before the epilogue function (gemm.h)
        if epi == EPI_BIAS:
            v = v + bias.to(f64)
        elif epi == EPI_BIAS_SIGMOID_RANGE:
            if bias is not None:
                v = v + bias.to(f64)
            rng = (cols >= c0) & (cols < c1)
            v = torch.where(rng, torch.sigmoid(v), v)
        elif epi == EPI_ADD_TANH:
            er = row if a_rows is None else int(a_rows[row])          # indexed by the GATHERED row
            if er < 0:
                raise ValueError("epilogue 3 with a negative a_rows entry has no e0 row")
            v = torch.tanh(v + e0[er].to(f64))
        elif epi == EPI_MUL_DTANH:
            u = e0[row].to(f64)
            v = v * (1.0 - u * u)
        elif epi == EPI_BIAS_RELU:
            v = v + bias.to(f64)
            v = torch.where(v < 0, torch.zeros_like(v), v)          # NaN stays NaN
        elif epi != EPI_NONE:
            raise ValueError("epilogue %d" % epi)
        C[o] = v
        written[o] = True
    return C, written, acc


def _fill_bits(t, fill):
    if isinstance(fill, int):
        t.view(_INT_OF[t.dtype]).fill_(fill)
    else:
        t.fill_(fill)


def framed(rows, cols, dtype, *, pad_cols=0, guard_rows=1, fill=float("nan"), offset_elems=0, device="cpu", aligned=None):
    """One allocation of offset_elems + (guard_rows + rows + guard_rows) x (cols + pad_cols) elements, all = fill (an int is a bit
    pattern).  Returns (whole, view): `whole` the flat allocation, `view` the logical rows x cols window with view.stride(0) =
    cols + pad_cols.  aligned=True / False asserts that the window does / does not start on a 16-byte boundary (the allocation does)."""
    ld = cols + pad_cols
    total_rows = rows + 2 * guard_rows
    whole = torch.empty(offset_elems + total_rows * ld, dtype=dtype, device=device)
    _fill_bits(whole, fill)
    assert whole.data_ptr() % 16 == 0
    view = whole[offset_elems:].view(total_rows, ld)[guard_rows:guard_rows + rows, :cols]
    if ld > 0 and rows > 1:
        assert view.stride(0) == ld
    if aligned is not None:
        assert (view.data_ptr() % 16 == 0) == aligned, "window alignment: offset %d bytes" % (view.data_ptr() % 16)
    return whole, view


def _window_index(whole, view):
    item = whole.element_size()
    off = (view.data_ptr() - whole.data_ptr()) // item
    rows, cols = (1, view.shape[0]) if view.dim() == 1 else view.shape
    ld = view.stride(0) if view.dim() == 2 and rows > 1 else cols
    if view.dim() == 2 and rows > 1:
        assert view.stride(1) == 1 or cols <= 1
    r = torch.arange(rows, device=whole.device)[:, None]
    c = torch.arange(cols, device=whole.device)[None, :]
    return off + r * ld + c          # (rows, cols) flat indices into `whole`


def assert_frame_untouched(whole, view, canary_bits, untouched_rows=None):
    """Every element of `whole` outside `view` (the window framed() returned, or a slice of it) has the bit pattern canary_bits; so do
    the window's rows `untouched_rows` (bool mask or indices: rows a scatter must not reach)."""
    bits = whole.view(_INT_OF[whole.dtype])
    idx = _window_index(whole, view)
    outside = torch.ones(whole.numel(), dtype=torch.bool, device=whole.device)
    outside[idx.reshape(-1)] = False
    if untouched_rows is not None:
        outside[idx[torch.as_tensor(untouched_rows).to(whole.device)].reshape(-1)] = True
    bad = torch.nonzero(outside & (bits != canary_bits)).reshape(-1)
    if bad.numel():
        first = int(bad[0])
        raise AssertionError("%d element(s) outside the logical window changed; first at flat index %d (window starts at %d): bits 0x%X"
                             % (bad.numel(), first, int(idx[0, 0]), int(bits[first]) & (0xFFFF if whole.element_size() == 2 else 0xFFFFFFFF)))
