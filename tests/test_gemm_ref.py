"""CPU: the helper of the GEMM store-path tests (tests/gemm_ref.py) - epilogue order, row maps, frames."""
import math

import pytest
import torch

import gemm_ref as G


def test_epilogue_runs_after_the_accumulate():
    """2x2 by hand: A = I, so A.B = B.  relu(old + acc + b) != relu(acc + b) + old wherever acc + b < 0."""
    A = torch.eye(2)
    B_logical = torch.tensor([[1.0, -3.0], [-2.0, 4.0]])          # (K, N)
    old = torch.tensor([[0.5, 1.0], [1.5, -1.0]])
    bias = torch.tensor([0.25, -0.5])
    C, written, acc = G.reference(A, B_logical, bmode=1, C_old=old, accumulate=True, epi=G.EPI_BIAS_RELU, bias=bias)
    assert torch.equal(acc, B_logical.double()) and bool(written.all())
    want = torch.tensor([[1.75, 0.0], [0.0, 2.5]], dtype=torch.float64)          # relu([[0.5+1+0.25, 1-3-0.5], [1.5-2+0.25, -1+4-0.5]])
    assert torch.equal(C, want)
    other_order = torch.relu(B_logical + bias) + old          # [[1.75, 1.0], [1.5, 2.5]]
    assert not torch.equal(other_order.double(), want)
    # the same through the row-major B form (B stored (N, K))
    C2, _, _ = G.reference(A, B_logical.t().contiguous(), bmode=0, C_old=old, accumulate=True, epi=G.EPI_BIAS_RELU, bias=bias)
    assert torch.equal(C2, want)
    # k-major A: A stored (K, M)
    A2 = torch.tensor([[1.0, 2.0], [0.0, 1.0]])          # logical A = A2^T = [[1, 0], [2, 1]]
    C3, _, _ = G.reference(A2, B_logical, amode=1, bmode=1)
    assert torch.equal(C3, torch.tensor([[1.0, -3.0], [0.0, -2.0]], dtype=torch.float64))


def test_epilogues_follow_ep_value():
    A = torch.tensor([[1.0, 2.0]]); B = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])          # (N, K): acc = [1, 2, 3]
    bias = torch.tensor([1.0, -1.0, 0.5])
    e0 = torch.tensor([[0.5, -0.25, 0.0]])
    ref = lambda **kw: G.reference(A, B, **kw)[0][0].tolist()          # noqa: E731
    assert ref() == [1.0, 2.0, 3.0]
    assert ref(epi=1, bias=bias) == [2.0, 1.0, 3.5]
    got = ref(epi=2, bias=bias, c0=1, c1=2)
    assert got[0] == 2.0 and got[2] == 3.5 and got[1] == pytest.approx(1 / (1 + math.exp(-1.0)), abs=1e-15)
    assert ref(epi=2, c0=0, c1=0) == [1.0, 2.0, 3.0]          # no bias, empty range
    assert ref(epi=3, e0=e0) == pytest.approx([math.tanh(1.5), math.tanh(1.75), math.tanh(3.0)], abs=1e-15)
    assert ref(epi=4, e0=e0) == [0.75, 2.0 * (1 - 0.0625), 3.0]
    assert ref(epi=5, bias=torch.tensor([-2.0, 0.0, 0.0])) == [0.0, 2.0, 3.0]
    nan = G.reference(torch.tensor([[float("nan"), 2.0], [1.0, 2.0]]), B, epi=5, bias=bias)[0]
    # NaN * 0 is NaN: the whole row, and it stays NaN under the ReLU
    assert bool(torch.isnan(nan[0]).all()) and nan[1].tolist() == [2.0, 1.0, 3.5]
    with pytest.raises(ValueError):
        ref(epi=6)


def test_inputs_rounded_to_bf16_first():
    A = torch.tensor([[1.0 + 2.0 ** -9]]); B = torch.tensor([[3.0]])
    assert G.reference(A, B)[0].item() == 3.0 * (1.0 + 2.0 ** -9)
    assert G.reference(A, B, round_inputs_to_bf16=True)[0].item() == 3.0          # 1 + 2^-9 is the tie: rounds to even, 1.0


def test_row_gather_and_scatter_with_negative_entries():
    src = torch.tensor([[1.0, 0.0], [0.0, 1.0], [float("nan"), float("nan")]])          # row 2 is never gathered
    B = torch.tensor([[1.0, 2.0], [3.0, 4.0]])          # (N, K)
    C, written, _ = G.reference(src, B, a_rows=torch.tensor([1, -1, 0], dtype=torch.int32))
    assert torch.equal(C, torch.tensor([[2.0, 4.0], [0.0, 0.0], [1.0, 3.0]], dtype=torch.float64)) and bool(written.all())
    # epilogue 3 reads e0 by the gathered row
    e0 = torch.tensor([[10.0, 10.0], [-2.0, -4.0], [0.0, 0.0]])
    C, _, _ = G.reference(src, B, a_rows=torch.tensor([1, 0], dtype=torch.int32), epi=3, e0=e0)
    assert C[0].tolist() == [0.0, 0.0] and C[1].tolist() == pytest.approx([math.tanh(11.0), math.tanh(13.0)])
    with pytest.raises(ValueError):
        G.reference(src, B, a_rows=torch.tensor([-1], dtype=torch.int32), epi=3, e0=e0)
    # scatter: GEMM row r lands in row c_rows[r]; a negative entry drops it; rows nobody lands on keep the old contents
    A = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    old = torch.full((4, 2), 7.0)
    C, written, _ = G.reference(A, B, c_rows=torch.tensor([3, -1, 0], dtype=torch.int32), out_rows=4, C_old=old)
    assert written.tolist() == [True, False, False, True]
    assert torch.equal(C, torch.tensor([[3.0, 7.0], [7.0, 7.0], [7.0, 7.0], [1.0, 3.0]], dtype=torch.float64))
    C, written, _ = G.reference(A, B, c_rows=torch.tensor([3, -1, 0], dtype=torch.int32), out_rows=4, C_old=old, accumulate=True)
    assert torch.equal(C[0], torch.tensor([10.0, 14.0], dtype=torch.float64)) and torch.equal(C[1], old[1].double())
    C, _, _ = G.reference(A, B, c_rows=torch.tensor([1, -1, 0], dtype=torch.int32))
    assert C.shape == (2, 2)


@pytest.mark.parametrize("dtype,canary", [(torch.bfloat16, G.CANARY_BF16), (torch.float32, G.CANARY_F32)])
def test_frame_check_sees_every_element_outside_the_window(dtype, canary):
    rows, cols, pad, guard = 5, 6, 2, 2
    whole, view = G.framed(rows, cols, dtype, pad_cols=pad, guard_rows=guard, fill=canary)
    ld = cols + pad
    assert whole.numel() == (rows + 2 * guard) * ld and view.shape == (rows, cols) and view.stride(0) == ld
    assert bool(torch.isnan(whole).all())          # the canary is a NaN
    G.assert_frame_untouched(whole, view, canary)
    view.copy_(torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols))          # writing the window is allowed
    view[2, 3] = float("nan")          # ... any value, NaNs included
    G.assert_frame_untouched(whole, view, canary)
    inside = set((guard + r) * ld + c for r in range(rows) for c in range(cols))
    for flat in range(whole.numel()):
        if flat in inside:
            continue
        keep = whole[flat].clone()
        whole[flat] = 1.0
        with pytest.raises(AssertionError):
            G.assert_frame_untouched(whole, view, canary)
        whole[flat] = float("nan")          # ANOTHER NaN is a change too: raw bits are compared
        with pytest.raises(AssertionError):
            G.assert_frame_untouched(whole, view, canary)
        whole[flat] = keep
        G.assert_frame_untouched(whole, view, canary)
    # rows a scatter must not reach
    G.assert_frame_untouched(whole, view, canary, untouched_rows=torch.tensor([], dtype=torch.long))
    with pytest.raises(AssertionError):
        G.assert_frame_untouched(whole, view, canary, untouched_rows=torch.tensor([1]))
    whole2, view2 = G.framed(rows, cols, dtype, pad_cols=pad, guard_rows=guard, fill=canary)
    view2[0].fill_(1.0); view2[4].fill_(2.0)
    mask = torch.tensor([False, True, True, True, False])
    G.assert_frame_untouched(whole2, view2, canary, untouched_rows=mask)
    view2[2, 5] = 0.0
    with pytest.raises(AssertionError):
        G.assert_frame_untouched(whole2, view2, canary, untouched_rows=mask)


def test_frame_offsets_and_alignment():
    whole, view = G.framed(4, 8, torch.bfloat16, pad_cols=8, guard_rows=1, fill=G.CANARY_BF16, aligned=True)
    assert view.data_ptr() % 16 == 0
    whole, view = G.framed(4, 8, torch.bfloat16, pad_cols=8, guard_rows=1, fill=G.CANARY_BF16, offset_elems=2, aligned=False)
    assert view.data_ptr() % 16 == 4 and whole.numel() == 2 + 6 * 16
    G.assert_frame_untouched(whole, view, G.CANARY_BF16)
    whole[1] = 0.0          # the elements in front of the shifted window belong to the frame
    with pytest.raises(AssertionError):
        G.assert_frame_untouched(whole, view, G.CANARY_BF16)
    with pytest.raises(AssertionError):
        G.framed(4, 8, torch.float32, pad_cols=1, guard_rows=1, aligned=True)          # 9 floats per row: the window starts at byte 36
    # NaN-filled operand frames, one-dimensional windows (bias) and empty windows (K = 0)
    whole, view = G.framed(1, 5, torch.float32, pad_cols=3, guard_rows=1)
    assert bool(torch.isnan(whole).all()) and view[0].shape == (5,)
    whole, view = G.framed(3, 0, torch.float32, pad_cols=4, guard_rows=1)
    assert view.shape == (3, 0) and view.stride(0) == 4
