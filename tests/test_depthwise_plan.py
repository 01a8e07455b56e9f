"""CPU: the launch plan of the depthwise 3x3 kernels (sat_dwconv3x3_plan: host arithmetic only, no device is touched).

The launchers of csrc/depthwise.hip take their kernel form, rows per thread, block shape and block count from the function this query
returns, so what is asserted here is what runs: every shape of tests/depthwise_cases.py lands on the form it was written for (which
test_gpu_depthwise_forms.py then runs), and the scratch that sat_dwconv3x3_wgrad_scratch_bytes reports holds every partial slice of the
filter gradient's plan, whichever storage type the call has."""
import ctypes
import itertools

import pytest

import depthwise_cases as D


@pytest.fixture(scope="module")
def lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def _id(c):
    return "x".join(str(v) for v in c["shape"])


@pytest.mark.parametrize("c", D.CASES, ids=_id)
def test_case_table_lands_on_the_form_it_was_written_for(lib, c):
    assert set(c["run"]) <= set(c["plans"])
    for dtype in (D.F32, D.BF16):
        if dtype not in c["plans"]:
            assert c["shape"][3] % D.VEC[dtype], "a plan is missing for a storage type the shape is valid for"
            continue
        for op in D.OPS:
            rc, got = D.query(lib, op, dtype, c["shape"])
            assert rc == 0, lib.sat_last_error()
            assert D.as_written(op, c["shape"], got) == c["plans"][dtype][op], "%s %s %s (%s)" % (_id(c), dtype, op, c["why"])


def test_case_table_reaches_every_form():
    """what the table is for, read off its own plans: each launch form in each storage type, with and without a row tail"""
    seen = set()
    for c in D.CASES:
        for dtype in c["run"]:
            for op, p in c["plans"][dtype].items():
                seen.add((op, dtype, p[0], "tail" if p[2] else "even", "rows" if p[1] > 1 else "row"))
                if op == "wgrad" and p[0] == 1:
                    seen.add(("cvb", dtype, p[3]))
    for dtype in (D.F32, D.BF16):
        for op in ("fwd", "dgrad"):
            assert (op, dtype, 1, "tail", "rows") in seen          # rolling window, last row block short
            assert any(k[:3] == (op, dtype, 0) and k[4] == "rows" for k in seen)          # stride 2, several rows per thread
        assert ("dgrad", dtype, 0, "tail", "rows") in seen
        assert ("wgrad", dtype, 1, "tail", "rows") in seen and ("wgrad", dtype, 1, "even", "rows") in seen
        assert ("wgrad", dtype, 0, "even", "row") in seen
        assert ("cvb", dtype, 11) in seen and ("cvb", dtype, 32) in seen
    assert ("fwd", D.F32, 0, "tail", "rows") in seen and ("fwd", D.F32, 1, "even", "rows") in seen
    assert ("cvb", D.F32, 1) in seen
    assert any(c["plans"][D.F32]["wgrad"][4] == 1024 for c in D.CASES if D.F32 in c["run"])          # the block cap


def _sweep():
    shapes = list(D.EXISTING) + [c["shape"] for c in D.CASES]
    # channel vectors per pixel around the block shapes: divisors of 32, primes, 33 = 3 x 11, more than one group of 32; maps on both sides of
    # the rolling-window threshold (N H W cv >= 131072) and of the 1024-block cap
    for cv, stride, (N, H, W) in itertools.product((1, 2, 31, 32, 33, 37, 44, 64, 120), (1, 2), ((1, 1, 1), (2, 9, 11), (3, 45, 47), (4, 64, 64), (2, 181, 182))):
        shapes.append((N, H, W, 8 * cv, stride))          # cv vectors in bf16, 2 cv in fp32
        shapes.append((N, H, W, 4 * cv, stride))          # cv vectors in fp32; bf16 only when cv is even
    return shapes


def test_scratch_holds_every_partial_of_either_storage_type(lib):
    checked = 0
    for shape in _sweep():
        N, H, W, C, stride = shape
        have = lib.sat_dwconv3x3_wgrad_scratch_bytes(*shape)
        for dtype in (D.F32, D.BF16):
            rc, got = D.query(lib, "wgrad", dtype, shape)
            if C % D.VEC[dtype]:
                assert rc != 0 and got == [0, 0, 0, 0]
                continue
            assert rc == 0, lib.sat_last_error()
            form, R, cvb, parts = got
            assert parts >= 1 and 1 <= cvb <= 32 and (C // D.VEC[dtype]) % cvb == 0 and (form == 0 or stride == 1)
            assert have >= parts * 9 * C * 4, "%s %s: %d bytes of scratch for %d partial slices" % (shape, dtype, have, parts)
            checked += 1
    assert checked > 200


def test_plan_argument_validation(lib):
    out = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    ok = (2, 9, 9, 8, 1)
    assert lib.sat_dwconv3x3_plan(0, 0, *ok, out) == 0 and list(out) == [0, 1, 0, 0]
    bad = [(0, 1, (2, 9, 9, 12, 1)),          # C % 8 in bf16
           (0, 0, (2, 9, 9, 6, 1)),           # C % 4 in fp32
           (1, 0, (2, 9, 9, 8, 3)), (1, 0, (2, 9, 9, 8, 0)),          # stride
           (2, 0, (0, 9, 9, 8, 1)), (2, 0, (2, 0, 9, 8, 1)), (2, 0, (2, 9, 0, 8, 1)), (2, 0, (2, 9, 9, 0, 1)), (2, 0, (2, 9, -9, 8, 1)),
           (3, 0, ok), (-1, 0, ok), (0, 2, ok)]          # op, dtype
    for op, dtype, shape in bad:
        out[:] = [7, 7, 7, 7]
        assert lib.sat_dwconv3x3_plan(op, dtype, *shape, out) != 0, (op, dtype, shape)
        assert list(out) == [0, 0, 0, 0]
        assert lib.sat_last_error()
    assert lib.sat_dwconv3x3_plan(0, 0, *ok, None) != 0 and b"null" in lib.sat_last_error()
    # the scratch query keeps answering 0 bytes for what no call accepts
    for shape in ((2, 9, 9, 8, 3), (2, 9, 9, 8, 0), (0, 9, 9, 8, 1), (2, 0, 9, 8, 1), (2, 9, 0, 8, 1), (2, 9, 9, 0, 1), (2, 9, 9, 6, 1)):
        assert lib.sat_dwconv3x3_wgrad_scratch_bytes(*shape) == 0, shape
    assert lib.sat_dwconv3x3_wgrad_scratch_bytes(2, 9, 9, 12, 1) > 0          # fp32 accepts C = 12
