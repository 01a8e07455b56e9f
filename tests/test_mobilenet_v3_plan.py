"""CPU: the launch plans of the kernels mobilenet_v3_small added, without a device.

The library has no plan query for these kernels, so the plans are the restatements of dw5_chunk / dw5_cvb (csrc/depthwise5x5.hip) and
hs_grid (csrc/mobilenet_v3.hip) in tests/mobilenet_v3_kernel_cases.py.  Asserted here: every shape of the table lands on the form it was
written for under the restatement (test_gpu_mobilenet_v3_forms.py then runs it), and the restatement agrees with what the library does
answer: sat_dwconv5x5_wgrad_scratch_bytes equals partials x 25 x C floats for every shape of a sweep (a retuned dw5_chunk fails it),
sat_se_bwd_scratch_bytes is N (2 C + S) floats, and the hard-swish partials fit sat_bn_scratch_bytes: inside the share that holds
partials, before its last 64 bytes and the reserved ticket words, with the default block targets."""
import itertools

import pytest

import mobilenet_v3_kernel_cases as K


@pytest.fixture(scope="module")
def lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    return _lib.lib()


def _ticket_bytes(C):
    return (-(-C // 32) * 4 + 63) // 64 * 64


# ------------------------------------------------------------------ depthwise 5x5
@pytest.mark.parametrize("c", K.DW5_CASES, ids=lambda c: "x".join(map(str, c["shape"])))
def test_dw5_case_lands_on_the_form_it_was_written_for(lib, c):
    N, H, W, C, stride = c["shape"]
    got = K.dw5_plan(c["shape"])
    assert got == c["plan"], c["why"]
    chunk, parts, cvb, lanes = got
    npix = N * K.dw5_out(H, stride) * K.dw5_out(W, stride)
    assert (parts - 1) * chunk < npix <= parts * chunk and (C // 4) % cvb == 0 and lanes == 256 // cvb
    assert lib.sat_dwconv5x5_wgrad_scratch_bytes(*c["shape"]) == parts * 25 * C * 4
    assert set(c["run"]) <= {K.F32, K.BF16} and c["why"]


def test_dw5_table_reaches_every_form():
    plans = {c["shape"]: c["plan"] for c in K.DW5_CASES}
    cvbs = {p[2] for p in plans.values()}
    assert {1, 3, 6, 11, 20} <= cvbs          # 256, 255, 252, 253, 240 live threads
    assert any(p[0] > 64 for p in plans.values()) and any(p[1] > 64 for p in plans.values())          # chunk above the floor; more partials than finish lanes
    assert any(s[3] // 4 > p[2] for s, p in plans.items())          # more than one channel group
    assert any(s[3] % 8 and K.BF16 in c["run"] for c in K.DW5_CASES for s in [c["shape"]])          # bf16 off the 16-byte boundaries
    strides = {(s[4], s[1] % 2, s[2] % 2) for s in plans}
    assert (2, 1, 1) in strides and (2, 0, 0) in strides
    assert (1, 1, 1, 4, 1) in plans


def test_dw5_scratch_holds_every_partial(lib):
    checked = 0
    shapes = [c["shape"] for c in K.DW5_CASES]
    for cv, stride, (N, H, W) in itertools.product((1, 2, 3, 31, 32, 33, 37, 40, 64, 120), (1, 2),
                                                   ((1, 1, 1), (2, 9, 11), (3, 45, 47), (4, 128, 128), (1, 256, 257), (8, 600, 601))):
        shapes.append((N, H, W, 4 * cv, stride))
    for shape in shapes:
        N, H, W, C, stride = shape
        chunk, parts, cvb, lanes = K.dw5_plan(shape)
        npix = N * K.dw5_out(H, stride) * K.dw5_out(W, stride)
        assert 64 <= chunk <= 2048 and chunk % 64 == 0 and (parts - 1) * chunk < npix <= parts * chunk
        assert 1 <= cvb <= 32 and (C // 4) % cvb == 0 and lanes == 256 // cvb and lanes * cvb * 16 <= 65536          # the LDS of a block
        assert lib.sat_dwconv5x5_wgrad_scratch_bytes(*shape) == parts * 25 * C * 4
        checked += 1
    assert checked > 100


def test_dw5_scratch_answers_zero_for_what_no_call_accepts(lib):
    for shape in ((2, 9, 9, 6, 1), (2, 9, 9, 0, 1), (2, 9, 9, -4, 1), (2, 9, 9, 8, 3), (2, 9, 9, 8, 0), (0, 9, 9, 8, 1), (2, 0, 9, 8, 1), (2, 9, 0, 8, 1)):
        assert lib.sat_dwconv5x5_wgrad_scratch_bytes(*shape) == 0, shape
    assert lib.sat_dwconv5x5_wgrad_scratch_bytes(2, 9, 9, 12, 1) == 3 * 25 * 12 * 4          # C = 12 is legal in both storage types
    assert K.dw5_plan((2, 9, 9, 8, 1)) == (64, 3, 2, 128)


# ------------------------------------------------------------------ BatchNorm + hard-swish
@pytest.mark.parametrize("c", K.HS_CASES, ids=lambda c: c["name"])
def test_hs_case_lands_on_the_form_it_was_written_for(lib, c):
    rows, C = c["rows"], c["C"]
    assert c["run"] and c["why"]
    have = lib.sat_bn_scratch_bytes(rows, C)
    for dtype in c["run"]:
        assert C % K.VEC[dtype] == 0
        got = K.hs_plan(lib, dtype, rows, C)
        assert got == c["plans"][dtype], "%s %s (%s)" % (c["name"], dtype, c["why"])
        parts = got[4]
        assert parts * C * 2 * 8 <= have
        assert parts * C * 2 * 8 <= have - 64 - _ticket_bytes(C), "the partials reach into the last 64 bytes / the ticket words"
    if c["tile_rows"]:
        assert c["run"] == (K.BF16,)


def test_hs_table_reaches_every_form():
    seen = set()
    for c in K.HS_CASES:
        for dtype in c["run"]:
            CV, RL, colblocks, rows_per, parts = c["plans"][dtype]
            cvt = c["C"] // K.VEC[dtype]
            seen.add((dtype, "RL", RL))
            seen.add((dtype, "parts" if parts > 1 else "part", "ragged" if c["rows"] % rows_per else "even"))
            if colblocks > 1:
                seen.add((dtype, "idle columns", colblocks * CV - cvt))
            if c["rows"] < RL:
                seen.add((dtype, "fewer rows than lanes"))
            if (c["rows"] * cvt) % 256:
                seen.add((dtype, "apply tail"))
            if c["tile_rows"]:
                seen.add((dtype, "tiles"))
    for dtype in (K.F32, K.BF16):
        assert (dtype, "RL", 1) in seen and (dtype, "RL", 256) in seen
        assert (dtype, "parts", "ragged") in seen and (dtype, "fewer rows than lanes") in seen and (dtype, "apply tail") in seen
    assert (K.F32, "idle columns", 6) in seen and (K.F32, "idle columns", 255) in seen and (K.BF16, "idle columns", 1) in seen
    assert (K.BF16, "tiles") in seen and (K.F32, "RL", 32) in seen and (K.BF16, "RL", 128) in seen
    assert any(c["rows"] == 1 and c["run"] == (K.BF16,) for c in K.HS_CASES)


def test_hs_partials_stay_inside_their_share_of_the_scratch(lib):
    checked = 0
    shapes = [(c["rows"], c["C"]) for c in K.HS_CASES]
    shapes += list(itertools.product((1, 2, 7, 63, 64, 65, 511, 513, 2047, 2049, 4096, 16385, 100352, 802816), (4, 8, 12, 16, 24, 40, 64, 576, 1024, 1028, 2048, 2056)))
    for rows, C in shapes:
        have = lib.sat_bn_scratch_bytes(rows, C)
        assert have > 0
        for dtype in (K.F32, K.BF16):
            if C % K.VEC[dtype]:
                continue
            CV, RL, colblocks, rows_per, parts = K.hs_plan(lib, dtype, rows, C)
            cvt = C // K.VEC[dtype]
            assert 256 % CV == 0 and CV <= cvt and RL == 256 // CV and colblocks * CV >= cvt > (colblocks - 1) * CV
            assert rows_per >= 8 * RL and parts >= 1 and (parts - 1) * rows_per < rows <= parts * rows_per
            assert parts * C * 2 * 8 <= have - 64 - _ticket_bytes(C), "%dx%d %s: %d parts in %d bytes" % (rows, C, dtype, parts, have)
            checked += 1
    assert checked > 250


# ------------------------------------------------------------------ squeeze-and-excitation
@pytest.mark.parametrize("c", K.SE_CASES, ids=lambda c: "x".join(map(str, c["shape"])))
def test_se_case_states_its_pass_structure_and_fits_its_scratch(lib, c):
    N, HW, C, S = c["shape"]
    assert K.se_passes(C) == c["passes"] and c["why"]
    for dtype in c["run"]:
        assert C % K.VEC[dtype] == 0
    assert C <= 1024 and S <= 256
    assert lib.sat_se_bwd_scratch_bytes(N, C, S) == 4 * K.se_scratch_floats(N, C, S) == 4 * N * (2 * C + S)


def test_se_table_reaches_every_form():
    shapes = [c["shape"] for c in K.SE_CASES]
    assert any(K.se_passes(C)[0] > 1 and K.se_passes(C)[1] < 64 for N, HW, C, S in shapes)          # a short last pass
    assert any(256 % K.se_passes(C)[1] for N, HW, C, S in shapes)          # idle threads
    assert any(HW < K.se_passes(C)[2] for N, HW, C, S in shapes)          # fewer pixels than lanes
    assert any(C == 1024 and S == 256 for N, HW, C, S in shapes) and any(C > 512 for N, HW, C, S in shapes)
    assert any(S < 8 and S > 1 for N, HW, C, S in shapes) and any((2 * S * C + S + C) % 256 and 2 * S * C + S + C > 256 for N, HW, C, S in shapes)
    assert any(HW // K.se_passes(C)[2] > 100 for N, HW, C, S in shapes) and any(N >= 5 for N, HW, C, S in shapes)
    assert sum(K.BF16 in c["run"] for c in K.SE_CASES) >= 5


def test_abi_version_is_unchanged(lib):
    assert lib.sat_abi_version() == 23
