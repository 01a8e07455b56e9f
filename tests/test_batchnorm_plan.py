"""CPU: the launch plan of the training-mode BatchNorm kernels (sat_bn_plan: host arithmetic only, no device is touched).

bn_train_fwd_t, bn_train_bwd_t, the two apply launchers and sat_bn_scratch_bytes of csrc/encoder.hip take the statistics form, the grid
of the column pass and the apply kernel's vectors per thread from the function this query returns, so what is asserted here is what runs:
every case of tests/batchnorm_cases.py lands on the plan it was written for (test_gpu_batchnorm_forms.py then runs it), the table reaches
every form, and the scratch that sat_bn_scratch_bytes reports holds the partials of every plan."""
import ctypes
import itertools

import pytest

import batchnorm_cases as B


@pytest.fixture(scope="module")
def lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    handle = _lib.lib()
    yield handle
    B.set_switches(handle)


@pytest.fixture(autouse=True)
def default_switches(lib):
    B.set_switches(lib)
    yield
    B.set_switches(lib)          # bn_vpt = 2, bn_onepass = 1: no later test sees them changed


@pytest.mark.parametrize("c", B.CASES, ids=lambda c: c["name"])
def test_case_table_lands_on_the_plan_it_was_written_for(lib, c):
    assert set(c["run"]) == set(c["plans"])
    B.set_switches(lib, c["vpt"], c["onepass"])
    for dtype in c["run"]:
        assert c["C"] % B.VEC[dtype] == 0
        assert B.case_plans(lib, c, dtype) == c["plans"][dtype], "%s %s (%s)" % (c["name"], dtype, c["why"])


def _forms_reached():
    """what the table is for, read off its own plans and options"""
    seen = set()
    for c in B.CASES:
        rows, C = c["rows"], c["C"]
        for dtype in c["run"]:
            E = B.VEC[dtype]
            for d, p in c["plans"][dtype].items():
                if p is None:
                    continue
                form, CV, colblocks, parts, rows_per, tiles, vpt, part_rows = p
                shortcut = c["kind"] == "resbn"
                seen.add(("apply", "resbn" if shortcut else d, dtype, vpt, "short last part" if rows % vpt else "even"))
                if vpt == 2 and c["vpt"] == 4:
                    seen.add(("apply", "vpt 4 falls back to 2", "resbn" if shortcut else d, dtype))
                if vpt == 1 and c["vpt"] == 1 and rows >= 4096:
                    seen.add(("apply", "bn_vpt = 1", d, dtype))
                if form != B.COLS:
                    seen.add(("tiles", form, d, "onepass" if c["onepass"] else "twopass"))
                    seen.add(("tile count", form, d, tiles))
                    if form == B.PAIR and tiles > 2048:
                        seen.add(("tiles", "pair above 2048 tiles", d))
                    continue
                seen.add(("cols", d, dtype))
                CVT, RL = C // E, 256 // CV
                UN = 4 if (d == "fwd" or E == 4) else 2
                if CVT % CV:
                    seen.add(("cols", "idle vector columns", d, dtype))
                if CVT > 256 and colblocks > 1:
                    seen.add(("cols", "several column blocks", d, dtype))
                if d == "fwd" and parts > 1 and rows - (parts - 1) * rows_per < 4 * RL:
                    seen.add(("cols", "a part that holds only a tail", dtype))
                if d == "fwd" and parts == 1 and rows < 4 * RL:
                    seen.add(("cols", "one part, tail loop only", dtype))
                if parts > 64:
                    seen.add(("cols", "more than 64 parts", d, dtype))
                if parts > 256:
                    seen.add(("cols", "more than 256 parts", d, dtype))
                if d == "bwd" and rows_per == -1 and parts > 1 and rows % (UN * RL) and rows // (UN * RL) % parts:
                    seen.add(("cols", "ragged interleaved groups", dtype))
            if c["kind"] == "pass":
                seen.add(("relu", c["relu"], dtype))
                seen.add(("backward reads", "mask" if c["mask"] else "output", dtype) if c["relu"] else ("relu", 0, dtype))
                seen.add(("residual", c["residual"], dtype))
                seen.add(("dres", c["dres"], dtype))
                if c["stats_only"]:
                    seen.add(("y = NULL", dtype))
                if c["eval_mode"]:
                    seen.add(("eval", "residual" if c["residual"] else "plain", dtype))
                if rows == 1:
                    seen.add(("rows = 1", dtype))
            elif c["stats_only"]:
                seen.add(("y = NULL", "tiles"))
    for shape in B.POOL_SHAPES:
        for dtype in (B.F32, B.BF16):
            seen.add(("maxpool", dtype, B.pool_form(dtype, shape[3])))
    return seen


def test_case_table_reaches_every_form():
    seen = _forms_reached()
    for dtype in (B.F32, B.BF16):
        # apply kernels with several row-parts per thread, the last part short; both sides of the threshold; the switch settings
        for d in ("fwd", "bwd"):
            assert ("apply", d, dtype, 2, "short last part") in seen
            assert ("apply", d, dtype, 4, "short last part") in seen
            assert ("apply", d, dtype, 1, "short last part") not in seen and ("apply", d, dtype, 1, "even") in seen
            assert ("apply", "vpt 4 falls back to 2", d, dtype) in seen
            assert ("apply", "bn_vpt = 1", d, dtype) in seen
            # bf16 (and fp32) storage through the column pass, statistics and apply, forward and backward (UNROLL_BWD_BF16 = 2)
            assert ("cols", d, dtype) in seen
            # bn_colstats_kernel grids
            assert ("cols", "idle vector columns", d, dtype) in seen
            assert ("cols", "several column blocks", d, dtype) in seen
            assert ("cols", "more than 64 parts", d, dtype) in seen
            assert ("cols", "more than 256 parts", d, dtype) in seen
        assert ("cols", "a part that holds only a tail", dtype) in seen
        assert ("cols", "one part, tail loop only", dtype) in seen
        assert ("cols", "ragged interleaved groups", dtype) in seen
        # other options of the calls
        for relu in (0, 1, 2):
            assert ("relu", relu, dtype) in seen
        assert ("backward reads", "mask", dtype) in seen and ("backward reads", "output", dtype) in seen
        assert ("residual", True, dtype) in seen and ("residual", False, dtype) in seen
        for dres in (None, "write", "acc"):
            assert ("dres", dres, dtype) in seen
        assert ("y = NULL", dtype) in seen
        assert ("eval", "residual", dtype) in seen and ("eval", "plain", dtype) in seen
        assert ("rows = 1", dtype) in seen
    # the projection-shortcut form
    assert ("apply", "resbn", B.BF16, 2, "short last part") in seen and ("apply", "resbn", B.BF16, 1, "even") in seen
    assert ("apply", "vpt 4 falls back to 2", "resbn", B.BF16) in seen
    # the tile-statistics reducers, mode 0 and mode 1
    for d in ("fwd", "bwd"):
        for n in (1, 31, 256):
            assert ("tile count", B.FINISH8, d, n) in seen          # finish <8,8> at its edges
        for n in (257, 263, 1025, 2048):
            assert ("tile count", B.FINISH4, d, n) in seen          # finish <4,16>
        assert ("tiles", "pair above 2048 tiles", d) in seen and ("tile count", B.PAIR, d, 2050) in seen
        assert ("tiles", B.PAIR, d, "twopass") in seen and ("tile count", B.PAIR, d, 257) in seen
    assert ("tiles", B.FUSED, "fwd", "twopass") in seen and ("tile count", B.FUSED, "fwd", 256) in seen
    assert ("tile count", B.PAIR, "bwd", 256) in seen          # (the backward has no fused finalize: 256 tiles with bn_onepass = 0 take the pair)
    assert ("y = NULL", "tiles") in seen
    # sat_maxpool3x3s2_*_t: the 16-byte kernel in both types, the 4-channel fallback in bf16
    assert ("maxpool", B.BF16, "vec16") in seen and ("maxpool", B.BF16, "c4") in seen and ("maxpool", B.F32, "vec16") in seen


def _sweep():
    shapes = [(c["rows"], c["C"]) for c in B.CASES]
    for rows, C in itertools.product((1, 2, 7, 63, 64, 65, 511, 513, 2047, 2049, 4096, 16385, 100352, 802816), (4, 8, 12, 24, 40, 64, 1024, 1028, 2048, 2056, 2064)):
        shapes.append((rows, C))
    return shapes


def test_scratch_holds_the_partials_of_every_plan(lib):
    checked = 0
    for (rows, C), vpt, onepass in itertools.product(_sweep(), (1, 2, 4), (0, 1)):
        B.set_switches(lib, vpt, onepass)
        have = lib.sat_bn_scratch_bytes(rows, C)
        assert have > 0
        for dtype, backward in itertools.product((B.F32, B.BF16), (0, 1)):
            if C % B.VEC[dtype]:
                rc, p = B.query(lib, backward, dtype, rows, C)
                assert rc != 0 and p == (0,) * 8
                continue
            for tile_rows in ((0,) if dtype == B.F32 else (0, 1, 2, 8, 64, 256)):
                rc, p = B.query(lib, backward, dtype, rows, C, tile_rows)
                assert rc == 0, lib.sat_last_error()
                form, CV, colblocks, parts, rows_per, tiles, v, part_rows = p
                assert have >= 8 * B.partial_doubles(p, C), "%dx%d %s: %d bytes of scratch for %d partials per channel" % (rows, C, dtype, have, parts)
                assert v in (1, 2, 4) and v <= max(vpt, 1) and part_rows == -(-rows // v)
                if form == B.COLS:
                    assert 256 % CV == 0 and CV <= C // B.VEC[dtype] and colblocks * CV >= C // B.VEC[dtype] > (colblocks - 1) * CV
                    assert parts >= 1 and (rows_per == -1 or (parts - 1) * rows_per < rows <= parts * rows_per)
                else:
                    assert tiles == -(-rows // tile_rows) and colblocks * CV >= C
                    assert (form == B.PAIR) == (parts > 0) and (parts == 0 or (parts - 1) * rows_per < tiles <= parts * rows_per)
                checked += 1
    assert checked > 2000


def test_every_case_fits_the_scratch_in_both_types_and_directions(lib):
    for c in B.CASES:
        B.set_switches(lib, c["vpt"], c["onepass"])
        have = lib.sat_bn_scratch_bytes(c["rows"], c["C"])
        for dtype, backward in itertools.product((B.F32, B.BF16), (0, 1)):
            if c["C"] % B.VEC[dtype]:
                continue
            for tile_rows in {0, c["tile_rows"] if dtype == B.BF16 else 0}:
                rc, p = B.query(lib, backward, dtype, c["rows"], c["C"], tile_rows)
                assert rc == 0 and have >= 8 * B.partial_doubles(p, c["C"]), (c["name"], dtype, backward, p, have)


def test_plan_argument_validation(lib):
    out = (ctypes.c_int64 * 8)(*([7] * 8))
    assert lib.sat_bn_plan(0, 0, 50, 12, 0, 0, out) == 0 and tuple(out) == (B.COLS, 2, 2, 1, 1024, 0, 1, 50)
    bad = [(0, 0, 50, 6, 0, 0), (0, 0, 50, 0, 0, 0), (0, 0, 50, -8, 0, 0),          # C % 4, C <= 0
           (0, 1, 50, 12, 0, 0), (1, 1, 50, 4, 0, 0),                               # C % 8 in bf16
           (0, 0, 0, 8, 0, 0), (1, 0, -5, 8, 0, 0),                                 # rows
           (0, 1, 50, 8, -1, 0), (0, 0, 50, 8, 8, 0), (1, 0, 50, 8, 8, 0),          # tile_rows < 0; tile statistics in fp32
           (0, 1, 50, 8, 0, 1), (1, 1, 50, 8, 8, 1), (0, 0, 50, 8, 0, 1),           # the projection shortcut without tiles / in the backward
           (2, 0, 50, 8, 0, 0), (-1, 0, 50, 8, 0, 0), (0, 2, 50, 8, 0, 0), (0, -1, 50, 8, 0, 0)]          # direction, dtype
    for args in bad:
        out[:] = [7] * 8
        assert lib.sat_bn_plan(*args, out) != 0, args
        assert tuple(out) == (0,) * 8
        assert lib.sat_last_error()
    assert lib.sat_bn_plan(0, 0, 50, 8, 0, 0, None) != 0 and b"null" in lib.sat_last_error()
    # the scratch query keeps answering 0 bytes for what no call accepts
    for rows, C in ((0, 8), (-1, 8), (5, 0), (5, 6), (5, -4)):
        assert lib.sat_bn_scratch_bytes(rows, C) == 0, (rows, C)
    assert lib.sat_bn_scratch_bytes(5, 12) > 0          # fp32 accepts C = 12


def test_abi_version_is_unchanged(lib):
    assert lib.sat_abi_version() == 23
