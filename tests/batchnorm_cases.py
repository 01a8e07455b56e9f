"""The shapes that pin every launch form of the training-mode BatchNorm kernels (csrc/encoder.hip), with the plan each was written for, and
the shapes of the max-pool test.

test_batchnorm_plan.py (no GPU) asserts that sat_bn_plan returns exactly these plans; test_gpu_batchnorm_forms.py runs the shapes.  When
bn_grid, the VPT thresholds or the tile-count thresholds are retuned the plans here are re-derived and, where a form is no longer reached,
the shape is changed until it is again: a mismatch fails, nothing is skipped.

A plan, as sat_bn_plan writes it (include/sat_hip.h):
    (form, CV, column blocks, row parts, rows per part | -1 interleaved, tiles, apply VPT, apply part length in rows)
form 0 = column-statistics pass, 1 = tile finish <8,8>, 2 = tile finish <4,16>, 3 = fused tile finalize, 4 = tile reduce + finalize pair.
The column pass: E = elements per 16-byte vector (4 fp32, 8 bf16), CV = the largest divisor of 256 up to C / E, RL = 256 / CV row lanes,
rows per part = max(ceil(rows / (512 (768 backward) / column blocks)), 8 RL).  The forward loop takes 4 RL rows per trip and leaves the
rest to a tail loop; the backward deals groups of UN RL rows (UN = 4 fp32, 2 bf16) round-robin to the parts and the last part takes the
ragged end.

kind "pass": sat_bn_train_fwd_t / sat_bn_train_bwd_t (statistics from a pass over the activation), in the storage types of `run`.
kind "tiles": sat_bn_train_fwd_tiles_bf16 / sat_bn_train_bwd_tiles_bf16 on tile statistics the test writes itself (bf16 only).
kind "resbn": sat_bn_train_fwd_tiles_bf16_resbn (forward only: the residual is raw and has its own BatchNorm).
"""

F32, BF16 = "fp32", "bf16"
VEC = {F32: 4, BF16: 8}          # elements per 16-byte vector

COLS, FINISH8, FINISH4, FUSED, PAIR = 0, 1, 2, 3, 4


def case(name, rows, C, run, why, kind="pass", tile_rows=0, vpt=2, onepass=1, relu=0, mask=False, residual=False, dres=None,
         stats_only=False, eval_mode=False, **plans):
    """relu 0 | 1 | 2; mask: the backward reads the sign mask (else the output tensor); residual: the forward adds one; dres: None | "write" |
    "acc"; stats_only: the forward is also called with y = NULL; eval_mode: the eval call runs on the shape too (with the residual if any);
    plans: one per storage type of `run`, dict(fwd=..., bwd=...)"""
    assert not mask or (relu and C % 8 == 0)
    assert relu != 2 or mask
    return dict(name=name, rows=rows, C=C, run=run, why=why, kind=kind, tile_rows=tile_rows, vpt=vpt, onepass=onepass, relu=relu, mask=mask,
                residual=residual, dres=dres, stats_only=stats_only, eval_mode=eval_mode, plans=plans)


def plan(fwd, bwd=None):
    return dict(fwd=fwd, bwd=bwd)


CASES = [
    # ---- statistics from a pass over the activation
    case("5x8", 5, 8, (F32, BF16), "row lanes mostly idle (RL = 128 / 256 for 5 rows), one part, the tail loop only",
         relu=1, mask=True, residual=True, dres="write", stats_only=True, eval_mode=True,
         fp32=plan((COLS, 2, 1, 1, 1024, 0, 1, 5), (COLS, 2, 1, 1, -1, 0, 1, 5)),
         bf16=plan((COLS, 1, 1, 1, 2048, 0, 1, 5), (COLS, 1, 1, 1, -1, 0, 1, 5))),
    case("1x8", 1, 8, (F32, BF16), "rows = 1: variance 0, the running variance takes the biased value, dx = 0",
         fp32=plan((COLS, 2, 1, 1, 1024, 0, 1, 1), (COLS, 2, 1, 1, -1, 0, 1, 1)),
         bf16=plan((COLS, 1, 1, 1, 2048, 0, 1, 1), (COLS, 1, 1, 1, -1, 0, 1, 1))),
    case("50x12", 50, 12, (F32,), "C / E = 3 -> CV = 2: the second column block has an idle vector column; backward reads the output tensor",
         relu=1, dres="acc", stats_only=True, eval_mode=True,
         fp32=plan((COLS, 2, 2, 1, 1024, 0, 1, 50), (COLS, 2, 2, 1, -1, 0, 1, 50))),
    case("50x24", 50, 24, (BF16,), "the same idle vector column in bf16 (C / E = 3)",
         relu=1, dres="acc", stats_only=True, eval_mode=True,
         bf16=plan((COLS, 2, 2, 1, 1024, 0, 1, 50), (COLS, 2, 2, 1, -1, 0, 1, 50))),
    case("70x2056", 70, 2056, (F32,), "514 vector columns: 3 column blocks, the last with 2 live columns; 9 row parts of 8 rows, the last has 6: tails only",
         relu=2, mask=True, residual=True, dres="write",
         fp32=plan((COLS, 256, 3, 9, 8, 0, 1, 70), (COLS, 256, 3, 9, -1, 0, 1, 70))),
    case("70x2064", 70, 2064, (BF16,), "258 vector columns: 2 column blocks, the last with 2 live columns; 9 row parts, the last has 6 rows",
         relu=2, mask=True, residual=True, dres="write",
         bf16=plan((COLS, 256, 2, 9, 8, 0, 1, 70), (COLS, 256, 2, 9, -1, 0, 1, 70))),
    case("16385x64", 16385, 64, (F32, BF16), "more than 64 row parts (129 fp32, 65 bf16), the last part is one row; ragged interleaved groups; VPT = 2 with an odd row count",
         relu=1, mask=True, residual=True, dres="acc",
         fp32=plan((COLS, 16, 1, 129, 128, 0, 2, 8193), (COLS, 16, 1, 129, -1, 0, 2, 8193)),
         bf16=plan((COLS, 8, 1, 65, 256, 0, 2, 8193), (COLS, 8, 1, 65, -1, 0, 2, 8193))),
    case("16385x64-vpt4", 16385, 64, (F32, BF16), "bn_vpt = 4 at its seam: parts of 4097 rows, the last has 4094",
         vpt=4, relu=2, mask=True,
         fp32=plan((COLS, 16, 1, 129, 128, 0, 4, 4097), (COLS, 16, 1, 129, -1, 0, 4, 4097)),
         bf16=plan((COLS, 8, 1, 65, 256, 0, 4, 4097), (COLS, 8, 1, 65, -1, 0, 4, 4097))),
    case("16383x16-vpt4", 16383, 16, (F32, BF16), "bn_vpt = 4 below 16384 rows falls back to VPT = 2; backward reads the output tensor",
         vpt=4, relu=1, residual=True, dres="write",
         fp32=plan((COLS, 4, 1, 32, 512, 0, 2, 8192), (COLS, 4, 1, 32, -1, 0, 2, 8192)),
         bf16=plan((COLS, 2, 1, 16, 1024, 0, 2, 8192), (COLS, 2, 1, 16, -1, 0, 2, 8192))),
    case("4100x512", 4100, 512, (F32,), "257 row parts of 16 rows, the last has 4: the finalize kernels' lane-strided loops make a fifth trip",
         fp32=plan((COLS, 128, 1, 257, 16, 0, 2, 2050), (COLS, 128, 1, 257, -1, 0, 2, 2050))),
    case("4100x1024", 4100, 1024, (BF16,), "257 row parts in bf16",
         bf16=plan((COLS, 128, 1, 257, 16, 0, 2, 2050), (COLS, 128, 1, 257, -1, 0, 2, 2050))),
    case("4095x16", 4095, 16, (F32, BF16), "one row below the VPT = 2 threshold",
         relu=1, mask=True, residual=True, dres="acc",
         fp32=plan((COLS, 4, 1, 8, 512, 0, 1, 4095), (COLS, 4, 1, 8, -1, 0, 1, 4095)),
         bf16=plan((COLS, 2, 1, 4, 1024, 0, 1, 4095), (COLS, 2, 1, 4, -1, 0, 1, 4095))),
    case("4097x16", 4097, 16, (F32, BF16), "VPT = 2 with an odd row count: the second half is one row short (the guard idx < totalv)",
         relu=1, mask=True, residual=True, dres="acc",
         fp32=plan((COLS, 4, 1, 9, 512, 0, 2, 2049), (COLS, 4, 1, 9, -1, 0, 2, 2049)),
         bf16=plan((COLS, 2, 1, 5, 1024, 0, 2, 2049), (COLS, 2, 1, 5, -1, 0, 2, 2049))),
    case("4097x16-vpt1", 4097, 16, (F32, BF16), "bn_vpt = 1 above the threshold keeps one vector per thread",
         vpt=1, relu=2, mask=True, dres="write",
         fp32=plan((COLS, 4, 1, 9, 512, 0, 1, 4097), (COLS, 4, 1, 9, -1, 0, 1, 4097)),
         bf16=plan((COLS, 2, 1, 5, 1024, 0, 1, 4097), (COLS, 2, 1, 5, -1, 0, 1, 4097))),
    # ---- the projection-shortcut form (forward only; bf16, tile statistics)
    case("resbn-4097x16", 4097, 16, (BF16,), "projection-shortcut form with VPT = 2, odd row count", kind="resbn", tile_rows=64, relu=1, mask=True, residual=True,
         bf16=plan((FINISH8, 8, 2, 0, 0, 65, 2, 2049))),
    case("resbn-50x24", 50, 24, (BF16,), "projection-shortcut form with VPT = 1", kind="resbn", tile_rows=8, relu=2, mask=True, residual=True,
         bf16=plan((FINISH8, 8, 3, 0, 0, 7, 1, 50))),
    case("resbn-16385x64-vpt4", 16385, 64, (BF16,), "the projection-shortcut form has no VPT = 4: bn_vpt = 4 runs VPT = 2", kind="resbn", tile_rows=16, vpt=4,
         relu=1, mask=True, residual=True,
         bf16=plan((FINISH4, 4, 16, 0, 0, 1025, 2, 8193))),
]


def _tiles(ntiles, rows, tile_rows, C, onepass, form_f, form_b, cv, **kw):
    """a tile case: forward and backward of the same shape.  The one-launch forms leave no partials; the pair's parts are derived below."""
    name = "tiles%d-%dx%d%s" % (ntiles, rows, C, "" if onepass else "-twopass")
    assert -(-rows // tile_rows) == ntiles
    vptn = 2 if rows >= 4096 else 1

    def p(form):
        if form != PAIR:
            return (form, {FINISH8: 8, FINISH4: 4, FUSED: 32}[form], -(-C // {FINISH8: 8, FINISH4: 4, FUSED: 32}[form]), 0, 0, ntiles, vptn, -(-rows // vptn))
        np_, per = kw["pair"]
        return (PAIR, 32, -(-C // 32), np_, per, ntiles, vptn, -(-rows // vptn))
    opts = dict(relu=1, mask=True, residual=True, dres="acc") if C == 8 else dict(dres="write")
    return case(name, rows, C, (BF16,), kw["why"], kind="tiles", tile_rows=tile_rows, onepass=onepass, stats_only=kw.get("stats_only", False),
                bf16=plan(p(form_f), p(form_b)), **opts)


# tile statistics of the test's own making, forward (mode 0) and backward (mode 1), C in {8, 40}
TILE_SHAPES = [
    # ntiles, rows, tile_rows, onepass, forward form, backward form, extra
    (1, 5, 8, 1, FINISH8, FINISH8, dict(why="one ragged tile: 31 of 32 tile lanes add nothing", stats_only=True)),
    (31, 61, 2, 1, FINISH8, FINISH8, dict(why="31 tiles: one short of the tile lanes of finish <8,8>")),
    (256, 767, 3, 1, FINISH8, FINISH8, dict(why="256 tiles: the last shape of finish <8,8>, every lane full")),
    (257, 513, 2, 1, FINISH4, FINISH4, dict(why="257 tiles: the first shape of finish <4,16>")),
    (263, 2100, 8, 1, FINISH4, FINISH4, dict(why="263 tiles with a ragged last tile")),
    (1025, 1025, 1, 1, FINISH4, FINISH4, dict(why="1025 tiles: one past a full trip of 64 lanes x 16 loads")),
    (2048, 4095, 2, 1, FINISH4, FINISH4, dict(why="2048 tiles: the last shape of finish <4,16>, two full trips")),
    (2050, 2050, 1, 1, PAIR, PAIR, dict(why="2050 tiles: above the finish kernels, the reduce + finalize pair", stats_only=True)),
    (256, 767, 3, 0, FUSED, PAIR, dict(why="bn_onepass = 0 at 256 tiles: fused finalize forward, the pair backward")),
    (257, 513, 2, 0, PAIR, PAIR, dict(why="bn_onepass = 0 at 257 tiles: the pair in both directions")),
]
# the pair's (parts, tiles per part): min(ceil(tiles / 64), row parts of the column pass), then evened out.  The column pass of C = 8 has
# CV = 1 and parts of at least 2048 rows (2, 1, 1 parts for 2050, 767, 513 rows), that of C = 40 has CV = 4 and parts of at least 512 rows (5, 2, 2)
_PAIR = {(2050, 8): (2, 1025), (2050, 40): (5, 410), (767, 8): (1, 256), (767, 40): (2, 128), (513, 8): (1, 257), (513, 40): (2, 129)}
for _nt, _rows, _tr, _op, _ff, _fb, _kw in TILE_SHAPES:
    for _C in (8, 40):
        CASES.append(_tiles(_nt, _rows, _tr, _C, _op, _ff, _fb, None, pair=_PAIR.get((_rows, _C)), **_kw))

# max pool 3x3 / 2: (N, H, W, C); bf16 C = 12 takes the 4-channel form, every other the 16-byte form
POOL_SHAPES = [(2, 11, 12, 8), (2, 11, 12, 12), (2, 11, 12, 16), (1, 7, 9, 8), (1, 7, 9, 12), (1, 7, 9, 16)]


def pool_form(dtype, C):
    return "vec16" if C % VEC[dtype] == 0 else "c4"


def query(lib, backward, dtype, rows, C, tile_rows=0, resbn=0):
    """(status, plan tuple) of sat_bn_plan under the library's current switches"""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    rc = lib.sat_bn_plan(int(backward), int(dtype == BF16), rows, C, tile_rows, resbn, out)
    return rc, tuple(out)


def set_switches(lib, vpt=2, onepass=1):
    assert lib.sat_debug_option(b"bn_vpt", vpt) == 0 and lib.sat_debug_option(b"bn_onepass", onepass) == 0


def case_plans(lib, c, dtype):
    """the library's plans for a case (the switches must be set): dict(fwd=..., bwd=... | None)"""
    tr, rb = c["tile_rows"], int(c["kind"] == "resbn")
    rc, f = query(lib, 0, dtype, c["rows"], c["C"], tr, rb)
    assert rc == 0, lib.sat_last_error()
    if c["kind"] == "resbn":
        return dict(fwd=f, bwd=None)
    rc, b = query(lib, 1, dtype, c["rows"], c["C"], tr, 0)
    assert rc == 0, lib.sat_last_error()
    return dict(fwd=f, bwd=b)


def partial_doubles(p, C):
    """doubles of scratch a plan's partials take: two [parts][C] arrays"""
    return 2 * p[3] * C
