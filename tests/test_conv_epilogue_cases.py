"""CPU: the case table of the convolution epilogues (conv_epilogue_cases.py) is well formed - unique ids, geometries conv_geom accepts, every
form pinned, tile heights that agree with the kernel names, every case inside the cost cap - and its inputs would SHOW the faults the GPU test
is there for.  On the float64 reference of every case (rounded to bf16: the values a correct kernel stores), for every tile:
  - dropping the tile's last row,
  - moving the tile boundaries by one row,
  - reading the mask one byte off
each move at least one statistic of the tile by more than 4x the tolerance the GPU test allows it (for a joined gradient without statistics
the mask moves at least one element of every tile by more than 4x its tolerance).  So none of these can hide inside the bound.  One
exception, by construction: every bit of the last row is set and 0xFF lies behind the mask, so a last tile that is that row alone reads the
same bits one byte further on."""
import collections

import torch

import batchnorm_ref as B
import conv_epilogue_cases as T
import conv_ref as R
from test_conv_cases import conv_geom_accepts

#: the scope names the table must reach: every launch form that can carry an epilogue
REQUIRED_NAMES = [
    "gemm_bf16_conv_fwd_64x64_b", "gemm_bf16_conv_fwd_128x128_b", "gemm_bf16_nt_64x64_b",
    "gemm_glds_conv_fwd_64x64", "gemm_glds_conv_fwd_128x64", "gemm_glds_conv_fwd_128x128", "gemm_glds_nt_64x64", "gemm_glds_nt_128x64",
    "gemm_bf16_conv_dgrad_64x64_b", "gemm_bf16_conv_dgrad_128x128_b", "gemm_bf16_nn_64x64_b",
    "gemm_glds_conv_dgrad_64x64", "gemm_glds_conv_dgrad_128x64", "gemm_glds_conv_dgrad_128x128", "gemm_glds_nn_64x64", "gemm_glds_nn_128x64",
]


def test_ids_are_unique_and_geometries_pass_conv_geom():
    ids = collections.Counter(c["id"] for c in T.TABLE)
    assert not [i for i, n in ids.items() if n > 1]
    assert T.BY_ID.keys() == ids.keys()
    for c in T.TABLE:
        g = c["g"]
        assert c["kind"] in ("fwd", "bnstats", "fused") and conv_geom_accepts(g, 8), c["id"]
        assert g["stride_w"] == 0 and g["stride"] in (1, 2), c["id"]
        assert c["kind"] == "fwd" or g["stride"] == 1, c["id"]          # a stride-2 data gradient runs by parity classes: declined, not a case
        assert not (c["accumulate"] and c["kind"] != "bnstats") and not (c["add_mask"] and c["kind"] != "fused"), c["id"]
        assert not (c["relu_mask"] and not c["stats"]) and (c["stats"] or c["kind"] == "fused"), c["id"]
    for g in (T.S2_GEOM, T.OFF_GEOM_DGRAD, T.OFF_GEOM_FWD):
        assert conv_geom_accepts(g, 8)
    assert T.S2_GEOM["stride"] == 2


def test_every_form_and_scope_name_is_reached():
    reached = {n for c in T.TABLE for n in c["names"]}
    assert not [n for n in REQUIRED_NAMES if n not in reached]
    assert not [n for n in reached if n not in REQUIRED_NAMES]
    assert {c["form"] for c in T.TABLE} == set(T.FORMS)
    by_kind = lambda kind, **kw: {c["names"][0] for c in T.TABLE if c["kind"] == kind and all(c[k] == v for k, v in kw.items())}
    # every backward form with and without the ReLU mask; the 64-row forms also accumulating
    assert by_kind("bnstats", relu_mask=False) == by_kind("bnstats", relu_mask=True) == {n for n in REQUIRED_NAMES if "dgrad" in n or "_nn_" in n}
    assert by_kind("bnstats", accumulate=True) == {n for n in REQUIRED_NAMES if ("dgrad" in n or "_nn_" in n) and "64x64" in n}
    # the joined gradient on its five forms, each with add_mask NULL / given x statistics off / on
    want = {"gemm_bf16_conv_dgrad_64x64_b", "gemm_glds_conv_dgrad_64x64", "gemm_glds_nn_64x64", "gemm_glds_conv_dgrad_128x64", "gemm_glds_conv_dgrad_128x128"}
    for am in (False, True):
        for st in (False, True):
            assert by_kind("fused", add_mask=am, stats=st) == want


def test_tile_rows_agree_with_the_kernel_names_and_the_geometries_with_their_comments():
    for c in T.TABLE:
        assert len(c["names"]) == 1, c["id"]
        assert c["tile_rows"] == (T.tile_rows_of(c["names"][0]) if c["stats"] else 0), c["id"]
    assert [T.tile_rows_of(n) for n in ("gemm_glds_conv_fwd_128x64", "gemm_bf16_nn_64x64_b", "gemm_glds_conv_dgrad_128x128")] == [128, 64, 128]
    t = T.BY_ID
    dims = lambda cid: T.gemm_dims(t[cid])
    assert dims("fwd-reg64") == (162, 72, 72) and dims("fwd-glds64-k136") == (65, 136, 576) and dims("fwd-glds64-onetile")[0] == 64
    assert dims("fwd-glds64-k8")[1] == 8 and dims("bn-glds64-c8")[1] == 8
    assert dims("fwd-glds128x64-tall") == (8281, 64, 576) and 8281 % 128 == 89
    assert dims("fwd-glds128x64-narrowed") == (24843, 128, 576) and -(-24843 // 128) == 195
    assert dims("fwd-glds128x128") == (8100, 1024, 1728) == dims("bn-glds128x128") == dims("join-glds128x128-mask-stats")
    assert dims("fwd-reg128x128") == (24642, 128, 392) == dims("bn-reg128x128") and -(-24642 // 128) == 193
    assert dims("bn-reg64") == (162, 72, 72) and dims("bn-glds128x64-narrowed") == (24843, 128, 576)
    # the request rule itself, restated: 128-wide exactly for the cases that say so
    for c in T.TABLE:
        M, N, Kr = T.gemm_dims(c)
        tiles = -(-M // 128) * -(-N // 128)
        wide = tiles >= 192 and M >= 128 and N >= 128 and not (tiles < 512 and Kr <= 256)
        assert wide == (c["names"][0] in (T.REG_FWD128, T.REG_DG128, T.GL_FWD128, T.GL_DG128) or "narrowed" in c["id"]), c["id"]


def test_cost_cap():
    for c in T.TABLE:
        M, N, K = T.gemm_dims(c)
        assert 2.0 * M * N * K <= T.COST_CAP, c["id"]
        assert T.largest_tensor_bytes(c) <= T.BYTES_CAP, c["id"]
        assert M * N * 2 <= T.BYTES_CAP, c["id"]          # bn_x, add_src, the result


def test_inputs_are_as_the_header_says():
    for c in T.TABLE:
        if c["kind"] == "fwd":
            continue
        s = T.inputs(c)
        M, N = s["M"], s["N"]
        last = T.last_rows(M)
        assert last[M - 1] and int(last.sum()) == M // 64 + (1 if M % 64 else 0), c["id"]
        for name in ("bn_x", "add_src"):
            assert torch.equal(R.bf16_round(s[name]), s[name]) and float(s[name][last].abs().min()) >= 1.5 and float(s[name][:, -1].abs().min()) >= 1.5, c["id"]
        assert s["relu_bits"][last].all() and s["add_bits"][last].all(), c["id"]
        for bits in (s["relu_bits"], s["add_bits"]):
            assert 0.4 < float(bits[~last].float().mean()) < 0.6, c["id"]
        assert 0.4 < float((s["relu_bits"] ^ s["add_bits"])[~last].float().mean()) < 0.6, c["id"]          # independent draws
        assert s["mean"].unique().numel() == N and s["invstd"].unique().numel() == N, c["id"]
        assert float(s["mean"].abs().max()) <= 0.5 and 0.5 <= float(s["invstd"].min()) and float(s["invstd"].max()) <= 2.0, c["id"]


def test_stats_ref_agrees_with_batchnorm_ref():
    """the helper the GPU test measures against, against batchnorm_ref's tile_sums / backward_tiles (which round to float32)"""
    for cid in ("fwd-reg64", "fwd-glds64-k136", "bn-reg64-relu", "bn-glds64-c136", "join-glds64-mask-stats"):
        c = T.BY_ID[cid]
        s = T.inputs(c)
        v = R.bf16_round(T.expected(c, s)[0]).to(T.F64)
        ref, tol = T.stats_ref(c, s, v, c["tile_rows"])
        if c["kind"] == "fwd":
            want = B.tile_sums(v, c["tile_rows"])
        else:
            mean, invstd = s["mean"].to(T.F64), s["invstd"].to(T.F64)
            gv = torch.where(s["relu_bits"], v, torch.zeros((), dtype=T.F64)) if c["relu_mask"] else v
            want = B.backward_tiles(gv, (s["bn_x"].to(T.F64) - mean) * invstd, c["tile_rows"])
        assert ref.shape == want.shape == tol.shape
        assert bool(((ref - want.to(T.F64)).abs() <= 2.0 ** -23 * ref.abs() + 1e-30).all()), cid
        assert bool((tol > 0).all()), cid


def _moved(a, b, tol):
    """per tile: does any statistic differ by more than 4x its tolerance"""
    return ((a - b).abs() > 4.0 * tol).flatten(1).any(1)


def test_every_case_would_show_a_dropped_row_a_moved_boundary_and_a_mask_read_one_byte_off():
    for c in T.TABLE:
        s = T.inputs(c)
        M = s["M"]
        ref, prod = T.expected(c, s)
        v = R.bf16_round(ref).to(T.F64)
        tr = c["tile_rows"] or T.tile_rows_of(c["names"][0])
        nt = -(-M // tr)
        tile_last = torch.zeros(M, dtype=torch.bool)
        tile_last[[min(M, (t + 1) * tr) - 1 for t in range(nt)]] = True
        if c["stats"]:
            st, tol = T.stats_ref(c, s, v, tr)
            assert st.shape == (nt, s["N"], 2)
            dropped = T.stats_ref(c, s, v, tr, drop_rows=tile_last)[0]
            assert bool(_moved(st, dropped, tol).all()), "%s: a dropped last row hides in tile(s) %s" % (c["id"], torch.nonzero(~_moved(st, dropped, tol)).flatten().tolist())
            shifted = T.stats_ref(c, s, v, tr, shift=1)[0]
            assert bool(_moved(st, shifted, tol).all()), "%s: a boundary one row off hides" % c["id"]
            if nt > 1:          # the wrong tile height altogether (64 for 128 and the reverse): the first tile alone shows it
                other = T.stats_ref(c, s, v, 192 - tr)[0]
                assert bool(_moved(st[:1], other[:1], tol[:1]).all()), c["id"]
            if c["relu_mask"]:
                off = T.stats_ref(c, s, v, tr, relu_bits=T.shifted_bits(s["relu_bits"]))[0]
                # (a last tile that is the last row alone has every bit set and 0xFF behind it: one byte further reads the same there)
                seen = _moved(st, off, tol) | torch.tensor([t == nt - 1 and M - t * tr == 1 for t in range(nt)])
                assert bool(seen.all()), "%s: bn_relu_mask read one byte off hides" % c["id"]
        if c["add_mask"]:
            ref_off = T.expected(c, s, add_bits=T.shifted_bits(s["add_bits"]))[0]
            big = ((ref_off - ref).abs() > 4.0 * T.element_tol(c, s, ref, prod)).any(1)
            per_tile = torch.zeros(nt).index_add_(0, T.tile_of_rows(M, tr), big.float())
            if M - (nt - 1) * tr == 1:
                per_tile[nt - 1] = 1          # (the same exception)
            assert bool((per_tile > 0).all()), "%s: add_mask read one byte off hides" % c["id"]
        if c["kind"] == "fused":          # the old contents of dx must not be needed: the reference never reads them
            assert not c["accumulate"]
