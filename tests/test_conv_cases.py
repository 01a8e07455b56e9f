"""CPU: the case table of the convolution gather forms (conv_cases.py) is well formed - unique ids, geometries that conv_geom
(csrc/encoder.hip) accepts, every scope name of the list below expected by at least one case (a form cannot drop out of the table
unnoticed), every form of the doc pinned, and every case inside the cost cap."""
import collections

import conv_cases as T
import conv_ref as R

#: the scope names the table must reach (the shipped launch forms of the three gathering kernel families and the two hand-offs)
REQUIRED_NAMES = [
    "gemm_f32_conv_fwd_64x64", "gemm_f32_conv_fwd_128x128", "gemm_f32_conv_dgrad_64x64", "gemm_f32_conv_wgrad_64x64", "gemm_f32_nn_64x64",
    "gemm_bf16_conv_fwd_64x64_b", "gemm_bf16_conv_dgrad_64x64_b", "gemm_bf16_conv_wgrad_64x64_b", "gemm_bf16_nn_64x64_b",
    "gemm_glds_conv_fwd_64x64", "gemm_glds_conv_fwd_128x64", "gemm_glds_conv_fwd_128x128",
    "gemm_glds_conv_dgrad_64x64", "gemm_glds_conv_dgrad_128x64", "gemm_glds_nn_128x64",
    "gemm_glds_conv_wgrad_64x64", "gemm_glds_conv_wgrad_128x128", "gemm_wgrad3x3",
]


def conv_geom_accepts(g, vec):
    """conv_geom's own conditions"""
    if not (g["N"] > 0 and g["H"] > 0 and g["W"] > 0 and g["C"] > 0 and g["K"] > 0 and g["R"] > 0 and g["S"] > 0 and g["stride"] > 0 and g["pad"] >= 0):
        return False
    sw = g["stride_w"] if (g["stride_w"] > 0 and g["stride_w"] != g["stride"]) else 0
    P = (g["H"] + 2 * g["pad"] - g["R"]) // g["stride"] + 1
    Q = (g["W"] + 2 * g["pad"] - g["S"]) // (sw or g["stride"]) + 1
    return P > 0 and Q > 0 and g["C"] % vec == 0 and g["K"] % vec == 0 and (P, Q) == R.out_hw(g)


def test_ids_are_unique():
    ids = collections.Counter(c["id"] for c in T.TABLE)
    assert not [i for i, n in ids.items() if n > 1]
    assert T.BY_ID.keys() == ids.keys()


def test_geometries_pass_conv_geom():
    for c in T.TABLE:
        assert c["op"] in ("fwd", "dgrad", "wgrad") and c["dt"] in ("f32", "bf16"), c["id"]
        assert conv_geom_accepts(c["g"], 8 if c["dt"] == "bf16" else 4), c["id"]
        assert c["names"] == sorted(c["names"]) and c["names"], c["id"]
        # stride_w is a bf16 forward / filter-gradient argument: every other call refuses it (test_gemm_validation.py)
        if c["g"]["stride_w"] not in (0, c["g"]["stride"]):
            assert c["dt"] == "bf16" and c["op"] in ("fwd", "wgrad"), c["id"]
        assert not (c["accumulate"] and c["op"] != "dgrad") and not (c["bias"] and c["op"] != "fwd"), c["id"]


def test_every_required_scope_name_and_form_is_reached():
    reached = {n for c in T.TABLE for n in c["names"]}
    assert not [n for n in REQUIRED_NAMES if n not in reached]
    assert not [n for n in reached if n not in REQUIRED_NAMES]          # a name nobody listed: extend the list above
    assert {c["form"] for c in T.TABLE} == set(T.FORMS)


def test_the_cases_the_doc_promises_are_there():
    t = T.BY_ID
    count = lambda cid: len(t[cid]["names"])
    # parity classes: four launches; H = 1 leaves two; a 1x1 / pad 0 leaves one under accumulate
    for fam in ("reg", "glds"):
        assert count("dgrad-%s-s2-3x3" % fam) == 4 and count("dgrad-%s-s2-h1" % fam) == 2
        assert count("dgrad-%s-s2-1x1" % fam) == 4 and count("dgrad-%s-s2-1x1-acc" % fam) == 1
    # every non-poisoned data-gradient case has its accumulate twin
    for c in T.TABLE:
        if c["op"] == "dgrad" and not c["poison"] and not c["accumulate"]:
            assert t[c["id"] + "-acc"]["accumulate"] and t[c["id"] + "-acc"]["g"] == c["g"], c["id"]
    # pixel counts: exactly one tile, and not a multiple of the tile height
    assert T.gemm_dims(t["fwd-glds-onetile"])[0] == 64 and T.gemm_dims(t["fwd-glds-3x3"])[0] % 64 != 0
    # k-tiles of 64 per reduction on the direct-to-LDS forward: 1, 2 and more
    assert [T.gemm_dims(t[i])[2] // 64 for i in ("fwd-glds-1x1s2", "fwd-glds-1x1s2-c128", "fwd-glds-c192")] == [1, 2, 27]
    # the split whose last chunk is shorter: 65 k-tiles over 8 splits of 9
    assert T.gemm_dims(t["wgrad-glds-128x128-short-last"])[2] == 65 * 64
    # register-staged filter gradients: N*P*Q % 64 != 0, or stride_w, or R*S > 32
    for c in T.TABLE:
        if c["op"] == "wgrad" and c["names"] == [T.REG_WG]:
            g = c["g"]
            assert T.gemm_dims(c)[2] % 64 != 0 or g["stride_w"] or g["R"] * g["S"] > 32, c["id"]
    for fam in ("f32", "reg", "glds"):
        assert sum(1 for c in T.TABLE if c["poison"] and c["id"].split("-")[1] == fam) >= 1


def test_cost_cap():
    worst = max(T.TABLE, key=lambda c: 2.0 * T.gemm_dims(c)[0] * T.gemm_dims(c)[1] * T.gemm_dims(c)[2])
    assert worst["id"] == "fwd-glds128x128"          # the case whose reference time the table's header states
    assert 0.0 < T.REF_SECONDS_LARGEST <= 5.0
    for c in T.TABLE:
        M, N, K = T.gemm_dims(c)
        assert 2.0 * M * N * K <= T.COST_CAP, c["id"]
        assert T.largest_tensor_bytes(c) <= T.BYTES_CAP, c["id"]
