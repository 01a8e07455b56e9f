"""The direct-to-LDS ring of csrc/gemm_glds_kernel.h and csrc/wgrad3x3.hip must exist in the generated code (tools/check_lds_ring_waits.py).

hipcc puts `s_waitcnt vmcnt(0)` in front of every group of ds_read_b64_tr_b16 reads made through the builtin: all k-tiles in flight are then
waited for at each k-step and the counted waits of the source decide nothing.  With the builtin the shipped units showed, per kernel,
    gemm_glds_t*.hip   forms (0,1) bf16, (0,1) float, (1,1) float, (1,2) float, (3,3) bf16:   3 such drains each   (k-steps 0, 1, 2)
                       forms (0,0), (2,0) (plain ds_read_b128):                               0
    wgrad3x3.hip       1, directly behind the counted vmcnt(4/3/2)
The units are compiled to assembly with the Makefile's flags (no GPU is needed); skipped where there is no hipcc.
"""
import concurrent.futures
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import check_lds_ring_waits as W  # noqa: E402

pytestmark = pytest.mark.skipif(W.hipcc() is None, reason="no hipcc on this machine")


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """{unit: [(kernel, drains, counted waits, missing counted waits)]}: every unit compiled once, side by side"""
    out = str(tmp_path_factory.mktemp("lds_ring"))
    units = W.units()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(4, len(units))) as pool:
        paths = list(pool.map(lambda u: W.compile_to_asm(u, out), units))
    return {u: W.check_unit(p) for u, p in zip(units, paths)}


def test_the_shipped_ring_units_are_the_ones_checked():
    assert W.units() == ["gemm_glds_t64.hip", "gemm_glds_t128.hip", "gemm_glds_t128x64.hip", "wgrad3x3.hip"]


def test_every_form_of_every_unit_is_found(rows):
    forms = {"(%d,%d),%s" % f for f in ((0, 0, "bf16"), (0, 0, "float"), (0, 1, "bf16"), (0, 1, "float"), (1, 1, "float"), (1, 2, "float"), (2, 0, "bf16"),
                                        (3, 3, "bf16"))}
    for unit, tile in (("gemm_glds_t64.hip", "64x64"), ("gemm_glds_t128.hip", "128x128"), ("gemm_glds_t128x64.hip", "128x64")):
        assert {r[0] for r in rows[unit]} == {"gemm_glds<%s,%s>" % (tile, f) for f in forms}
    assert [r[0] for r in rows["wgrad3x3.hip"]] == ["wgrad3x3"]


def test_no_fragment_read_drains_the_tiles_in_flight(rows):
    bad = [(unit, label, drains) for unit, rs in rows.items() for label, drains, _, _ in rs if drains]
    assert not bad, "`s_waitcnt vmcnt(0)` directly in front of a ds_read: %s" % bad


def test_the_counted_waits_of_the_source_are_in_the_code(rows):
    bad = [(unit, label, counted, missing) for unit, rs in rows.items() for label, _, counted, missing in rs if missing]
    assert not bad, "counted vmcnt waits missing: %s" % bad


def test_the_analysis_sees_a_drain():
    """the two patterns on a hand-written listing: a drain directly before a read counts, one separated from it by the barrier does not"""
    insts = ["s_waitcnt vmcnt(6)", "s_waitcnt lgkmcnt(0)", "s_barrier", "s_waitcnt vmcnt(0)", "ds_read_b64_tr_b16 v[2:3], v1", "v_mfma_f32_32x32x16_bf16 a, b, c",
             "s_waitcnt vmcnt(0) lgkmcnt(0)", "ds_read_b128 v[4:7], v1", "s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(0)", "s_barrier", "ds_read_b128 v[4:7], v1",
             "s_waitcnt vmcnt(12)"]
    assert W.analyse(insts) == (2, {6, 12})
