"""CPU: the case table of the optimizer-step forms (tests/optimizer_cases.py) reaches every form that test_gpu_optimizer_forms.py is meant
to run, through the Python mirror of the kernels' width and extent predicates.  Nothing here touches a device."""
import pytest

import optimizer_cases as O


def test_chunk_size_is_the_library_s():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    assert _lib.lib().sat_optimizer_chunk_elems() == O.CHUNK


def test_case_names_are_unique_and_rows_are_well_formed():
    names = [c["name"] for c in O.CASES]
    assert len(names) == len(set(names))
    for c in O.CASES:
        assert c["kernel"] in (O.STEP, O.AVG, O.SWAP) and c["kind"] in O.KINDS
        assert any(not t["omit"] for t in c["tensors"])
        for t in c["tensors"]:
            assert 0 < t["n"] < 200000, "a case stays well under a second"
            assert t["mis"] is None or t["mis"] in O.STREAMS[c["kernel"]], (c["name"], t["mis"])
            off = O.offsets(c["kernel"], c["kind"], t)
            for s in O.reads(c["kernel"], c["kind"]):
                assert off[s] is not None, "%s: %s reads %s" % (c["name"], c["kind"], s)
        code, h = O.KINDS[c["kind"]]
        for beta in (h.get("beta1"), h.get("beta2")):
            assert beta is None or 0.5 <= beta < 1.0
        if c["exact"]:
            assert code == O.SGD and not h and c["clip_coef"] is None and c["clip_value"] == 0
            assert all(t["wd"] == 0 and not t["m"] and t["lr"] == 2.0 ** -6 for t in c["tensors"])
            assert c["avg_coef"] in (None, 1.0)


def test_extent_arithmetic():
    for n, start in O.sweep():
        for wide in (True, False):
            ln, nv, tail, body, tails = O.extent(n, start, wide)
            assert 0 < ln <= O.CHUNK and start + ln <= n and (start + ln == n or ln == O.CHUNK)
            assert 4 * nv + tail == ln
            if wide:
                assert tail < 4 and body == -(-nv // 256) and body <= 64          # 64 trips of 256 lanes x 4 elements fill a chunk
            else:
                assert nv == 0 and tails == -(-ln // 256)
    for n in O.all_tensor_sizes():
        assert O.n_chunks(n) == len(range(0, n, O.CHUNK))
    assert O.chunk_rows([O.tensor(131075), O.tensor(7, omit=True), O.tensor(65536)]) == [(0, 0), (0, 65536), (0, 131072), (2, 0)]


def test_width_predicate_mirror():
    t = O.tensor(100)
    for kernel, kind in ((O.STEP, "adam"), (O.AVG, "adam"), (O.SWAP, "sgd")):
        assert O.is_wide(kernel, kind, O.offsets(kernel, kind, t))
        for s in O.STREAMS[kernel]:
            assert not O.is_wide(kernel, kind, O.offsets(kernel, kind, dict(t, mis=s))), (kernel, s)
        # the bf16 copy: 8-byte stores
        assert not O.is_wide(kernel, kind, O.offsets(kernel, kind, dict(t, shadow=2)))
        assert O.is_wide(kernel, kind, O.offsets(kernel, kind, dict(t, shadow=8)))
        assert O.is_wide(kernel, kind, O.offsets(kernel, kind, dict(t, shadow=0)))
    # the plain kernel looks at every pointer it was given, the averaging kernel not at what ASGD leaves alone
    assert not O.is_wide(O.STEP, "sgd", O.offsets(O.STEP, "sgd", dict(t, mis="v")))
    assert not O.is_wide(O.AVG, "sgd", O.offsets(O.AVG, "sgd", dict(t, mis="m")))
    assert O.is_wide(O.AVG, "asgd", O.offsets(O.AVG, "asgd", dict(t, mis="m"))) and O.is_wide(O.AVG, "asgd", O.offsets(O.AVG, "asgd", dict(t, mis="v")))
    assert not O.is_wide(O.AVG, "asgd", O.offsets(O.AVG, "asgd", dict(t, mis="a")))
    # NULL pointers count as aligned
    assert O.is_wide(O.STEP, "sgd", O.offsets(O.STEP, "sgd", dict(t, m=False)))
    assert O.is_wide(O.AVG, "sgd", O.offsets(O.AVG, "sgd", dict(t, m=False, avg=False)))


def test_case_table_reaches_every_form():
    seen = O.forms_reached()
    # kernels and entry points
    for e in ("sat_optimizer_step", "sat_optimizer_step_dev", "sat_optimizer_step_avg", "sat_optimizer_step_avg_dev", "sat_optimizer_swap",
              "sat_grad_clip_coef"):
        assert ("entry", e) in seen
    for kernel in (O.STEP, O.AVG, O.SWAP):
        # width: wide, and narrow forced by each stream alone
        for s in O.STREAMS[kernel]:
            assert ("one float off", kernel, s, "narrow") in seen
        assert ("copy", kernel, 2, "narrow") in seen          # one bf16 off
        assert ("copy", kernel, 8, "wide") in seen            # 8 but not 16 bytes: stays wide (in the plain kernel too, now that it looks)
        assert ("copy", kernel, 0, "wide") in seen and ("copy", kernel, 0, "narrow") in seen
        for by in ("body", "tail", "narrow"):
            assert ("copy written by", kernel, by) in seen
        # extent
        for n in O.EXTENTS:
            assert ("wide", kernel, "n", n) in seen
        for tail in (0, 1, 3):
            assert ("wide", kernel, "tail", tail) in seen
        for trips in (0, 1, 2):          # no vector at all (n < 4), one trip, a lane's second trip (n >= 1025)
            assert ("wide", kernel, "body trips", trips) in seen
        for n in O.NARROW_EXTENTS:
            assert ("narrow", kernel, "n", n) in seen
        assert ("narrow", kernel, "chunk start > 0", "full") in seen and ("narrow", kernel, "chunk start > 0", "ragged") in seen
        # table shape
        assert ("several lr / wd", kernel) in seen and ("shuffled rows", kernel) in seen and ("both paths in one launch", kernel) in seen
        assert ("omitted tensor", kernel) in seen
    assert ("one float off", O.AVG, "m", "wide") in seen          # ASGD: m and v do not count
    for kernel in (O.STEP, O.AVG):
        kinds = ["sgd", "sgd_first", "sgd_nesterov", "adam", "adamw"] + (["asgd"] if kernel == O.AVG else [])
        for kind in kinds:
            assert ("kind", kernel, kind) in seen and ("weight decay", kernel, kind) in seen
        assert ("m NULL", kernel) in seen
        for what in ("clip_coef", "clip_value"):
            assert len({k for k in seen if k[:2] == (what, kernel)}) == 2          # NULL and set; 0 and > 0
    for kernel in (O.AVG, O.SWAP):
        assert ("NULL beside non-NULL averages", kernel) in seen
    for coef in ("0", "1", "between"):
        assert ("avg coef", coef, "ema") in seen
    assert ("avg coef", "1", "asgd") in seen and ("avg coef", "between", "asgd") in seen
    # sat_grad_clip_coef
    for what in ("randn", "zeros", "1e20", "nan", "inf", "ragged last chunks", "misaligned g"):
        assert ("norm", what) in seen
    # ASGD is a kind of the averaging entry points only
    with pytest.raises(AssertionError):
        O.case("x", O.STEP, "asgd", [O.tensor(4)], "")
