"""GPU: the activation-regularisation kernels through the C ABI (sat_activation_reg_fwd / _bwd) against the float64 specification
(tests/activation_reg_ref.py).  ``hidden`` and ``dH`` lie inside NaN guard bands, rows of ``hidden`` that are not live hold NaN and ``dH``
is pre-filled with random values: a kernel that loads a finished row, multiplies a term away instead of skipping it, or writes outside the
live rows shows as a NaN or as a changed word.

Bounds.  Forward: every non-negative term carries at most 3 x 2^-24 of relative error (the rounding of the difference counts twice in
the square, the square rounds once; the sums are in double) and the result is rounded to fp32 once, so ar and tar are good to about
2.4e-7 relative; the bound is 1e-6.
Backward, per element: 8 * 2^-24 * (|a h_t| + |b| (2 |h_t| + |h_t-1| + |h_t+1|) + |prefill|) with a = g0 2/(P n), b = g1 2/(Q n) and only
the terms that are on: each product and difference rounds once, a and b once each, the two sums once each - at most six roundings on the
TAR part, four on the AR part, one on the pre-fill."""
import ctypes as C

import pytest
import torch

import activation_reg_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64          # floats: 256 bytes, so the framed tensor starts 16-byte aligned
U = 2.0 ** -24

CASES = {
    # name: (N, T1, n, lengths, hidden moved by this many floats)
    "narrow_ragged": (5, 4, 7, [4, 1, 3, 0, 2], 0),                              # n % 4 != 0: the 4-byte form
    "wide_full": (3, 6, 8, [6, 6, 6], 0),                                        # the 16-byte form, equal lengths: the plain means
    "two_trips_ragged_tail": (70, 3, 260, [1 + i % 3 for i in range(70)], 0),    # 65 units for 64 lanes; 210 rows = 52 blocks and a half
    "steps_never_reached": (4, 6, 8, [2, 1, 2, 0], 0),                           # ts = 2 < T1
    "wide_shape_moved_by_one_float": (3, 6, 8, [6, 6, 6], 1),                    # n % 4 == 0 but the base is not 16-byte aligned
    "no_pairs": (5, 4, 8, [1, 0, 1, 1, 0], 0),                                   # Q = 0: tar is 0.0 and the backward has no TAR term
    "nothing_live": (4, 3, 8, [0, 0, 0, 0], 0),                                  # P = 0
}


def _lib():
    import sat_amd  # noqa: F401
    from sat_amd import _lib as L
    return L


def framed(t, shift=0):
    """a copy of the fp32 tensor ``t`` inside a NaN-filled buffer, ``shift`` floats past the aligned position: (whole, view)"""
    flat = t.contiguous().reshape(-1)
    whole = torch.full((2 * GUARD + flat.numel() + shift,), float("nan"), dtype=torch.float32, device="cuda")
    view = whole[GUARD + shift:GUARD + shift + flat.numel()]
    view.copy_(flat)
    return whole, view.reshape(t.shape)


def bits(t):
    return t.contiguous().view(torch.int32)


def make_case(name):
    N, T1, n, lengths, shift = CASES[name]
    g = torch.Generator().manual_seed(100 + len(name))
    hidden = torch.rand(T1, N, n, generator=g) * 2 - 1
    prefill = (torch.rand(T1, N, n, generator=g) * 2 - 1) * 0.05
    live = R.live_mask(lengths, T1)
    g0, g1 = float(torch.tensor(1.7, dtype=torch.float32)), float(torch.tensor(-0.6, dtype=torch.float32))
    if name == "no_pairs":
        g1 = float("nan")                                   # no TAR term may be formed, so its scale never matters
    h64 = hidden.double()
    ar, tar, P, Q = R.reg_terms(h64, lengths)
    ref = dict(ar=float(ar), tar=float(tar), P=P, Q=Q, grad=R.reg_grad(h64, lengths, g0, g1), mag=R.reg_grad_magnitude(h64, lengths, g0, g1))
    hidden = hidden.clone()
    hidden[~live] = float("nan")                            # finished rows may hold anything
    return dict(N=N, T1=T1, n=n, lengths=lengths, shift=shift, hidden=hidden, prefill=prefill, live=live, g=(g0, g1), ref=ref)


def run(c):
    """one forward and one backward through the C ABI; returns (out (2,) on the host, dH whole buffer bits, dH view on the host)"""
    L = _lib()
    lib = L.lib()
    N, T1, n = c["N"], c["T1"], c["n"]
    hid_whole, hid = framed(c["hidden"], c["shift"])
    dh_whole, dh = framed(c["prefill"])
    dh_before = bits(dh_whole).clone()
    hid_before = bits(hid_whole).clone()
    lengths = torch.tensor(c["lengths"], dtype=torch.int32, device="cuda")
    nbytes = lib.sat_activation_reg_scratch_bytes(N, T1, n)
    assert nbytes >= 16
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out_whole, out = framed(torch.full((2,), 7.0))
    gscale = torch.tensor(c["g"], dtype=torch.float32, device="cuda")
    P, Q = c["ref"]["P"], c["ref"]["Q"]
    st = L.stream_ptr()
    L.check(lib.sat_activation_reg_fwd(L.ptr(hid), L.ptr(lengths), N, T1, n, P, Q, L.ptr(scratch), L.ptr(out), st), "sat_activation_reg_fwd")
    L.check(lib.sat_activation_reg_bwd(L.ptr(hid), L.ptr(lengths), N, T1, n, P, Q, L.ptr(gscale), L.ptr(dh), st), "sat_activation_reg_bwd")
    torch.cuda.synchronize()
    assert torch.equal(bits(hid_whole), hid_before), "hidden or its guard bands were written"
    assert bool(torch.isnan(out_whole[:GUARD]).all()) and bool(torch.isnan(out_whole[GUARD + 2:]).all()), "out's guard bands were written"
    return out.cpu(), bits(dh_whole).cpu(), dh_before.cpu(), dh.cpu()


@pytest.fixture(scope="module")
def cases():
    return {name: make_case(name) for name in CASES}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernels_match_the_float64_specification(cases, name):
    c = cases[name]
    ref = c["ref"]
    out, dh_bits, dh_before, dh = run(c)
    for k, got in (("ar", float(out[0])), ("tar", float(out[1]))):
        print("%s %s: got %.9g ref %.9g rel %.3e" % (name, k, got, ref[k], abs(got - ref[k]) / max(ref[k], 1e-300)))
        assert abs(got - ref[k]) <= 1e-6 * ref[k], (name, k, got, ref[k])
    if ref["Q"] == 0:
        assert float(out[1]) == 0.0
    if ref["P"] == 0:
        assert float(out[0]) == 0.0
    # every word outside the live rows of dH, the guard bands included, keeps its bits
    live_whole = torch.zeros(dh_bits.numel(), dtype=torch.bool)
    live_whole[GUARD:GUARD + dh.numel()] = c["live"].unsqueeze(-1).expand(c["T1"], c["N"], c["n"]).reshape(-1)
    assert torch.equal(dh_bits[~live_whole], dh_before[~live_whole]), "dH changed outside the live rows"
    if ref["P"] == 0:
        assert torch.equal(dh_bits, dh_before)
        return
    want = c["prefill"].double() + ref["grad"]
    bound = 8 * U * (ref["mag"] + c["prefill"].double().abs())
    err = (dh.double() - want).abs()
    livem = c["live"].unsqueeze(-1).expand_as(err)
    assert bool(torch.isfinite(dh[livem]).all()), "NaN or inf in a live row of dH: a finished row was read or a term multiplied away"
    worst = float((err[livem] / bound[livem].clamp_min(1e-300)).max())
    print("%s backward: worst error / bound = %.3f" % (name, worst))
    assert bool((err[livem] <= bound[livem]).all()), (name, worst)
    assert bool((dh[livem] != c["prefill"][livem]).any()), "the backward added nothing"


def test_equal_lengths_are_the_plain_means(cases):
    c = cases["wide_full"]
    out, _, _, _ = run(c)
    h = c["hidden"].double()
    for got, ref in ((float(out[0]), float(h.pow(2).mean())), (float(out[1]), float((h[1:] - h[:-1]).pow(2).mean()))):
        assert abs(got - ref) <= 1e-6 * ref, (got, ref)


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_runs_give_the_same_bits(cases, name):
    a, b = run(cases[name]), run(cases[name])
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1])


def test_the_two_access_widths_agree_on_what_they_compute(cases):
    """the same values through the 16-byte and, moved by one float, through the 4-byte form: same specification, both within the bounds,
    and sums that agree to the forward bound (their orders differ, so not bit for bit)"""
    a, b = run(cases["wide_full"])[0], run(dict(cases["wide_full"], shift=1))[0]
    for x, y in zip(a.tolist(), b.tolist()):
        assert abs(x - y) <= 2e-6 * abs(y)
