"""GPU: every launch form of the training-mode BatchNorm kernels and of the 3x3 / 2 max pool (csrc/encoder.hip) against the float64
references of tests/batchnorm_ref.py.  The shapes and the plans they were written for are in tests/batchnorm_cases.py;
test_batchnorm_plan.py proves without a GPU that each shape lands on its form.

The C ABI is called directly, so every allocation is the test's own:
  inputs    views inside buffers that are NaN on both sides (masks and argmax bytes: 0xFF, which is no window position);
  outputs   y, mask, save_mean, save_invstd, the running statistics, dx, dres, dgamma, dbeta, the pooled map and its argmax are views inside
            canary buffers; after the call every element outside the view still has the canary's bits;
  scratch   exactly sat_bn_scratch_bytes long, NaN inside (a partial that is summed without having been written shows), canaries around it.
bn_vpt / bn_onepass are set per case through sat_debug_option and put back to 2 / 1 by a fixture.  Every call runs twice on fresh output
buffers and must repeat itself bit for bit.

Data set "int": x = a per-channel integer offset + {-2 .. 2}, dy and the residual from {-2 .. 2}: every sum is an integer below 2^24 whatever
the order.  Data set "real": oracle.prng.uniform values, per-channel mean, gamma, beta differing by O(1) from channel to channel, some gamma
negative (a wrong channel index shows), max|ref| a few units; rounded to bf16 first for bf16 storage.

The backward calls get save_mean, save_invstd and the mask (or the output tensor) of the REFERENCE, rounded to float / the reference's own
bits, and the reference's backward uses exactly those values: a sign flipped by rounding near zero in the forward cannot blur the backward.

Bounds, each against the float64 reference (u = 2^-24):
  statistics from a pass, int    mean within 1 fp32 ulp.
  statistics from a pass         |mean - ref| <= 2 u |ref| + 4 u A with A = the channel's mean |x - x[0]|;
                                 |invstd - ref| <= ref (2 u + 4 u (1 + (mean - x[0])^2 / (var + eps))).
                                 (the kernel subtracts row 0 in fp32, adds groups of four in fp32 and everything else in double; factor two)
  statistics from tiles          mean, invstd, dbeta, dgamma within 1 fp32 ulp of the float64 formula on the float tile values.
  running statistics             within 4 u max(|old|, |new|) of the fp32 formula on the float mean (the one the call stored) / the unbiased variance.
  y, eval output                 fp32 1e-5 max(1, max|ref|); bf16 adds 2^-8 |ref| per element.   dx: 2e-5 instead of 1e-5.
  dbeta                          exact on int data.
  dbeta, dgamma from a pass      per channel 8 u sum|g xhat| + 2 u |ref| (groups of at most four in fp32, three fp32 operations for xhat).
  dres                           bit-equal in both storage types.
  mask                           fp32: equals y > 0 (0 < y < 6 for ReLU6) of the kernel's own output.  bf16: equals the reference's bits
                                 except where the reference value lies within the output tolerance of 0 (or 6); at most 0.5 % left out.
  max pool                       output and argmax bit-equal (NaNs as NaNs); gradient exact on int data, within 4 u sum|terms| (+ 2^-8 |ref|
                                 for the bf16 rounding) on real data.
The projection-shortcut form rounds the shortcut's normalised value to bf16 before the add.  Where the float64 value lies within the fp32
error of that expression (8 u of its terms) of a bf16 rounding boundary either neighbour is the correct result, and an element is accepted
against either; everywhere else there is one reference.

Largest measured error as a fraction of its bound on the MI355X, over all cases (fp32 / bf16; the module prints these as "WORST" lines):
  pass mean, int data (1 ulp)  0.50 / 0.50        pass mean          0.34 / 0.33        pass invstd      0.17 / 0.15
  tile mean, invstd, dbeta, dgamma (1 ulp)  - / 0.50 each (correctly rounded: half an ulp)   running statistics  0.47 / 0.42
  y  0.016 / 0.99      eval y  0.010 / 0.96      dx  0.007 / 0.99      (bf16: the rounding of the stored value itself, 2^-9 .. 2^-8 |ref|)
  pass dbeta  0.071 / 0.022      pass dgamma  0.12 / 0.11      max-pool gradient  0.23 / 1.00 (0.996: one bf16 rounding)
  mask bits left out near a threshold: at most 1.7e-3 of a case (bound 5e-3); shortcut values on a bf16 rounding boundary: at most 8e-4.
"""
import pytest
import torch

import batchnorm_cases as B
import batchnorm_ref as R
from gemm_ref import CANARY_BF16, CANARY_F32

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64
EPS, MOMENTUM = 1e-5, 0.1
U = 2.0 ** -24
GUARD = 4096          # elements on either side of every view (a multiple of 16: views start 16-byte aligned in every type)
CANARY_U8 = 0xA5


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)
    B.set_switches(_lib.lib())
    _CACHE.clear()
    for k in sorted(WORST):
        print("WORST %s %s %.4f" % (k[0], k[1], WORST[k]))


@pytest.fixture(autouse=True)
def switches_restored(L):
    yield
    B.set_switches(L.lib())          # bn_vpt = 2, bn_onepass = 1


WORST = {}


def note(what, dtype, ratio):
    WORST[(what, dtype)] = max(WORST.get((what, dtype), 0.0), float(ratio))


# ------------------------------------------------------------------ frames
def _kind(dtype):
    if dtype == torch.bfloat16:
        return torch.int16, CANARY_BF16
    if dtype == torch.uint8:
        return torch.uint8, CANARY_U8
    return torch.int32, CANARY_F32


def framed_input(t, dtype):
    """t (host) as a view inside a device buffer that is NaN (bytes: 0xFF) on both sides"""
    n = t.numel()
    whole = torch.full((GUARD + n + GUARD,), 255 if dtype == torch.uint8 else NAN, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + n]
    view.copy_(t.reshape(-1).to(dtype))
    assert view.data_ptr() % 16 == 0
    return view


def framed_output(n, dtype, inside=None):
    """n elements inside a canary-filled device buffer (the view itself = the canary too, or `inside`): (view, frame)"""
    bits, canary = _kind(dtype)
    whole = torch.empty(GUARD + n + GUARD, dtype=dtype, device="cuda")
    whole.view(bits).fill_(canary)
    view = whole[GUARD:GUARD + n]
    if inside is not None:
        view.copy_(inside.reshape(-1).to(dtype)) if torch.is_tensor(inside) else view.fill_(inside)
    assert view.data_ptr() % 16 == 0
    return view, (whole, bits, canary, n)


def assert_guards_intact(frame, what):
    whole, bits, canary, n = frame
    b = whole.view(bits)
    bad = int((b[:GUARD] != canary).sum()) + int((b[GUARD + n:] != canary).sum())
    assert bad == 0, "%s: %d element(s) outside the output changed" % (what, bad)


def same_bits(a, b):
    if a.dtype == torch.uint8:
        return torch.equal(a, b)
    v = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.view(v), b.view(v))


# ------------------------------------------------------------------ data
_CACHE = {}


def _seed(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c["name"])) % 100000


def make_data(c, dataset, bf):
    """inputs (float64, exactly representable in the storage type) of a case; the last set is kept for the next test of the case"""
    from oracle import prng
    key = (c["name"], dataset, bf)
    if key in _CACHE:
        return _CACHE[key]
    _CACHE.clear()
    rows, C, s = c["rows"], c["C"], _seed(c)
    rnd = lambda t: R.to_storage(t, bf)
    uni = lambda shp, k: torch.from_numpy(prng.uniform(shp, s + k)).to(F64)
    ints = lambda shp, k, lo, hi: torch.from_numpy(prng.integers(shp, s + k, 0, hi - lo) + lo).to(F64)          # (prng.integers takes lo >= 0)
    d = dict(rows=rows, C=C)
    if dataset == "int":
        d["x"] = ints((C,), 1, -3, 4) + ints((rows, C), 2, -2, 3)
        d["dy"], d["res"], d["dres_old"] = ints((rows, C), 3, -2, 3), ints((rows, C), 4, -2, 3), ints((rows, C), 5, -2, 3)
        g = ints((C,), 6, 1, 3)
        d["gamma"], d["beta"] = torch.where(ints((C,), 7, 0, 2) > 0, g, -g), ints((C,), 8, -2, 2) + 0.5          # (half-integer beta: x = mean does not put v on the ReLU threshold)
        # the shortcut's BatchNorm in exact arithmetic: integer mean and beta, power-of-two invstd, gamma +-1, +-2
        d["raw"] = ints((rows, C), 9, -2, 3)
        d["rmean"], d["rinvstd"] = ints((C,), 10, -1, 2), 2.0 ** ints((C,), 11, -1, 2)
        d["rgamma"], d["rbeta"] = torch.where(ints((C,), 12, 0, 2) > 0, g, -g), ints((C,), 13, -1, 2)
    else:
        chan_mean, chan_std = 2.0 * uni((C,), 1), 0.5 + uni((C,), 14).abs()
        d["x"] = rnd(chan_mean + chan_std * uni((rows, C), 2))
        d["dy"], d["res"], d["dres_old"] = rnd(uni((rows, C), 3)), rnd(2.0 * uni((rows, C), 4)), rnd(uni((rows, C), 5))
        g = 0.5 + 1.5 * uni((C,), 6).abs()
        d["gamma"], d["beta"] = torch.where(uni((C,), 7) > -0.3, g, -g).float().to(F64), uni((C,), 8).float().to(F64)
        d["raw"] = rnd(1.0 + 2.0 * uni((rows, C), 9))
        d["rmean"], d["rinvstd"] = (1.0 + 0.5 * uni((C,), 10)).float().to(F64), (0.5 + uni((C,), 11).abs()).float().to(F64)
        d["rgamma"], d["rbeta"] = torch.where(uni((C,), 12) > 0, g, -g).float().to(F64), uni((C,), 13).float().to(F64)
    d["run_mean"], d["run_var"] = uni((C,), 15).float(), (0.5 + uni((C,), 16).abs()).float()
    _CACHE[key] = d
    return d


def tol_out(ref, scale, bf, ref_max=None):
    """the output tolerance per element: scale max(1, max|ref|), + 2^-8 |ref| in bf16"""
    m = float(ref.abs().max()) if ref_max is None else ref_max
    t = torch.full_like(ref, scale * max(1.0, m))
    return t + 2.0 ** -8 * ref.abs() if bf else t


def check_close(got, ref, scale, bf, what, dtype, label, alt=None):
    got = got.double().cpu().reshape(ref.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    ratio = (got - ref).abs() / tol_out(ref, scale, bf)
    if alt is not None:          # a second, equally correct reference for some elements (see the module docstring)
        ratio = torch.minimum(ratio, (got - alt).abs() / tol_out(alt, scale, bf, float(ref.abs().max())))
    worst = float(ratio.max())
    note(label, dtype, worst)
    print("%s: worst err / tol %.3f" % (what, worst))
    assert worst <= 1.0, what


def check_vector(got, ref, tol, what, dtype, label):
    got = got.double().cpu()
    assert not bool(torch.isnan(got).any()), "%s: NaN in the result" % what
    err = (got - ref).abs()
    worst = float((err / tol.clamp(min=1e-300)).max())
    note(label, dtype, worst)
    print("%s: worst err / tol %.3f" % (what, worst))
    assert bool((err <= tol).all()), what


def check_mask(mask, got_y, v_ref, y_ref, relu, bf, what, v_alt=None):
    """mask bytes against the kernel's own fp32 output, or (bf16) against the reference away from the thresholds"""
    n = v_ref.numel()
    bits = R.unpack_mask(mask.cpu(), n)
    if not bf:
        y = got_y.float().cpu().reshape(-1)
        own = (y > 0) & (y < 6) if relu == 2 else y > 0
        assert torch.equal(bits, own), "%s: %d mask bit(s) differ from the kernel's own output" % (what, int((bits != own).sum()))
        return
    v = v_ref.reshape(-1)
    tol = tol_out(v, 1e-5, True, float(y_ref.abs().max()))
    near = v.abs() <= tol
    if relu == 2:
        near |= (v - 6.0).abs() <= tol
    want = R.activate(v, relu)[1]
    ok = bits == want
    if v_alt is not None:
        ok |= bits == R.activate(v_alt.reshape(-1), relu)[1]
    left_out = float(near.sum()) / n
    print("%s: %.2e of the mask bits left out near a threshold" % (what, left_out))
    assert left_out <= 0.005, "%s: %.3f %% of the elements lie within the tolerance of a threshold" % (what, 100 * left_out)
    assert bool((ok | near).all()), "%s: %d mask bit(s) differ from the reference away from the thresholds" % (what, int((~(ok | near)).sum()))


def scratch_frame(lib, rows, C):
    need = lib.sat_bn_scratch_bytes(rows, C)
    assert need > 0 and need % 4 == 0
    return framed_output(need // 4, torch.float32, inside=NAN)


# ------------------------------------------------------------------ the calls (fresh outputs each time; everything that was written comes back)
def call_forward(L, c, d, bf, y_null=False):
    lib, adt = L.lib(), torch.bfloat16 if bf else torch.float32
    rows, C, n = d["rows"], d["C"], d["rows"] * d["C"]
    f32 = torch.float32
    x, gamma, beta = framed_input(d["x"], adt), framed_input(d["gamma"], f32), framed_input(d["beta"], f32)
    out, frames = {}, {}
    for k, size, dt, inside in (("y", n, adt, None), ("mask", n // 8 if c["mask"] else 0, torch.uint8, None), ("mean", C, f32, None), ("invstd", C, f32, None),
                                ("run_mean", C, f32, d["run_mean"]), ("run_var", C, f32, d["run_var"])):
        if size and not (y_null and k in ("y", "mask")):
            out[k], frames[k] = framed_output(size, dt, inside)
    out["scratch"], frames["scratch"] = scratch_frame(lib, rows, C)
    y, mask = out.get("y"), out.get("mask")
    common = (L.ptr(out["run_mean"]), L.ptr(out["run_var"]), L.ptr(out["mean"]), L.ptr(out["invstd"]))
    tail = (c["relu"], L.ptr(y), L.ptr(mask), L.ptr(out["scratch"]), L.stream_ptr())
    keep = [x, gamma, beta]
    if c["kind"] == "pass":
        res = framed_input(d["res"], adt) if c["residual"] and not y_null else None
        keep.append(res)
        L.check(lib.sat_bn_train_fwd_t(int(bf), L.ptr(x), rows, C, L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM, *common, L.ptr(res), *tail), "sat_bn_train_fwd_t")
    else:
        tiles = framed_input(d["tiles_f"], f32)
        keep.append(tiles)
        if c["kind"] == "tiles":
            res = framed_input(d["res"], adt) if c["residual"] and not y_null else None
            keep.append(res)
            L.check(lib.sat_bn_train_fwd_tiles_bf16(L.ptr(x), rows, C, L.ptr(tiles), c["tile_rows"], L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM, *common, L.ptr(res), *tail),
                    "sat_bn_train_fwd_tiles_bf16")
        else:
            rb = [framed_input(d[k], adt if k == "raw" else f32) for k in ("raw", "rmean", "rinvstd", "rgamma", "rbeta")]
            keep += rb
            L.check(lib.sat_bn_train_fwd_tiles_bf16_resbn(L.ptr(x), rows, C, L.ptr(tiles), c["tile_rows"], L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM, *common,
                                                          *[L.ptr(t) for t in rb], *tail), "sat_bn_train_fwd_tiles_bf16_resbn")
    torch.cuda.synchronize()
    for k, f in frames.items():
        assert_guards_intact(f, "%s forward %s" % (c["name"], k))
    out.pop("scratch")
    return out


def call_backward(L, c, d, bf, ref):
    lib, adt = L.lib(), torch.bfloat16 if bf else torch.float32
    rows, C, n = d["rows"], d["C"], d["rows"] * d["C"]
    f32 = torch.float32
    x, dy, gamma = framed_input(d["x"], adt), framed_input(d["dy"], adt), framed_input(d["gamma"], f32)
    mean, invstd = framed_input(ref["mean32"], f32), framed_input(ref["invstd32"], f32)
    y = framed_input(ref["y_in"], adt) if c["relu"] and not c["mask"] else None
    mask = framed_input(ref["mask_in"], torch.uint8) if c["mask"] else None
    out, frames = {}, {}
    out["dx"], frames["dx"] = framed_output(n, adt)
    out["dgamma"], frames["dgamma"] = framed_output(C, f32)
    out["dbeta"], frames["dbeta"] = framed_output(C, f32)
    if c["dres"]:
        out["dres"], frames["dres"] = framed_output(n, adt, d["dres_old"] if c["dres"] == "acc" else None)
    out["scratch"], frames["scratch"] = scratch_frame(lib, rows, C)
    tail = (L.ptr(mean), L.ptr(invstd), L.ptr(gamma), c["relu"], L.ptr(out["dx"]), L.ptr(out["dgamma"]), L.ptr(out["dbeta"]), L.ptr(out.get("dres")),
            int(c["dres"] == "acc"), L.ptr(mask), L.ptr(out["scratch"]), L.stream_ptr())
    if c["kind"] == "pass":
        L.check(lib.sat_bn_train_bwd_t(int(bf), L.ptr(dy), L.ptr(x), L.ptr(y), rows, C, *tail), "sat_bn_train_bwd_t")
    else:
        tiles = framed_input(ref["tiles_b"], f32)
        L.check(lib.sat_bn_train_bwd_tiles_bf16(L.ptr(dy), L.ptr(x), rows, C, L.ptr(tiles), c["tile_rows"], *tail), "sat_bn_train_bwd_tiles_bf16")
    torch.cuda.synchronize()
    for k, f in frames.items():
        assert_guards_intact(f, "%s backward %s" % (c["name"], k))
    out.pop("scratch")
    return out


def call_eval(L, c, d, bf):
    lib, adt = L.lib(), torch.bfloat16 if bf else torch.float32
    rows, C = d["rows"], d["C"]
    f32 = torch.float32
    x, gamma, beta = framed_input(d["x"], adt), framed_input(d["gamma"], f32), framed_input(d["beta"], f32)
    rm, rv = framed_input(d["run_mean"], f32), framed_input(d["run_var"], f32)
    res = framed_input(d["res"], adt) if c["residual"] else None
    y, frame = framed_output(rows * C, adt)
    L.check(lib.sat_bn_eval_fwd_t(int(bf), L.ptr(x), rows, C, L.ptr(rm), L.ptr(rv), EPS, L.ptr(gamma), L.ptr(beta), L.ptr(res), c["relu"], L.ptr(y), L.stream_ptr()),
            "sat_bn_eval_fwd_t")
    torch.cuda.synchronize()
    assert_guards_intact(frame, "%s eval y" % c["name"])
    return dict(y=y)


def twice(fn, what):
    a, b = fn(), fn()
    for k in a:
        assert same_bits(a[k], b[k]), "%s: %s does not repeat itself bit for bit" % (what, k)
    return a


def forward_inputs(c, d):
    """the tile statistics of a tile / shortcut case: the float sums of x per row tile (distinct from tile to tile)"""
    if c["kind"] != "pass" and "tiles_f" not in d:
        d["tiles_f"] = R.tile_sums(d["x"], c["tile_rows"])
    return d


def backward_reference(c, d, bf):
    """the forward's reference values the backward call is given, and the backward's reference on exactly those"""
    if "bwd" in d:
        return d["bwd"]
    x = d["x"]
    mean, var, invstd, unb = R.train_stats(x, EPS)
    mean32, invstd32 = mean.float(), invstd.float()
    res = d["res"] if c["residual"] else None
    y, bits, v = R.forward(x, mean32.to(F64), invstd32.to(F64), d["gamma"], d["beta"], res, c["relu"])
    y_in = R.to_storage(y, bf)
    if c["relu"] and not c["mask"]:
        bits = y_in > 0          # the backward reads the stored output
    ref = dict(mean32=mean32, invstd32=invstd32, y_in=y_in, mask_in=R.pack_mask(bits) if c["mask"] else None)
    first = R.backward(x, d["dy"], bits, mean32.to(F64), invstd32.to(F64), d["gamma"], c["relu"])
    if c["kind"] == "tiles":
        ref["tiles_b"] = R.backward_tiles(first["g"], first["xhat"], c["tile_rows"])
        first = R.backward(x, d["dy"], bits, mean32.to(F64), invstd32.to(F64), d["gamma"], c["relu"], tiles=ref["tiles_b"])
    ref.update(first)
    d["bwd"] = ref
    return ref


def _params(kinds):
    return [pytest.param(c, dataset, dtype, id="%s-%s-%s" % (c["name"], dataset, dtype))
            for c in B.CASES if c["kind"] in kinds for dataset in ("int", "real") for dtype in c["run"]]


def assert_planned(L, c, dtype):
    B.set_switches(L.lib(), c["vpt"], c["onepass"])
    assert B.case_plans(L.lib(), c, dtype) == c["plans"][dtype]          # (test_batchnorm_plan.py asserts the same without a GPU)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("c,dataset,dtype", _params(("pass", "tiles", "resbn")))
def test_bn_forward_form(L, c, dataset, dtype):
    bf = dtype == B.BF16
    assert_planned(L, c, dtype)
    d = forward_inputs(c, make_data(c, dataset, bf))
    rows, C, x = d["rows"], d["C"], d["x"]
    tag = "%s %s %s forward" % (c["name"], dataset, dtype)
    got = twice(lambda: call_forward(L, c, d, bf), tag)

    # statistics
    if c["kind"] == "pass":
        mean, var, invstd, unb = R.train_stats(x, EPS)
        if dataset == "int":
            check_vector(got["mean"], mean, R.ulp32(mean), tag + " mean (1 ulp)", dtype, "pass mean, int (1 ulp)")
        A = (x - x[0]).abs().mean(0)
        check_vector(got["mean"], mean, 2 * U * mean.abs() + 4 * U * A, tag + " mean", dtype, "pass mean")
        check_vector(got["invstd"], invstd, invstd * (2 * U + 4 * U * (1 + (mean - x[0]) ** 2 / (var + EPS))), tag + " invstd", dtype, "pass invstd")
    else:
        mean, var, invstd, unb = R.stats_from_tiles(d["tiles_f"], rows, EPS)
        check_vector(got["mean"], mean, R.ulp32(mean), tag + " mean", dtype, "tile mean (1 ulp)")
        check_vector(got["invstd"], invstd, R.ulp32(invstd), tag + " invstd", dtype, "tile invstd (1 ulp)")
    # the update formula on the float mean the call itself stored (checked against the reference above: its own error, which follows the
    # scale of the data and not that of the mean, is not charged a second time to a channel whose running value is small)
    for k, new in (("run_mean", got["mean"].double().cpu()), ("run_var", unb)):
        want = R.running_update(d[k], new, MOMENTUM)
        check_vector(got[k], want, 4 * U * torch.maximum(d[k].to(F64).abs(), want.abs()), tag + " " + k, dtype, "running statistics")

    # output and mask
    res = alt = v_alt = None
    if c["kind"] == "resbn":
        s = R.normalize(d["raw"], d["rmean"], d["rinvstd"], d["rgamma"], d["rbeta"])
        delta = 8 * U * (((d["raw"] - d["rmean"]) * d["rinvstd"] * d["rgamma"]).abs() + d["rbeta"].abs())
        lo, hi = R.to_storage(s - delta, bf), R.to_storage(s + delta, bf)
        boundary = (hi - lo).abs() > 4 * delta          # a rounding step lies inside the fp32 uncertainty (not: bf16 resolves the uncertainty itself, as around 0)
        res, res_alt = torch.where(boundary, lo, R.to_storage(s, bf)), torch.where(boundary, hi, R.to_storage(s, bf))
        print("%s: %d shortcut value(s) on a bf16 rounding boundary" % (tag, int(boundary.sum())))
        assert float(boundary.sum()) <= 0.002 * res.numel()
        alt, _, v_alt = R.forward(x, mean, invstd, d["gamma"], d["beta"], res_alt, c["relu"])
    elif c["residual"]:
        res = d["res"]
    y, bits, v = R.forward(x, mean, invstd, d["gamma"], d["beta"], res, c["relu"])
    check_close(got["y"], y, 1e-5, bf, tag + " y", dtype, "y", alt=alt)
    if c["mask"]:
        check_mask(got["mask"], got["y"], v, y, c["relu"], bf, tag + " mask", v_alt)

    if c["stats_only"]:          # y = NULL: the same statistics, nothing else written
        only = twice(lambda: call_forward(L, c, d, bf, y_null=True), tag + " (y = NULL)")
        assert set(only) == {"mean", "invstd", "run_mean", "run_var"}
        for k in only:
            assert same_bits(only[k], got[k]), "%s: %s differs between the statistics-only call and the full call" % (tag, k)

    if c["eval_mode"]:
        ev = twice(lambda: call_eval(L, c, d, bf), tag + " eval")
        want = R.eval_forward(x, d["run_mean"].to(F64), d["run_var"].to(F64), EPS, d["gamma"], d["beta"], d["res"] if c["residual"] else None, c["relu"])
        check_close(ev["y"], want, 1e-5, bf, tag + " eval y", dtype, "eval y")


@pytest.mark.parametrize("c,dataset,dtype", _params(("pass", "tiles")))
def test_bn_backward_form(L, c, dataset, dtype):
    bf = dtype == B.BF16
    assert_planned(L, c, dtype)
    d = make_data(c, dataset, bf)
    ref = backward_reference(c, d, bf)
    tag = "%s %s %s backward" % (c["name"], dataset, dtype)
    got = twice(lambda: call_backward(L, c, d, bf, ref), tag)

    if c["kind"] == "tiles":
        check_vector(got["dbeta"], ref["dbeta"], R.ulp32(ref["dbeta"]), tag + " dbeta", dtype, "tile dbeta (1 ulp)")
        check_vector(got["dgamma"], ref["dgamma"], R.ulp32(ref["dgamma"]), tag + " dgamma", dtype, "tile dgamma (1 ulp)")
    else:
        if dataset == "int":
            assert torch.equal(got["dbeta"].double().cpu(), ref["dbeta"]), tag + ": dbeta is not exact"
        for k in ("dbeta", "dgamma"):
            check_vector(got[k], ref[k], 8 * U * ref["s_abs"] + 2 * U * ref[k].abs(), tag + " " + k, dtype, "pass " + k)
    check_close(got["dx"], ref["dx"], 2e-5, bf, tag + " dx", dtype, "dx")
    if c["dres"]:
        want = R.dres(ref["g"], d["dres_old"] if c["dres"] == "acc" else None, bf)
        g = got["dres"].double().cpu().reshape(want.shape)
        assert torch.equal(g, want), "%s: %d element(s) of dres differ from the exact result" % (tag, int((g != want).sum()))


def _pool_data(shape, dataset, bf):
    from oracle import prng
    N, H, W, C = shape
    P, Q = R.pool_size(H), R.pool_size(W)
    s = 100 * H + 10 * W + C
    if dataset == "int":
        x = torch.from_numpy(prng.integers(shape, s, 0, 5) - 2).to(F64).clamp(min=0.0)          # post-ReLU: zeros and many exact ties
        dy = torch.from_numpy(prng.integers((N, P, Q, C), s + 1, 0, 5) - 2).to(F64)
    else:
        x = R.to_storage(torch.from_numpy(prng.uniform(shape, s)).to(F64).clamp(min=0.0), bf)
        x = torch.where(torch.from_numpy(prng.integers(shape, s + 2, 0, 4)) == 0, (x * 4).round() / 4, x)          # a quarter on a coarse grid: ties above 0
        dy = R.to_storage(torch.from_numpy(prng.uniform((N, P, Q, C), s + 1)).to(F64), bf)
        if dataset == "nan":
            x = torch.where(torch.from_numpy(prng.integers(shape, s + 3, 0, 16)) == 0, torch.full_like(x, NAN), x)
    return x, dy, P, Q


@pytest.mark.parametrize("dtype", (B.F32, B.BF16))
@pytest.mark.parametrize("dataset", ("int", "real", "nan"))
@pytest.mark.parametrize("shape", B.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_form(L, shape, dataset, dtype):
    bf = dtype == B.BF16
    lib, adt = L.lib(), torch.bfloat16 if bf else torch.float32
    N, H, W, C = shape
    x, dy, P, Q = _pool_data(shape, dataset, bf)
    y_ref, arg_ref = R.maxpool_fwd(x)
    dx_ref, s_abs = R.maxpool_bwd(dy, arg_ref, H, W)
    tag = "maxpool %s %s %s (%s)" % (shape, dataset, dtype, B.pool_form(dtype, C))

    def fwd():
        xv = framed_input(x, adt)
        y, yf = framed_output(N * P * Q * C, adt)
        a, af = framed_output(N * P * Q * C, torch.uint8)
        L.check(lib.sat_maxpool3x3s2_fwd_t(int(bf), L.ptr(xv), L.ptr(y), L.ptr(a), N, H, W, C, L.stream_ptr()), "sat_maxpool3x3s2_fwd_t")
        torch.cuda.synchronize()
        assert_guards_intact(yf, tag + " y")
        assert_guards_intact(af, tag + " argmax")
        return dict(y=y, argmax=a)

    def bwd():
        g, a = framed_input(dy, adt), framed_input(arg_ref, torch.uint8)
        dx, f = framed_output(N * H * W * C, adt)
        L.check(lib.sat_maxpool3x3s2_bwd_t(int(bf), L.ptr(g), L.ptr(a), L.ptr(dx), N, H, W, C, L.stream_ptr()), "sat_maxpool3x3s2_bwd_t")
        torch.cuda.synchronize()
        assert_guards_intact(f, tag + " dx")
        return dict(dx=dx)

    got = twice(fwd, tag)
    y = got["y"].double().cpu().reshape(y_ref.shape)
    assert torch.equal(torch.isnan(y), torch.isnan(y_ref)), tag + ": NaNs are not where the reference has them"
    assert torch.equal(torch.nan_to_num(y, nan=-1.0), torch.nan_to_num(y_ref, nan=-1.0)), tag + ": the pooled map differs from the reference"
    a = got["argmax"].cpu().reshape(arg_ref.shape)
    assert torch.equal(a, arg_ref), "%s: %d argmax byte(s) differ (first-maximum rule)" % (tag, int((a != arg_ref).sum()))

    dx = twice(bwd, tag + " gradient")["dx"].double().cpu().reshape(dx_ref.shape)
    if dataset == "int":
        assert torch.equal(dx, dx_ref), "%s: %d gradient element(s) differ from the exact result" % (tag, int((dx != dx_ref).sum()))
    else:
        tol = 4 * U * s_abs + (2.0 ** -8 * dx_ref.abs() if bf else 0.0)
        err = (dx - dx_ref).abs()
        note("maxpool gradient", dtype, float((err / tol.clamp(min=1e-300)).max()))
        assert bool((err <= tol).all()), tag + " gradient"
