"""GPU: the geometries of the nine-wave 3x3 weight-gradient kernel (csrc/wgrad3x3.hip) that test_gpu_encoder.py's BCONVS do not reach:
the W = 8 halo (10 x 10 pixels, 21 LDS-DMA pieces per k-tile: the only geometry in which waves issue two pieces and wait on vmcnt(2)),
a pipeline of one, two and three k-tiles, H = 1 (both halo rows outside the image), a short last pixel split, and the slab-limited split.

Every case goes through sat_conv2d_wgrad_bf16 with nothing forced and asserts
  (a) dW = sum dy[n, p, q, k] * x[n, p + r - 1, q + s - 1, c] against a float64 reference: bit-equal on small integers in {-2 .. 2}
      (bf16-exact operands, fp32-exact sums of at most 4 * N H W <= 4096), and within the bound of test_conv_bf16_fwd_dgrad_wgrad,
      1e-5 * sqrt(N P Q) * max(1, max|ref|), on bf16-rounded normal deviates;
  (b) the path: a profiler scope gemm_wgrad3x3 ran - or, for the two geometries just outside the eligibility rules, did not;
  (c) the number of pixel splits Z, read off the slab: it starts as a canary, afterwards exactly its first Z * K * 9 * C floats are
      overwritten (none when Z = 1: the kernel then writes dW itself);
  (d) x and dy sit inside NaN-filled buffers with guards of at least (W + 2) * max(C, K) elements - the kernel masks its halo reads by an
      out-of-range offset, not by the extent of the buffer descriptor, so a wrong mask reads a neighbour and poisons dW - and dW and the
      slab inside canary buffers that must stay intact around them.
A mismatch of (b) or (c) FAILS: when the eligibility or split rules change the cases are re-derived, not skipped."""
import ctypes

import pytest
import torch

from gemm_ref import CANARY_F32

pytestmark = pytest.mark.gpu

NAN = float("nan")


def case(N, H, W, C, K, slab, Z, own=True, why=""):
    """slab: floats of scratch in units of K * 9 * C (None: a null slab); Z: pixel splits expected; own: the nine-wave kernel runs"""
    return dict(N=N, H=H, W=W, C=C, K=K, slab=slab, Z=Z, own=own, why=why)


CASES = [
    case(1, 8, 8, 64, 64, 2, 1, why="W = 8, one k-tile: the prologue issues a single tile"),
    case(1, 16, 8, 64, 64, 2, 1, why="W = 8, two k-tiles"),
    case(3, 8, 8, 128, 64, 2, 1, why="W = 8, three k-tiles, each a new image"),
    case(1, 1, 64, 64, 64, 2, 1, why="W = 64, H = 1: the rows above and below are both outside the image"),
    case(1, 2, 32, 64, 64, 2, 1, why="W = 32, one k-tile"),
    case(19, 4, 16, 64, 64, 2, 2, why="19 k-tiles in two splits of 10 + 9; a slab of exactly two partials"),
    case(16, 8, 8, 512, 512, 3, 2, why="ResNet layer4 at 256 px: 16 k-tiles, Z = 2"),
    case(16, 8, 8, 512, 512, 1, 1, why="the same, the slab holds one partial only: Z = 1, written straight to dW"),
    case(16, 8, 8, 512, 512, None, 1, why="the same without a slab"),
    # just outside the eligibility rules: the implicit-GEMM form computes the same values
    case(2, 8, 8, 64, 72, 2, None, own=False, why="K = 72 is no multiple of 64"),
    case(1, 7, 8, 64, 64, 2, None, own=False, why="H = 7 is no multiple of the 8 rows of a k-tile"),
]


def case_id(c):
    return "%dx%dx%dx%dx%d-slab%s" % (c["N"], c["H"], c["W"], c["C"], c["K"], c["slab"])


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))          # the float64 references
    yield _lib
    torch.set_num_threads(threads)


def reference(dy, x):
    """dy (N, H, W, K), x (N, H, W, C) -> float64 dW (K, 9, C)"""
    N, H, W, K = dy.shape
    C = x.shape[3]
    xp = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    g = dy.double().reshape(-1, K).t().contiguous()
    dw = torch.empty(K, 9, C, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            dw[:, 3 * r + s] = g @ xp[:, r:r + H, s:s + W].reshape(-1, C)
    return dw


def nan_framed(t, guard):
    whole = torch.full((guard + t.numel() + guard,), NAN, dtype=torch.bfloat16, device="cuda")
    view = whole[guard:guard + t.numel()]
    view.copy_(t.reshape(-1).to(torch.bfloat16))
    assert view.data_ptr() % 16 == 0
    return whole, view


def canary_framed(n, guard):
    whole = torch.empty(guard + n + guard, dtype=torch.float32, device="cuda")
    whole.view(torch.int32).fill_(CANARY_F32)
    view = whole[guard:guard + n]
    assert view.data_ptr() % 16 == 0
    return whole, view


def canaries(t):
    return int((t.view(torch.int32) == CANARY_F32).sum())


def run(L, c, dy, x):
    """one call; returns dW on the host after the path, split and frame assertions"""
    N, H, W, C, K = (c[k] for k in "NHWCK")
    out_elems = K * 9 * C
    guard = -(-((W + 2) * max(C, K)) // 8) * 8
    xw, xv = nan_framed(x, guard)
    gw, gv = nan_framed(dy, guard)
    dww, dwv = canary_framed(out_elems, 1024)
    slab_elems = 0 if c["slab"] is None else c["slab"] * out_elems
    sw, sv = canary_framed(slab_elems, 1024)
    geom = L.ConvGeom(N=N, H=H, W=W, C=C, K=K, R=3, S=3, stride=1, pad=1)
    L.profile_start()
    rc = L.lib().sat_conv2d_wgrad_bf16(L.ptr(gv), L.ptr(xv), L.ptr(dwv), ctypes.byref(geom), L.ptr(sv) if slab_elems else None, slab_elems, L.stream_ptr())
    torch.cuda.synchronize()
    names = [e["name"] for e in L.profile_stop()]
    L.check(rc, "sat_conv2d_wgrad_bf16")
    own = [n for n in names if n.startswith("gemm_wgrad3x3")]
    assert bool(own) == c["own"], "%s: the scopes that ran are %s" % (c["why"], names)
    assert canaries(dww[:1024]) == 1024 and canaries(dww[1024 + out_elems:]) == 1024, "dW: the frame around it changed"
    assert canaries(sw[:1024]) == 1024 and canaries(sw[1024 + slab_elems:]) == 1024, "slab: the frame around it changed"
    if c["own"]:
        used = 0 if c["Z"] == 1 else c["Z"] * out_elems
        assert canaries(sv[:used]) == 0, "%d pixel splits were expected: part of their partials was not written" % c["Z"]
        assert canaries(sv[used:]) == slab_elems - used, "%d pixel splits were expected: the slab is written beyond them" % c["Z"]
    assert bool(torch.isnan(xw[:guard]).all()) and bool(torch.isnan(gw[:guard]).all())
    got = dwv.cpu().reshape(K, 9, C)
    assert not bool(torch.isnan(got).any()), "NaN in dW: a read went beyond x or dy"
    return got


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_wgrad3x3_geometry(L, c):
    N, H, W, C, K = (c[k] for k in "NHWCK")
    g = torch.Generator().manual_seed(1000 * N + 100 * H + W + C + K)
    # small integers: exact whatever the order of the additions
    x = torch.randint(-2, 3, (N, H, W, C), generator=g).float()
    dy = torch.randint(-2, 3, (N, H, W, K), generator=g).float()
    ref = reference(dy, x)
    assert float(ref.abs().max()) < 2 ** 24
    got = run(L, c, dy, x)
    assert torch.equal(got, ref.float()), "%s: %d element(s) of dW differ from the exact result" % (c["why"], int((got != ref.float()).sum()))
    # bf16-rounded normal deviates: the arithmetic
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16).float()
    dy = torch.randn(N, H, W, K, generator=g).to(torch.bfloat16).float()
    ref = reference(dy, x)
    got = run(L, c, dy, x)
    tol = 1e-5 * (N * H * W) ** 0.5 * max(1.0, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print("%s: max |err| %.3e, bound %.3e" % (case_id(c), err, tol))
    assert err <= tol, c["why"]
