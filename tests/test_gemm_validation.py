"""CPU: sat_gemm_f32 / sat_gemm_ex refuse a launch whose epilogue operand, epilogue number or split-K slab is unusable BEFORE any kernel is
chosen - for the bf16 kernels as for the fp32 one.  Nothing is launched here: the operand addresses are dummies, every status below
comes from the argument checks of launch_gemm (csrc/gemm.hip).  Likewise the convolution entry points refuse a stride_w that no kernel of theirs
reads (conv_*_any, csrc/encoder.hip)."""
import ctypes

import pytest

DUMMY = 0x10000          # non-null, 16-byte aligned; never dereferenced


@pytest.fixture(scope="module")
def L():
    import sat_amd  # noqa: F401
    from sat_amd import _lib
    _lib.lib()
    return _lib


def _desc(L, **over):
    kw = dict(A=DUMMY, lda=64, B=2 * DUMMY, ldb=64, C=3 * DUMMY, ldc=64, M=64, N=64, K=64, amode=0, bmode=0, accumulate=0, epi=0,
              bias=None, e0=None, lde0=64, c0=0, c1=0, slab=None, slab_elems=0)
    kw.update(over)
    return L.GemmDesc(**kw)


#: how the request reaches launch_gemm: the fp32 entry, fp32 operands on the bf16 MFMA kernel (decoder), bf16 operands and result (encoder:
#: the direct-to-LDS kernel would take this shape), bf16 operands with an fp32 result
ROUTES = {"f32": None, "f32_on_bf16_mfma": (0, 0, 0, 1), "bf16": (1, 1, 1, 1), "bf16_f32_out": (1, 1, 0, 1)}


def _call(L, route, **over):
    lib = L.lib()
    d = _desc(L, **over)
    if ROUTES[route] is None:
        rc = lib.sat_gemm_f32(ctypes.byref(d), None)
    else:
        a, b, c, m = ROUTES[route]
        t = L.GemmTypes(a_bf16=a, b_bf16=b, c_bf16=c, bf16_mfma=m)
        rc = lib.sat_gemm_ex(ctypes.byref(d), ctypes.byref(t), None)
    return rc, lib.sat_last_error().decode()


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("epi", [1, 5])
def test_bias_epilogue_without_bias_is_refused(L, route, epi):
    rc, msg = _call(L, route, epi=epi, e0=DUMMY)
    assert rc != 0 and "bias" in msg and "epilogue %d" % epi in msg, (rc, msg)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("epi", [3, 4])
def test_e0_epilogue_without_e0_is_refused(L, route, epi):
    rc, msg = _call(L, route, epi=epi, bias=DUMMY)
    assert rc != 0 and "e0" in msg and "epilogue %d" % epi in msg, (rc, msg)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("epi", [-1, 6, 1 << 20])
def test_unknown_epilogue_is_refused(L, route, epi):
    rc, msg = _call(L, route, epi=epi, bias=DUMMY, e0=DUMMY)
    assert rc != 0 and "epi" in msg and str(epi) in msg, (rc, msg)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_split_k_slab_of_some_size_at_address_zero_is_refused(L, route):
    rc, msg = _call(L, route, K=8192, slab=None, slab_elems=1 << 20)
    assert rc != 0 and "slab" in msg, (rc, msg)
    rc, msg = _call(L, route, K=8192, slab=DUMMY, slab_elems=-1)
    assert rc != 0 and "slab" in msg, (rc, msg)


def test_checks_apply_to_the_strided_and_k_major_forms_too(L):
    for amode, bmode in ((0, 1), (1, 1)):
        rc, msg = _call(L, "bf16_f32_out", amode=amode, bmode=bmode, epi=5, lda=72, ldb=72, ldc=68)
        assert rc != 0 and "bias" in msg, (amode, bmode, rc, msg)


# ----------------------------------------------------------------------------- sat_conv_geom.stride_w
def _geom(L, **over):
    kw = dict(N=2, H=21, W=14, C=8, K=64, R=7, S=4, stride=2, pad=0, stride_w=1)
    kw.update(over)
    return L.ConvGeom(**kw)


def _conv_call(L, name, geom):
    lib = L.lib()
    g = ctypes.byref(geom)
    if "fwd" in name:
        rc = getattr(lib, name)(DUMMY, 2 * DUMMY, None, 3 * DUMMY, g, None)
    elif "dgrad" in name:
        rc = getattr(lib, name)(DUMMY, 2 * DUMMY, 3 * DUMMY, g, 0, None)
    else:
        rc = getattr(lib, name)(DUMMY, 2 * DUMMY, 3 * DUMMY, g, None, 0, None)
    return rc, lib.sat_last_error().decode()


@pytest.mark.parametrize("name", ["sat_conv2d_fwd", "sat_conv2d_wgrad", "sat_conv2d_dgrad", "sat_conv2d_dgrad_bf16"])
def test_stride_w_is_refused_where_no_kernel_reads_it(L, name):
    """stride_w is the bf16 forward / filter-gradient stem view.  The fp32 kernel has one stride and no data gradient looks at it: such a
    call used to return SAT_OK with an output of the anisotropic shape holding another convolution's values."""
    rc, msg = _conv_call(L, name, _geom(L))
    assert rc == 1 and "stride_w" in msg, (rc, msg)          # SAT_EINVAL


@pytest.mark.parametrize("name", ["sat_conv2d_fwd", "sat_conv2d_wgrad", "sat_conv2d_dgrad", "sat_conv2d_dgrad_bf16"])
@pytest.mark.parametrize("stride_w", [0, 2])
def test_stride_w_equal_to_stride_or_zero_is_not_refused_for_it(L, name, stride_w):
    """0 and the value of stride itself mean "isotropic": the stride_w check lets them through (the call then stops at the next check, an
    empty output, before anything is launched)"""
    rc, msg = _conv_call(L, name, _geom(L, stride_w=stride_w, H=3))
    assert rc != 0 and "stride_w" not in msg and "empty output" in msg, (rc, msg)
