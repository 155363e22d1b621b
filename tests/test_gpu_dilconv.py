"""Dilated convolution (ConvLayer dilation): the ops tn_dilconv_* (fp32 NCHW) and tn_c8_dilconv_* (the 16-bit conv stack,
float16 with gradient scale 4096 and bfloat16) through the C-ABI against a plain float64 convolution with the zero-stuffed
weights (tests/test_dilconv_cpu.dil_ref) of the inputs as stored -- for the 16-bit types inputs and weights rounded with
tests/c8_util.r16 / tests/c8b_util.rbf16.  Every c8 output is pre-filled with garbage (0x5555) and read back through
tests/test_gpu_c8_conv1._get, which wants pad cells as exact 0; the float32 outputs are filled with 7; the guard bands and
the 0xFF poison catch a cell the op forgot or overran.

Tolerances are the project's own for the same arithmetic (tests/test_gpu_gconv.py): float32 assert_close's defaults;
stored 16-bit tensors TOL16; dW / db the larger of the project's bound and the worst case of ANY fp32 summation order,
n u sum|terms| with n = N So So, u = 2^-24, the sum of absolute terms taken from the float64 reference.

Without the feature every test fails at the first call: the library exports no tn_dilconv_fwd / tn_c8_dilconv_fwd."""
import numpy as np
import pytest

from tests.gpu_util import act_code, assert_close, call, ctx, dev
from tests.test_dilconv_cpu import CASES, as_gconv, dil_ref, pad_of
from tests.test_gconv_cpu import SLOPE, check_grads, inputs
from tests.test_gpu_c8_conv1 import TOL16, _R, _c8, _garbage, _get
from tests.test_gpu_c8_convg import _own_the_context  # noqa: F401  (autouse: dW / db are read right after the call)
from tests.test_gpu_c8_mean import GS
from tests.test_gpu_dwconv import _close16
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%d-%d@%d-f%dd%d%s" % c[:8] for c in CASES])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_dilconv_ops(dtype, case):
    N, C, K, S, P, f, d, mode, So, Po = case
    pad = pad_of(f, d, mode)
    c8 = dtype != "float32"
    gs = GS[dtype] if c8 else 1.
    ctx().set_matmul_dtype(dtype, gs)
    if c8 and (C % 8 or K % 8):                                # ragged octets: as the general family answers; float32 runs
        lib = ctx().lib
        assert lib.tn_c8_dilconv_supported(N, C, S, P, K, d, f, 1, pad, So, Po) == \
            lib.tn_c8_convg_supported(N, C, S, P, K, (f - 1) * d + 1, 1, pad, So, Po) == 1
        return
    R = _R(dtype) if c8 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    x, dzs, W, b, prev = inputs(as_gconv(case), R, gs)
    # weights at fan-in scale, as a layer's initialisation draws them: pre-activations of unit variance at every C, so that
    # fp32's rounding of a sum of C f f terms (2304 at 256 maps) is held to assert_close's absolute term at the scale of z
    W = (W / np.sqrt(C)).astype(np.float32)
    z, dx, dW, db, aW, ab = dil_ref(x, R(W), b.astype(np.float64), dzs, d, pad)
    if c8:
        op, geom = "tn_c8_dilconv_", (N, C, S, P, K, d, f, 1, pad, So, Po)
        put = lambda a, p: _c8(a, p, dtype)
        get = lambda t, m, side: _get(t, m, side, dtype)
        close = lambda got, want, what: _close16(got, R(want), TOL16[dtype], what)
    else:
        op, geom = "tn_dilconv_", (N, C, S, S, K, d, f, 1, pad, So, So)
        put = lambda a, p: dev(a.astype(np.float32))
        get = lambda t, m, side: t.get_value()
        close = lambda got, want, what: assert_close(got, want, what=what)
    assert getattr(ctx().lib, op + "supported")(*geom)
    xd, dzd, pd, Wd, bd = put(x, P), put(dzs, Po), put(prev, P), dev(W), dev(b)
    for name in ("relu10", "linear"):
        act, prm = act_code(name)
        y = _out(c8, N, K, So, Po)
        call(op + "fwd", xd.ptr, Wd.ptr, bd.ptr, y.ptr, *geom, act, prm)
        close(get(y, K, So), np.where(z > 0, z, SLOPE * z) if name == "relu10" else z, "fwd " + name)
    act, prm = act_code("relu10")
    for p_, deriv in ((pd.ptr, np.where(prev > 0, 1., np.where(prev < 0, SLOPE, 1 + SLOPE))), (None, 1.)):
        o = _out(c8, N, C, S, P)
        call(op + "dgrad", dzd.ptr, Wd.ptr, o.ptr, *geom, p_, act, prm)
        close(get(o, C, S), dx * deriv, "dgrad with prev_a" if p_ else "dgrad")
    gW, gb = dev(np.full(W.shape, 7., np.float32)), dev(np.full((K,), 7., np.float32))
    call(op + "wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *geom)
    check_grads(gW.get_value(), gb.get_value(), dW, db, aW, ab, N * So * So, c8, gs)


def _out(c8, N, maps, side, pitch):
    """An output tensor with its fill: garbage cells on the stack, 7 in float32."""
    return _garbage(N, maps, pitch) if c8 else dev(np.full((N, maps, side, side), 7., np.float32))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_dilconv_refuses_bad_arguments(dtype):
    """Bad geometry and NULL tensors: BackendError naming the entry point, nothing launched (the output keeps its fill)."""
    from theanet_amd import _lib
    c8 = dtype != "float32"
    ctx().set_matmul_dtype(dtype, 1.)
    op = "tn_c8_dilconv_" if c8 else "tn_dilconv_"
    x, y = (_c8(np.zeros((2, 16, 8, 8)), 8, dtype), _out(True, 2, 16, 8, 8)) if c8 else \
        (dev(np.zeros((2, 16, 8, 8), np.float32)), _out(False, 2, 16, 8, 8))
    W, b = dev(np.zeros((16, 16, 3, 3), np.float32)), dev(np.zeros((16,), np.float32))
    fill = np.asarray(y.get_value()).copy()
    ok = (2, 16, 8, 8, 16, 2, 3, 1, 2, 8, 8)
    # d = 0; d = 2 with stride 2; inconsistent So
    for g in ((2, 16, 8, 8, 16, 0, 3, 1, 1, 8, 8), (2, 16, 8, 8, 16, 2, 3, 2, 2, 4, 4), (2, 16, 8, 8, 16, 2, 3, 1, 2, 9, 9)):
        assert not getattr(ctx().lib, op + "supported")(*g)
        with pytest.raises(_lib.BackendError, match=op + "fwd: bad arguments"):
            call(op + "fwd", x.ptr, W.ptr, b.ptr, y.ptr, *g, 0, 0.)
    with pytest.raises(_lib.BackendError, match=op + "fwd: bad arguments"):
        call(op + "fwd", x.ptr, None, b.ptr, y.ptr, *ok, 0, 0.)
    with pytest.raises(_lib.BackendError, match=op + "dgrad: bad arguments"):
        call(op + "dgrad", None, W.ptr, y.ptr, *ok, None, 0, 0.)
    with pytest.raises(_lib.BackendError, match=op + "wgrad: bad arguments"):
        call(op + "wgrad", x.ptr, None, W.ptr, b.ptr, *ok)
    assert np.array_equal(np.asarray(y.get_value()), fill)
