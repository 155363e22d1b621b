"""Grouped convolution (ConvLayer groups): the ops tn_gconv_* (fp32 NCHW) and tn_c8_gconv_* (the 16-bit conv stack, float16
with gradient scale 4096 and bfloat16) through the C-ABI against a plain float64 grouped convolution of the inputs as
stored (tests/test_gconv_cpu.ref) -- for the 16-bit types inputs and weights rounded with tests/c8_util.r16 /
tests/c8b_util.rbf16.  Every c8 output is pre-filled with garbage (0x5555) and read back through
tests/test_gpu_c8_conv1._get, which wants pad cells as exact 0; the guard bands and the 0xFF poison catch a cell the op
forgot or overran.

Tolerances are the project's own for the same arithmetic (tests/test_gpu_dwconv.py): float32 assert_close's defaults;
stored 16-bit tensors TOL16; dW / db the larger of the project's bound and the worst case of ANY fp32 summation order,
n u sum|terms| with n = N So So, u = 2^-24, the sum of absolute terms taken from the float64 reference.

Without the feature every test fails at the first call: the library exports no tn_gconv_fwd / tn_c8_gconv_fwd."""
import numpy as np
import pytest

from tests.gpu_util import act_code, assert_close, call, ctx, dev
from tests.test_gconv_cpu import CASES, SLOPE, check_grads, inputs, pad_of, ref
from tests.test_gpu_c8_conv1 import TOL16, _R, _c8, _garbage, _get
from tests.test_gpu_c8_convg import _own_the_context  # noqa: F401  (autouse: dW / db are read right after the call)
from tests.test_gpu_c8_mean import GS
from tests.test_gpu_dwconv import _close16
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%dg%d-%d@%d-f%d%ss%d" % c[:9] for c in CASES])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_gconv_ops(dtype, case):
    N, C, K, g, S, P, f, mode, stride, So, Po = case
    pad = pad_of(f, mode)
    c8 = dtype != "float32"
    gs = GS[dtype] if c8 else 1.
    ctx().set_matmul_dtype(dtype, gs)
    if c8 and ((C // g) % 8 or (K // g) % 8):               # a group that is no whole number of cells: float32 only
        assert ctx().lib.tn_c8_gconv_supported(N, C, S, P, K, g, f, stride, pad, So, Po) == 0
        return
    R = _R(dtype) if c8 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    x, dzs, W, b, prev = inputs(case, R, gs)
    z, dx, dW, db, aW, ab = ref(x, R(W), b.astype(np.float64), dzs, g, stride, pad)
    if c8:
        op, geom = "tn_c8_gconv_", (N, C, S, P, K, g, f, stride, pad, So, Po)
        put = lambda a, p: _c8(a, p, dtype)
        get = lambda t, m, side: _get(t, m, side, dtype)
        close = lambda got, want, what: _close16(got, R(want), TOL16[dtype], what)
    else:
        op, geom = "tn_gconv_", (N, C, S, S, K, g, f, stride, pad, So, So)
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
        if stride == 2 and S == 10:                           # row / column 9 lie in no window: +0, the bits
            raw = np.asarray(o.get_value())
            edge = (raw[:, :, 9:], raw[:, :, :, 9:]) if c8 else (raw[:, :, 9], raw[:, :, :, 9])
            assert not any(e.view(np.uint32 if not c8 else np.uint16).any() for e in edge)
    gW, gb = dev(np.full(W.shape, 7., np.float32)), dev(np.full((K,), 7., np.float32))
    call(op + "wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *geom)
    check_grads(gW.get_value(), gb.get_value(), dW, db, aW, ab, N * So * So, c8, gs)


def _out(c8, N, maps, side, pitch):
    """An output tensor with its fill: garbage cells on the stack, 7 in float32."""
    return _garbage(N, maps, pitch) if c8 else dev(np.full((N, maps, side, side), 7., np.float32))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_gconv_refuses_bad_arguments(dtype):
    """Bad geometry and NULL tensors: BackendError naming the entry point, nothing launched (the output keeps its fill)."""
    from theanet_amd import _lib
    c8 = dtype != "float32"
    ctx().set_matmul_dtype(dtype, 1.)
    op = "tn_c8_gconv_" if c8 else "tn_gconv_"
    x, y = (_c8(np.zeros((2, 16, 8, 8)), 8, dtype), _out(True, 2, 16, 8, 8)) if c8 else \
        (dev(np.zeros((2, 16, 8, 8), np.float32)), _out(False, 2, 16, 8, 8))
    W, b = dev(np.zeros((16, 8, 3, 3), np.float32)), dev(np.zeros((16,), np.float32))
    fill = np.asarray(y.get_value()).copy()
    ok = (2, 16, 8, 8, 16, 2, 3, 1, 1, 8, 8)
    # g not dividing K; g = 0; inconsistent So
    for g in ((2, 16, 8, 8, 24, 16, 3, 1, 1, 8, 8), (2, 16, 8, 8, 16, 0, 3, 1, 1, 8, 8), (2, 16, 8, 8, 16, 2, 3, 1, 1, 9, 9)):
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
