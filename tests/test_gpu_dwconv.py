"""Depthwise convolution (ConvLayer depthwise): the ops tn_dwconv_* (fp32 NCHW) and tn_c8_dwconv_* (the 16-bit conv stack,
float16 with gradient scale 4096 and bfloat16) through the C-ABI against a plain float64 depthwise convolution of the
inputs as stored -- for the 16-bit types inputs and weights rounded with tests/c8_util.r16 / tests/c8b_util.rbf16.
Every c8 output is pre-filled with garbage (0x5555) and read back through tests/test_gpu_c8_conv1._get, which wants pad
cells and channels past C as exact 0; the guard bands and the 0xFF poison catch a cell the op forgot or overran.

Tolerances are the project's own for the same arithmetic: float32 assert_close's defaults; stored 16-bit tensors 1e-3
(fp16) / 1e-2 (bf16) of the largest entry and fp32 dW / db 2e-5 of the largest entry (tests/test_gpu_c8_convg.py).  dW
and db sum N So So terms in fp32 in an order of the kernel's own, so for them the bound is the larger of that and the
worst case of ANY fp32 summation order, n u sum|terms| with n = N So So terms, u = 2^-24, taken from the float64 sum of
absolute terms of the reference -- never from the kernel's output.

Without the feature every test fails at the first call: the library exports no tn_dwconv_fwd / tn_c8_dwconv_fwd."""
import numpy as np
import pytest

from tests.gpu_util import act_code, assert_close, call, ctx, dev
from tests.test_gpu_c8_conv1 import TOL16, _R, _c8, _garbage, _get, _rel
from tests.test_gpu_c8_convg import _own_the_context  # noqa: F401  (autouse: dW / db are read right after the call)
from tests.test_gpu_c8_mean import GS
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

# (N, C, S, P, f, mode, stride, So, Po)
CASES = [
    (2, 8, 8, 8, 3, "same", 1, 8, 8),          # base case, one octet, whole plane per block
    (3, 12, 7, 8, 5, "same", 1, 7, 8),         # ragged octet, pitch above side, 5x5 weights, pad cells as +0
    (2, 3, 10, 16, 3, "valid", 2, 4, 8),       # fewer than 8 channels, stride 2, row / column 9 in no window (dx +0)
    (2, 16, 12, 16, 5, "valid", 2, 4, 8),      # 5x5 with stride
    (3, 8, 33, 64, 3, "same", 1, 33, 64),      # several row tiles with halo between them, ragged strip, slabs
    (2, 8, 36, 64, 3, "valid", 2, 17, 32),     # stride 2 on a large tile: the 16-bit halo tile outgrows LDS, strips idle
]
SLOPE = .1


def ref(x, W, b, dz, stride, pad):
    """float64: z, dx (before act'), dW, db of z[n,c,i,j] = b[c] + sum xpad[n,c,i s+u,j s+v] W[c,0,f-1-u,f-1-v]; and the
    sums of absolute terms of dW and db."""
    N, C, S, _ = x.shape
    f, So = W.shape[-1], dz.shape[-1]
    xp = np.zeros((N, C, S + 2 * f, S + 2 * f))
    xp[:, :, pad:pad + S, pad:pad + S] = x
    z, dxp, dW, aW = np.zeros(dz.shape) + b[None, :, None, None], np.zeros(xp.shape), np.zeros(W.shape), np.zeros(W.shape)
    for u in range(f):
        for v in range(f):
            win = (slice(None), slice(None), slice(u, u + stride * So, stride), slice(v, v + stride * So, stride))
            w = W[:, 0, f - 1 - u, f - 1 - v][None, :, None, None]
            z += xp[win] * w
            dxp[win] += dz * w
            dW[:, 0, f - 1 - u, f - 1 - v] = (dz * xp[win]).sum((0, 2, 3))
            aW[:, 0, f - 1 - u, f - 1 - v] = np.abs(dz * xp[win]).sum((0, 2, 3))
    return z, dxp[:, :, pad:pad + S, pad:pad + S], dW, dz.sum((0, 2, 3)), aW, np.abs(dz).sum((0, 2, 3))


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d@%d-f%d%ss%d" % c[:7] for c in CASES])
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_dwconv_ops(dtype, case):
    N, C, S, P, f, mode, stride, So, Po = case
    pad = f - 1 - (f - 1) // 2 if mode == "same" else 0
    c8 = dtype != "float32"
    gs = GS[dtype] if c8 else 1.
    ctx().set_matmul_dtype(dtype, gs)
    R = _R(dtype) if c8 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    rng = np.random.RandomState(0)
    x, dzs = R(rng.randn(N, C, S, S)), R(gs * rng.randn(N, C, So, So) * 1e-3)
    W = (rng.randn(C, 1, f, f) / f).astype(np.float32)
    b = (rng.randn(C) * .1).astype(np.float32)
    prev = R(rng.randn(N, C, S, S))
    prev[0, 0, 0, :2] = 0                                     # the tie derivative
    z, dx, dW, db, aW, ab = ref(x, R(W), b.astype(np.float64), dzs, stride, pad)
    if c8:
        op, g = "tn_c8_dwconv_", (N, C, S, P, f, stride, pad, So, Po)
        put = lambda a, p: _c8(a, p, dtype)
        out, get = (lambda side, p: _garbage(N, C, p)), (lambda t, side: _get(t, C, side, dtype))
        close = lambda got, want, what: _close16(got, R(want), TOL16[dtype], what)
    else:
        op, g = "tn_dwconv_", (N, C, S, S, f, stride, pad, So, So)
        put = lambda a, p: dev(a.astype(np.float32))
        out, get = (lambda side, p: dev(np.full((N, C, side, side), 7., np.float32))), (lambda t, side: t.get_value())
        close = lambda got, want, what: assert_close(got, want, what=what)
    assert getattr(ctx().lib, op + "supported")(*g)
    xd, dzd, pd, Wd, bd = put(x, P), put(dzs, Po), put(prev, P), dev(W), dev(b)
    for name in ("relu10", "linear"):
        act, prm = act_code(name)
        y = out(So, Po)
        call(op + "fwd", xd.ptr, Wd.ptr, bd.ptr, y.ptr, *g, act, prm)
        close(get(y, So), np.where(z > 0, z, SLOPE * z) if name == "relu10" else z, "fwd " + name)
    act, prm = act_code("relu10")
    for p_, deriv in ((pd.ptr, np.where(prev > 0, 1., np.where(prev < 0, SLOPE, 1 + SLOPE))), (None, 1.)):
        o = out(S, P)
        call(op + "dgrad", dzd.ptr, Wd.ptr, o.ptr, *g, p_, act, prm)
        close(get(o, S), dx * deriv, "dgrad with prev_a" if p_ else "dgrad")
        if stride == 2 and S == 10:                           # row / column 9 lie in no window: +0, the bits
            raw = np.asarray(o.get_value())
            edge = (raw[:, :, 9:] , raw[:, :, :, 9:]) if c8 else (raw[:, :, 9], raw[:, :, :, 9])
            assert not any(e.view(np.uint32 if not c8 else np.uint16).any() for e in edge)
    gW, gb = dev(np.full((C, 1, f, f), 7., np.float32)), dev(np.full((C,), 7., np.float32))
    call(op + "wgrad", xd.ptr, dzd.ptr, gW.ptr, gb.ptr, *g)
    n_u = (N * So * So + 1) * 2.0 ** -24                       # (+ 1: an fp32 product is rounded, a 16-bit one exact)
    for what, got, want, absum in (("dW", gW.get_value(), dW / gs, aW / gs), ("db", gb.get_value(), db / gs, ab / gs)):
        own = 2e-5 * np.abs(want).max() if c8 else 1e-5 + 1e-4 * np.abs(want)
        err, bound = np.abs(got - want), np.maximum(own, n_u * absum)
        print("%s: max err %.3g, smallest bound %.3g" % (what, err.max(), bound.min()))
        assert (err <= bound).all(), (what, err.max())


def _close16(got, want, tol, what):
    e = _rel(got, want)
    print("%s: %.3g (bound %g)" % (what, e, tol))
    assert e < tol, (what, e, tol)


def test_dwconv_refuses_bad_arguments():
    """Bad geometry and NULL tensors: BackendError naming the entry point, nothing launched (the output keeps its fill)."""
    from theanet_amd import _lib
    ctx().set_matmul_dtype("float32", 1.)
    x, y = dev(np.zeros((2, 8, 8, 8), np.float32)), dev(np.full((2, 8, 8, 8), 7., np.float32))
    W, b = dev(np.zeros((8, 1, 3, 3), np.float32)), dev(np.zeros((8,), np.float32))
    ok = (2, 8, 8, 8, 3, 1, 1, 8, 8)
    for g in ((2, 8, 8, 8, 4, 1, 1, 7, 7), (2, 8, 8, 8, 3, 1, 1, 9, 9), (2, 8, 8, 8, 3, 0, 1, 8, 8), (0, 8, 8, 8, 3, 1, 1, 8, 8)):
        assert not ctx().lib.tn_dwconv_supported(*g)
        with pytest.raises(_lib.BackendError, match="tn_dwconv_fwd: bad arguments"):
            call("tn_dwconv_fwd", x.ptr, W.ptr, b.ptr, y.ptr, *g, 0, 0.)
    with pytest.raises(_lib.BackendError, match="tn_dwconv_dgrad: bad arguments"):
        call("tn_dwconv_dgrad", None, W.ptr, y.ptr, *ok, None, 0, 0.)
    with pytest.raises(_lib.BackendError, match="tn_dwconv_wgrad: bad arguments"):
        call("tn_dwconv_wgrad", x.ptr, None, W.ptr, b.ptr, *ok)
    assert (y.get_value() == 7.).all()
