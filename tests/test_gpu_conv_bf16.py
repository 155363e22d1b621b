"""CONV 'bfloat16' (tn_set_conv_matmul mode 2, theanet_amd/csrc/conv_bf16.hip), op by op through the C-ABI.

The statement, written here: with R = tests.c8b_util.rbf16 (nearest bf16, ties to even) and conv the true convolution of
the oracle (oracle.theanet_oracle.conv2d_fwd / conv2d_bwd, any filter, mode and stride)

    forward         a  = act(conv(R(x), R(W)) + b)
    input gradient  dx = conv^T(R(dz), R(W)) * act'(prev_a)              (prev_a NULL: no derivative)
    weight gradient dW = R(x) (*) R(dz),   db = sum of dz over samples and pixels (no product: dz unrounded)

products and sums in float64, the epilogue in float64.  The device accumulates in fp32, so the tolerance is the project's
own for this arithmetic, _tol of tests/test_gpu_fc_bf16.py: 2e-5 of the largest entry for EVERY product; only a product
that misses it and whose own reduction has >= 2048 terms may fall back to 2x the error of the same product with numpy
float32 accumulation of the same rounded operands, and says so.  Every shape also asserts that the mode is not a no-op:
the result lies further from the unrounded statement than from the rounded one."""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import act_code, call, ctx, dev, empty
from tests.test_gpu_fc_bf16 import _tol
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

R = CB.rbf16

# (N, C, S, K, f, mode, stride): the smallest shapes at which the kernels can still go wrong
SHAPES = [(3, 1, 12, 4, 3, "valid", 1),        # reduction of 9 < 16, K < 8, first layer
          (5, 4, 13, 20, 3, "valid", 1),       # odd maps (13 -> 11), K = 20, reduction 36 not a multiple of 16
          (2, 3, 16, 16, 5, "same", 1),        # halo of 2, reduction 75
          (4, 16, 14, 24, 5, "valid", 1),      # reduction 400
          (3, 8, 9, 10, 2, "same", 1),         # even filter, asymmetric padding
          (6, 12, 16, 16, 1, "valid", 2),      # 1x1 stride 2
          (2, 6, 17, 9, 3, "valid", 3),        # (17-3+1) // 3 = 5, stride 3 in dgrad
          (70, 32, 16, 40, 3, "same", 1),      # several row tiles, N*Ho*Wo not a multiple of 32
          (1, 40, 6, 33, 3, "same", 1),        # fewer than 64 output pixels
          (256, 8, 8, 8, 3, "same", 1)]        # weight-gradient reduction 16384: several slabs, the only deep case


@pytest.fixture(autouse=True)
def _mode():
    yield
    call("tn_set_conv_matmul", 0)
    ctx()._conv_mm = "float32"


def _case(N, C, S, K, f, mode, stride, seed=0):
    rng = np.random.RandomState(seed)
    pad_lo, _, So = O.conv_geometry(S, f, stride, mode)
    x = rng.randn(N, C, S, S).astype(np.float32)
    W = (rng.randn(K, C, f, f) / np.sqrt(C * f * f)).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    dz = (rng.randn(N, K, So, So) * .1).astype(np.float32)
    return rng, x, W, b, dz, (N, C, S, S, K, f, stride, pad_lo, So, So)


def _f64(a):
    return np.asarray(a, np.float64)


def _statement(x, W, b, dz, mode, stride, rnd):
    """(z, dx, dW, db) in float64; rnd rounds the operands of the three products (db sums the unrounded dz)."""
    z = O.conv2d_fwd(rnd(x), rnd(W), _f64(b), stride, mode)
    dx, dW, _ = O.conv2d_bwd(rnd(x), rnd(W), rnd(dz), stride, mode)
    return z, dx, dW, _f64(dz).sum(axis=(0, 2, 3))


def _acc32(x, W, b, dz, mode, stride):
    """The same products on the same rounded operands with numpy float32 accumulation."""
    f32 = lambda a: R(a).astype(np.float32)
    z = O.conv2d_fwd(f32(x), f32(W), b, stride, mode)
    dx, dW, _ = O.conv2d_bwd(f32(x), f32(W), f32(dz), stride, mode)
    return z, dx, dW, dz.sum(axis=(0, 2, 3), dtype=np.float32)


def _run(xd, Wd, bd, dzd, geom, act="linear", prev=None, pact="linear"):
    N, C, S, _, K, f, stride, pad_lo, So, _ = geom
    a, dx, dW, db = empty((N, K, So, So)), empty((N, C, S, S)), empty((K, C, f, f)), empty((K,))
    kind, prm = act_code(act)
    pkind, pprm = act_code(pact)
    call("tn_conv2d_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, *geom, kind, prm)
    call("tn_conv2d_dgrad", dzd.ptr, Wd.ptr, dx.ptr, *geom, prev.ptr if prev is not None else None, pkind, pprm)
    call("tn_conv2d_wgrad", xd.ptr, dzd.ptr, dW.ptr, db.ptr, *geom)
    return [v.get_value() for v in (a, dx, dW, db)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_bf16_three_products_match_rounded_operand_statement(shape):
    N, C, S, K, f, mode, stride = shape
    rng, x, W, b, dz, geom = _case(*shape)
    So = geom[8]
    call("tn_set_conv_matmul", 2)
    got = _run(dev(x), dev(W), dev(b), dev(dz), geom)
    want = _statement(x, W, b, dz, mode, stride, R)
    plain = _statement(x, W, b, dz, mode, stride, _f64)
    depth = [C * f * f, K * f * f, N * So * So, N * So * So]         # the reduction of each product
    acc = {}

    def f32_acc(i):
        if not acc:
            acc["v"] = _acc32(x, W, b, dz, mode, stride)
        return acc["v"][i]

    for i, name in enumerate(("fwd", "dgrad", "wgrad", "db")):
        err = _tol(got[i], want[i], "%s %s" % (name, shape), depth[i], lambda i=i: f32_acc(i))
        if name != "db":
            err_plain = np.abs(got[i].astype(np.float64) - plain[i]).max()
            print("%s %s: against the unrounded statement %.3g" % (name, shape, err_plain))
            assert err < err_plain, (name, err, err_plain)


@pytest.mark.parametrize("act", ["relu10", "tanh", "sigmoid", "linear"])
def test_conv_bf16_epilogues(act):
    """Bias + activation of the forward; act'(prev_a) of the input gradient, prev_a with planted exact zeros (the tie
    derivative of the leaky family) and prev_a NULL -- on a ragged shape."""
    shape = (5, 4, 13, 20, 3, "valid", 1)
    N, C, S, K, f, mode, stride = shape
    rng, x, W, b, dz, geom = _case(*shape, seed=3)
    z, dx, _, _ = _statement(x, W, b, dz, mode, stride, R)
    prev = O.activation(act)[0](rng.randn(N, C, S, S)).astype(np.float32)
    prev[rng.rand(N, C, S, S) < .1] = 0.
    xd, Wd, bd, dzd, pd = dev(x), dev(W), dev(b), dev(dz), dev(prev)
    call("tn_set_conv_matmul", 2)
    for with_prev in (True, False):
        got = _run(xd, Wd, bd, dzd, geom, act, pd if with_prev else None, act)
        _tol(got[0], O.activation(act)[0](z), "fwd %s" % act)
        want = dx * O.act_grad_from_out(act, prev.astype(np.float64)) if with_prev else dx
        _tol(got[1], want, "dgrad %s prev_a %s" % (act, with_prev))


@pytest.mark.parametrize("shape", [(256, 8, 8, 8, 3, "same", 1), (2, 6, 17, 9, 3, "valid", 3)], ids=["slabs", "stride3"])
def test_conv_bf16_is_deterministic_and_leaves_mode_0_untouched(shape):
    """Two calls of each op give equal bits (the weight gradient's slabs included), every product differs from mode 0's,
    and mode 0 afterwards gives the bits it gave before the mode was set."""
    rng, x, W, b, dz, geom = _case(*shape, seed=5)
    prev = rng.randn(*x.shape).astype(np.float32)
    xd, Wd, bd, dzd, pd = dev(x), dev(W), dev(b), dev(dz), dev(prev)
    call("tn_set_conv_matmul", 0)
    before = _run(xd, Wd, bd, dzd, geom, "relu10", pd, "relu10")
    call("tn_set_conv_matmul", 2)
    one = _run(xd, Wd, bd, dzd, geom, "relu10", pd, "relu10")
    two = _run(xd, Wd, bd, dzd, geom, "relu10", pd, "relu10")
    for u, v in zip(one, two):
        np.testing.assert_array_equal(u, v)
    assert all((u != v).any() for u, v in zip(one[:3], before[:3]))
    call("tn_set_conv_matmul", 0)
    for u, v in zip(before, _run(xd, Wd, bd, dzd, geom, "relu10", pd, "relu10")):
        np.testing.assert_array_equal(u, v)


def test_conv_bf16_refuses_bad_arguments():
    """By name, nothing launched: modes 1 and 3, NULL tensors, a zero dimension, a shape whose index arithmetic would
    overflow 32 bits, and mode 2 while a 16-bit DTYPE is set."""
    for bad in (1, 3, -1):
        with pytest.raises(Exception, match="tn_set_conv_matmul"):
            call("tn_set_conv_matmul", bad)
    N, C, S, K, f = 2, 3, 6, 4, 3
    geom = (N, C, S, S, K, f, 1, 0, 4, 4)
    sent = np.float32(-77.5)
    x, W, b = dev(np.ones((N, C, S, S), np.float32)), dev(np.ones((K, C, f, f), np.float32)), dev(np.ones((K,), np.float32))
    dz = dev(np.ones((N, K, 4, 4), np.float32))
    a, dx = dev(np.full((N, K, 4, 4), sent)), dev(np.full((N, C, S, S), sent))
    dW, db = dev(np.full((K, C, f, f), sent)), dev(np.full((K,), sent))
    call("tn_set_conv_matmul", 2)
    for args in ((None, W.ptr, b.ptr, a.ptr), (x.ptr, None, b.ptr, a.ptr), (x.ptr, W.ptr, None, a.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(Exception, match="tn_conv2d_fwd"):
            call("tn_conv2d_fwd", *args, *geom, 0, 0.)
    for args in ((None, W.ptr, dx.ptr), (dz.ptr, None, dx.ptr), (dz.ptr, W.ptr, None)):
        with pytest.raises(Exception, match="tn_conv2d_dgrad"):
            call("tn_conv2d_dgrad", *args, *geom, None, 0, 0.)
    for args in ((None, dz.ptr, dW.ptr, db.ptr), (x.ptr, None, dW.ptr, db.ptr), (x.ptr, dz.ptr, None, db.ptr), (x.ptr, dz.ptr, dW.ptr, None)):
        with pytest.raises(Exception, match="tn_conv2d_wgrad"):
            call("tn_conv2d_wgrad", *args, *geom)
    zero = [geom[:i] + (0,) + geom[i + 1:] for i in (0, 1, 2, 3, 4, 5, 6, 8, 9)]
    huge = [(1 << 16, 1 << 10, 8, 8, K, f, 1, 0, 6, 6), (1 << 16, C, 8, 8, 1 << 10, f, 1, 1, 8, 8),
            (N, 1 << 14, S, S, 1 << 14, f, 1, 0, 4, 4)]
    for g in zero + huge:
        with pytest.raises(Exception, match="tn_conv2d_fwd"):
            call("tn_conv2d_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *g, 0, 0.)
        with pytest.raises(Exception, match="tn_conv2d_dgrad"):
            call("tn_conv2d_dgrad", dz.ptr, W.ptr, dx.ptr, *g, None, 0, 0.)
        with pytest.raises(Exception, match="tn_conv2d_wgrad"):
            call("tn_conv2d_wgrad", x.ptr, dz.ptr, dW.ptr, db.ptr, *g)
    # a 16-bit DTYPE: the mode cannot be set, and the fp32-tensor entry points keep refusing
    call("tn_set_conv_matmul", 0)
    for dt in (1, 2):
        call("tn_set_matmul_dtype", dt, 1.0)
        try:
            with pytest.raises(Exception, match="tn_set_conv_matmul"):
                call("tn_set_conv_matmul", 2)
            with pytest.raises(Exception, match="tn_conv2d_fwd"):
                call("tn_conv2d_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *geom, 0, 0.)
        finally:
            call("tn_set_matmul_dtype", 0, 1.0)
    for t in (a, dx, dW, db):
        assert (t.get_value() == sent).all()               # nothing was launched
