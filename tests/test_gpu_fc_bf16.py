"""MATMUL 'bfloat16' (tn_set_fc_matmul mode 2, theanet_amd/csrc/gemm_bf16.hip), op by op through the C-ABI.

The statement, written here: with R = tests.c8b_util.rbf16 (nearest bf16, ties to even)

    forward         a  = act(R(x) @ R(W) + b) [* mask]
    input gradient  dx = (R(dz) @ R(W).T) * act'(prev_a) [* mask]
    weight gradient dW = R(x).T @ R(dz),   db = column sums of dz (no product: dz unrounded)

products and sums in float64, the epilogue in float64.  The device accumulates in fp32, so the tolerance is the project's
own for this arithmetic (rounded operands, exact products, fp32 accumulation, fp32 result): 2e-5 of the largest entry, as
tests/test_gpu_c8_conv1.py uses for dW and db, for EVERY product of every shape.  Only a product that misses it and whose
own reduction is deep (K >= DEEP_K) may fall back to 2x the error of the same product with numpy float32 accumulation of
the same rounded operands against float64 (_tol), and says so in its output."""
import numpy as np
import pytest

from tests import c8b_util as CB
from tests.gpu_util import act_code, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

R = CB.rbf16

# (B, n_in, n_out): the headline layer, a wide layer, and every ragged edge tn_b3_fc_ok rejects
SHAPES = [(4096, 500, 500),        # mnist.prms' dense layer at batch 4096; the weight gradient runs 8 split-K slabs
          (2048, 2048, 2048),      # wide
          (126, 64, 48),           # B not a multiple of 4
          (64, 50, 37),            # n_in, n_out not multiples of 4
          (64, 24, 40),            # n_in < 32
          (32, 40, 10),            # n_out <= 16
          (3, 33, 5),              # B < 4, everything ragged
          (8192, 96, 72)]          # K of the weight gradient deep enough for several slabs, few tiles


@pytest.fixture(autouse=True)
def _mode():
    yield
    call("tn_set_fc_matmul", 0)
    ctx()._fc_mm = "float32"


def _act(name, z):
    from oracle import theanet_oracle as O
    return O.activation(name)[0](z)


def _grad_from_out(name, a):
    from oracle import theanet_oracle as O
    return O.act_grad_from_out(name, a)


DEEP_K = 2048


def _tol(got, want, what, K=0, f32_acc=None):
    """2e-5 of the largest entry.  A product that misses it, with a reduction of K >= DEEP_K terms, is held to 2x the
    error of float32 accumulation (f32_acc(): numpy, same rounded operands) against float64 instead."""
    scale = np.abs(want).max()
    err = np.abs(got.astype(np.float64) - want).max()
    bound = 2e-5 * scale
    print("%s: max err %.3g, 2e-5 * max %.3g" % (what, err, bound))
    if err > bound and K >= DEEP_K and f32_acc is not None:
        bound = 2. * np.abs(f32_acc().astype(np.float64) - want).max()
        print("%s: deep reduction (K = %d): 2x the float32-accumulation error %.3g" % (what, K, bound))
    assert err <= bound, (what, err, bound)
    return err


def _case(B, n_in, n_out, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randn(B, n_in).astype(np.float32)
    W = (rng.randn(n_in, n_out) / np.sqrt(n_in)).astype(np.float32)
    b = (rng.randn(n_out) * .1).astype(np.float32)
    dz = (rng.randn(B, n_out) * .1).astype(np.float32)
    return rng, x, W, b, dz


def _f32_acc(a, b):
    return np.matmul(a.astype(np.float32), b.astype(np.float32))


def _ws(B, n_in, n_out):
    n = ctx().lib.tn_fc_wgrad_ws_bytes(B, n_in, n_out)
    return empty(((n + 3) // 4,))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fc_bf16_three_products_match_rounded_operand_statement(shape):
    """Every product of a layer, any shape, and closer to the rounded-operand statement than the unrounded float64
    product is (the mode is not a no-op).  Every product is first held to 2e-5 of its largest entry; the reduction depth
    passed to _tol is that product's own (n_in, n_out, B, B)."""
    B, n_in, n_out = shape
    rng, x, W, b, dz = _case(B, n_in, n_out)
    x64, W64, dz64 = x.astype(np.float64), W.astype(np.float64), dz.astype(np.float64)
    Rx, RW, Rdz = R(x), R(W), R(dz)
    xd, Wd, bd, dzd = dev(x), dev(W), dev(b), dev(dz)
    a, dx, dW, db = empty((B, n_out)), empty((B, n_in)), empty((n_in, n_out)), empty((n_out,))
    ws = _ws(B, n_in, n_out)
    kind, prm = act_code("linear")
    call("tn_set_fc_matmul", 2)
    call("tn_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, n_in, n_out, kind, prm, None)
    call("tn_fc_dgrad", dzd.ptr, Wd.ptr, dx.ptr, B, n_in, n_out, None, kind, prm, None)
    call("tn_fc_wgrad", xd.ptr, dzd.ptr, dW.ptr, db.ptr, B, n_in, n_out, ws.ptr)
    got = [v.get_value() for v in (a, dx, dW, db)]
    # the fused backward entry point gives the same bits as its two halves
    dx2, dW2, db2 = empty((B, n_in)), empty((n_in, n_out)), empty((n_out,))
    call("tn_fc_bwd", xd.ptr, dzd.ptr, Wd.ptr, dW2.ptr, db2.ptr, dx2.ptr, B, n_in, n_out, ws.ptr, None, kind, prm, None)
    for u, v in zip(got[1:], (dx2, dW2, db2)):
        np.testing.assert_array_equal(u, v.get_value())
    want = [Rx @ RW + b, Rdz @ RW.T, Rx.T @ Rdz, dz64.sum(0)]
    plain = [x64 @ W64 + b, dz64 @ W64.T, x64.T @ dz64, None]
    acc32 = [lambda: _f32_acc(Rx, RW) + b, lambda: _f32_acc(Rdz, RW.T), lambda: _f32_acc(Rx.T, Rdz),
             lambda: dz.sum(0, dtype=np.float32)]
    depth = [n_in, n_out, B, B]                       # the reduction of each product
    for name, g, w, p, f, K in zip(("fwd", "dgrad", "wgrad", "db"), got, want, plain, acc32, depth):
        err = _tol(g, w, "%s %s" % (name, shape), K, f)
        if p is not None:
            err_plain = np.abs(g.astype(np.float64) - p).max()
            err_stmt = np.abs(w - p).max()         # what the rounding of the operands is worth
            assert err < .5 * err_stmt + 1e-7 * np.abs(w).max(), (name, err, err_stmt)
            assert err < err_plain or err_stmt == 0, (name, err, err_plain)


ACTS = ["relu", "relu01", "relu10", "tanh", "sigmoid", "softplus", "scaled_tanh", "linear"]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_fc_bf16_epilogues(act, masked):
    """Bias + activation (+ mask) of the forward; act'(prev_a) (+ mask) of the input gradient, prev_a with planted
    exact zeros (the tie derivative of the leaky family) and prev_a NULL."""
    B, n_in, n_out = 70, 52, 45
    rng, x, W, b, dz = _case(B, n_in, n_out, seed=3)
    kind, prm = act_code(act)
    mask = (rng.rand(B, n_out) > .4).astype(np.uint8)
    xd, Wd, bd, dzd, md = dev(x), dev(W), dev(b), dev(dz), dev(mask)
    a = empty((B, n_out))
    call("tn_set_fc_matmul", 2)
    call("tn_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, n_in, n_out, kind, prm, md.ptr if masked else None)
    want = _act(act, R(x) @ R(W) + b)
    if masked:
        want = want * mask
    _tol(a.get_value(), want, "fwd %s" % act)
    # input gradient: prev_a is the OUTPUT of the layer below (act applied), with exact zeros planted
    prev = _act(act, rng.randn(B, n_in)).astype(np.float32)
    prev[rng.rand(B, n_in) < .1] = 0.
    pmask = (rng.rand(B, n_in) > .3).astype(np.uint8)
    pd, pmd = dev(prev), dev(pmask)
    dx = empty((B, n_in))
    for with_prev in (True, False):
        call("tn_fc_dgrad", dzd.ptr, Wd.ptr, dx.ptr, B, n_in, n_out, pd.ptr if with_prev else None, kind, prm,
             pmd.ptr if masked else None)
        want = R(dz) @ R(W).T
        if with_prev:
            want = want * _grad_from_out(act, prev.astype(np.float64))
        if masked:
            want = want * pmask
        _tol(dx.get_value(), want, "dgrad %s prev_a %s" % (act, with_prev))


def test_fc_bf16_is_deterministic_and_leaves_fp32_path_intact():
    """Same input twice -> same bits (weight gradient with its split-K slabs included), every product differs from the
    fp32 path's, and after mode 0 is set again the calls return the bits they returned in mode 0 before (run alone, that
    is before mode 2 was ever set in the process)."""
    B, n_in, n_out = 4096, 500, 500
    rng, x, W, b, dz = _case(B, n_in, n_out, seed=5)
    xd, Wd, bd, dzd = dev(x), dev(W), dev(b), dev(dz)
    ws = _ws(B, n_in, n_out)
    kind, prm = act_code("relu10")

    def run():
        a, dx, dW, db = empty((B, n_out)), empty((B, n_in)), empty((n_in, n_out)), empty((n_out,))
        call("tn_fc_fwd", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, n_in, n_out, kind, prm, None)
        call("tn_fc_bwd", xd.ptr, dzd.ptr, Wd.ptr, dW.ptr, db.ptr, dx.ptr, B, n_in, n_out, ws.ptr, xd.ptr, kind, prm, None)
        return [v.get_value() for v in (a, dx, dW, db)]

    call("tn_set_fc_matmul", 0)
    before = run()
    call("tn_set_fc_matmul", 2)
    one, two = run(), run()
    for u, v in zip(one, two):
        np.testing.assert_array_equal(u, v)
    assert all((u != v).any() for u, v in zip(one[:3], before[:3]))        # the mode does something, in every product
    call("tn_set_fc_matmul", 0)
    for u, v in zip(before, run()):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("shape", [(256, 500, 500), (62, 50, 37)], ids=["aligned", "ragged"])
def test_fc_bf16_fwd_dropout_draws_the_fp32_paths_mask(shape):
    """tn_fc_fwd_dropout in mode 2: mask bytes equal those of the same call in mode 0 (and tn_dropout_mask's), and the
    output is the masked forward statement."""
    B, n_in, n_out = shape
    rng, x, W, b, dz = _case(B, n_in, n_out, seed=7)
    xd, Wd, bd = dev(x), dev(W), dev(b)
    kind, prm = act_code("relu10")
    masks, outs = [], []
    for mode in (0, 2):
        call("tn_set_fc_matmul", mode)
        a, m = empty((B, n_out)), dev(np.full((B, n_out), 7, np.uint8))
        call("tn_fc_fwd_dropout", xd.ptr, Wd.ptr, bd.ptr, a.ptr, B, n_in, n_out, kind, prm, m.ptr, .5, 1234567, 3, None, 96)
        masks.append(m.get_value())
        outs.append(a.get_value())
    ref = dev(np.full((B, n_out), 7, np.uint8))
    call("tn_dropout_mask", ref.ptr, B * n_out, .5, 1234567, 3, None, 96)
    np.testing.assert_array_equal(masks[0], masks[1])
    np.testing.assert_array_equal(masks[1], ref.get_value())
    assert 0 < (masks[1] != 0).mean() < 1
    _tol(outs[1], _act("relu10", R(x) @ R(W) + b) * (masks[1] != 0), "fwd_dropout %s" % (shape,))


def test_fc_bf16_refuses_bad_arguments():
    with pytest.raises(Exception, match="tn_set_fc_matmul"):
        call("tn_set_fc_matmul", 3)
    with pytest.raises(Exception):
        call("tn_set_fc_matmul", -1)
    B, n_in, n_out = 8, 12, 20
    x, W, b = dev(np.ones((B, n_in), np.float32)), dev(np.ones((n_in, n_out), np.float32)), dev(np.ones((n_out,), np.float32))
    dz = dev(np.ones((B, n_out), np.float32))
    sent = np.float32(-77.5)
    a, dx = dev(np.full((B, n_out), sent)), dev(np.full((B, n_in), sent))
    dW, db = dev(np.full((n_in, n_out), sent)), dev(np.full((n_out,), sent))
    m = dev(np.full((B, n_out), 0x55, np.uint8))
    ws = _ws(B, n_in, n_out)
    call("tn_set_fc_matmul", 2)
    g = (B, n_in, n_out)
    for args in ((None, W.ptr, b.ptr, a.ptr), (x.ptr, None, b.ptr, a.ptr), (x.ptr, W.ptr, None, a.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(Exception):
            call("tn_fc_fwd", *args, *g, 0, 0., None)
        with pytest.raises(Exception):
            call("tn_fc_fwd_dropout", *args, *g, 0, 0., m.ptr if args[3] is not None else None, .5, 1, 0, None, 0)
    for args in ((None, W.ptr, dx.ptr), (dz.ptr, None, dx.ptr), (dz.ptr, W.ptr, None)):
        with pytest.raises(Exception):
            call("tn_fc_dgrad", *args, *g, None, 0, 0., None)
    for args in ((None, dz.ptr, dW.ptr, db.ptr), (x.ptr, None, dW.ptr, db.ptr), (x.ptr, dz.ptr, None, db.ptr), (x.ptr, dz.ptr, dW.ptr, None)):
        with pytest.raises(Exception):
            call("tn_fc_wgrad", *args, *g, ws.ptr)
    with pytest.raises(Exception):
        call("tn_fc_wgrad", x.ptr, dz.ptr, dW.ptr, db.ptr, *g, None)
    for args in ((None, dz.ptr, W.ptr, dW.ptr, db.ptr, dx.ptr), (x.ptr, None, W.ptr, dW.ptr, db.ptr, dx.ptr),
                 (x.ptr, dz.ptr, None, dW.ptr, db.ptr, dx.ptr), (x.ptr, dz.ptr, W.ptr, None, db.ptr, dx.ptr),
                 (x.ptr, dz.ptr, W.ptr, dW.ptr, None, dx.ptr), (x.ptr, dz.ptr, W.ptr, dW.ptr, db.ptr, None)):
        with pytest.raises(Exception):
            call("tn_fc_bwd", *args, *g, ws.ptr, None, 0, 0., None)
    for bad in ((0, n_in, n_out), (B, 0, n_out), (B, n_in, 0)):
        with pytest.raises(Exception):
            call("tn_fc_fwd", x.ptr, W.ptr, b.ptr, a.ptr, *bad, 0, 0., None)
        with pytest.raises(Exception):
            call("tn_fc_dgrad", dz.ptr, W.ptr, dx.ptr, *bad, None, 0, 0., None)
        with pytest.raises(Exception):
            call("tn_fc_wgrad", x.ptr, dz.ptr, dW.ptr, db.ptr, *bad, ws.ptr)
        with pytest.raises(Exception):
            call("tn_fc_bwd", x.ptr, dz.ptr, W.ptr, dW.ptr, db.ptr, dx.ptr, *bad, ws.ptr, None, 0, 0., None)
    for t in (a, dx, dW, db):
        assert (t.get_value() == sent).all()               # nothing was launched
    assert (m.get_value() == 0x55).all()
