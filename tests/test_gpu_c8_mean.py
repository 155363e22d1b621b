"""MeanLayer on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16'): the ops tn_c8_mean_fwd / tn_c8_mean_bwd
through the C-ABI, and all-convolutional nets (conv stack -> MeanLayer -> dense head) against the stored-16-bit oracle.

Stored-16-bit semantics of Mean.  Forward: the fp32 mean of the STORED 16-bit values of the block below, not rounded -- it
is the input of fp32 dense products (oracle.theanet_oracle states this already: c["c8"] is False above a Mean layer).
Backward: the c8 gradient the block below consumes, R(grad_scale * dy / (H W) * act'(stored output below)) -- the
oracle's _f16_down applied to mean_bwd.  The oracle's own Mean backward hands the conv branch an unscaled, unrounded
gradient without act', so the net tests state the device's semantics by patching O.mean_bwd (_mean_bwd_16).

Tolerances: forward 1e-6 of the largest mean (fp32 accumulation only); backward one ulp of the 16-bit type per stored
element (the fp32 products may round once before the store does); nets those of tests/test_gpu_f16.py (fp16) and
tests/test_gpu_bf16.py (bf16); schedules bit for bit."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8_util as U
from tests import c8b_util as CB
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty, load_prms
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

GS = {"float16": 4096.0, "bfloat16": 1.0}
TOL = {"float16": ((2e-3, 2e-4), 2e-6), "bfloat16": ((1.6e-2, 1.6e-3), 1.6e-5)}     # (logprob / cost), weights abs
R16 = O.r16             # the oracle's fp16 rounding, before any test swaps it


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request, monkeypatch):
    """The element type; for bfloat16 the oracle's stored-16-bit mode rounds to bf16 (tests/test_gpu_bf16.py)."""
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    yield request.param
    monkeypatch.setattr(O, "r16", R16)


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 8, 4, 4), (37, 24, 4, 4), (5, 64, 8, 8), (128, 256, 16, 16), (3, 40, 64, 64), (2, 16, 128, 128),
          (9, 12, 6, 6)]
ACTS = ["linear", "relu10", "relu", "tanh", "sigmoid"]


def _to_c8(a, dtype):
    return CB.to_c8(a) if dtype == "bfloat16" else U.to_c8(a).view(np.uint16)


def _stored(raw, C, dtype):
    """raw c8 bits -> the stored values, (N, C, H, W) float64."""
    v = CB.from_c8(raw, C) if dtype == "bfloat16" else U.from_c8(raw.view(np.float16), C)
    return v.astype(np.float64)


def _bits(a, dtype):
    """float64 -> the 16-bit patterns of its nearest-even rounding."""
    return CB.bf16_bits(CB.rbf16(a)) if dtype == "bfloat16" else np.asarray(a, np.float64).astype(np.float16).view(np.uint16)


def _ordinal(bits):
    """16-bit float patterns (sign in bit 15) -> integers in value order, consecutive for neighbouring values, +-0 -> 0."""
    b = bits.astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_c8_mean_ops_match_numpy(dtype, shape, act):
    N, C, H, W = shape
    C8, HW, gs = (C + 7) // 8, H * W, GS[dtype]
    rng = np.random.default_rng(10 * SHAPES.index(shape) + ACTS.index(act))
    z = rng.standard_normal((N, C, H, W)) + .25
    a = z if act == "linear" else O.activation(act)[0](z)
    raw = _to_c8(a, dtype)                   # the block's stored output
    x = _stored(raw, C, dtype)
    ctx().set_matmul_dtype(dtype, gs)
    xd = dev(raw)

    y = empty((N, C))
    call("tn_c8_mean_fwd", xd.ptr, y.ptr, N, C, H, W)
    want = x.mean(axis=(2, 3))
    got = y.get_value()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (dtype, shape, act, np.abs(got - want).max())

    dy = rng.standard_normal((N, C)).astype(np.float32)
    dx = dev(np.full(raw.shape, 0x5555, np.uint16))           # garbage: every cell must be written
    kind, prm = act_code(act)
    call("tn_c8_mean_bwd", dev(dy).ptr, dx.ptr, N, C, H, W, None if act == "linear" else xd.ptr, kind, prm)
    g = gs * dy.astype(np.float64)[:, :, None, None] / HW * O.act_grad_from_out(act, x)
    got = dx.get_value()
    gb = got.transpose(0, 1, 4, 2, 3).reshape(N, C8 * 8, H, W)
    d = np.abs(_ordinal(gb[:, :C]) - _ordinal(_bits(g, dtype)))
    assert d.max() <= 1, (dtype, shape, act, "%d elements off by more than one ulp" % (d > 1).sum())
    assert (d == 0).mean() > .9                                # (one rounding apart only at rare boundaries)
    assert not gb[:, C:].any(), "padding channels must be written as 0"


def test_c8_mean_ops_refuse_bad_arguments():
    ctx().set_matmul_dtype("float16", 4096.)
    x, y = dev(np.zeros((1, 1, 4, 4, 8), np.uint16)), empty((1, 8))
    for args in ((1, 0, 4, 4), (0, 8, 4, 4), (1, 8, 0, 4)):
        with pytest.raises(Exception):
            call("tn_c8_mean_fwd", x.ptr, y.ptr, *args)
        with pytest.raises(Exception):
            call("tn_c8_mean_bwd", y.ptr, x.ptr, *args, None, 0, 0.)


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
def _wide6_gap(img, B):
    """wide6.prms with its last PoolLayer replaced by a MeanLayer: Mean straight on an unpooled conv (256 maps), the
    dense head above it as it is."""
    prms = load_prms("wide6.prms", img, batch=B)
    lyrs = prms["layers"]
    i = max(k for k, (name, _) in enumerate(lyrs) if name == "PoolLayer")
    lyrs[i] = ("MeanLayer", {})
    return prms


def _prms(name, img, B):
    return _wide6_gap(img, B) if name == "wide6_gap" else load_prms(name, img, batch=B)


def _tr(prms, dtype):
    return dict(prms["training_params"], DTYPE=dtype, GRAD_SCALE=GS[dtype])


def _mean_bwd_16(monkeypatch, ora):
    """The device's Mean backward in the oracle: R(grad_scale * mean_bwd * act'(stored output below)) (_f16_down)."""
    i = next(k for k, l in enumerate(ora.L) if l.kind == "Mean")
    below = ora.L[i - 1]
    actvn = ora.L[i - 2].actvn if below.kind == "Pool" else below.actvn
    orig, gs = O.mean_bwd, ora.grad_scale

    def mean_bwd(x, dy):
        return O.r16(orig(x, dy) * O.act_grad_from_out(actvn, np.asarray(x, np.float64)), gs)

    monkeypatch.setattr(O, "mean_bwd", mean_bwd)


NETS = [("cifar_gap.prms", 32, 16), ("wide6_gap", 32, 6)]


@pytest.mark.parametrize("name,img,B", NETS)
def test_gap_nets_match_16bit_oracle(dtype, name, img, B, monkeypatch):
    """Two training steps (forward, every gradient, momentum update, maxnorm) of a net whose conv stack ends in a
    MeanLayer, against the stored-16-bit oracle -- and measurably closer to it than to the fp32 oracle."""
    from theanet_amd import NeuralNet
    prms = _prms(name, img, B)
    tr = _tr(prms, dtype)
    rng = np.random.RandomState(1)
    x = rng.rand(2 * B, 3, img, img).astype(np.float32)
    y = rng.randint(0, 10, 2 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    convs = [l for l in net.tr_layers if type(l).__name__ == "ConvLayer"]
    assert convs and all(l.f16 for l in convs) and all(l.f16 for l in net.tr_layers if hasattr(l, "f16"))
    ora = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float32"), dtype=np.float64)
    _mean_bwd_16(monkeypatch, ora)
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, 3, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:      # the mode is not a no-op: the fp32 oracle is measurably further away
            lp32 = ora32.forward(x[:B], True, draws)[0]
            assert np.abs(lp - lp_w).max() < .5 * np.abs(lp32 - lp_w).max() + 1e-6
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            assert_close(w, ol.params[j], rt, wat, what="%s %s w %d %d" % (name, dtype, i, j))


def test_gap_net_schedules_are_bit_identical(dtype, monkeypatch):
    """Two steps in flight against one at a time, and replayed (tn_net_plan_*) against interpreted steps: costs,
    logprobs, a test-function result and the weights in the middle of training, and the final weights, bit for bit."""
    from theanet_amd import NeuralNet
    prms = load_prms("cifar_gap.prms", 32, batch=16)
    rng = np.random.RandomState(5)
    x = rng.rand(16 * 6, 3, 32, 32).astype(np.float32)
    y = rng.randint(0, 10, 16 * 6).astype(np.int32)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms, dtype))
        fn = net.get_trin_model(x, y)
        te = net.get_test_model(x, y)
        outs, mids = [], []
        for s in range(40):
            if s in (30, 39):
                outs.append(fn(s % 6))
            else:
                fn.enqueue(s % 6)
            if s == 34:
                mids.append((te(1), [w.copy() for l in net.tr_layers for w in l.get_wts()]))
        outs.append(fn.fetch())
        pl = getattr(fn, "_plan", None)
        replayed = pl is not None and pl.ready
        if fn.__class__.__name__ == "_PipeTrainFn" and fn._seq is not None:
            replayed = fn._seq._plan.ready
        assert replayed == (plan == "1"), (pipe, plan)
        runs.append((outs, mids, [w for l in net.tr_layers for w in l.get_wts()]))
    for outs, mids, ws in runs[1:]:
        for a, b in zip(runs[0][0], outs):
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[2], b[2])
        for (t0, w0), (t1, w1) in zip(runs[0][1], mids):
            for u, v in zip(t0, t1):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(w0, w1):
                np.testing.assert_array_equal(u, v)
        for a, b in zip(runs[0][2], ws):
            np.testing.assert_array_equal(a, b)


def test_gap_full_size_cifar_gap_b2048(dtype):
    """cifar_gap at its stated size (32x32x3, 2048 images, elastic stage on): step 0 applies the zero velocity, the cost
    is finite and falls, exp(logprob) sums to 1; then a test-mode forward of 256 rows with the trained weights against the
    stored-16-bit oracle (its forward needs no patch)."""
    from theanet_amd import NeuralNet
    B, img, rows, steps = 2048, 32, 256, 12
    prms = load_prms("cifar_gap.prms", img, batch=B)
    tr = _tr(prms, dtype)
    rng = np.random.default_rng(0)
    x = rng.random((2 * B, 3, img, img), dtype=np.float32)
    y = np.random.default_rng(1).integers(0, 10, 2 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    fn = net.get_trin_model(x, y)
    conv = [l for l in net.tr_layers if getattr(l, "params", None)][1]
    w0 = conv.get_wts()[0]
    cost0, _, lp = fn(0)
    np.testing.assert_array_equal(conv.get_wts()[0], w0)            # step 0 applies the zero velocity (layer.py:86)
    assert np.isfinite(cost0) and abs(cost0 - np.log(10)) < 1.5
    np.testing.assert_allclose(np.exp(lp).sum(1), 1, rtol=1e-4)
    costs = [fn(i % 2)[0] for i in range(1, steps)]
    assert np.isfinite(costs).all() and min(costs[-2:]) < cost0, (cost0, costs)
    assert not np.array_equal(conv.get_wts()[0], w0)
    ora = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), allwts=net.get_init_params()["allwts"])
    tfn = net.get_test_model(x, y, preds_feats=True)
    sym, pm, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:B + rows], y[B:B + rows])
    assert_close(feats[:rows], lp_w, *TOL[dtype][0], what="cifar_gap %s test logprob rows 0..%d" % (dtype, rows - 1))
    np.testing.assert_array_equal(preds[:rows], preds_w)
    assert 0 <= sym <= 1 and 0 < pm <= 1


def test_gap_data_test_model_returns_the_means():
    """get_data_test_model with the Mean layer and the unpooled conv layer below it: the Mean output is the float64 mean
    of the returned (stored fp16) conv map, within 1e-6 of the largest mean."""
    from theanet_amd import NeuralNet
    B, img = 6, 32
    prms = _wide6_gap(img, B)
    net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms, "float16"))
    i_mean = next(i for i, l in enumerate(net.te_layers) if type(l).__name__ == "MeanLayer")
    assert type(net.te_layers[i_mean - 1]).__name__ == "ConvLayer" and net.te_layers[i_mean - 1].f16
    fn = net.get_data_test_model(get_output_of_layers=(i_mean, i_mean - 1))
    x = np.random.default_rng(7).random((B, 3, img, img), dtype=np.float32)
    feats, preds, mean, conv = fn(x)
    assert mean.shape == (B, 256) and conv.shape == (B, 256, 8, 8) and preds.shape == (B,)
    want = conv.astype(np.float64).mean(axis=(2, 3))
    assert np.abs(mean - want).max() <= 1e-6 * np.abs(want).max()
    assert np.abs(want).max() > 0
