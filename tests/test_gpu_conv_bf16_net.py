"""CONV 'bfloat16' through NeuralNet: every ConvLayer's three products on bf16-rounded operands with fp32 accumulation
(theanet_amd/csrc/conv_bf16.hip), for the conv shapes the 16-bit conv stack refuses; pools, dense layers and the head in
fp32.

The two-step statement is the float64 oracle with the operands of the conv layers' three products rounded by
R = tests.c8b_util.rbf16 inside this test (_rounded: forward conv(R(x), R(W)), gradients from R(x), R(W), R(dz); db from
the unrounded dz), draws injected -- built as tests/test_gpu_mlp_bf16.py builds its own, at that file's tolerances."""
import contextlib
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import assert_close, load_prms
from tests.test_gpu_c8_mean import TOL
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

R = CB.rbf16
TP = {"SEED": 11, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


@pytest.fixture(autouse=True)
def _back_to_float32():
    """CONV is context state (tn_set_conv_matmul): the tests of other files that follow find the fp32 conv kernels."""
    yield
    from theanet_amd.device import get_context
    get_context().set_conv_matmul("float32")


def _three_shapes():
    """3x3 'valid' + pool 2, 5x5 'same', 1x1 stride 2: the three conv shapes the 16-bit stack refuses (18 -> 16 -> 8 -> 8 -> 4)."""
    return [("InputLayer", {"img_sz": 18, "num_maps": 3}),
            ("ConvLayer", {"num_maps": 8, "filter_sz": 3, "stride": 1, "mode": "valid", "actvn": "relu10"}),
            ("PoolLayer", {"pool_sz": 2}),
            ("ConvLayer", {"num_maps": 12, "filter_sz": 5, "stride": 1, "mode": "same", "actvn": "tanh"}),
            ("ConvLayer", {"num_maps": 16, "filter_sz": 1, "stride": 2, "mode": "valid", "actvn": "relu05"}),
            ("HiddenLayer", {"n_out": 32, "pdrop": .5, "reg": {"L2": .001, "maxnorm": 2.}}),
            ("SoftmaxLayer", {"n_out": 10})]


def _data(B, n=2, seed=1, img=18, C=3):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, C, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


@contextlib.contextmanager
def _rounded():
    """The oracle's conv products on bf16-rounded operands while the block runs."""
    fwd, bwd = O.conv2d_fwd, O.conv2d_bwd

    def cf(x, W, b, stride=1, mode="valid", f16=False):
        return fwd(R(x), R(W), b, stride, mode)

    def cb(x, W, dz, stride=1, mode="valid", need_dx=True, f16=False, grad_scale=1.0):
        dx, dW, _ = bwd(R(x), R(W), R(dz), stride, mode, need_dx)
        return dx, dW, np.asarray(dz, np.float64).sum(axis=(0, 2, 3))

    O.conv2d_fwd, O.conv2d_bwd = cf, cb
    try:
        yield
    finally:
        O.conv2d_fwd, O.conv2d_bwd = fwd, bwd


def _nets():
    prms = load_prms("mnist_wide.prms", 28, batch=16)
    return {"three-shapes": (_three_shapes(), dict(TP), 18, 3),
            "mnist_wide": (prms["layers"], {k: v for k, v in prms["training_params"].items() if k != "CONV"}, 28, 1)}


def test_conv_bfloat16_net_builds_where_the_16_bit_stack_refuses():
    """Fails on a build without the mode: CONV is not a known param (the context has no set_conv_matmul)."""
    from theanet_amd import NeuralNet
    B = TP["BATCH_SZ"]
    x, y = _data(B)
    net = NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="bfloat16"))
    assert net.conv_mm == "bfloat16" and net.ctx._conv_mm == "bfloat16" and net.dtype == "float32"
    assert all(l.fused_pool is None for l in net.tr_layers + net.te_layers if hasattr(l, "fused_pool"))
    fn = net.get_trin_model(x, y)
    for s in range(2):
        assert np.isfinite(fn(s)[0])
    with pytest.raises(AssertionError, match="CONV"):
        NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="float16"))
    for dt in ("float16", "bfloat16"):
        with pytest.raises(AssertionError, match="already runs 16-bit products"):
            NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="bfloat16", DTYPE=dt))
    with pytest.raises(AssertionError, match="DTYPE bfloat16 needs"):       # the stack's own refusal stays
        NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, DTYPE="bfloat16"))
    # MATMUL is independent
    net = NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="bfloat16", MATMUL="bfloat16"))
    assert np.isfinite(net.get_trin_model(x, y)(0)[0])
    net.ctx.set_fc_matmul("float32")


@pytest.mark.parametrize("name", ["three-shapes", "mnist_wide"])
def test_conv_bfloat16_net_matches_rounded_operand_statement(name, monkeypatch):
    """Two training steps (forward, every gradient, momentum update, maxnorm) against the statement at the 16-bit net
    tolerances of tests/test_gpu_c8_mean.py, equal argmax, closer to it than the plain float32 oracle net is -- and,
    layer-locally on the device's own input, one conv layer's output is the rounded-operand product."""
    from theanet_amd import NeuralNet
    layers, tp, img, C = _nets()[name]
    B = tp["BATCH_SZ"]
    monkeypatch.setenv("TN_PIPELINE", "0")           # one step at a time: the layers' buffers hold the step just returned
    x, y = _data(B, img=img, C=C)
    net = NeuralNet(copy.deepcopy(layers), dict(tp, CONV="bfloat16"))
    ora = O.OracleNet(copy.deepcopy(layers), dict(tp), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(layers), dict(tp), dtype=np.float32)
    (rt, at), wat = TOL["bfloat16"]
    fn = net.get_trin_model(x, y)
    ic = max(i for i, l in enumerate(net.tr_layers) if type(l).__name__ == "ConvLayer" and l.stride == 1)
    conv = net.tr_layers[ic]
    Wc, bc = [w.copy() for w in conv.get_wts()]
    for s in range(2):
        draws = _inject_draws(net, ora, B, C, img)
        xs, ys = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        if s == 0:
            lp32 = np.asarray(ora32.forward(xs, True, draws)[0], np.float64)
        with _rounded():
            cost_w, lp_w, _ = ora.train_step(xs, ys, draws)
        cost, _, lp = fn(s)
        print("%s step %d: cost %.6f (statement %.6f), max |dlogprob| %.3g" % (name, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="logprob step %d" % s)
        assert_close(cost, cost_w, rt, at, what="cost step %d" % s)
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:
            e16, e32 = np.abs(lp - lp_w).max(), np.abs(lp32 - lp_w).max()
            print("  against the statement %.3g, the float32 oracle against the statement %.3g" % (e16, e32))
            assert e16 < .5 * e32 + 1e-6
            # layer-local: conv layer ic on the device's own input
            h = conv.inpt.get_value().astype(np.float64).reshape(B, conv.num_prev_maps, conv.in_sz, conv.in_sz)
            a = conv.output.get_value()
            act = O.activation(ora.L[ic].actvn)[0]
            a_r = act(O.conv2d_fwd(R(h), R(Wc), bc.astype(np.float64), conv.stride, conv.mode))
            a_p = act(O.conv2d_fwd(h, Wc.astype(np.float64), bc.astype(np.float64), conv.stride, conv.mode))
            er, ep = np.abs(a - a_r).max(), np.abs(a_p - a_r).max()
            print("  layer %d output: against the rounded-operand product %.3g, fp32 product against it %.3g" % (ic, er, ep))
            assert er <= 2e-5 * np.abs(a_r).max() and er < .5 * ep
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
            assert_close(w, ol.params[j], rt, wat, what="w %d %d" % (i, j))


def test_conv_bfloat16_dense_layers_and_head_stay_fp32(monkeypatch):
    """MATMUL left at 'float32': the dense layer and the head of a CONV 'bfloat16' net compute what a CONV 'float32' net
    of those layers computes from the same input -- the check at the first dense layer's input: a dense-only net fed the
    conv stack's outputs of two steps, with the same weights, returns the same cost and logprob bits and ends on the same
    dense weights.  (Two steps: the reference's update applies the velocity of the step before, so the first moves
    nothing.)"""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    B = TP["BATCH_SZ"]
    layers = copy.deepcopy(_three_shapes())
    layers[5][1]["pdrop"] = 0
    x, y = _data(B, n=2)
    net = NeuralNet(copy.deepcopy(layers), dict(TP, CONV="bfloat16"))
    wts = [[w.copy() for w in l.get_wts()] for l in net.tr_layers]
    top = net.tr_layers[4]
    fn = net.get_trin_model(x, y)
    outs, feats = [], []
    for s in range(2):
        outs.append(fn(s))
        feats.append(top.output.get_value().reshape(B, top.num_maps, top.out_sz, top.out_sz).copy())
    dense = [("InputLayer", {"img_sz": top.out_sz, "num_maps": top.num_maps})] + copy.deepcopy(layers[5:])
    ref = NeuralNet(dense, dict(TP, CONV="float32"), allwts=[[]] + wts[5:])
    assert ref.ctx._conv_mm == "float32"
    fr = ref.get_trin_model(np.concatenate(feats), y)
    for s in range(2):
        cost_r, _, lp_r = fr(s)
        assert outs[s][0] == cost_r
        np.testing.assert_array_equal(outs[s][2], lp_r)
    for i, (a, b) in enumerate(zip(net.tr_layers[5:], ref.tr_layers[1:])):
        got = a.get_wts()
        for u, v in zip(got, b.get_wts()):
            np.testing.assert_array_equal(u, v)
        assert any((u != w0).any() for u, w0 in zip(got, wts[5 + i]))      # the steps moved them


def test_conv_bfloat16_schedules_are_bit_identical(monkeypatch):
    """Two steps in flight against one at a time, replayed (tn_net_plan_*) against interpreted steps, a test-model call
    in the middle: bit for bit (the products go through the same calls in every schedule)."""
    from theanet_amd import NeuralNet
    B = TP["BATCH_SZ"]
    x, y = _data(B, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="bfloat16"))
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


def test_conv_float32_and_bfloat16_nets_share_their_initial_weights():
    from theanet_amd import NeuralNet
    n32 = NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="float32"))
    nbf = NeuralNet(copy.deepcopy(_three_shapes()), dict(TP, CONV="bfloat16"))
    assert n32.conv_mm == "float32" and nbf.conv_mm == "bfloat16"
    for a, b in zip(n32.tr_layers, nbf.tr_layers):
        for u, v in zip(a.get_wts(), b.get_wts()):
            np.testing.assert_array_equal(u, v)
    x, y = _data(TP["BATCH_SZ"], n=1)
    n32.tr_layers[5].drop.inject(np.ones((TP["BATCH_SZ"], 32), np.float32))
    nbf.tr_layers[5].drop.inject(np.ones((TP["BATCH_SZ"], 32), np.float32))
    lp32, lpbf = n32.get_trin_model(x, y)(0)[2], nbf.get_trin_model(x, y)(0)[2]
    assert (lp32 != lpbf).any() and np.abs(lp32 - lpbf).max() < .05


def test_mnist_wide_prms_parses_builds_and_steps():
    from theanet_amd import NeuralNet
    prms = load_prms("mnist_wide.prms", 28, batch=32)
    assert prms["training_params"]["CONV"] == "bfloat16"
    assert [l[1].get("num_maps") for l in prms["layers"] if l[0] == "ConvLayer"] == [32, 64]
    net = NeuralNet(prms["layers"], prms["training_params"])
    assert [l.out_sz for l in net.tr_layers[1:5]] == [26, 13, 11, 6]
    rng = np.random.RandomState(2)
    x, y = rng.rand(64, 1, 28, 28).astype(np.float32), rng.randint(0, 10, 64).astype(np.int32)
    fn = net.get_trin_model(x, y)
    for s in range(2):
        assert np.isfinite(fn(s)[0])
