"""Nets with ConvLayers of any filter, mode and stride on the 16-bit-resident conv stack: DTYPE 'float16' / 'bfloat16' with
the training param CONV_SHAPES 'any' (the general family tn_c8_convg_*, theanet_amd/csrc/convg_c8.hip, for every shape the
two tiled families refuse; the PoolLayers above such layers stand alone).

Whole nets run against the unchanged stored-16-bit oracle (OracleNet with DTYPE 'float16'; for bf16 its rounding is
swapped) taught the DropOut handling from outside by tests/test_gpu_c8_dropout.py's _oracle_16, at TOL of
tests/test_gpu_c8_mean.py.  One more thing is taught here, as tests/test_gpu_c8_pool.py teaches it: the oracle's
16-bit Pool takes its ties from the UNROUNDED activation (the fused block's rule), a stand-alone PoolLayer
(theanet_amd/csrc/pool_c8.hip) compares the STORED values, where two elements of a window tie more often -- every pool
of these nets stands alone, so the oracle's pool_bwd is handed the rounded activation.  The forward is the same either
way (rounding is monotone).

On the parent commit test_convg_nets_build_16bit_resident fails (and with it every test here that builds such a net):
construction with CONV_SHAPES 'any' asserts "DTYPE ... needs 3x3 stride-1 'same' conv layers", and tn_c8_convg_fwd is not
exported."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import assert_close, load_prms
from tests.test_gpu_c8_conv1 import dtype  # noqa: F401  (fixture: the element type, the oracle's rounding swapped for bf16)
from tests.test_gpu_c8_dropout import _oracle_16
from tests.test_gpu_c8_mean import GS, TOL
from tests.test_gpu_conv_bf16_net import _three_shapes
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

B = 16
TP = {"SEED": 11, "BATCH_SZ": B, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


def _conv(k, f, mode, act, stride=1):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": stride, "mode": mode, "actvn": act})


def _mixed():
    """Tiled and general layers in one net, 16 -> 16 -> 14 -> 7 -> 7 -> 4: a tiled 3x3 'same' layer of 16 filters below a
    general one, a general layer's pool, a tiled layer on the odd 7 x 7 maps at pitch 8 and its 2x2 pool -- which stands
    alone, the fused block taking even maps only."""
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, 3, "same", "relu10"), _conv(20, 3, "valid", "tanh"),
            ("PoolLayer", {"pool_sz": 2}), _conv(16, 3, "same", "relu10"), ("PoolLayer", {"pool_sz": 2}),
            ("HiddenLayer", {"n_out": 32, "pdrop": .5}), ("SoftmaxLayer", {"n_out": 10})]


# name -> (layers, training params, image side, channels, (family per conv layer, c8_alone per pool layer))
def _nets():
    mnist = load_prms("mnist.prms", 28, seed=11, batch=B)
    return {"mnist": (mnist["layers"], mnist["training_params"], 28, 1, ("gg", (True, True))),
            "three-shapes": (_three_shapes(), dict(TP), 18, 3, ("ggg", (True,))),
            "mixed": (_mixed(), dict(TP), 16, 3, ("tgt", (True, True)))}


NAMES = ["mnist", "three-shapes", "mixed"]


def _tr(tp, dtype, shapes="any"):
    tr = dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype]) if dtype in GS else dict(tp, DTYPE=dtype)
    return dict(tr, CONV_SHAPES=shapes) if shapes else tr


def _data(img, C, n=3, seed=1):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, C, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _convs(graph):
    return [l for l in graph if type(l).__name__ == "ConvLayer"]


def _pools(graph):
    return [l for l in graph if type(l).__name__ == "PoolLayer"]


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", NAMES)
def test_convg_nets_build_16bit_resident(name, dt):
    """The conv layers report f16 and their family, general ('g': tn_c8_convg_*, never fused) or tiled ('t'); the pools
    above general layers -- and the 2x2 pool on the odd map above a tiled one -- are c8_alone.  Both graphs."""
    from theanet_amd import NeuralNet
    layers, tp, img, C, (fams, alone) = _nets()[name]
    net = NeuralNet(copy.deepcopy(layers), _tr(tp, dt))
    assert net.conv_shapes == "any"
    for graph in (net.tr_layers, net.te_layers):
        convs, pools = _convs(graph), _pools(graph)
        assert all(l.f16 and l.args[-1] == "any" for l in convs) and all(l.f16 for l in pools)
        assert "".join("g" if l.c8_fam.fwd == "tn_c8_convg_fwd" else "t" for l in convs) == fams
        for l in convs:
            general = l.c8_fam.fwd == "tn_c8_convg_fwd"
            assert l.c8_fam.pools == (not general) and l.c8_fam.tiles == (not general and not l.c8_1x1)
            assert l.fused_pool is None
        assert tuple(l.c8_alone for l in pools) == alone and all(l.fused_conv is None for l in pools)
    if name == "mnist":
        c1, c2 = _convs(net.tr_layers)
        assert (c1.pitch, c1.output.pitch, c2.pitch, c2.output.pitch) == (32, 32, 16, 16)
        assert c1.c8_fam.geom == (B, 1, 28, 32, 4, 3, 1, 0, 26, 32) and c2.c8_fam.geom == (B, 4, 13, 16, 20, 3, 1, 0, 11, 16)
        assert [p.output.pitch for p in _pools(net.tr_layers)] == [16, 8]


@pytest.mark.parametrize("name", NAMES)
def test_convg_nets_match_16bit_oracle(dtype, name, monkeypatch):
    """Three training steps (cost, logprob, argmax; every dW / db through the weights after each update) with the oracle's
    elastic draws and dropout masks injected into both sides, then the test mode of the trained net."""
    from theanet_amd import NeuralNet
    layers, tp, img, C, _ = _nets()[name]
    tr = _tr(tp, dtype)
    x, y = _data(img, C)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    ora = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float16"), dtype=np.float64)
    _oracle_16(monkeypatch, ora)
    pool_bwd = O.pool_bwd
    monkeypatch.setattr(O, "pool_bwd", lambda x_, g, p, ib: pool_bwd(O.r16(x_), g, p, ib))       # ties of the stored values
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
    w0 = _convs(net.tr_layers)[0].get_wts()[0].copy()
    for s in range(3):
        draws = _inject_draws(net, ora, B, C, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        print("%s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (name, dtype, s, cost, cost_w, np.abs(lp - lp_w).max()))
        for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
            for j, w in enumerate(lyr.get_wts()):
                print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
            for j, w in enumerate(lyr.get_wts()):
                assert_close(w, ol.params[j], rt, wat, what="%s %s w %d %d step %d" % (name, dtype, i, j, s))
    assert not np.array_equal(w0, _convs(net.tr_layers)[0].get_wts()[0])         # the gradient reached the bottom
    tfn = net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
    print("%s %s test: max |dlogprob| %.3g" % (name, dtype, np.abs(feats[:B] - lp_w).max()))
    assert_close(feats[:B], lp_w, rt, at, what="%s %s test logprob" % (name, dtype))
    np.testing.assert_array_equal(preds[:B], preds_w)


def test_convg_net_schedules_are_bit_identical(dtype, monkeypatch):
    """mnist.prms on the general family, device RNG: two steps in flight against one at a time, replayed (tn_net_plan_*)
    against interpreted steps -- the plan really taken: costs, logprobs, a test-function result and the weights in the
    middle of training, and the final weights, bit for bit."""
    from theanet_amd import NeuralNet
    layers, tp, img, C, _ = _nets()["mnist"]
    x, y = _data(img, C, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(layers), _tr(tp, dtype))
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
        assert replayed == (plan == "1"), (pipe, plan, getattr(pl, "why", None))
        runs.append((outs, mids, [w for l in net.tr_layers for w in l.get_wts()]))
    assert np.isfinite(runs[0][0][-1][0])
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


@pytest.mark.parametrize("name", ["mnist", "mixed"])
def test_convg_fused_step_equals_separate_launches(dtype, name, monkeypatch):
    """NeuralNet.fused_step False against True on the sequential schedule (tests/test_gpu_net.py): costs, log-probs,
    gradients and weights bit for bit.  (Not the three-shapes net: with a weight cost the generic schedule adds up the
    reported cost in another fixed order, tests/test_gpu_wtcost_net.py.)"""
    from theanet_amd import NeuralNet
    layers, tp, img, C, _ = _nets()[name]
    x, y = _data(img, C, n=4, seed=3)
    monkeypatch.setenv("TN_PIPELINE", "0")
    nets = []
    for fused in (True, False):
        monkeypatch.setattr(NeuralNet, "fused_step", fused)
        net = NeuralNet(copy.deepcopy(layers), _tr(tp, dtype))
        fn = net.get_trin_model(x, y)
        nets.append((net, [fn(s % 4) for s in range(6)]))
    for (c0, _, l0), (c1, _, l1) in zip(nets[0][1], nets[1][1]):
        assert c0 == c1 and np.isfinite(c0)
        np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(nets[0][0].flat_grads.get_value(), nets[1][0].flat_grads.get_value())
    for la, lb in zip(nets[0][0].tr_layers, nets[1][0].tr_layers):
        for wa, wb in zip(la.get_wts(), lb.get_wts()):
            np.testing.assert_array_equal(wa, wb)


def test_convg_net_cost_ring_order_averaging_and_sweep(dtype, monkeypatch):
    """mnist.prms on the general family with WT_AVG, device RNG, through the other schedules, each against its plain
    form bit for bit: the cost ring (step_cost / drain_costs) against fn(i) one step at a time, a row order (set_order)
    against the dataset gathered by hand, sweep() against one test call per minibatch at the averaged weights."""
    from theanet_amd import NeuralNet
    layers, tp, img, C, _ = _nets()["mnist"]
    tr = dict(_tr(tp, dtype), WT_AVG=.9)
    x, y = _data(img, C, n=4, seed=9)
    order = np.random.RandomState(2).permutation(4 * B)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    fn = net.get_trin_model(x, y)
    fn.set_order(order)
    got = []
    for s in range(9):
        got += fn.step_cost(s % 4)
    got += fn.drain_costs()
    assert [k for k, _ in got] == list(range(9))
    monkeypatch.setenv("TN_PIPELINE", "0")
    net2 = NeuralNet(copy.deepcopy(layers), dict(tr))
    fn2 = net2.get_trin_model(x[order], y[order])
    want = [fn2(s % 4)[0] for s in range(9)]
    np.testing.assert_array_equal(np.asarray([c for _, c in got], np.float32).view(np.uint32),
                                  np.asarray(want, np.float32).view(np.uint32))
    assert np.isfinite(want).all()
    for la, lb in zip(net.tr_layers, net2.tr_layers):
        for wa, wb in zip(la.get_wts(), lb.get_wts()):
            np.testing.assert_array_equal(wa, wb)
    for a, b in zip(net.get_avg_wts(), net2.get_avg_wts()):
        for u, v in zip(a or (), b or ()):
            np.testing.assert_array_equal(u, v)
    te = net.get_test_model(x, y)
    assert te.sweep(range(4)) == [te(i) for i in range(4)]


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_conv_shapes_is_opt_in(dt):
    """Without the key (and with 'tiled') the same layers raise AssertionError with today's message; a bogus value names
    the key; CONV 'bfloat16' with a 16-bit DTYPE stays refused."""
    from theanet_amd import NeuralNet
    for name in NAMES:
        layers, tp, _, _, _ = _nets()[name]
        for shapes in (None, "tiled"):
            with pytest.raises(AssertionError, match="DTYPE %s needs 3x3 stride-1 'same' conv layers with a multiple of 8 "
                                                     "filters on maps of at most 64 pixels a side" % dt):
                NeuralNet(copy.deepcopy(layers), _tr(tp, dt, shapes))
    with pytest.raises(AssertionError, match="CONV_SHAPES must be 'tiled' or 'any'"):
        NeuralNet(copy.deepcopy(_three_shapes()), _tr(TP, dt, "general"))
    with pytest.raises(AssertionError, match="already runs 16-bit products"):
        NeuralNet(copy.deepcopy(_three_shapes()), dict(_tr(TP, dt), CONV="bfloat16"))


def test_conv_shapes_any_changes_nothing_for_float32_and_tiled_nets(monkeypatch):
    """DTYPE float32 with 'any' builds and gives the bits of the net without the key; so does a 16-bit net of tiled
    shapes only (mnist_c8.prms at batch 16: the fused blocks and their kernels as today)."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    c8 = load_prms("mnist_c8.prms", 28, seed=11, batch=B)
    for layers, tp, img, C in ((_three_shapes(), dict(TP), 18, 3), (c8["layers"], c8["training_params"], 28, 1)):
        x, y = _data(img, C, n=2)
        runs = []
        for shapes in (None, "any"):
            net = NeuralNet(copy.deepcopy(layers), dict(tp, CONV_SHAPES=shapes) if shapes else dict(tp))
            if net.dtype != "float32":
                assert all(l.fused_pool is not None and l.c8_fam.tiles for l in _convs(net.tr_layers))
                assert not any(l.c8_alone for l in _pools(net.tr_layers))
            fn = net.get_trin_model(x, y)
            runs.append(([fn(s) for s in range(2)], [w for l in net.tr_layers for w in l.get_wts()]))
        for (c0, _, l0), (c1, _, l1) in zip(runs[0][0], runs[1][0]):
            assert c0 == c1 and np.isfinite(c0)
            np.testing.assert_array_equal(l0, l1)
        for a, b in zip(runs[0][1], runs[1][1]):
            np.testing.assert_array_equal(a, b)


def test_convg_data_test_model_returns_logical_shapes(dtype):
    """get_data_test_model on mnist.prms: the unfused general layers' outputs come back as logical NCHW arrays -- conv1's
    (B, 4, 26, 26) map, whose 2x2 maxima the first pooled map is, exactly."""
    from theanet_amd import NeuralNet
    layers, tp, img, C, _ = _nets()["mnist"]
    net = NeuralNet(copy.deepcopy(layers), _tr(tp, dtype))
    fn = net.get_data_test_model(get_output_of_layers=(0, 1, 2, 3, 4))
    x = np.random.default_rng(7).random((B, 1, 28, 28), dtype=np.float32)
    _, preds, x0, c1, p1, c2, p2 = fn(x)
    assert c1.shape == (B, 4, 26, 26) and p1.shape == (B, 4, 13, 13) and c2.shape == (B, 20, 11, 11) and p2.shape == (B, 20, 6, 6)
    assert preds.shape == (B,) and np.abs(c1).max() > 0 and np.abs(c2).max() > 0
    np.testing.assert_array_equal(p1, O.pool_fwd(c1, 2, False))
    np.testing.assert_array_equal(p2, O.pool_fwd(c2, 2, False))
    # conv1's map is the oracle's stored-16-bit forward of what the test-mode input stage hands it
    W, b = net.te_layers[1].get_wts()
    assert x0.shape == (B, 1, 28, 28)
    want = O.r16(O.activation("relu10")[0](O.conv2d_fwd(x0.astype(np.float64), W.astype(np.float64), b.astype(np.float64),
                                                        1, "valid", f16=True)))
    assert np.abs(c1 - want).max() <= {"float16": 1e-3, "bfloat16": 1e-2}[dtype] * np.abs(want).max()
