"""Nets with PoolLayers whose stride differs from their window (``stride``: overlapping 3x3 stride-2 pools, a gapped 2x2
stride-3 one, a stride-1 window of two), on the 16-bit conv stack in both element types (tn_c8_pool_st_*) and in float32
(tn_pool_st_*), against the oracle.

The oracle knows no stride, so it is taught from outside, the way tests/test_gpu_c8_pool.py teaches it the stand-alone
pool: O.pool_out_sz / O.pool_fwd / O.pool_bwd are replaced by the numpy statement of tests/test_pool_st_cpu.py, which looks
the stride up by the window size (one stride per window size in a test net; OracleNet gets the layers without the key).
In the stored-16-bit mode the backward's sum is rounded once to the element type at the gradient scale, as the device
stores it; _teach_pool supplies the rest (a pool standing for the block below it, the Mean backward).  Dropout masks are
injected on both sides.

Bounds: stored-16-bit nets the TOL of tests/test_gpu_c8_mean.py; float32 nets the bounds of tests/test_gpu_net.py's
_random_net_case (1e-4 / 1e-5 on log-probabilities and cost, 1e-4 / 1e-6 on the weights); schedules bit for bit."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import assert_close, ctx
from tests.test_gpu_c8_mean import GS, R16, TOL
from tests.test_gpu_c8_pool import _teach_pool
from tests.test_gpu_f16 import _inject_draws
from tests.test_pool_st_cpu import out_side, pool_st_bwd, pool_st_fwd
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

TP = {"SEED": 7, "BATCH_SZ": 6, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}
B = TP["BATCH_SZ"]
F32_TOL = ((1e-4, 1e-5), 1e-6, 1e-4)        # (logprob / cost), weights abs, weights rel


@pytest.fixture(params=["float16", "bfloat16", "float32"])
def dt(request, monkeypatch):
    """The net's DTYPE; for bfloat16 the oracle's stored-16-bit mode rounds to bf16 (tests/test_gpu_bf16.py)."""
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    yield request.param
    monkeypatch.setattr(O, "r16", R16)


def _conv(k, act="relu10", f=3, mode="same"):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": 1, "mode": mode, "actvn": act})


def _pool(p, st, ib=False):
    return ("PoolLayer", dict({"pool_sz": p, "stride": st}, **({"ignore_border": True} if ib else {})))


def _hid(n, act="relu10"):
    return ("HiddenLayer", {"n_out": n, "actvn": act})


DROP = ("DropOutLayer", {"pdrop": .25})
SOFTMAX = ("SoftmaxLayer", {"n_out": 10})
# name -> (image side, layers above the 3-map input, window -> stride, the pooled sides, more training params)
NETS = {
    "a_two_pool32": (16, [_conv(16), _pool(3, 2), _conv(24), _pool(3, 2), _hid(32), SOFTMAX], {3: 2}, [8, 4], {}),
    "b_1x1_drop_gap": (14, [_conv(16), _conv(16, f=1), _pool(3, 2), DROP, _conv(24), _pool(2, 3, True), _hid(32), SOFTMAX],
                       {3: 2, 2: 3}, [7, 2], {}),
    "c_pool_pool_mean": (12, [_conv(16), _pool(3, 2), _pool(2, 1), ("MeanLayer", {}), SOFTMAX], {3: 2, 2: 1}, [6, 5], {}),
    "d_valid_any": (13, [_conv(16, mode="valid"), _pool(3, 2), _hid(32), SOFTMAX], {3: 2}, [5], {"CONV_SHAPES": "any"}),
}


def _layers(name):
    img, lyrs, strides, sides, more = NETS[name]
    return img, [("InputLayer", {"img_sz": img, "num_maps": 3})] + copy.deepcopy(lyrs), strides, sides, more


def _tr(dt, more=()):
    tr = dict(TP, **dict(more))
    return dict(tr, DTYPE=dt, GRAD_SCALE=GS[dt]) if dt != "float32" else tr


def _data(img, n=3, seed=1):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, 3, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _build(name, dt, **kw):
    """The net of NETS[name]: every pool strided, never fused, on the stack a layer of its own with the sides of the table."""
    from theanet_amd import NeuralNet
    img, lyrs, strides, sides, more = _layers(name)
    net = NeuralNet(lyrs, _tr(dt, more), **kw)
    for graph in (net.tr_layers, net.te_layers):
        pools = [l for l in graph if type(l).__name__ == "PoolLayer"]
        assert [l.out_sz for l in pools] == sides
        for l in pools:
            assert l.strided and l.stride == strides[l.pool_sz] and l.fused_conv is None and "Stride:%d" % l.stride in l.representation
            assert l.f16 == l.c8_alone == (dt != "float32")
        assert not any(getattr(l, "fused_pool", None) is not None for l in graph)
    return net, lyrs, img


def _teach_stride(monkeypatch, strides, ora=None):
    """The oracle's three pool functions replaced by the statement, the stride looked up by the window size.  ``ora`` in
    the stored-16-bit mode: the backward's sum is rounded once at the gradient scale, as the device stores it."""
    def side(in_sz, p, ib):
        return out_side(in_sz, p, strides[p], ib)

    def fwd(x, p, ib=False):
        return pool_st_fwd(x, p, strides[p], ib)

    def bwd(x, dy, p, ib=False):
        g = pool_st_bwd(np.asarray(x), np.asarray(dy, np.asarray(x).dtype), p, strides[p], ib)
        return O.r16(g, ora.grad_scale) if ora is not None and ora.f16 else g

    monkeypatch.setattr(O, "pool_out_sz", side)
    monkeypatch.setattr(O, "pool_fwd", fwd)
    monkeypatch.setattr(O, "pool_bwd", bwd)


def _oracle(monkeypatch, net, lyrs, strides, dt, more):
    """OracleNet on the layers without the ``stride`` key, taught the stride (and, in the 16-bit mode, the stand-alone pool)."""
    bare = [(k, {a: v for a, v in args.items() if not (k == "PoolLayer" and a == "stride")}) for k, args in copy.deepcopy(lyrs)]
    _teach_stride(monkeypatch, strides)
    ora = O.OracleNet(bare, dict(_tr(dt, more), DTYPE="float16") if dt != "float32" else dict(_tr(dt, more)), dtype=np.float64)
    _teach_stride(monkeypatch, strides, ora)
    if dt != "float32":
        _teach_pool(monkeypatch, ora, {i for i, l in enumerate(net.tr_layers) if getattr(l, "c8_alone", False)})
    return ora


@pytest.mark.parametrize("name", sorted(NETS))
def test_strided_pool_nets_match_oracle(dt, name, monkeypatch):
    """Three training steps (cost, logprob, argmax; every dW / db through the weights after each update) with the oracle's
    dropout masks injected into both sides, then the test mode of the trained net."""
    net, lyrs, img = _build(name, dt)
    strides, more = NETS[name][2], NETS[name][4]
    x, y = _data(img)
    ora = _oracle(monkeypatch, net, lyrs, strides, dt, more)
    (rt, at), wat, wrt = (TOL[dt] + (TOL[dt][0][0],)) if dt != "float32" else F32_TOL
    fn = net.get_trin_model(x, y)
    w0 = net.tr_layers[1].get_wts()[0].copy()
    for s in range(3):
        draws = _inject_draws(net, ora, B, 3, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        print("%s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (name, dt, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dt, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dt, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
            for j, w in enumerate(lyr.get_wts()):
                print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
                assert_close(w, ol.params[j], wrt, wat, what="%s %s w %d %d step %d" % (name, dt, i, j, s))
    assert not np.array_equal(w0, net.tr_layers[1].get_wts()[0])       # the gradient reached the bottom through the pools
    tfn = net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
    print("%s %s test: max |dlogprob| %.3g" % (name, dt, np.abs(feats[:B] - lp_w).max()))
    assert_close(feats[:B], lp_w, rt, at, what="%s %s test logprob" % (name, dt))
    np.testing.assert_array_equal(preds[:B], preds_w)


def _names(fn, steps):
    """The entry points of ``steps`` interpreted steps, in order.  (The spy is an attribute of the context OBJECT, taken
    away again afterwards: the class's own method -- which tests/guard_util.py wraps and unwraps -- stays in charge.)"""
    c = ctx()
    log, real = [], c.call

    def spy(name, *args):
        log.append(name)
        return real(name, *args)

    c.call = spy
    try:
        costs = [fn(s)[0] for s in range(steps)]
    finally:
        del c.call
    return log, costs


def test_stride_equal_to_window_is_the_old_layer(monkeypatch):
    """Net b in float32 with every pool's stride set to its window, against the same net without the key: the same
    representation, the same entry points in the same order -- none of the new ones -- and the same costs, bit for bit;
    with the strides of the table the steps go through tn_pool_st_fwd / tn_pool_st_bwd."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    monkeypatch.setenv("TN_NET_PLAN", "0")
    img, lyrs, _, _, _ = _layers("b_1x1_drop_gap")
    x, y = _data(img)
    runs = []
    for how in ("absent", "none", "window", "table"):
        ls = copy.deepcopy(lyrs)
        for k, args in ls:
            if k == "PoolLayer" and how != "table":
                args.pop("stride")
                if how != "absent":
                    args["stride"] = None if how == "none" else args["pool_sz"]
        net = NeuralNet(ls, dict(TP))
        log, costs = _names(net.get_trin_model(x, y), 2)
        runs.append((log, costs, [l.representation for l in net.tr_layers], [l.n_out for l in net.tr_layers]))
    for log, costs, reps, n_out in runs[1:3]:
        assert log == runs[0][0] and costs == runs[0][1] and reps == runs[0][2] and n_out == runs[0][3]
    assert not any("_st_" in n for n in runs[0][0])
    assert not any("Stride" in r for r in runs[0][2] if r.startswith("Pool"))
    log = runs[3][0]
    assert log.count("tn_pool_st_fwd") == 4 and log.count("tn_pool_st_bwd") == 4 and "tn_pool_fwd" not in log


def test_strided_pool_net_schedules_are_bit_identical(dt, monkeypatch):
    """Net b (device RNG for its DropOutLayer): two steps in flight against one at a time, and replayed (tn_net_plan_*)
    against interpreted steps -- the plan really taken: costs, logprobs, a test-function result and the weights in the
    middle of training, and the final weights, bit for bit."""
    x, y = _data(14, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net, _, _ = _build("b_1x1_drop_gap", dt)
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


def test_data_test_model_returns_the_pooled_maps(dt):
    """get_data_test_model on net b: the logical NCHW arrays of both pools and of the 1x1 conv map under the first --
    whose maximum over 3x3 windows at stride 2 the first pooled map is, exactly."""
    net, _, img = _build("b_1x1_drop_gap", dt)
    fn = net.get_data_test_model(get_output_of_layers=(2, 3, 6))
    x = np.random.default_rng(7).random((B, 3, img, img), dtype=np.float32)
    _, preds, conv, pool, last = fn(x)
    assert conv.shape == (B, 16, 14, 14) and pool.shape == (B, 16, 7, 7) and last.shape == (B, 24, 2, 2) and preds.shape == (B,)
    assert np.abs(pool).max() > 0 and np.abs(last).max() > 0
    np.testing.assert_array_equal(pool, pool_st_fwd(conv, 3, 2, False))


def test_conv_bfloat16_net_builds_and_steps(monkeypatch):
    """CONV 'bfloat16' (fp32 tensors, bf16 conv products, nothing fused): the pools are the fp32 strided ops."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    monkeypatch.setenv("TN_NET_PLAN", "0")
    img, lyrs, _, sides, _ = _layers("a_two_pool32")
    net = NeuralNet(lyrs, dict(TP, CONV="bfloat16"))
    assert [l.out_sz for l in net.tr_layers if type(l).__name__ == "PoolLayer"] == sides
    x, y = _data(img)
    w0 = net.tr_layers[1].get_wts()[0].copy()
    log, costs = _names(net.get_trin_model(x, y), 3)
    assert np.isfinite(costs).all() and not np.array_equal(w0, net.tr_layers[1].get_wts()[0])
    assert log.count("tn_pool_st_fwd") == 6 and log.count("tn_pool_st_bwd") == 6 and "tn_pool_fwd" not in log
    assert np.isfinite(net.get_test_model(x, y, preds_feats=True)(1)[2]).all()


def test_refused_geometries_fail_at_construction():
    from theanet_amd import NeuralNet
    lyrs = [("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16), _pool(3, 2), _hid(16), SOFTMAX]
    for bad, match in ((0, "stride must be an integer >= 1"), (1.5, "stride must be an integer >= 1"),
                       (65, "at a stride of 1 to 64")):
        ls = copy.deepcopy(lyrs)
        ls[2][1]["stride"] = bad
        with pytest.raises(AssertionError, match=match):
            NeuralNet(ls, _tr("bfloat16"))
    ls = copy.deepcopy(lyrs)
    ls[2] = _pool(13, 2, True)
    with pytest.raises(AssertionError, match="does not fit a map"):
        NeuralNet(ls, dict(TP))
