"""MATMUL 'bfloat16' through NeuralNet: every HiddenLayer's three products on bf16-rounded operands with fp32
accumulation (theanet_amd/csrc/gemm_bf16.hip), the Softmax head in fp32.

The statement of the small MLP is assembled here from the oracle's own helpers (activations, log-softmax / NLL,
wtcost_grad, the momentum / maxnorm update) in float64, with R = tests.c8b_util.rbf16 applied to the operands of the
hidden layers' three products ONLY: forward R(x) @ R(W), input gradient R(dz) @ R(W).T, weight gradient R(x).T @ R(dz);
db, the head and the update are unrounded."""
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
TP = {"SEED": 11, "BATCH_SZ": 48, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


@pytest.fixture(autouse=True)
def _back_to_float32():
    """MATMUL is context state (tn_set_fc_matmul): the tests of other files that follow find the fp32 products."""
    yield
    from theanet_amd.device import get_context
    get_context().set_fc_matmul("float32")


def _mlp():
    return [("InputLayer", {"img_sz": 12, "num_maps": 1}),
            ("HiddenLayer", {"n_out": 48, "actvn": "relu10", "pdrop": .5, "reg": {"L2": .001, "maxnorm": 2.}}),
            ("HiddenLayer", {"n_out": 40, "actvn": "tanh"}),
            ("SoftmaxLayer", {"n_out": 10})]


def _data(B, n=2, seed=1, img=12, C=1):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, C, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _statement_step(ora, x, y, draws):
    """One training step of a dense net (Input -> Hidden* -> Softmax/nll) on the parameters of ``ora`` (float64), hidden
    products on bf16-rounded operands; updates ora's parameters like OracleNet.train_step.  Returns (cost, logprob)."""
    h = np.asarray(x, np.float64).reshape(len(x), -1)
    cache = {}
    for i, l in enumerate(ora.L):
        if l.kind == "Hidden":
            z = R(h) @ R(l.params[0]) + l.params[1]
            a = O.activation(l.actvn)[0](z)
            m = None
            if l.pdrop:
                m = np.asarray(draws[i], np.float64).reshape(a.shape)
                a = a * m
            cache[i] = (h, z, m)
            h = a
        elif l.kind == "Softmax":
            cache[i] = (h, None, None)
            h = O.log_softmax(h @ l.params[0] + l.params[1])                 # the head: fp32 by design, unrounded here
    logprob = h
    cost = O.nll(logprob, y) + sum(O.wtcost(l.params, l.reg) for l in ora.L if l.params)
    grads, g = {}, None
    first = min(i for i, l in enumerate(ora.L) if l.params)
    for i in range(len(ora.L) - 1, -1, -1):
        l = ora.L[i]
        if l.kind == "Softmax":
            xin = cache[i][0]
            dz = O.nll_dlogits(logprob, y)
            dW, db, g = xin.T @ dz, dz.sum(0), dz @ l.params[0].T
        elif l.kind == "Hidden":
            xin, z, m = cache[i]
            if m is not None:
                g = g * m
            dz = g * O.activation(l.actvn)[1](z)
            dW, db = R(xin).T @ R(dz), dz.sum(0)
            g = R(dz) @ R(l.params[0]).T if i > first else None
        else:
            continue
        grads[i] = [dW + O.wtcost_grad(l.params[0], l.reg), db + O.wtcost_grad(l.params[1], l.reg)]
    for i, gr in grads.items():
        l = ora.L[i]
        if l.vel is None:
            l.vel = [np.zeros_like(p) for p in l.params]
        for j in range(2):
            l.params[j], l.vel[j] = O.sgd_update(l.params[j], l.vel[j], gr[j], ora.cur_learn_rate, l.reg)
    return cost, logprob


def test_matmul_bfloat16_net_builds():
    """Fails on a build without the mode: construction asserts."""
    from theanet_amd import NeuralNet
    net = NeuralNet(copy.deepcopy(_mlp()), dict(TP, MATMUL="bfloat16"))
    assert net.matmul == "bfloat16" and net.ctx._fc_mm == "bfloat16"
    with pytest.raises(AssertionError, match="MATMUL"):
        NeuralNet(copy.deepcopy(_mlp()), dict(TP, MATMUL="fp8"))
    for dt in ("float16", "bfloat16"):       # independent of DTYPE
        net = NeuralNet(copy.deepcopy(_mlp()), dict(TP, MATMUL="bfloat16", DTYPE=dt))
        assert net.matmul == "bfloat16" and net.dtype == dt


def test_matmul_bfloat16_mlp_matches_rounded_operand_statement():
    """Two training steps (forward, every gradient, L2, momentum update, maxnorm) against the statement above at the
    16-bit net tolerances of tests/test_gpu_c8_mean.py, equal argmax -- and closer to it than to the plain float32
    oracle net."""
    from theanet_amd import NeuralNet
    B = TP["BATCH_SZ"]
    x, y = _data(B)
    tr = dict(TP, MATMUL="bfloat16")
    net = NeuralNet(copy.deepcopy(_mlp()), dict(tr))
    ora = O.OracleNet(copy.deepcopy(_mlp()), dict(TP), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(_mlp()), dict(TP), dtype=np.float32)
    (rt, at), wat = TOL["bfloat16"]
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, 1, 12)
        xs, ys = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        if s == 0:
            lp32 = np.asarray(ora32.forward(xs, True, draws)[0], np.float64)
        cost_w, lp_w = _statement_step(ora, xs, ys, draws)
        cost, _, lp = fn(s)
        print("step %d: cost %.6f (statement %.6f), max |dlogprob| %.3g" % (s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="logprob step %d" % s)
        assert_close(cost, cost_w, rt, at, what="cost step %d" % s)
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:
            e16, e32 = np.abs(lp - lp_w).max(), np.abs(lp32 - lp_w).max()
            print("  against the statement %.3g, the float32 oracle against the statement %.3g" % (e16, e32))
            assert e16 < .5 * e32 + 1e-6
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
            assert_close(w, ol.params[j], rt, wat, what="w %d %d" % (i, j))


def _conv_net():
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}),
            ("ConvLayer", {"num_maps": 16, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
            ("PoolLayer", {"pool_sz": 2}),
            ("HiddenLayer", {"n_out": 64, "pdrop": .5}), ("HiddenLayer", {"n_out": 40, "actvn": "tanh"}),
            ("SoftmaxLayer", {"n_out": 10})]


def _round_second_dense(monkeypatch, ora, i2):
    """The stored-16-bit oracle taught, from outside, that Hidden layer ``i2`` (a dense layer NOT on the conv stack) runs
    its three products on bf16-rounded operands: forward R(h) @ R(W); the backward goes down the oracle's own 16-bit
    branch (cache["c8"]: R(x).T @ R(dz), R(dz) @ R(W).T) with the input gradient handed down unrounded (an fp32 tensor)
    and db put back to the column sum of the UNROUNDED dz."""
    class RoundedW:
        __array_ufunc__ = None                       # ndarray @ RoundedW defers to __rmatmul__

        def __init__(self, w):
            self.w = w

        def __rmatmul__(self, h):
            return O.r16(h) @ O.r16(self.w)

    forward, backward, down = ora.forward, ora.backward, ora._f16_down

    def fwd(x, train, draws=None, keep=False, aux=None):
        w = ora.L[i2].params[0]
        ora.L[i2].params[0] = RoundedW(w)
        try:
            h, cache = forward(x, train, draws, keep, aux)
        finally:
            ora.L[i2].params[0] = w
        cache[i2]["c8"] = True
        return h, cache

    def dn(g, i, cache):
        return np.asarray(g, np.float64) if i == i2 else down(g, i, cache)

    def bwd(cache, y):
        grads = backward(cache, y)
        l, top = ora.L[i2], ora.L[i2 + 1]
        assert top.kind == "Softmax" and "mask" not in cache[i2]
        dz = (O.nll_dlogits(cache[i2 + 1]["out"], y) @ top.params[0].T) * O.activation(l.actvn)[1](cache[i2]["z"])
        grads[i2][1] = dz.sum(0) + O.wtcost_grad(l.params[1], l.reg)
        return grads

    monkeypatch.setattr(ora, "forward", fwd)
    monkeypatch.setattr(ora, "_f16_down", dn)
    monkeypatch.setattr(ora, "backward", bwd)


def test_matmul_bfloat16_conv_net_rounds_the_second_dense_layer(monkeypatch):
    """A conv net under DTYPE 'bfloat16' with two hidden layers: the dense layer on the 16-bit stack keeps
    tn_c8_fc_* (the oracle's stored-16-bit mode rounds it), the second HiddenLayer takes the bf16 dense path (the test
    rounds it: _round_second_dense).  Two training steps at the 16-bit net tolerances, equal argmax, closer to that
    statement than to the plain float32 OracleNet -- and, layer-locally on the device's own input, the second layer's
    output is the rounded-operand product, not the fp32 one."""
    from theanet_amd import NeuralNet
    from tests.test_gpu_c8_mean import GS
    B, i2, dt = 16, 4, "bfloat16"
    layers = _conv_net()
    tr = dict(TP, BATCH_SZ=B, DTYPE=dt, GRAD_SCALE=GS[dt])
    monkeypatch.setattr(O, "r16", CB.rbf16)
    monkeypatch.setenv("TN_PIPELINE", "0")           # one step at a time: the layers' buffers hold the step just returned
    x, y = _data(B, img=16, C=3)
    net = NeuralNet(copy.deepcopy(layers), dict(tr, MATMUL="bfloat16"))
    assert net.tr_layers[3].c8 is not None and net.tr_layers[i2].c8 is None
    ora = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float16"), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float32"), dtype=np.float64)
    _round_second_dense(monkeypatch, ora, i2)
    (rt, at), wat = TOL[dt]
    fn = net.get_trin_model(x, y)
    W2, b2 = net.tr_layers[i2].get_wts()
    for s in range(2):
        draws = _inject_draws(net, ora, B, 3, 16)
        xs, ys = x[s * B:(s + 1) * B], y[s * B:(s + 1) * B]
        if s == 0:
            lp32 = ora32.forward(xs, True, draws)[0]
        cost_w, lp_w, _ = ora.train_step(xs, ys, draws)
        cost, _, lp = fn(s)
        print("%s step %d: cost %.6f (statement %.6f), max |dlogprob| %.3g" % (dt, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="logprob step %d" % s)
        assert_close(cost, cost_w, rt, at, what="cost step %d" % s)
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:
            e16, e32 = np.abs(lp - lp_w).max(), np.abs(lp32 - lp_w).max()
            print("  against the statement %.3g, the float32 oracle against the statement %.3g" % (e16, e32))
            assert e16 < .5 * e32 + 1e-6
            # layer-local: the second dense layer on the device's own input (fp32 tensors; always bf16 operands)
            h = net.tr_layers[i2 - 1].output.get_value().astype(np.float64)
            a = net.tr_layers[i2].output.get_value()
            a_r = np.tanh(CB.rbf16(h) @ CB.rbf16(W2) + b2)
            a_p = np.tanh(h @ W2.astype(np.float64) + b2)
            er, ep = np.abs(a - a_r).max(), np.abs(a_p - a_r).max()
            print("  layer %d output: against the rounded-operand product %.3g, fp32 product against it %.3g" % (i2, er, ep))
            assert er <= 2e-5 * np.abs(a_r).max() and er < .5 * ep
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
            assert_close(w, ol.params[j], rt, wat, what="w %d %d" % (i, j))


def _head_nets():
    inp = ("InputLayer", {"img_sz": 12, "num_maps": 1})
    return {"softmax57": [inp, ("SoftmaxLayer", {"n_out": 57})],
            "softmax57-hidden": [inp, ("HiddenLayer", {"n_out": 48}), ("SoftmaxLayer", {"n_out": 57})],
            "hinge": [inp, ("HingeLayer", {"n_out": 24})],
            "exploss": [inp, ("ExpLossLayer", {"n_out": 24})]}


@pytest.mark.parametrize("head", sorted(_head_nets()))
def test_matmul_bfloat16_heads_stay_fp32(head):
    """The output heads stay fp32 by design, also where their affine map goes through the generic products (a Softmax
    head wider than 16 outputs, the Hinge / ExpLoss heads): a net that is only a head gives the bits of the same net
    under MATMUL 'float32'; with a HiddenLayer under the head the results differ (the hidden layer is bf16), the head's
    own step on identical inputs is covered by the first three cases."""
    from theanet_amd import NeuralNet
    B = 16
    x, y = _data(B)
    y = y % 24
    res = {}
    for mm in ("float32", "bfloat16"):
        net = NeuralNet(copy.deepcopy(_head_nets()[head]), dict(TP, BATCH_SZ=B, MATMUL=mm))
        fn = net.get_trin_model(x, y)
        outs = [fn(s) for s in range(2)]
        te = net.get_test_model(x, y)(1)
        res[mm] = ([np.asarray(o[2]) for o in outs] + [np.asarray(v) for v in te], [w for l in net.tr_layers for w in l.get_wts()])
    same = all((u == v).all() for a, b in zip(res["float32"], res["bfloat16"]) for u, v in zip(a, b))
    assert same == (head != "softmax57-hidden"), head


@pytest.mark.parametrize("case", ["mlp", "conv-bf16"])
def test_matmul_bfloat16_schedules_are_bit_identical(case, monkeypatch):
    """Two steps in flight against one at a time, replayed (tn_net_plan_*) against interpreted steps, a test-model call
    in the middle: bit for bit (the products go through the same calls in every schedule)."""
    from theanet_amd import NeuralNet
    B = 16
    layers, tp, img, C = (_mlp(), dict(TP, BATCH_SZ=B, MATMUL="bfloat16"), 12, 1) if case == "mlp" else \
        (_conv_net(), dict(TP, BATCH_SZ=B, MATMUL="bfloat16", DTYPE="bfloat16"), 16, 3)
    x, y = _data(B, n=6, seed=5, img=img, C=C)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(layers), dict(tp))
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


def test_matmul_float32_weights_load_into_bfloat16_net():
    """The checkpoint route: weights of a MATMUL 'float32' net loaded through allwts into a 'bfloat16' net -- get_wts
    equal, first-step logprob within the bf16 net tolerance of the fp32 net's (and not the same bits)."""
    from theanet_amd import NeuralNet
    B = TP["BATCH_SZ"]
    layers = copy.deepcopy(_mlp())
    layers[1][1]["pdrop"] = 0
    x, y = _data(B)
    n32 = NeuralNet(copy.deepcopy(layers), dict(TP, MATMUL="float32"))
    wts = n32.get_init_params()["allwts"]
    nbf = NeuralNet(copy.deepcopy(layers), dict(TP, SEED=12, MATMUL="bfloat16"), allwts=wts)
    for a, b in zip(n32.tr_layers, nbf.tr_layers):
        for u, v in zip(a.get_wts(), b.get_wts()):
            np.testing.assert_array_equal(u, v)
    lp32 = n32.get_trin_model(x, y)(0)[2]
    lpbf = nbf.get_trin_model(x, y)(0)[2]
    (rt, at), _ = TOL["bfloat16"]
    print("max |dlogprob| bfloat16 - float32: %.3g" % np.abs(lpbf - lp32).max())
    assert_close(lpbf, lp32, rt, at, what="bfloat16 logprob against the float32 net's")
    assert (lpbf != lp32).any()


def test_mlp3_prms_parses_builds_and_steps():
    from theanet_amd import NeuralNet
    prms = load_prms("mlp3.prms", 28, batch=64)
    assert prms["training_params"]["MATMUL"] == "bfloat16"
    assert [l[1].get("n_out") for l in prms["layers"][1:]] == [2048, 2048, 1000, 10]
    net = NeuralNet(prms["layers"], prms["training_params"])
    assert net.matmul == "bfloat16"
    rng = np.random.RandomState(2)
    x, y = rng.rand(128, 1, 28, 28).astype(np.float32), rng.randint(0, 10, 128).astype(np.int32)
    fn = net.get_trin_model(x, y)
    for s in range(2):
        assert np.isfinite(fn(s)[0])
