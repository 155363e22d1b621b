"""DTYPE='bfloat16' nets: NeuralNet with bf16-RESIDENT conv stacks (tests/test_gpu_c8_bf16.py has the ops) against the
float64 oracle in its stored-16-bit mode with bf16 rounding -- oracle.theanet_oracle's DTYPE 'float16' statement with
its one rounding function r16 replaced by tests/c8b_util.py's rbf16 (every stored-fp16 rounding of the oracle goes
through that module-global function).

Tolerances.  As in tests/test_gpu_f16.py, scaled by the precision: one bf16 ulp is 2^-7 of the value (fp16: 2^-10), so a
value on a rounding boundary that rounds the other way moves by up to 8 times more than in fp16: logprob and cost
1.6e-2 rel + 1.6e-3 abs, weights after two steps 1.6e-2 rel, argmax exact.  Bit-identity claims (grad-scale invariance,
schedules, two dtypes in one process) are exact."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import assert_close, load_prms
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

RT, AT = 1.6e-2, 1.6e-3
R16 = O.r16             # the oracle's fp16 rounding, before any test swaps it


@pytest.fixture
def bf16_oracle(monkeypatch):
    """The oracle's stored-16-bit mode rounds to bf16 while the fixture is active."""
    monkeypatch.setattr(O, "r16", CB.rbf16)
    yield
    monkeypatch.setattr(O, "r16", R16)


def _tr(prms, **kw):
    return dict(prms["training_params"], **dict(dict(DTYPE="bfloat16", GRAD_SCALE=1.0), **kw))


def _oracle(prms, tr, **kw):
    """The stored-16-bit oracle with the device net's GRAD_SCALE (rounding: whatever O.r16 is when it runs)."""
    return O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), dtype=np.float64, **kw)


@pytest.mark.parametrize("name,img,B", [("cifar_like.prms", 32, 16), ("wide6.prms", 64, 4), ("wide6.prms", 32, 6)])
def test_bf16_nets_match_bf16_oracle(name, img, B, bf16_oracle, monkeypatch):
    """Two training steps (forward, every gradient, momentum update, maxnorm) in DTYPE bfloat16 against the stored-bf16
    oracle; and the device is measurably closer to it than to the stored-fp16 and the fp32 oracles -- a build whose
    kernels rounded to half (or not at all) fails."""
    from theanet_amd import NeuralNet
    prms = load_prms(name, img, batch=B)
    tr = _tr(prms)
    rng = np.random.RandomState(1)
    x = rng.rand(2 * B, 3, img, img).astype(np.float32)
    y = rng.randint(0, 10, 2 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    assert net.grad_scale == 1.0 and net.ctx.lib.tn_get_matmul_dtype(net.ctx.h) == 2
    assert all(l.f16 for l in net.tr_layers if hasattr(l, "f16"))
    ora = _oracle(prms, tr)
    ora16 = _oracle(prms, dict(tr, GRAD_SCALE=4096.))
    ora32 = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float32"), dtype=np.float64)
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, 3, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        assert_close(lp, lp_w, RT, AT, what="%s bf16 logprob step %d" % (name, s))
        assert_close(cost, cost_w, RT, AT, what="%s bf16 cost step %d" % (name, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:
            lp_bf = lp_w                                  # (the oracles below have not trained yet: same weights)
            lp32 = ora32.forward(x[:B], True, draws)[0]
            monkeypatch.setattr(O, "r16", R16)
            lp16 = ora16.forward(x[:B], True, draws)[0]
            monkeypatch.setattr(O, "r16", CB.rbf16)
            d = np.abs(lp - lp_bf).max()
            assert d < .5 * np.abs(lp16 - lp_bf).max() and d < .5 * np.abs(lp32 - lp_bf).max(), (
                d, np.abs(lp16 - lp_bf).max(), np.abs(lp32 - lp_bf).max())
            assert np.abs(lp - lp16).max() > 2 * d          # ... and measurably away from the fp16 statement
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            assert_close(w, ol.params[j], RT, 1.6e-5, what="%s bf16 w %d %d" % (name, i, j))


def _steps(prms, tr, x, y, n, env=(), monkeypatch=None):
    from theanet_amd import NeuralNet
    for k, v in env:
        monkeypatch.setenv(k, v)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    fn = net.get_trin_model(x, y)
    outs = [fn(s % 2) for s in range(n)]
    return net, outs, [w.copy() for l in net.tr_layers for w in l.get_wts()]


def test_bf16_grad_scale_is_exact():
    """A power-of-two gradient scale commutes with every rounding in bf16's range: GRAD_SCALE 1 and 4096 give
    bit-identical weights after three steps (in fp16 they do not: the small gradients of the unscaled run fall into
    fp16's subnormals)."""
    prms = load_prms("cifar_like.prms", 32, batch=16)
    rng = np.random.RandomState(2)
    x = rng.rand(32, 3, 32, 32).astype(np.float32)
    y = rng.randint(0, 10, 32).astype(np.int32)
    _, o1, w1 = _steps(prms, _tr(prms), x, y, 3)
    _, o2, w2 = _steps(prms, _tr(prms, GRAD_SCALE=4096.), x, y, 3)
    for a, b in zip(o1, o2):
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[2], b[2])
    for a, b in zip(w1, w2):
        np.testing.assert_array_equal(a, b)
    assert any(not np.array_equal(a, b) for a, b in zip(w1, _steps(prms, _tr(prms), x, y, 1)[2]))   # (the steps moved them)


def test_bf16_range_beyond_fp16(bf16_oracle):
    """Inputs scaled so that the first conv block's stored activations exceed fp16's largest value (65504): the read-back
    holds them, and one training step is finite and matches the stored-bf16 oracle (cost, logprob, updated weights)."""
    from theanet_amd import NeuralNet
    from theanet_amd.device import C8Array
    B_, img = 16, 32
    prms = load_prms("cifar_like.prms", img, batch=B_)
    tr = _tr(prms)
    rng = np.random.RandomState(4)
    x = (rng.rand(B_, 3, img, img) * 1e5).astype(np.float32)
    y = rng.randint(0, 10, B_).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    ora = _oracle(prms, tr)
    fn = net.get_trin_model(x, y)
    draws = _inject_draws(net, ora, B_, 3, img)
    cost_w, lp_w, _ = ora.train_step(x, y, draws)
    cost, _, lp = fn(0)
    # the first STORED 16-bit tensor: the first block's pooled output (its conv map is never materialised)
    first = next(l.output for l in net.tr_layers
                 if isinstance(getattr(l, "output", None), C8Array) and getattr(l, "fused_pool", None) is None)
    assert first.elem == "bfloat16"
    big = np.abs(first.get_value()).max()
    assert np.isfinite(big) and big > 65504, big
    assert np.isfinite(cost) and np.isfinite(lp).all()
    assert_close(lp, lp_w, RT, AT * max(1.0, float(np.abs(lp_w).max())), what="range logprob")
    assert_close(cost, cost_w, RT, AT, what="range cost")
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            assert np.isfinite(w).all()
            assert_close(w, ol.params[j], RT, 1.6e-5 * max(1.0, float(np.abs(ol.params[j]).max())),
                         what="range w %d %d" % (i, j))


def _full_size(name, img, B, rows, steps):
    """tests/test_gpu_f16.py's _full_size in bf16: the cost falls, and a test-mode forward of the first `rows` rows with
    the trained weights matches the stored-bf16 oracle."""
    from theanet_amd import NeuralNet
    prms = load_prms(name, img, batch=B)
    tr = _tr(prms)
    rng = np.random.default_rng(0)
    x = rng.random((2 * B, 3, img, img), dtype=np.float32)
    y = np.random.default_rng(1).integers(0, 10, 2 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    fn = net.get_trin_model(x, y)
    conv = [l for l in net.tr_layers if getattr(l, "params", None)][1]
    w0 = conv.get_wts()[0]
    cost0, _, lp = fn(0)
    assert np.isfinite(cost0) and abs(cost0 - np.log(10)) < 1.5
    np.testing.assert_allclose(np.exp(lp).sum(1), 1, rtol=1e-4)
    costs = [fn(i % 2)[0] for i in range(1, steps)]
    assert np.isfinite(costs).all() and min(costs[-2:]) < cost0, (cost0, costs)
    assert not np.array_equal(conv.get_wts()[0], w0)
    ora = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), allwts=net.get_init_params()["allwts"])
    tfn = net.get_test_model(x, y, preds_feats=True)
    sym, pm, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:B + rows], y[B:B + rows])
    assert_close(feats[:rows], lp_w, RT, AT, what="%s bfloat16 test logprob rows 0..%d" % (name, rows - 1))
    np.testing.assert_array_equal(preds[:rows], preds_w)
    assert 0 <= sym <= 1 and 0 < pm <= 1


def test_bf16_full_size_wide6_64x64_b128(bf16_oracle):
    _full_size("wide6.prms", 64, 128, 16, 8)


def test_bf16_full_size_cifar_like_b2048(bf16_oracle):
    _full_size("cifar_like.prms", 32, 2048, 256, 12)


@pytest.mark.parametrize("name,img,B", [("cifar_like.prms", 32, 16), ("wide6.prms", 32, 4)])
def test_bf16_pipelined_steps_equal_sequential(monkeypatch, name, img, B):
    """Two steps in flight against one at a time: costs, logprobs and weights bit for bit."""
    from theanet_amd.neuralnet import _PipeTrainFn, _TrainFn
    prms = load_prms(name, img, batch=B)
    rng = np.random.RandomState(9)
    x = rng.rand(4 * B, 3, img, img).astype(np.float32)
    y = rng.randint(0, 10, 4 * B).astype(np.int32)
    runs = []
    for pipe in ("1", "0"):
        net, outs, ws = _steps(prms, _tr(prms), x, y, 7, [("TN_PIPELINE", pipe)], monkeypatch)
        runs.append((outs, ws))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a[0] == b[0]
        np.testing.assert_array_equal(a[2], b[2])
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_bf16_planned_steps_equal_interpreted_steps(pipeline, monkeypatch):
    """Replayed steps (tn_net_plan_*) against interpreted ones: costs, outputs and weights bit for bit."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", pipeline)
    prms = load_prms("cifar_like.prms", 32, batch=16)
    rng = np.random.RandomState(5)
    x = rng.rand(16 * 6, 3, 32, 32).astype(np.float32)
    y = rng.randint(0, 10, 16 * 6).astype(np.int32)

    def run(plan):
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms))
        fn = net.get_trin_model(x, y)
        outs = []
        for s in range(30):
            if s in (20, 29):
                outs.append(fn(s % 6))
            else:
                fn.enqueue(s % 6)
        pl = getattr(fn, "_plan", None)
        replayed = pl is not None and pl.ready
        if fn.__class__.__name__ == "_PipeTrainFn" and fn._seq is not None:
            replayed = fn._seq._plan.ready
        return outs, [w for l in net.tr_layers for w in l.get_wts()], replayed

    o1, w1, r1 = run("1")
    o0, w0, r0 = run("0")
    assert r1 and not r0
    for a, b in zip(o1, o0):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
    for a, b in zip(w1, w0):
        np.testing.assert_array_equal(a, b)


def test_bf16_dp_pipelined_equals_sequential(monkeypatch):
    """The one-rank data-parallel step with two steps in flight against one at a time, bit for bit."""
    from theanet_amd import NeuralNet
    from theanet_amd.neuralnet import _PipeTrainFn
    prms = load_prms("wide6.prms", 32, batch=8)
    rng = np.random.RandomState(10)
    x = rng.rand(32, 3, 32, 32).astype(np.float32)
    y = rng.randint(0, 10, 32).astype(np.int32)
    runs = []
    for pipe in ("1", "0"):
        monkeypatch.setenv("TN_DP_FORCE", "1")
        monkeypatch.setenv("TN_DP_PIPELINE", pipe)
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_DP_OVERLAP", "0")
        net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms))
        fn = net.get_trin_model(x, y)
        assert isinstance(fn, _PipeTrainFn) == (pipe == "1")
        outs = []
        for s in range(8):
            fn.enqueue(s % 4)
            if s in (3, 7):
                outs.append(fn.fetch())
        if pipe == "1":
            assert fn._seq is None and net.dp_schedule == "pipelined"
        runs.append((outs, [w.copy() for l in net.tr_layers for w in l.get_wts()]))
        net.ctx.call("tn_comm_destroy")
        net._dev_group = None
    for (c0, _, l0), (c1, _, l1) in zip(runs[0][0], runs[1][0]):
        assert c0 == c1
        np.testing.assert_array_equal(l0, l1)
    for wa, wb in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(wa, wb)


def test_bf16_and_f16_nets_alternate_in_one_process():
    """An fp16 net and a bf16 net on the same context, stepping in turn: each ends bit-identical to the same net run
    alone (the mode is context state; every enqueue sets its net's mode first)."""
    from theanet_amd import NeuralNet
    prms = load_prms("cifar_like.prms", 32, batch=16)
    rng = np.random.RandomState(12)
    x = rng.rand(32, 3, 32, 32).astype(np.float32)
    y = rng.randint(0, 10, 32).astype(np.int32)
    trs = {"float16": dict(prms["training_params"], DTYPE="float16", GRAD_SCALE=4096.), "bfloat16": _tr(prms)}
    alone = {k: _steps(prms, tr, x, y, 4) for k, tr in trs.items()}
    nets = {k: NeuralNet(copy.deepcopy(prms["layers"]), dict(tr)) for k, tr in trs.items()}
    fns = {k: n.get_trin_model(x, y) for k, n in nets.items()}
    outs = {k: [] for k in trs}
    for s in range(4):
        for k in ("float16", "bfloat16"):
            outs[k].append(fns[k](s % 2))
    for k in trs:
        for a, b in zip(outs[k], alone[k][1]):
            assert a[0] == b[0], k
            np.testing.assert_array_equal(a[2], b[2])
        for a, b in zip([w for l in nets[k].tr_layers for w in l.get_wts()], alone[k][2]):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(outs["float16"][-1][2], outs["bfloat16"][-1][2])
