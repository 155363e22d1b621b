"""Nets with L1 / L2 weight costs (``reg: {'L1': ..., 'L2': ...}``, layer.py:70-117) on the fast schedules: the step's
cost as one launch (tn_wtcost_net), the pipelined update with the weight-cost gradient terms (TN_UPD_PIPE_REG), and the
nets themselves -- two steps in flight against one step at a time bit for bit, the cost ring, the fused against the
generic schedule, optimiser state, leaving the pipeline, and the float64 oracle."""
import copy
import functools

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import assert_close, call, ctx, dev, empty, load_prms
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from theanet_amd import _lib

pytestmark = pytest.mark.gpu

CH = _lib.TN_WTCOST_CHUNK
WC_DT = np.dtype([('p', 'u8'), ('n', 'u8'), ('L1', 'f4'), ('L2', 'f4')])
SIZES = (1, 3, 1000, CH - 1, CH, CH + 1, 3 * CH + 5)
#        L1 only     L2 only     both        all zero  both          L1 only     L2 only
REGS = ((.01, 0.), (0., .02), (.003, .004), (0., 0.), (.0005, .001), (.02, 0.), (0., .0007))


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _table():
    """Seven tensors (the 1000-element one starts 4 bytes off a 16-byte boundary), their tn_wc_seg table, and the float64
    weight cost."""
    rng = np.random.RandomState(17)
    host, arrs, rows, want = [], [], [], 0.0
    for n, (l1, l2) in zip(SIZES, REGS):
        p = rng.randn(n).astype(np.float32)
        if n == 1000:
            buf = dev(np.concatenate([[9.], p]).astype(np.float32))
            d = buf.view(1, (n,))
        else:
            d = dev(p)
        host.append(p)
        arrs.append(d)
        rows.append((d.ptr, n, l1, l2))
        p64 = p.astype(np.float64)
        want += np.float64(np.float32(l1)) * np.abs(p64).sum() + np.float64(np.float32(l2)) * (p64 * p64).sum()
    return np.array(rows, dtype=WC_DT), arrs, want


@pytest.mark.parametrize("nrow", [1, 37, 300])
def test_wtcost_net_against_float64(nrow):
    assert WC_DT.itemsize == 24
    tab, keep, want_w = _table()
    rng = np.random.RandomState(nrow)
    rl = (rng.rand(nrow) * 3).astype(np.float32)
    rld, scale = dev(rl), 1.0 / 300
    want_c = scale * rl.astype(np.float64).sum()
    cost = dev(np.array([777.], np.float32))
    call("tn_wtcost_net", tab.ctypes.data, len(tab), rld.ptr, nrow, scale, cost.ptr, 0)
    assert_close(cost.get_value()[0], want_c + want_w, what="cost + weight costs")
    # rowloss = NULL: the weight costs alone
    call("tn_wtcost_net", tab.ctypes.data, len(tab), None, 0, 0.0, cost.ptr, 0)
    assert_close(cost.get_value()[0], want_w, what="weight costs alone")
    # ... added to what d_cost holds (the data-parallel form), and with the row losses as well
    cost.set_value(np.array([2.5], np.float32))
    call("tn_wtcost_net", tab.ctypes.data, len(tab), None, 0, 0.0, cost.ptr, 1)
    assert_close(cost.get_value()[0], 2.5 + want_w, what="accumulate")
    cost.set_value(np.array([-1.25], np.float32))
    call("tn_wtcost_net", tab.ctypes.data, len(tab), rld.ptr, nrow, scale, cost.ptr, 1)
    assert_close(cost.get_value()[0], -1.25 + want_c + want_w, what="accumulate with row losses")
    # a table of nothing but rows that add nothing
    zero = tab[3:4].copy()
    call("tn_wtcost_net", zero.ctypes.data, 1, None, 0, 0.0, cost.ptr, 0)
    assert cost.get_value()[0] == 0.0


@pytest.mark.parametrize("nrow", [1, 37, 300])
def test_empty_table_gives_the_rider_bits(nrow):
    rl = dev((np.random.RandomState(nrow + 5).rand(nrow) * 5).astype(np.float32))
    lr = dev(np.array([.1], np.float32))
    a, b = dev(np.array([5.], np.float32)), dev(np.array([6.], np.float32))
    call("tn_sgd_update_net", _lib.TN_UPD_PLAIN, None, None, 0, 0, lr.ptr, 1.0, None, 0, 0, rl.ptr, nrow, 1.0 / 64, a.ptr)
    call("tn_wtcost_net", None, 0, rl.ptr, nrow, 1.0 / 64, b.ptr, 0)
    assert _bits(a.get_value())[0] == _bits(b.get_value())[0]


def test_wtcost_net_repeats_bit_for_bit_and_resets_its_ticket():
    tab, keep, want_w = _table()
    rl = (np.random.RandomState(2).rand(37) * 3).astype(np.float32)
    rld = dev(rl)
    want = rl.astype(np.float64).sum() / 37 + want_w
    cost = dev(np.zeros(1, np.float32))
    got = []
    for _ in range(3):
        cost.set_value(np.array([np.nan], np.float32))
        call("tn_wtcost_net", tab.ctypes.data, len(tab), rld.ptr, 37, 1.0 / 37, cost.ptr, 0)
        got.append(_bits(cost.get_value())[0])
    # other launches in between (another table, other kernels), then the same call again
    other = dev(np.zeros(1, np.float32))
    call("tn_wtcost_net", tab[:3].ctypes.data, 3, None, 0, 0.0, other.ptr, 0)
    call("tn_wtcost", keep[2].ptr, 1000, .01, .02, other.ptr, 1)
    call("tn_reduce_sum", rld.ptr, 37, 1.0, other.ptr, 0)
    cost.set_value(np.array([np.nan], np.float32))
    call("tn_wtcost_net", tab.ctypes.data, len(tab), rld.ptr, 37, 1.0 / 37, cost.ptr, 0)
    got.append(_bits(cost.get_value())[0])
    assert len(set(got)) == 1, got
    assert_close(cost.get_value()[0], want, what="the fourth call")


# ---- TN_UPD_PIPE_REG -------------------------------------------------------------------------------------------
PIPE_DT = np.dtype([('p', 'u8'), ('psrc', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'), ('momentum', 'f4'), ('rate', 'f4')])
REG_DT = np.dtype(PIPE_DT.descr + [('L1', 'f4'), ('L2', 'f4')])
SGD_DT = np.dtype([('p', 'u8'), ('v', 'u8'), ('g', 'u8'), ('n', 'u8'), ('momentum', 'f4'), ('rate', 'f4'), ('L1', 'f4'),
                   ('L2', 'f4')])
NS = (1, 5, 1024, 4099)
MOM, RATE, LR = .9, .5, .1


def _pipe_case(l1l2, mode, flags):
    """One launch over four tensors: (new p_own, new v, inputs)."""
    rng = np.random.RandomState(41)
    rows, outs, ins = [], [], []
    for n, (l1, l2) in zip(NS, l1l2):
        po, ps, v, g = (rng.randn(n).astype(np.float32) for _ in range(4))
        po[0] = 0.0                         # sign(0) = 0
        d = [dev(a) for a in (po, ps, v, g)]
        row = (d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n, MOM, RATE)
        rows.append(row + ((l1, l2) if mode == _lib.TN_UPD_PIPE_REG else ()))
        outs.append(d)
        ins.append((po, ps, v, g))
    host = np.array(rows, dtype=REG_DT if mode == _lib.TN_UPD_PIPE_REG else PIPE_DT)
    lr = dev(np.array([LR], np.float32))
    call("tn_sgd_update_net", mode, dev(host.view(np.uint8)).ptr, host.ctypes.data, len(NS), max(NS), lr.ptr, 1.0, None, 0,
         flags, None, 0, 0.0, None)
    return [d[0].get_value() for d in outs], [d[2].get_value() for d in outs], ins


def test_pipe_reg_without_terms_is_the_pipelined_update():
    assert REG_DT.itemsize == 56 and PIPE_DT.itemsize == 48
    p0, v0, _ = _pipe_case([(0., 0.)] * 4, _lib.TN_UPD_PIPE, 1)
    p1, v1, _ = _pipe_case([(0., 0.)] * 4, _lib.TN_UPD_PIPE_REG, 1)
    for a, b in zip(p0 + v0, p1 + v1):
        np.testing.assert_array_equal(_bits(a), _bits(b))


def test_pipe_reg_velocity_is_the_plain_update_at_the_old_weights():
    l1l2 = [(.01, .02), (.01, 0.), (0., .02), (.0005, .001)]
    p1, v1, ins = _pipe_case(l1l2, _lib.TN_UPD_PIPE_REG, 1)
    lr = dev(np.array([LR], np.float32))
    for (po, ps, v, g), (l1, l2), pn, vn in zip(ins, l1l2, p1, v1):
        pd, vd = dev(po), dev(v)
        seg = np.array([(pd.ptr, vd.ptr, dev(g).ptr, po.size, MOM, RATE, l1, l2)], dtype=SGD_DT)
        call("tn_sgd_update_net", _lib.TN_UPD_PLAIN, dev(seg.view(np.uint8)).ptr, None, 1, po.size, lr.ptr, 1.0, None, 0, 0,
             None, 0, 0.0, None)
        np.testing.assert_array_equal(_bits(vn), _bits(vd.get_value()))
        if po.size > 1:                     # (the one-element tensor is the weight 0: its term is 0) the term is in
            assert not np.array_equal(vn, O.sgd_update(po, v, g, LR, dict(O.DEFAULT_REG, momentum=MOM, rate=RATE))[1])
        want = ps.astype(np.float64) - np.float64(np.float32(RATE) * np.float32(LR)) * vn.astype(np.float64)
        assert_close(pn, want, atol=1e-6, what="p of %d elements" % po.size)
        reg = dict(O.DEFAULT_REG, momentum=MOM, rate=RATE, L1=l1, L2=l2)
        v_w = O.sgd_update(po, v, g + O.wtcost_grad(po, reg), LR, reg)[1]
        assert_close(vn, v_w, atol=1e-6, what="v of %d elements" % po.size)


def test_pipe_reg_with_bit_0_clear_leaves_the_velocity():
    l1l2 = [(.01, .02)] * 4
    p1, v1, ins = _pipe_case(l1l2, _lib.TN_UPD_PIPE_REG, 0)
    p0, v0, _ = _pipe_case(l1l2, _lib.TN_UPD_PIPE, 0)
    for (po, ps, v, g), pn, vn, pp, vp in zip(ins, p1, v1, p0, v0):
        np.testing.assert_array_equal(_bits(vn), _bits(v))
        np.testing.assert_array_equal(_bits(pn), _bits(pp))


@pytest.mark.parametrize("n", NS)
def test_delayed_velocity_fold_with_bit_2_is_the_plain_velocity(n):
    """TN_UPD_DELAYED, "v only" (3) + flags bit 2: the segment's L1 / L2 at seg.p -- the velocity TN_UPD_PLAIN leaves, bit for
    bit; p untouched; without the bit no term."""
    rng = np.random.RandomState(n)
    p, v, g = (rng.randn(n).astype(np.float32) for _ in range(3))
    lr = dev(np.array([LR], np.float32))
    got = {}
    for which in (3 | 4, 3, None):
        pd, vd = dev(p), dev(v)
        seg = np.array([(pd.ptr, vd.ptr, dev(g).ptr, n, MOM, RATE, .01, .02)], dtype=SGD_DT)
        ds = dev(seg.view(np.uint8))
        if which is None:
            call("tn_sgd_update_net", _lib.TN_UPD_PLAIN, ds.ptr, None, 1, n, lr.ptr, 1.0, None, 0, 0, None, 0, 0.0, None)
        else:
            call("tn_sgd_update_net", _lib.TN_UPD_DELAYED, ds.ptr, None, 1, n, lr.ptr, 1.0, None, 0, which, None, 0, 0.0, None)
            np.testing.assert_array_equal(_bits(pd.get_value()), _bits(p))
        got[which] = vd.get_value()
    np.testing.assert_array_equal(_bits(got[3 | 4]), _bits(got[None]))
    assert not np.array_equal(got[3], got[None])
    reg = dict(O.DEFAULT_REG, momentum=MOM, rate=RATE)
    assert_close(got[3], O.sgd_update(p, v, g, LR, reg)[1], atol=1e-6, what="no term without the bit")


# ---- nets ------------------------------------------------------------------------------------------------------
def _layers(kind):
    if kind == "mlp":
        return [("InputLayer", {"img_sz": 12, "num_maps": 1}),
                ("HiddenLayer", {"n_out": 100, "pdrop": .5, "actvn": "relu10", "reg": {"L2": .001}}),
                ("HiddenLayer", {"n_out": 30, "actvn": "scaled_tanh"}),
                ("SoftmaxLayer", {"n_out": 57})], 48, 12, 1, 57
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}),
            ("ConvLayer", {"num_maps": 8, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10",
                           "reg": {"L1": .0005, "maxnorm": 2}}),
            ("PoolLayer", {"pool_sz": 2}),
            ("HiddenLayer", {"n_out": 40, "pdrop": .5, "actvn": "relu05", "reg": {"L2": .001, "rate": 0}}),
            ("SoftmaxLayer", {"n_out": 10})], 32, 16, 3, 10


@functools.lru_cache(maxsize=None)
def _data(kind):
    layers, B, img, C, n_cls = _layers(kind)
    rng = np.random.RandomState(9)
    x = rng.rand(4 * B, C, img, img).astype(np.float32)
    y = rng.randint(0, n_cls, 4 * B).astype(np.int32)
    x.setflags(write=False)
    y.setflags(write=False)
    return layers, {"SEED": 31, "BATCH_SZ": B, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 1}, x, y


def _net(kind):
    from theanet_amd import NeuralNet
    layers, tr, x, y = _data(kind)
    return NeuralNet(copy.deepcopy(layers), dict(tr)), x, y


def _weights(net):
    return [w.copy() for l in net.tr_layers for w in l.get_wts()]


def _nine_steps(kind, pipe, every, monkeypatch):
    from theanet_amd.neuralnet import _PipeTrainFn, _TrainFn
    monkeypatch.setenv("TN_PIPELINE", pipe)
    net, x, y = _net(kind)
    fn = net.get_trin_model(x, y)
    assert isinstance(fn, _PipeTrainFn if pipe == "1" else _TrainFn)
    te = net.get_test_model(x, y)
    outs, mids = [], []
    for s in range(9):
        if s == 5:
            net.inc_epoch_set_rate()
        if every:
            outs.append(fn(s % 4))
        else:
            fn.enqueue(s % 4)
        if s in (2, 5):
            mids.append((te(1), _weights(net)))
    outs.append(fn.fetch())
    if pipe == "1":
        assert fn._seq is None and fn.t == 9
    return outs, mids, _weights(net)


@functools.lru_cache(maxsize=None)
def _sequential(kind, every):
    mp = pytest.MonkeyPatch()
    try:
        return _nine_steps(kind, "0", every, mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("kind", ["mlp", "conv"])
def test_weight_cost_nets_take_the_pipelined_schedule(monkeypatch, kind):
    from theanet_amd.neuralnet import _PipeTrainFn
    monkeypatch.setenv("TN_PIPELINE", "1")
    net, x, y = _net(kind)
    fn = net.get_trin_model(x, y)
    assert net._has_wtcost and isinstance(fn, _PipeTrainFn)
    for s in range(3):
        fn.enqueue(s)
    assert fn._seq is None and fn.t == 3
    assert np.isfinite(fn.fetch()[0])


@pytest.mark.parametrize("every", [True, False], ids=["fn(i)", "enqueue"])
@pytest.mark.parametrize("kind", ["mlp", "conv"])
def test_pipelined_steps_of_weight_cost_nets_equal_sequential(monkeypatch, kind, every):
    got, want = _nine_steps(kind, "1", every, monkeypatch), _sequential(kind, every)
    assert len(got[0]) == len(want[0]) == (10 if every else 1)
    for (c0, _, l0), (c1, _, l1) in zip(got[0], want[0]):
        assert _bits(c0) == _bits(c1), (c0, c1)
        np.testing.assert_array_equal(l0, l1)
    for (t0, w0), (t1, w1) in zip(got[1], want[1]):
        assert t0 == t1
        for u, v in zip(w0, w1):
            np.testing.assert_array_equal(u, v)
    for u, v in zip(got[2], want[2]):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("pipe", ["1", "0"])
@pytest.mark.parametrize("kind", ["mlp", "conv"])
def test_cost_ring_of_weight_cost_nets(monkeypatch, kind, pipe):
    monkeypatch.setenv("TN_PIPELINE", pipe)
    net, x, y = _net(kind)
    fn = net.get_trin_model(x, y)
    got = []
    for s in range(9):
        got += fn.step_cost(s % 4)
    got += fn.drain_costs()
    assert [k for k, _ in got] == list(range(9))
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("TN_PIPELINE", "0")
        net2, _, _ = _net(kind)
        fn2 = net2.get_trin_model(x, y)
        want = [fn2(s % 4)[0] for s in range(9)]
    finally:
        mp.undo()
    np.testing.assert_array_equal(_bits([c for _, c in got]), _bits(want))
    for u, v in zip(_weights(net), _weights(net2)):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("kind", ["mlp", "conv"])
def test_fused_schedule_of_weight_cost_nets_against_the_generic_one(monkeypatch, kind):
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(NeuralNet, "fused_step", fused)
        net, x, y = _net(kind)
        fn = net.get_trin_model(x, y)
        outs = [fn(s % 4) for s in range(4)]
        runs.append((outs, net.flat_grads.get_value()[:net.n_flat - 1], _weights(net)))
    for (c0, _, l0), (c1, _, l1) in zip(runs[0][0], runs[1][0]):
        np.testing.assert_allclose(c0, c1, rtol=1e-6)           # a different but fixed summation order
        np.testing.assert_array_equal(l0, l1)
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    for u, v in zip(runs[0][2], runs[1][2]):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("kind", ["mlp", "conv"])
def test_optimiser_state_and_leaving_the_pipeline(monkeypatch, kind):
    from theanet_amd.neuralnet import _PipeTrainFn
    states, nets, fns = [], [], []
    for pipe in ("1", "0"):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        net, x, y = _net(kind)
        fn = net.get_trin_model(x, y)
        for s in range(5):
            fn.enqueue(s % 4)
        states.append(net.get_init_params(with_opt_state=True))
        nets.append(net)
        fns.append(fn)
    assert isinstance(fns[0], _PipeTrainFn) and fns[0]._seq is None
    a, b = states
    for wa, wb in zip(a["allwts"], b["allwts"]):
        for u, v in zip(wa, wb):
            np.testing.assert_array_equal(u, v)
    assert a["opt_state"]["rng_step"] == b["opt_state"]["rng_step"] == 5
    for ra, rb in zip(a["opt_state"]["velocities"], b["opt_state"]["velocities"]):
        assert len(ra) == len(rb)
        for u, v in zip(ra, rb):
            np.testing.assert_array_equal(_bits(u), _bits(v))
    # a second training function on the same net: the first one leaves the pipeline (_fall_back)
    cont = []
    for net, pipe in zip(nets, ("1", "0")):
        monkeypatch.setenv("TN_PIPELINE", "0")
        fn = net.get_trin_model(x, y)
        cont.append([fn(s % 4)[0] for s in range(5, 8)])
    assert fns[0]._seq is not None
    np.testing.assert_array_equal(_bits(cont[0]), _bits(cont[1]))
    for u, v in zip(_weights(nets[0]), _weights(nets[1])):
        np.testing.assert_array_equal(u, v)


def test_pipelined_weight_cost_net_matches_the_oracle(monkeypatch):
    """What shows that the gradient term is right and not merely self-consistent: four pipelined steps against the float64
    oracle (_random_net_case's bounds)."""
    from theanet_amd import NeuralNet
    from theanet_amd.neuralnet import _PipeTrainFn
    monkeypatch.setenv("TN_PIPELINE", "1")
    layers = [("InputLayer", {"img_sz": 12, "num_maps": 1}),
              ("HiddenLayer", {"n_out": 100, "actvn": "relu10", "reg": {"L1": .0005}}),
              ("HiddenLayer", {"n_out": 30, "actvn": "scaled_tanh", "reg": {"L2": .001}}),
              ("SoftmaxLayer", {"n_out": 57})]
    B = 48
    tr = {"SEED": 3, "BATCH_SZ": B, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 1}
    rng = np.random.RandomState(3)
    x = rng.rand(4 * B, 1, 12, 12).astype(np.float32)
    y = rng.randint(0, 57, 4 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    ora = O.OracleNet(copy.deepcopy(layers), dict(tr), dtype=np.float64)
    fn = net.get_trin_model(x, y)
    assert isinstance(fn, _PipeTrainFn)
    for s in range(4):
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], {})
        cost, _, lp = fn(s)
        assert_close(lp, lp_w, 1e-4, 1e-5, what="logprob step %d" % s)
        assert_close(cost, cost_w, 1e-4, 1e-5, what="cost step %d" % s)
    assert fn._seq is None and fn.t == 4
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            assert_close(w, ol.params[j], 1e-4, 1e-6, what="w %d %d" % (i, j))


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_recorded_steps_of_the_weight_cost_mlp_equal_interpreted_ones(monkeypatch, pipe):
    """Forty enqueued steps with the weights read after steps 8 and 30: by step 30 the steps are replayed (plan.py; the
    table of tn_wtcost_net is a baked pointer there), the read puts one step back through the interpreter (the update
    that leaves the velocity alone is not a recorded one), replay resumes -- against TN_NET_PLAN=0 bit for bit."""
    monkeypatch.setenv("TN_PIPELINE", pipe)
    runs = []
    for plan in ("1", "0"):
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net, x, y = _net("mlp")
        fn = net.get_trin_model(x, y)
        mids, ready = [], []
        for s in range(40):
            fn.enqueue(s % 4)
            if s in (8, 30):
                ready.append(fn._plan.ready)
                mids.append(_weights(net))
        ready.append(fn._plan.ready)
        assert ready == ([False, True, True] if plan == "1" else [False] * 3), (ready, fn._plan.why)
        assert getattr(fn, "_seq", None) is None
        runs.append((fn.fetch(), mids, _weights(net)))
    (o0, m0, w0), (o1, m1, w1) = runs
    assert _bits(o0[0]) == _bits(o1[0])
    np.testing.assert_array_equal(o0[2], o1[2])
    for a, b in zip(m0[0] + m0[1] + w0, m1[0] + m1[1] + w1):
        np.testing.assert_array_equal(a, b)


# ---- launch counts ---------------------------------------------------------------------------------------------
def _record(monkeypatch, net, fn, steps):
    """[(entry point, first argument)] of the C-ABI calls of ``steps`` interpreted steps (the one before them is not counted)."""
    c = ctx()
    fn.enqueue(0)
    log, real = [], c.call

    def spy(name, *args):
        log.append((name, args[0] if args else None, args))
        return real(name, *args)

    monkeypatch.setattr(c, "call", spy)
    try:
        for s in range(steps):
            fn.enqueue((s + 1) % 4)
    finally:
        monkeypatch.undo()
    c.sync()
    return log


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_a_fused_step_sums_its_cost_in_one_launch(monkeypatch, pipe):
    monkeypatch.setenv("TN_PIPELINE", pipe)
    net, x, y = _net("mlp")
    fn = net.get_trin_model(x, y)
    log = _record(monkeypatch, net, fn, 1)
    names = [n for n, _, _ in log]
    assert names.count("tn_wtcost_net") == 1
    assert "tn_wtcost" not in names and "tn_reduce_sum" not in names


# the entry points of steps 1 .. 3 of mnist.prms at batch 64 with two steps in flight, recorded on an MI355X from the commit
# before weight costs reached the pipelined schedule (tn_alloc: buffers made on first use)
MNIST_CALLS = [
    "tn_stream_select", "tn_event_wait", "tn_set_f32", "tn_sgd_update_net", "tn_event_record",
    "tn_elastic_field_gen", "tn_alloc", "tn_elastic_convpool_fwd_mask", "tn_alloc", "tn_convpool_fwd_mask",
    "tn_fc_fwd_dropout", "tn_defer_reductions", "tn_alloc", "tn_alloc", "tn_fc_softmax_train",
    "tn_rider_elastic_field", "tn_alloc", "tn_alloc", "tn_fc_bwd", "tn_alloc", "tn_convblock_bwd_mask",
    "tn_convpool_bwd_mask", "tn_stream_select", "tn_stream_select", "tn_event_wait", "tn_set_f32",
    "tn_sgd_update_net", "tn_event_record", "tn_elastic_convpool_fwd_mask", "tn_convpool_fwd_mask",
    "tn_fc_fwd_dropout", "tn_defer_reductions", "tn_fc_softmax_train", "tn_rider_elastic_field", "tn_fc_bwd",
    "tn_convblock_bwd_mask", "tn_convpool_bwd_mask", "tn_stream_select", "tn_stream_select", "tn_event_wait",
    "tn_sgd_update_net", "tn_event_record", "tn_elastic_convpool_fwd_mask", "tn_convpool_fwd_mask",
    "tn_fc_fwd_dropout", "tn_defer_reductions", "tn_fc_softmax_train", "tn_rider_elastic_field", "tn_fc_bwd",
    "tn_convblock_bwd_mask", "tn_convpool_bwd_mask", "tn_stream_select"]


def test_nets_without_weight_costs_issue_the_calls_they_always_did(monkeypatch):
    from theanet_amd import NeuralNet
    logs = []
    for _ in range(2):
        prms = load_prms("mnist.prms", 28, batch=64)
        rng = np.random.RandomState(5)
        x = rng.rand(256, 1, 28, 28).astype(np.float32)
        y = rng.randint(0, 10, 256).astype(np.int32)
        net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
        fn = net.get_trin_model(x, y)
        assert not net._has_wtcost and not net._cost_net and net._cost_rider and len(net._wc_tab) == 0
        log = _record(monkeypatch, net, fn, 3)
        assert fn._seq is None and not fn._reg
        logs.append(log)
    for name, first, args in logs[0]:
        assert name != "tn_wtcost_net"
        if name in ("tn_sgd_update_net", "tn_sgd_update_net_maxnorm"):
            assert first in (_lib.TN_UPD_PLAIN, _lib.TN_UPD_PIPE), first       # never TN_UPD_PIPE_REG
            assert first != _lib.TN_UPD_DELAYED and args[9] in (0, 1)          # flags: bit 0 only
    assert [n for n, _, _ in logs[0]] == [n for n, _, _ in logs[1]]
    if _lib.backend() == "hip":    # (the C++ backend picks other kernels)
        # (allocations on first use are not part of the schedule: whether a buffer exists depends on what ran before)
        assert [n for n, _, _ in logs[0] if n != "tn_alloc"] == [n for n in MNIST_CALLS if n != "tn_alloc"]
    ups = [a for n, _, a in logs[0] if n.startswith("tn_sgd_update_net")]
    assert len(ups) == 3 and all(a[0] == _lib.TN_UPD_PIPE for a in ups)
