"""WT_AVG: an exponential moving average of the weights (Polyak averaging) for evaluation and checkpoints -- the op
(tn_avg_net), the rule step by step, every train schedule against one step at a time bit for bit, evaluation at the averaged
weights, and the switch being off.

The rule (include/theanet_hip.h): c = fl(1 - d) rounded once on the host; a_t = fma(c, fl(p_t - a_{t-1}), a_{t-1}).  Its
reference here: the difference in float32 (one rounding, reproduced bit for bit), then a + c * diff in float64, where the
product of two float32 values is exact; the sum is within 2^-53 of the true value, so a correctly rounded result meets
tests/upd_ref.check_rounded's half-ulp bound, which is derived there and not measured."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_util import ROOT, call, ctx, dev
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.upd_ref import check_rounded
from theanet_amd import _lib

pytestmark = pytest.mark.gpu

AVG_DT = np.dtype([('p', 'u8'), ('a', 'u8'), ('n', 'u8'), ('reserved', 'u8')])
BIG = (1 << 20) + 3
SIZES = (1, 7, 256, 257, 4099, BIG)
# every size as a table of its own, three segments, thirty-three (the sizes in turn; the large one once)
TABLES = {"n%d" % n: (n,) for n in SIZES}
TABLES["3seg"] = (BIG, 7, 257)
TABLES["33seg"] = tuple(SIZES[i % 6] if i == 5 or i % 6 != 5 else 4099 for i in range(33))
DECAYS = (.5, .99, .9999)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _c(d):
    return np.float32(1.0 - d)


def _want(p, a, c):
    """a + c * fl(p - a) in float64."""
    diff = np.asarray(p, np.float32) - np.asarray(a, np.float32)        # float32 - float32: one rounding
    return np.asarray(a, np.float32).astype(np.float64) + np.float64(np.float32(c)) * diff.astype(np.float64)


def _carve(sizes, seed, bits=False):
    """Two buffers (weights, averages) and the segments carved from them at odd float offsets: segment i of the averages
    sits i % 4 floats further on than its weights, so both the 16-byte walk (equal offsets from a 16-byte boundary, with
    a head) and the one-by-one walk are taken.  The floats between segments are sentinels nobody may touch."""
    rng = np.random.RandomState(seed)
    offs, o = [], 1
    for n in sizes:
        offs.append(o)
        o += n + 5
        o += 1 - (o & 1)                      # odd
    total = o + 8
    if bits:                                  # any bit pattern: NaNs with payloads, subnormals, infinities
        hp = rng.randint(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32).view(np.float32)
        ha = rng.randint(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32).view(np.float32)
    else:
        hp = (rng.randn(total) * 10.0 ** rng.randint(-3, 3, total)).astype(np.float32)
        ha = (hp + rng.randn(total) * .1 * np.abs(hp)).astype(np.float32)
        ha[::7] = rng.randn(len(ha[::7])).astype(np.float32)           # ... and averages far from their weights
    dp, da = dev(hp), dev(ha)
    segs = [(off, off + (i % 4), n) for i, (off, n) in enumerate(zip(offs, sizes))]
    assert segs[-1][1] + segs[-1][2] <= total
    rows = [(dp.ptr + 4 * po, da.ptr + 4 * ao, n, 0) for po, ao, n in segs]
    tab = dev(np.array(rows, dtype=AVG_DT).view(np.uint8))
    return hp, ha, dp, da, segs, tab


# ---- the op ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DECAYS)
@pytest.mark.parametrize("table", sorted(TABLES))
def test_avg_net_update_is_the_rounded_rule(table, d):
    assert AVG_DT.itemsize == 32
    sizes, c = TABLES[table], _c(d)
    hp, ha, dp, da, segs, tab = _carve(sizes, len(sizes) + int(d * 1e4))
    call("tn_avg_net", tab.ptr, len(sizes), max(sizes), float(c), _lib.TN_AVG_UPDATE)
    got_a, got_p = da.get_value(), dp.get_value()
    np.testing.assert_array_equal(_bits(got_p), _bits(hp))              # p comes back bit for bit
    want = ha.astype(np.float64)
    for po, ao, n in segs:
        want[ao:ao + n] = _want(hp[po:po + n], ha[ao:ao + n], c)
    check_rounded(got_a, want, what="%s d=%g" % (table, d))
    touched = np.zeros(len(ha), bool)
    for _, ao, n in segs:
        touched[ao:ao + n] = True
    np.testing.assert_array_equal(_bits(got_a)[~touched], _bits(ha)[~touched])      # nothing between the segments
    assert not np.array_equal(got_a[touched], ha[touched])
    # equal inputs, a second launch: equal bits
    da2 = dev(ha)
    rows = np.array([(dp.ptr + 4 * po, da2.ptr + 4 * ao, n, 0) for po, ao, n in segs], dtype=AVG_DT)
    call("tn_avg_net", dev(rows.view(np.uint8)).ptr, len(sizes), max(sizes), float(c), _lib.TN_AVG_UPDATE)
    np.testing.assert_array_equal(_bits(da2.get_value()), _bits(got_a))


@pytest.mark.parametrize("table", sorted(TABLES))
def test_avg_net_exchange_is_exact_and_twice_is_the_identity(table):
    sizes = TABLES[table]
    hp, ha, dp, da, segs, tab = _carve(sizes, 77 + len(sizes), bits=True)
    wp, wa = _bits(hp).copy(), _bits(ha).copy()
    for po, ao, n in segs:
        wp[po:po + n], wa[ao:ao + n] = _bits(ha)[ao:ao + n], _bits(hp)[po:po + n]
    call("tn_avg_net", tab.ptr, len(sizes), max(sizes), .25, _lib.TN_AVG_EXCHANGE)
    np.testing.assert_array_equal(_bits(dp.get_value()), wp)
    np.testing.assert_array_equal(_bits(da.get_value()), wa)
    call("tn_avg_net", tab.ptr, len(sizes), max(sizes), .25, _lib.TN_AVG_EXCHANGE)
    np.testing.assert_array_equal(_bits(dp.get_value()), _bits(hp))
    np.testing.assert_array_equal(_bits(da.get_value()), _bits(ha))


def test_avg_net_refuses_bad_input_and_launches_nothing():
    hp, ha, dp, da, segs, tab = _carve((257, 7), 5)
    bad = [(None, 2, 257, .5, 0),                   # no table
           (tab.ptr, 2, 0, .5, 0),                  # empty segments
           (tab.ptr, -1, 257, .5, 0),
           (tab.ptr, 2, 257, -.001, 0), (tab.ptr, 2, 257, 1.001, 0), (tab.ptr, 2, 257, float("nan"), 0),
           (tab.ptr, 2, 257, .5, 2), (tab.ptr, 2, 257, .5, -1)]      # unknown modes
    for args in bad:
        with pytest.raises(_lib.BackendError, match=r"rc=-2"):        # TN_E_ARG
            call("tn_avg_net", *args)
    call("tn_avg_net", None, 0, 0, .5, 0)           # no segments: nothing to do
    call("tn_avg_net", tab.ptr, 2, 257, 0.0, 0)     # c == 0 and c == 1 are inside the range
    np.testing.assert_array_equal(_bits(da.get_value()), _bits(ha))
    np.testing.assert_array_equal(_bits(dp.get_value()), _bits(hp))
    call("tn_avg_net", tab.ptr, 2, 257, 1.0, 0)
    got = da.get_value()
    for po, ao, n in segs:
        check_rounded(got[ao:ao + n], _want(hp[po:po + n], ha[ao:ao + n], 1.0), what="c = 1")


# ---- nets -----------------------------------------------------------------------------------------------------------
D = .9


def _layers(kind):
    """(layers, batch, image side, maps).  'small': the step-by-step net; 'l2': the same with an L2 weight cost (the
    pipelined update is TN_UPD_PIPE_REG); a DTYPE name: the 16-bit conv stack."""
    if kind in ("small", "l2"):
        reg = {"maxnorm": 1.5, "L2": .001} if kind == "l2" else {"maxnorm": 1.5}
        return [("InputLayer", {"img_sz": 12, "num_maps": 1}),
                ("ConvLayer", {"num_maps": 4, "filter_sz": 3, "stride": 1, "actvn": "relu10"}),
                ("PoolLayer", {"pool_sz": 2}),
                ("HiddenLayer", {"n_out": 24, "pdrop": .5, "actvn": "relu05", "reg": reg}),
                ("HiddenLayer", {"n_out": 16, "actvn": "scaled_tanh", "reg": {"rate": 0}}),
                ("SoftmaxLayer", {"n_out": 10})], 16, 12, 1
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}),
            ("ConvLayer", {"num_maps": 16, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
            ("PoolLayer", {"pool_sz": 2}),
            ("HiddenLayer", {"n_out": 32, "actvn": "relu10"}),
            ("SoftmaxLayer", {"n_out": 10})], 16, 16, 3


FROZEN = 4          # the rate: 0 layer of 'small' / 'l2'


@functools.lru_cache(maxsize=None)
def _data(kind):
    layers, B, img, C = _layers(kind)
    rng = np.random.RandomState(11)
    x = rng.rand(4 * B, C, img, img).astype(np.float32)
    y = rng.randint(0, 10, 4 * B).astype(np.int32)
    x.setflags(write=False)
    y.setflags(write=False)
    tr = {"SEED": 23, "BATCH_SZ": B, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 1}
    if kind in ("float16", "bfloat16"):
        tr["DTYPE"] = kind
    return layers, tr, x, y


def _net(kind, d=D, allwts=None):
    from theanet_amd import NeuralNet
    layers, tr, x, y = _data(kind)
    tr = dict(tr)
    if d is not None:
        tr["WT_AVG"] = d
    return NeuralNet(copy.deepcopy(layers), tr, allwts=allwts), x, y


def _flat(nested):
    return [np.array(w, copy=True) for l in nested for w in l]


def _weights(net):
    return _flat(l.get_wts() for l in net.tr_layers)


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(_bits(u), _bits(v))


def test_wt_avg_param_is_checked_at_construction():
    for bad in (1, 1.5, -.1, "0.9", True):
        with pytest.raises(AssertionError, match="WT_AVG"):
            _net("small", bad)
    for off in (None, 0, 0.0):
        net, x, y = _net("small", off)
        assert net.get_avg_wts() is None and net._avg is None and net._avg_tab is None
        assert "avg_wts" not in net.get_init_params()
        with pytest.raises(AssertionError, match="WT_AVG"):
            net.get_test_model(x, y, averaged=True)
        with pytest.raises(AssertionError, match="WT_AVG"):
            net.get_data_test_model(averaged=True)
        assert net.get_test_model(x, y).averaged is False


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_average_follows_the_rule_step_by_step(monkeypatch, pipe):
    """Seven steps, one at a time: after each, the average against the rule applied to the average read before it and the
    weights read now (max-norm and dropout on; the rate: 0 layer has no average)."""
    monkeypatch.setenv("TN_PIPELINE", pipe)
    net, x, y = _net("small")
    c = _c(D)
    assert net._avg[FROZEN] is None and [a is None for a in net._avg] == [True, False, True, False, True, False]
    prev = _flat(net.get_avg_wts())
    _same(prev, _weights(net))                      # a_0 = the weights the net starts from
    fn = net.get_trin_model(x, y)
    moved = False
    for s in range(7):
        fn(s % 4)
        p = _weights(net)
        nested = net.get_avg_wts()
        np.testing.assert_array_equal(nested[FROZEN][0], net.tr_layers[FROZEN].get_wts()[0])      # evaluated as it is
        avg = _flat(nested)
        k = 0
        for i, lyr in enumerate(net.tr_layers):
            for j in range(len(lyr.params)):
                if net._avg[i] is None:
                    np.testing.assert_array_equal(_bits(avg[k]), _bits(p[k]))
                else:
                    check_rounded(avg[k], _want(p[k], prev[k], c), what="step %d layer %d tensor %d" % (s, i, j))
                    moved = moved or not np.array_equal(avg[k], prev[k])
                k += 1
        prev = avg
    assert moved
    _same(_flat(net.get_avg_wts()), prev)           # reading twice adds nothing to the average


SCHEDULES = {
    # name: (environment, fused_step, how the steps are driven)
    "pipelined": ({"TN_PIPELINE": "1"}, True, "enqueue"),
    "one-at-a-time": ({"TN_PIPELINE": "0"}, True, "enqueue"),
    "generic": ({"TN_PIPELINE": "1"}, False, "enqueue"),
    "step_cost": ({"TN_PIPELINE": "1"}, True, "step_cost"),
    "step_cost-one-at-a-time": ({"TN_PIPELINE": "0"}, True, "step_cost"),
    "set_order": ({"TN_PIPELINE": "1"}, True, "set_order"),
    "dp-overlap0": ({"TN_PIPELINE": "0", "TN_DP_FORCE": "1", "TN_DP_OVERLAP": "0"}, True, "enqueue"),
    "dp-overlap0-pipelined": ({"TN_PIPELINE": "1", "TN_DP_FORCE": "1", "TN_DP_OVERLAP": "0"}, True, "enqueue"),
    "dp-overlap2": ({"TN_PIPELINE": "0", "TN_DP_FORCE": "1", "TN_DP_OVERLAP": "2"}, True, "enqueue"),
}
STEPS, READ_AT, RATE_AT = 40, (7, 31), 9


def _forty_steps(kind, sched, monkeypatch):
    """40 steps with the averages read after steps 7 and 31 (with two steps in flight that forces the catch-up) and a new
    learning rate from step 9 on: (averages read mid-run, final averages, final weights, the plan was replaying)."""
    from theanet_amd import NeuralNet
    env, fused, drive = SCHEDULES[sched]
    for k in ("TN_DP_FORCE", "TN_DP_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(NeuralNet, "fused_step", fused)
    net, x, y = _net(kind)
    try:
        fn = net.get_trin_model(x, y)
        if drive == "set_order":
            fn.set_order(np.arange(x.shape[0]))     # the dataset's own order, staged through the row order's gathers
        mids, costs = [], []
        for s in range(STEPS):
            if s == RATE_AT:
                net.inc_epoch_set_rate()
            if drive == "step_cost":
                costs += fn.step_cost(s % 4)
            else:
                fn.enqueue(s % 4)
            if s in READ_AT:
                mids.append(_flat(net.get_avg_wts()))
        if drive == "step_cost":
            costs += fn.drain_costs()
            assert [k for k, _ in costs] == list(range(STEPS))
        ready = fn._plan.ready
        return mids, _flat(net.get_avg_wts()), _weights(net), ready
    finally:
        if net._dev_group is not None:
            net.ctx.call("tn_comm_destroy")
            net._dev_group = None


@functools.lru_cache(maxsize=None)
def _reference(kind):
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("TN_NET_PLAN", "0")               # every step through the interpreter, one at a time
        return _forty_steps(kind, "one-at-a-time", mp)
    finally:
        mp.undo()


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("kind", ["small", "l2", "bfloat16"])
def test_schedules_keep_the_same_average_bit_for_bit(monkeypatch, kind, sched):
    want = _reference(kind)
    got = _forty_steps(kind, sched, monkeypatch)
    for a, b in zip(got[0], want[0]):
        _same(a, b)
    _same(got[1], want[1])
    _same(got[2], want[2])
    assert any(not np.array_equal(a, w) for a, w in zip(got[1], got[2]))       # (an average, not a copy of the weights)
    if sched in ("pipelined", "one-at-a-time"):
        assert got[3] and not want[3]               # the last steps were replayed ones (plan.py); the reference's never


# ---- evaluation -----------------------------------------------------------------------------------------------------
EVAL_KINDS = ["small", "float16", "bfloat16"]


def _train(net, x, y, steps, first=0):
    fn = net._test_train_fn = getattr(net, "_test_train_fn", None) or net.get_trin_model(x, y)
    for s in range(first, first + steps):
        fn.enqueue(s % 4)
    return fn


@pytest.mark.parametrize("kind", EVAL_KINDS)
def test_averaged_evaluation_is_a_fresh_net_at_the_averages(kind):
    net, x, y = _net(kind)
    _train(net, x, y, 7)                            # (an odd count: the twin of the pipelined schedule holds the weights)
    te = net.get_test_model(x, y)
    assert te.averaged is True
    got = [te(i) for i in range(4)]
    swept = te.sweep([3, 0, 0, 2])
    avg = net.get_avg_wts()
    fresh, _, _ = _net(kind, None, allwts=avg)
    tf = fresh.get_test_model(x, y)
    assert tf.averaged is False
    want = [tf(i) for i in range(4)]
    assert [[float(e), float(p)] for e, p in got] == [[float(e), float(p)] for e, p in want]
    assert swept == tf.sweep([3, 0, 0, 2]) == [[float(v) for v in want[i]] for i in (3, 0, 0, 2)]
    # preds_feats and the data test model go the same way
    f1 = net.get_test_model(x, y, preds_feats=True)(1)
    f2 = fresh.get_test_model(x, y, preds_feats=True)(1)
    np.testing.assert_array_equal(_bits(f1[2]), _bits(f2[2]))
    np.testing.assert_array_equal(f1[3], f2[3])
    B = net.batch_sz
    d1 = net.get_data_test_model()(x[:B])
    d2 = fresh.get_data_test_model()(x[:B])
    np.testing.assert_array_equal(_bits(d1[0]), _bits(d2[0]))
    np.testing.assert_array_equal(d1[1], d2[1])
    # ... and the average is not the last iterate (the evaluation above could tell them apart)
    raw = net.get_data_test_model(averaged=False)(x[:B])
    assert not np.array_equal(raw[0], d1[0])


@pytest.mark.parametrize("kind", EVAL_KINDS)
def test_unaveraged_evaluation_is_the_run_without_averaging(kind):
    net, x, y = _net(kind)
    off, _, _ = _net(kind, None)
    _train(net, x, y, 7)
    _train(off, x, y, 7)
    _same(_weights(net), _weights(off))             # averaging does not touch the weights
    a = net.get_test_model(x, y, averaged=False)
    b = off.get_test_model(x, y)
    assert a.averaged is False
    assert [a(i) for i in range(4)] == [b(i) for i in range(4)]
    assert a.sweep(range(4)) == b.sweep(range(4))


@pytest.mark.parametrize("first", [6, 7])
@pytest.mark.parametrize("kind", EVAL_KINDS)
def test_weights_and_further_steps_survive_an_averaged_evaluation(kind, first):
    """... also one that raises half-way; five further steps equal an uninterrupted run's.  ``first``: the steps before
    the evaluation -- with two steps in flight an even count leaves the weights with the net and the next update to the
    other stream, an odd count with the twin."""
    net, x, y = _net(kind)
    ref, _, _ = _net(kind)
    fn = _train(net, x, y, first)
    fr = _train(ref, x, y, first)
    before, avg_before = _weights(net), _flat(net.get_avg_wts())
    te = net.get_test_model(x, y)
    te(2)
    te.sweep([0, 1, 2, 3])
    _same(_weights(net), before)
    _same(_flat(net.get_avg_wts()), avg_before)

    class Boom(Exception):
        pass

    real, seen = te._enqueue, []

    def failing(i, d_stats):
        if seen:
            raise Boom()
        seen.append(i)
        return real(i, d_stats)

    te._enqueue = failing
    with pytest.raises(Boom):
        te.sweep([1, 2, 3])
    te._enqueue = real
    assert seen == [1]
    _same(_weights(net), before)
    _same(_flat(net.get_avg_wts()), avg_before)
    assert te(2) == te(2)
    # (a 16-bit stack whose operand tiles were still the averages' would train on from them here)
    for s in range(first, first + 4):               # (enqueued: nothing holds the streams back between the steps)
        fn.enqueue(s % 4)
        fr.enqueue(s % 4)
    a, b = fn((first + 4) % 4), fr((first + 4) % 4)
    assert _bits(a[0]) == _bits(b[0])
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]))
    _same(_weights(net), _weights(ref))
    _same(_flat(net.get_avg_wts()), _flat(ref.get_avg_wts()))


# ---- off is off; round trips ------------------------------------------------------------------------------------------
def _calltrace(prms_path, tmp_path):
    env = dict(os.environ, PRMS=str(prms_path), B="64", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "calltrace.py")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = [l.strip() for l in r.stdout.splitlines() if l.startswith("   ")]
    assert len(names) > 5, r.stdout
    return names


def test_a_step_without_wt_avg_issues_the_calls_it_always_did(tmp_path):
    """tools/calltrace.py's step trace of mnist.prms: with WT_AVG: 0 the trace of the file without the param, no tn_avg_net
    in either; params/mnist_avg.prms adds exactly that call."""
    src = open(os.path.join(ROOT, "params", "mnist.prms")).read()
    assert "WT_AVG" not in src
    zero = tmp_path / "mnist_zero.prms"
    zero.write_text(src.replace("'BATCH_SZ': 20,", "'BATCH_SZ': 20, 'WT_AVG': 0,"))
    assert "'WT_AVG': 0" in zero.read_text()
    plain = _calltrace(os.path.join(ROOT, "params", "mnist.prms"), tmp_path)
    assert "tn_avg_net" not in plain
    assert _calltrace(zero, tmp_path) == plain
    on = _calltrace(os.path.join(ROOT, "params", "mnist_avg.prms"), tmp_path)
    assert on.count("tn_avg_net") == 1
    assert [n for n in on if n != "tn_avg_net"] == plain
    assert on[on.index("tn_avg_net") - 1].startswith("tn_sgd_update_net")        # right behind the update


@pytest.mark.parametrize("pipe", ["1", "0"])
def test_checkpoint_round_trip(monkeypatch, pipe):
    """get_init_params -> a new net from "allwts", load_avg_wts("avg_wts"), load_opt_state: training carries on bit for bit,
    averages included; "allwts" stays the raw weights."""
    monkeypatch.setenv("TN_PIPELINE", pipe)
    net, x, y = _net("small")
    fn = _train(net, x, y, 7)
    ck = net.get_init_params(with_opt_state=True)
    _same(_flat(ck["allwts"]), _weights(net))
    _same(_flat(ck["avg_wts"]), _flat(net.get_avg_wts()))
    assert ck["training_params"]["WT_AVG"] == D
    from theanet_amd import NeuralNet
    res = NeuralNet(copy.deepcopy(ck["layers"]), dict(ck["training_params"]), allwts=ck["allwts"])
    _same(_flat(res.get_avg_wts()), _weights(net))          # a_0 of a net built from weights: those weights
    res.load_avg_wts(ck["avg_wts"])
    res.load_opt_state(ck["opt_state"])
    _same(_flat(res.get_avg_wts()), _flat(ck["avg_wts"]))
    fr = res.get_trin_model(x, y)
    for s in range(7, 12):
        a, b = fn(s % 4), fr(s % 4)
        assert _bits(a[0]) == _bits(b[0])
    _same(_weights(res), _weights(net))
    _same(_flat(res.get_avg_wts()), _flat(net.get_avg_wts()))
    with pytest.raises(AssertionError, match="load_avg_wts"):
        res.load_avg_wts(ck["avg_wts"][:-1])
