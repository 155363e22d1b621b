"""set_order(order) of the training functions (theanet_amd/trainfn.py): a device-resident row order for shuffled epochs.
One tn_gather_batch launch per step stages rows order[i*B:(i+1)*B]; the step is recorded, replayed and pipelined like an
in-order one.  Pinned against the two routes that already exist, bit for bit: the take_index_list function fed the same
slices of the order, and an in-order function on physically permuted data.  mnist.prms geometry with its elastic stage
active (the device RNG is in play: draws are keyed by the position in the minibatch and the step, not by dataset row)."""
import copy
import functools

import numpy as np
import pytest

from tests.gpu_util import load_prms
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

B, NB = 32, 6                   # minibatch, minibatches in the dataset
PERM = np.random.RandomState(11).permutation(B * NB)
PERM2 = np.random.RandomState(12).permutation(B * NB)


@functools.lru_cache(maxsize=None)
def _mnist():
    prms = load_prms("mnist.prms", 28, batch=B)
    rng = np.random.RandomState(5)
    x = rng.rand(B * NB, 1, 28, 28).astype(np.float32)
    y = rng.randint(0, 10, B * NB).astype(np.int32)
    x.setflags(write=False)
    y.setflags(write=False)
    return prms, x, y


def _net(prms, tr=None):
    from theanet_amd import NeuralNet
    return NeuralNet(copy.deepcopy(prms["layers"]), dict(tr or prms["training_params"]))


def _weights(net):
    return [w.copy() for l in net.tr_layers for w in l.get_wts()]


def _same(got, want):
    """(outs, weights) pairs: costs and logprobs of the steps that returned them, and the final weights, bit for bit."""
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])
    for a, b in zip(got[0], want[0]):
        assert np.float32(a[0]).view(np.uint32) == np.float32(b[0]).view(np.uint32), (a[0], b[0])
        np.testing.assert_array_equal(a[2], b[2])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


READ = (0, 3, 30, 39, 45, 51)       # the steps whose outputs are read (fn(i)); all others are enqueue(i)


def _drive(fn, batch_of, lo, hi, outs):
    for s in range(lo, hi):
        if s in READ:
            outs.append(fn(batch_of(s)))
        else:
            fn.enqueue(batch_of(s))


@functools.lru_cache(maxsize=None)
def _index_list_reference(second):
    """40 steps of the take_index_list function fed PERM's slices (then 12 more fed ``second``'s: "perm2", "none" = dataset
    order, or nothing)."""
    prms, x, y = _mnist()
    net = _net(prms)
    fn = net.get_trin_model(x, y, take_index_list=True)
    outs = []
    _drive(fn, lambda s: PERM[(s % NB) * B:(s % NB + 1) * B].astype(np.int32), 0, 40, outs)
    if second:
        order = PERM2 if second == "perm2" else np.arange(B * NB)
        _drive(fn, lambda s: order[(s % NB) * B:(s % NB + 1) * B].astype(np.int32), 40, 52, outs)
    return outs, _weights(net)


def _replays(fn):
    pl = fn._plan
    if type(fn).__name__ == "_PipeTrainFn" and fn._seq is not None:
        pl = fn._seq._plan
    return pl is not None and pl.ready


@pytest.mark.parametrize("plan", ["1", "0"])
@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_ordered_steps_equal_the_index_list_route(pipeline, plan, monkeypatch):
    """Every schedule: two steps in flight or one, replayed (one C call per step) or interpreted."""
    monkeypatch.setenv("TN_PIPELINE", pipeline)
    monkeypatch.setenv("TN_NET_PLAN", plan)
    prms, x, y = _mnist()
    net = _net(prms)
    fn = net.get_trin_model(x, y)
    fn.set_order(PERM)
    outs = []
    _drive(fn, lambda s: s % NB, 0, 40, outs)
    assert _replays(fn) == (plan == "1"), (fn._plan.why, fn._plan.off)
    if pipeline == "1":
        assert type(fn).__name__ == "_PipeTrainFn" and fn._seq is None
    else:
        assert type(fn).__name__ == "_TrainFn"
    _same((outs, _weights(net)), _index_list_reference(""))


def test_ordered_steps_equal_in_order_steps_on_permuted_data():
    prms, x, y = _mnist()
    net = _net(prms)
    fn = net.get_trin_model(x, y)
    fn.set_order(PERM)
    outs = []
    _drive(fn, lambda s: s % NB, 0, 40, outs)
    ref_net = _net(prms)
    ref_fn = ref_net.get_trin_model(x[PERM], y[PERM])
    ref_outs = []
    _drive(ref_fn, lambda s: s % NB, 0, 40, ref_outs)
    _same((outs, _weights(net)), (ref_outs, _weights(ref_net)))


def test_a_new_order_keeps_plan_pipeline_and_buffer(monkeypatch):
    monkeypatch.setenv("TN_PIPELINE", "1")
    monkeypatch.setenv("TN_NET_PLAN", "1")
    prms, x, y = _mnist()
    net = _net(prms)
    fn = net.get_trin_model(x, y)
    fn.set_order(PERM)
    outs = []
    _drive(fn, lambda s: s % NB, 0, 40, outs)
    assert fn._plan.ready, fn._plan.why
    handles = [h[0].value for h in fn._plan.plans]
    ptr, seen = fn._ord.buf.ptr, fn._plan.n
    fn.set_order(PERM2)
    assert fn._plan.ready and [h[0].value for h in fn._plan.plans] == handles and fn._plan.n == seen
    assert fn._ord.buf.ptr == ptr
    assert type(fn).__name__ == "_PipeTrainFn" and fn._seq is None
    _drive(fn, lambda s: s % NB, 40, 52, outs)
    assert fn._plan.ready and [h[0].value for h in fn._plan.plans] == handles and fn._seq is None
    _same((outs, _weights(net)), _index_list_reference("perm2"))


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_step_cost_rides_the_ring_with_an_order(pipeline, monkeypatch):
    """step_cost() with an order: every cost once, in order, equal to fn(i)[0]'s -- through the ring (not the synchronous
    branch), also across a new order in the middle of the loop (what the ring still owes is handed out afterwards)."""
    monkeypatch.setenv("TN_PIPELINE", pipeline)
    prms, x, y = _mnist()
    ref_net = _net(prms)
    ref_fn = ref_net.get_trin_model(x, y)
    ref_fn.set_order(PERM)
    net = _net(prms)
    fn = net.get_trin_model(x, y)
    fn.set_order(PERM)
    want, got = [], []
    for s in range(36):
        if s == 21:
            ref_fn.set_order(PERM2)
            fn.set_order(PERM2)
            assert fn._led.live
        want.append((s, np.float32(ref_fn(s % NB)[0])))
        got += fn.step_cost(s % NB)
        assert fn._led.live
    got += fn.drain_costs()
    assert [k for k, _ in got] == list(range(36))
    np.testing.assert_array_equal(np.array([c for _, c in got], np.float32), np.array([c for _, c in want], np.float32))
    assert _replays(fn)
    for a, b in zip(_weights(net), _weights(ref_net)):
        np.testing.assert_array_equal(a, b)


def test_set_order_none_returns_to_dataset_order():
    prms, x, y = _mnist()
    net = _net(prms)
    fn = net.get_trin_model(x, y)
    fn.set_order(PERM)
    outs = []
    _drive(fn, lambda s: s % NB, 0, 40, outs)
    fn.set_order(None)
    _drive(fn, lambda s: s % NB, 40, 52, outs)
    _same((outs, _weights(net)), _index_list_reference("none"))


# ---- the 16-bit conv stack reads the input slot lazily: tn_c8_pack from the first conv layer (InputLayer first) or
# ---- tn_c8_elastic_apply (an active ElasticLayer first) -- both must see the stage
FIRST16 = {"input": ("InputLayer", {"img_sz": 16, "num_maps": 3}),
           "elastic": ("ElasticLayer", {"img_sz": 16, "num_maps": 3, "translation": 2, "zoom": 1.1, "magnitude": 30, "sigma": 4,
                                        "pflip": 0.1, "angle": 5, "nearest": False})}


@pytest.mark.parametrize("first", ["input", "elastic"])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_16bit_stack_reads_the_stage(dtype, first):
    conv = lambda k: ("ConvLayer", {"num_maps": k, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"})
    layers = [FIRST16[first], conv(16), ("PoolLayer", {"pool_sz": 2}), conv(32), ("PoolLayer", {"pool_sz": 2}),
              ("HiddenLayer", {"n_out": 64}), ("SoftmaxLayer", {"n_out": 10})]
    tr = {"SEED": 7, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2, "DTYPE": dtype,
          "GRAD_SCALE": 1024.0}
    prms = {"layers": layers, "training_params": tr}
    rng = np.random.RandomState(3)
    x = rng.rand(16 * 4, 3, 16, 16).astype(np.float32)
    y = rng.randint(0, 10, 16 * 4).astype(np.int32)
    perm = rng.permutation(16 * 4)
    net = _net(prms)
    assert all(l.f16 for l in net.tr_layers if type(l).__name__ == "ConvLayer")
    if first == "elastic":
        assert net.tr_layers[0].active and net.tr_layers[0]._c8_consumer is not None
    else:
        assert net.tr_layers[0]._packed_by_conv
    fn = net.get_trin_model(x, y)
    fn.set_order(perm)
    ref_net = _net(prms)
    ref_fn = ref_net.get_trin_model(x, y, take_index_list=True)
    outs, ref_outs = [], []
    for s in range(10):
        outs.append(fn(s % 4))
        ref_outs.append(ref_fn(perm[(s % 4) * 16:(s % 4 + 1) * 16].astype(np.int32)))
    _same((outs, _weights(net)), (ref_outs, _weights(ref_net)))


def test_aux_net_equals_in_order_steps_on_permuted_data():
    """The AuxConcatLayer net of tests/test_gpu_net.py::test_aux_input_layers_match_oracle (its layers are local to that
    test: repeated here), device draws: the aux rows travel in the same gather launch and the mixing draws are keyed by
    i*B + position, so the ordered run IS the in-order run on x[perm], y[perm], aux[perm]."""
    layers = [("InputLayer", {"img_sz": 8, "num_maps": 1}),
              ("ConvLayer", {"num_maps": 3, "filter_sz": 3, "stride": 1, "actvn": "relu10"}),
              ("HiddenLayer", {"n_out": 16, "actvn": "tanh", "pdrop": .5}),
              ("AuxConcatLayer", {"n_aux": (5, 4), "aux_type": "LocationInfo", "boost": 2}),
              ("SoftmaxLayer", {"n_out": 6})]
    tr = {"SEED": 31, "BATCH_SZ": 8, "INIT_LEARNING_RATE": .2, "EPOCHS_TO_HALF_RATE": 1}
    prms = {"layers": layers, "training_params": tr}
    rng = np.random.RandomState(12)
    x = rng.rand(3 * 8, 1, 8, 8).astype(np.float32)
    y = rng.randint(0, 6, 3 * 8).astype(np.int32)
    aux = rng.rand(3 * 8, 2, 2).astype(np.float32)
    perm = rng.permutation(3 * 8)
    net = _net(prms)
    assert net.takes_aux()
    fn = net.get_trin_model(x, y, aux)
    fn.set_order(perm)
    ref_net = _net(prms)
    ref_fn = ref_net.get_trin_model(x[perm], y[perm], aux[perm])
    outs, ref_outs = [], []
    for s in range(9):
        outs.append(fn(s % 3))
        ref_outs.append(ref_fn(s % 3))
    _same((outs, _weights(net)), (ref_outs, _weights(ref_net)))


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_set_order_errors(pipeline, monkeypatch):
    monkeypatch.setenv("TN_PIPELINE", pipeline)
    prms, x, y = _mnist()
    net = _net(prms)
    rows = B * NB
    fn = net.get_trin_model(x, y)
    with pytest.raises(IndexError):
        fn.set_order(np.r_[PERM[:-1], rows])                    # an entry past the dataset
    with pytest.raises(IndexError):
        fn.set_order(np.r_[PERM[:-1], -1])
    with pytest.raises(ValueError):
        fn.set_order(PERM.astype(np.float32))                   # dtype
    with pytest.raises(ValueError):
        fn.set_order(PERM.reshape(NB, B))                       # ndim
    with pytest.raises(ValueError):
        fn.set_order(PERM[:B - 1])                              # shorter than a minibatch
    with pytest.raises(ValueError):
        fn.set_order(np.r_[PERM, 0])                            # longer than the dataset
    assert fn._ord.len is None                                  # (none of them took effect)
    fn.set_order(np.zeros(2 * B + 5, np.int64))                 # not a permutation, not a whole number of minibatches
    assert np.isfinite(fn(1)[0])
    with pytest.raises(IndexError):
        fn(2)                                                   # (2 + 1) * B > len(order)
    with pytest.raises(IndexError):
        fn.step_cost(-1)
    fn.set_order(None)
    assert np.isfinite(fn(NB - 1)[0])
    with pytest.raises(IndexError):
        fn(NB)
    fn2 = _net(prms).get_trin_model(x, y, take_index_list=True)
    with pytest.raises(ValueError):
        fn2.set_order(PERM)
