"""``sweep(indices)`` of the test functions (theanet_amd/trainfn.py): a run of minibatches evaluated with one weight sync
and one copy back, minibatch k's statistics in row k of a device array (tn_error_stats at ``rows + 2 k``).  Pinned against
the per-call path ``fn(i)``, bit for bit, behind training steps of each net's default schedule (two steps in flight where
that is the default: the sweep must bring the weights up to date like a call does)."""
import copy

import numpy as np
import pytest

from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

NB = 6                          # minibatches in every corpus
IDX = [0, 1, 2, 1, 0]


def _conv_net(img, maps, k, **tr):
    layers = [("InputLayer", {"img_sz": img, "num_maps": maps}),
              ("ConvLayer", {"num_maps": k, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
              ("PoolLayer", {"pool_sz": 2}),
              ("HiddenLayer", {"n_out": 32, "actvn": "tanh"}),
              ("SoftmaxLayer", {"n_out": 10})]
    return layers, dict({"SEED": 7, "BATCH_SZ": 8, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}, **tr), 10, None


def _head_net(head, aux=False):
    """The nets of tests/test_gpu_net.py's head and aux tests (their layers are local to those tests: repeated here)."""
    layers = [("InputLayer", {"img_sz": 8, "num_maps": 1}),
              ("ConvLayer", {"num_maps": 3, "filter_sz": 3, "stride": 1, "actvn": "relu10"}),
              ("HiddenLayer", {"n_out": 16, "actvn": "tanh"})]
    if aux:
        layers.append(("AuxConcatLayer", {"n_aux": (5, 4), "aux_type": "LocationInfo", "boost": 2}))
    layers.append(head)
    return layers, {"SEED": 31, "BATCH_SZ": 8, "INIT_LEARNING_RATE": .2, "EPOCHS_TO_HALF_RATE": 1}, 6, (2, 2) if aux else None


NETS = {
    "fp32": lambda: _conv_net(12, 1, 6),
    "bfloat16": lambda: _conv_net(16, 3, 16, DTYPE="bfloat16", GRAD_SCALE=1024.0),
    "float16": lambda: _conv_net(16, 3, 16, DTYPE="float16", GRAD_SCALE=1024.0),
    "auxconcat": lambda: _head_net(("SoftmaxLayer", {"n_out": 6}), aux=True),
    "hinge": lambda: _head_net(("HingeLayer", {"n_out": 6, "reg": {"maxnorm": 2}})),
}


def _build(name):
    """(net, training function, test function) on a corpus of NB minibatches."""
    from theanet_amd import NeuralNet
    layers, tr, n_cls, aux_shape = NETS[name]()
    first, B = layers[0][1], tr["BATCH_SZ"]
    rng = np.random.RandomState(5)
    x = rng.rand(NB * B, first["num_maps"], first["img_sz"], first["img_sz"]).astype(np.float32)
    y = rng.randint(0, n_cls, NB * B).astype(np.int32)
    aux = rng.rand(NB * B, *aux_shape).astype(np.float32) if aux_shape else None
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    return net, net.get_trin_model(x, y, aux), net.get_test_model(x, y, aux)


def _bits(pairs):
    return np.array(pairs, np.float32).view(np.uint32).tolist()


def _check(te, idx):
    """sweep(idx) against the calls, made afterwards and before: neither path may depend on what the other left."""
    got = te.sweep(idx)
    want = [te(i) for i in idx]
    assert all(type(v) is float for pair in got for v in pair), got
    assert got == want and _bits(got) == _bits(want), (got, want)
    assert te.sweep(idx) == want
    return got


@pytest.mark.parametrize("name", list(NETS))
def test_sweep_equals_calls(name):
    net, fn, te = _build(name)
    if name in ("bfloat16", "float16"):
        assert all(l.f16 for l in net.tr_layers if type(l).__name__ == "ConvLayer")
    for s in range(3):
        fn(s)
    first = _check(te, IDX)
    assert first[0] == first[4] and first[1] == first[3]
    assert len({p for _, p in first[:3]}) == 3, first       # (rows that cannot be told apart would pin nothing)
    for s in range(3, 5):
        fn(s)
    second = _check(te, IDX)
    assert second != first                                   # two more steps: stale weights or operand tiles would show


def test_sweep_takes_any_iterable():
    _, fn, te = _build("fp32")
    fn(0)
    want = [te(i) for i in IDX]
    assert te.sweep(iter(IDX)) == want
    assert te.sweep(np.array(IDX)) == want
    assert te.sweep(i % 3 for i in (0, 1, 2, 4, 3)) == want


def test_sweep_out_of_range_raises_like_a_call_and_leaves_nothing_behind():
    _, fn, te = _build("fp32")
    fn(0)
    with pytest.raises(IndexError) as call_err:
        te(99)
    with pytest.raises(IndexError) as sweep_err:
        te.sweep([0, 99])
    assert str(sweep_err.value) == str(call_err.value)
    with pytest.raises(IndexError):
        te.sweep([1, -1])
    assert te._sweep_stats is None                           # (refused before anything was allocated or enqueued)
    assert te.sweep([0]) == [te(0)]


def test_empty_sweep():
    _, _, te = _build("fp32")
    assert te.sweep([]) == []
    assert te.sweep(iter(())) == []
    assert te._sweep_stats is None


def test_preds_feats_function_refuses_sweep():
    from theanet_amd import NeuralNet
    layers, tr, _, _ = NETS["fp32"]()
    rng = np.random.RandomState(5)
    x = rng.rand(NB * 8, 1, 12, 12).astype(np.float32)
    y = rng.randint(0, 10, NB * 8).astype(np.int32)
    te = NeuralNet(copy.deepcopy(layers), dict(tr)).get_test_model(x, y, preds_feats=True)
    with pytest.raises(AssertionError, match="preds_feats"):
        te.sweep([0])
    assert len(te(0)) == 4


def test_sweep_buffer_grows():
    _, fn, te = _build("fp32")
    fn(0)
    calls = [te(i) for i in range(NB)]
    short, longer = [3, 4, 5], [5, 0, 4, 1, 3, 2, 5]
    assert te.sweep(short) == [calls[i] for i in short]
    assert te._sweep_stats.shape == (3, 2)
    assert te.sweep(longer) == [calls[i] for i in longer]
    assert te._sweep_stats.shape == (7, 2)
    buf = te._sweep_stats
    assert te.sweep(short) == [calls[i] for i in short]      # a shorter one uses the rows it needs of the same array
    assert te._sweep_stats is buf
