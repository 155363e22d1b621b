"""Depthwise ConvLayers through NeuralNet, float32 and bfloat16: a small net built twice from the same weights -- once
with ConvLayer(depthwise=True) layers, once with dense ConvLayers whose (C, C, f, f) weights hold the depthwise filters
on the diagonal and zeros elsewhere, the only way to say the layer without the feature.  The twins compute the same
function in the first step, and the update is elementwise, so the diagonal of a dense W then holds what the depthwise
W must be.  (The reference's update moves a parameter by the velocity of the step BEFORE, layer.py:82-86: the first
step's gradient reaches the weights in the second step, whose forward still runs on the initial weights -- so the
weights are compared after two steps and hold the first step's gradients alone.  From then on the zeros off the
diagonal are trained away and the twins part.)  That holds the whole plumbing: the stand-alone pool above a depthwise
layer in a net that fuses (the depthwise net is built with the default, fusing NeuralNet), below_info, pitches, the flat
gradient buffer and the update.

Agreement: float32 to float32 rounding (assert_close's defaults; a parameter to 1e-4 of the largest step the dense twin
took on it plus fp32 rounding of the parameter itself, which asks more than the defaults on the whole weight).
bfloat16: the twins differ only in the fp32 summation order before one rounding to the stored type, so a stored value
differs by at most one ulp of bf16, 2^-7 relative:
logprob and cost agree to 2^-7 of the largest logprob, and a parameter -- old value minus rate times a gradient that is
linear in those stored values -- to 2^-7 of the largest step the dense twin took on that parameter (plus fp32 rounding
of the parameter itself).

Without the feature the depthwise net does not build: ConvLayer takes no ``depthwise`` keyword."""
import copy

import numpy as np
import pytest

from tests.gpu_util import assert_close
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

B = 8
TP = {"SEED": 5, "BATCH_SZ": B, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


def _conv(k, f, mode, **kw):
    return ("ConvLayer", dict({"num_maps": k, "filter_sz": f, "stride": 1, "mode": mode, "actvn": "relu10",
                               "reg": {"maxnorm": 0}}, **kw))


def _layers(depthwise):
    kw = {"depthwise": True} if depthwise else {}
    return [("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(8, 3, "same"), _conv(8, 3, "same", **kw),
            ("PoolLayer", {"pool_sz": 2}), _conv(16, 1, "valid"), _conv(16, 5, "valid", **kw),
            ("HiddenLayer", {"n_out": 24, "pdrop": 0, "reg": {"maxnorm": 0}}), ("SoftmaxLayer", {"n_out": 10, "reg": {"maxnorm": 0}})]


DW = (2, 5)         # the depthwise layers


def _dense(w):
    """(C, 1, f, f) -> (C, C, f, f), the filters on the diagonal."""
    out = np.zeros((w.shape[0],) + w.shape, np.float32)[:, :, 0]
    out[np.arange(w.shape[0]), np.arange(w.shape[0])] = w[:, 0]
    return out


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_depthwise_net_matches_its_dense_twin(dtype, monkeypatch):
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")          # one step at a time: a step's update has landed when it returns
    tp = dict(TP, DTYPE=dtype)
    rng = np.random.RandomState(3)
    x, y = rng.rand(4 * B, 3, 12, 12).astype(np.float32), rng.randint(0, 10, 4 * B).astype(np.int32)
    dw = NeuralNet(_layers(True), dict(tp))
    wts = [[w.copy() for w in l.get_wts()] for l in dw.tr_layers]
    assert [wts[i][0].shape for i in DW] == [(8, 1, 3, 3), (16, 1, 5, 5)]
    assert all(" Depthwise" in dw.tr_layers[i].representation and dw.te_layers[i].depthwise for i in DW)
    twin_wts = [[_dense(w[0]), w[1]] if i in DW else w for i, w in enumerate(copy.deepcopy(wts))]
    # The depthwise net above is a default, FUSING net: its pool stands alone and its depthwise layers stay unfused because
    # the family says so (c8.pool_stands_alone, ConvLayer.can_fuse_with).  The dense twin must not fuse its 3x3 layer with
    # the pool either -- on the 16-bit stack the fused block breaks pooling ties by the unrounded activation, a stand-alone
    # PoolLayer by the stored values -- and is told so: the switch is read at construction only.
    assert NeuralNet.fuse_conv_pool and all(dw.tr_layers[i].fused_pool is None for i in DW)
    assert dw.tr_layers[3].fused_conv is None and dw.te_layers[3].fused_conv is None
    monkeypatch.setattr(NeuralNet, "fuse_conv_pool", False)
    # (the dense 5x5 'valid' twin needs the general family; the depthwise layers are accepted under either CONV_SHAPES)
    dense = NeuralNet(_layers(False), dict(tp, **({"CONV_SHAPES": "any"} if dtype == "bfloat16" else {})), allwts=twin_wts)
    if dtype == "bfloat16":
        assert dw.tr_layers[3].c8_alone and dw.tr_layers[2].c8_fam.fwd == "tn_c8_dwconv_fwd"
    assert dw.tr_layers[2].fused_pool is None
    fn, fd = dw.get_trin_model(x, y), dense.get_trin_model(x, y)
    (cost, _, lp), (cost_d, _, lp_d) = fn(0), fd(0)
    ulp = 2.0 ** -7
    rt, at = (0., ulp * np.abs(lp_d).max()) if dtype == "bfloat16" else (1e-4, 1e-5)
    print("%s: cost %.6f twin %.6f, max |dlogprob| %.3g" % (dtype, cost, cost_d, np.abs(lp - lp_d).max()))
    assert_close(lp, lp_d, rt, at, what="logprob")
    assert_close(cost, cost_d, rt, at, what="cost")
    fn(1), fd(1)                                              # the first step's velocity lands
    for i, (a, d) in enumerate(zip(dw.tr_layers, dense.tr_layers)):
        for j, (w, v) in enumerate(zip(a.get_wts(), d.get_wts())):
            step = np.abs(v - twin_wts[i][j]).max()
            if i in DW and j == 0:
                v = v[np.arange(len(v)), np.arange(len(v))][:, None]
                assert not np.array_equal(w, wts[i][0]), "the depthwise filters did not move"
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - v).max(), np.abs(v).max()))
            # the STEP agrees: to 1e-4 of the largest one (float32: assert_close's rtol) / one ulp of bf16
            assert_close(w, v, 2.0 ** -22, (ulp if dtype == "bfloat16" else 1e-4) * step, what="w %d %d" % (i, j))
    for s in range(2, 4):                                     # three steps after the first: the recorded step is entered
        assert np.isfinite(fn(s)[0])


@pytest.mark.parametrize("kw", [{"num_maps": 16}, {"filter_sz": 4}, {"stride": 3}], ids=lambda k: next(iter(k)))
def test_depthwise_constructor_refuses(kw):
    from theanet_amd.layer import ConvLayer
    args = dict({"num_maps": 8, "filter_sz": 3, "stride": 1}, **kw)
    with pytest.raises(AssertionError):
        ConvLayer(None, None, np.random.RandomState(0), B, 8, 12, mode="valid", depthwise=True, **args)
