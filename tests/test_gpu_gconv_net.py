"""Grouped ConvLayers through NeuralNet, float32 and bfloat16, by the method of tests/test_gpu_dwconv_net.py: a small net
built twice from the same weights -- once with ConvLayer(groups=2) layers, once with dense ConvLayers whose (K, C, f, f)
weights hold the groups' filters on the block diagonal and zeros elsewhere.  The twins compute the same function in the
first step and the update is elementwise, so after the first velocity has landed (two steps: the reference's update moves
a parameter by the velocity of the step before) the block diagonal of a dense W holds what the grouped W must be.  The
grouped net is a default, FUSING NeuralNet: the pool above its grouped layer stands alone because the family says so.

Agreement (that test's): float32 to assert_close's defaults, a parameter to 1e-4 of the largest step the dense twin took
on it; bfloat16 to one ulp of bf16 (2^-7) of the largest logprob / of the largest step -- the twins differ only in the
fp32 summation order before one rounding to the stored type.

Without the feature the grouped net does not build: ConvLayer takes no ``groups`` keyword."""
import copy

import numpy as np
import pytest

from tests.gpu_util import assert_close
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_dwconv_net import B, TP, _conv

pytestmark = pytest.mark.gpu


def _layers(grouped):
    kw = {"groups": 2} if grouped else {}
    return [("InputLayer", {"img_sz": 12, "num_maps": 3}), _conv(16, 3, "same"), _conv(16, 3, "same", **kw),
            ("PoolLayer", {"pool_sz": 2}), _conv(32, 1, "valid"), _conv(32, 5, "valid", **kw),
            ("HiddenLayer", {"n_out": 24, "pdrop": 0, "reg": {"maxnorm": 0}}), ("SoftmaxLayer", {"n_out": 10, "reg": {"maxnorm": 0}})]


GR = (2, 5)         # the grouped layers


def _dense(w, g=2):
    """(K, C/g, f, f) -> (K, C, f, f), the groups' filters on the block diagonal."""
    K, Cg = w.shape[:2]
    out = np.zeros((K, Cg * g) + w.shape[2:], np.float32)
    for grp in range(g):
        ks = slice(grp * K // g, (grp + 1) * K // g)
        out[ks, grp * Cg:(grp + 1) * Cg] = w[ks]
    return out


def _blocks(v, g=2):
    """The block diagonal of a dense (K, C, f, f): (K, C/g, f, f)."""
    K, C = v.shape[:2]
    return np.concatenate([v[grp * K // g:(grp + 1) * K // g, grp * C // g:(grp + 1) * C // g] for grp in range(g)])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_grouped_net_matches_its_dense_twin(dtype, monkeypatch):
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")          # one step at a time: a step's update has landed when it returns
    tp = dict(TP, DTYPE=dtype)
    rng = np.random.RandomState(3)
    x, y = rng.rand(4 * B, 3, 12, 12).astype(np.float32), rng.randint(0, 10, 4 * B).astype(np.int32)
    gr = NeuralNet(_layers(True), dict(tp))
    wts = [[w.copy() for w in l.get_wts()] for l in gr.tr_layers]
    assert [wts[i][0].shape for i in GR] == [(16, 8, 3, 3), (32, 16, 5, 5)]
    assert all(" Groups:2" in gr.tr_layers[i].representation and gr.te_layers[i].groups == 2 for i in GR)
    twin_wts = [[_dense(w[0]), w[1]] if i in GR else w for i, w in enumerate(copy.deepcopy(wts))]
    assert NeuralNet.fuse_conv_pool and all(gr.tr_layers[i].fused_pool is None for i in GR)
    assert gr.tr_layers[3].fused_conv is None and gr.te_layers[3].fused_conv is None      # the pool stands alone
    # the dense twin must not fuse its 3x3 layer with the pool either (tests/test_gpu_dwconv_net.py says why)
    monkeypatch.setattr(NeuralNet, "fuse_conv_pool", False)
    dense = NeuralNet(_layers(False), dict(tp, **({"CONV_SHAPES": "any"} if dtype == "bfloat16" else {})), allwts=twin_wts)
    if dtype == "bfloat16":
        assert gr.tr_layers[3].c8_alone and gr.tr_layers[2].c8_fam.fwd == "tn_c8_gconv_fwd"
    fn, fd = gr.get_trin_model(x, y), dense.get_trin_model(x, y)
    (cost, _, lp), (cost_d, _, lp_d) = fn(0), fd(0)
    ulp = 2.0 ** -7
    rt, at = (0., ulp * np.abs(lp_d).max()) if dtype == "bfloat16" else (1e-4, 1e-5)
    print("%s: cost %.6f twin %.6f, max |dlogprob| %.3g" % (dtype, cost, cost_d, np.abs(lp - lp_d).max()))
    assert_close(lp, lp_d, rt, at, what="logprob")
    assert_close(cost, cost_d, rt, at, what="cost")
    fn(1), fd(1)                                              # the first step's velocity lands
    for i, (a, d) in enumerate(zip(gr.tr_layers, dense.tr_layers)):
        for j, (w, v) in enumerate(zip(a.get_wts(), d.get_wts())):
            step = np.abs(v - twin_wts[i][j]).max()
            if i in GR and j == 0:
                v = _blocks(v)
                assert not np.array_equal(w, wts[i][0]), "the grouped filters did not move"
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - v).max(), np.abs(v).max()))
            assert_close(w, v, 2.0 ** -22, (ulp if dtype == "bfloat16" else 1e-4) * step, what="w %d %d" % (i, j))
    for s in range(2, 4):                                     # three steps after the first: the recorded step is entered
        assert np.isfinite(fn(s)[0])


@pytest.mark.parametrize("kw, says", [({"groups": 3}, "groups must divide"),
                                      ({"groups": 2, "depthwise": True, "num_maps": 8}, "not both"),
                                      ({"groups": 2, "dtype": "bfloat16"}, "multiples of 8")], ids=["divides", "depthwise", "cells"])
def test_grouped_constructor_refuses(kw, says):
    """g dividing neither map count; groups with depthwise; on bfloat16 C/g = 4."""
    from theanet_amd.layer import ConvLayer
    args = dict({"num_maps": 16, "filter_sz": 3, "stride": 1}, **kw)
    with pytest.raises(AssertionError, match=says):
        ConvLayer(None, None, np.random.RandomState(0), B, 8, 12, mode="valid", **args)
