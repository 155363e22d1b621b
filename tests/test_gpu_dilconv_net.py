"""Dilated ConvLayers through NeuralNet, float32 and bfloat16, by the method of tests/test_gpu_gconv_net.py: a small net
built twice from the same weights -- once with ConvLayer(dilation=2) layers, once with dense ConvLayers of filter 5 whose
weights hold the 3x3 filters zero-stuffed.  The twins compute the same function in the first step and the update is
elementwise, so after the first velocity has landed (two steps: the reference's update moves a parameter by the velocity
of the step before) the taps [::2, ::2] of a dense W hold what the dilated W must be: the first step's gradient of every
dilated layer.  The dilated net is a default, FUSING NeuralNet: the pool above its dilated layer stands alone because the
family says so.

Agreement (that test's): float32 to assert_close's defaults, a parameter to 1e-4 of the largest step the dense twin took
on it; bfloat16 to one ulp of bf16 (2^-7) of the largest logprob / of the largest step -- the twins differ only in the
fp32 summation order before one rounding to the stored type.

Without the feature the dilated net does not build: ConvLayer takes no ``dilation`` keyword."""
import copy

import numpy as np
import pytest

from tests.gpu_util import assert_close
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_dwconv_net import TP, _conv

pytestmark = pytest.mark.gpu

B = 16
DIL = (2, 4)        # the dilated layers


def _layers(dilated):
    mid = (lambda mode: _conv(16, 3, mode, dilation=2)) if dilated else (lambda mode: _conv(16, 5, mode))
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, 3, "same"), mid("same"), ("PoolLayer", {"pool_sz": 2}),
            mid("valid"), ("MeanLayer", {}), ("SoftmaxLayer", {"n_out": 10, "reg": {"maxnorm": 0}})]


def _stuffed(w):
    """(K, C, 3, 3) -> (K, C, 5, 5), the taps two apart."""
    out = np.zeros(w.shape[:2] + (5, 5), np.float32)
    out[:, :, ::2, ::2] = w
    return out


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_dilated_net_matches_its_dense_twin(dtype, monkeypatch):
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")          # one step at a time: a step's update has landed when it returns
    tp = dict(TP, DTYPE=dtype, BATCH_SZ=B)
    rng = np.random.RandomState(3)
    x, y = rng.rand(4 * B, 3, 16, 16).astype(np.float32), rng.randint(0, 10, 4 * B).astype(np.int32)
    dl = NeuralNet(_layers(True), dict(tp))
    wts = [[w.copy() for w in l.get_wts()] for l in dl.tr_layers]
    assert [wts[i][0].shape for i in DIL] == [(16, 16, 3, 3)] * 2 and [dl.tr_layers[i].out_sz for i in DIL] == [16, 4]
    assert all(" Dilation:2" in dl.tr_layers[i].representation and dl.te_layers[i].dilation == 2 for i in DIL)
    twin_wts = [[_stuffed(w[0]), w[1]] if i in DIL else w for i, w in enumerate(copy.deepcopy(wts))]
    assert NeuralNet.fuse_conv_pool and all(dl.tr_layers[i].fused_pool is None for i in DIL)
    assert dl.tr_layers[3].fused_conv is None and dl.te_layers[3].fused_conv is None      # the pool stands alone
    # the dense twin must not fuse its 5x5 layer with the pool either (tests/test_gpu_dwconv_net.py says why)
    monkeypatch.setattr(NeuralNet, "fuse_conv_pool", False)
    dense = NeuralNet(_layers(False), dict(tp, **({"CONV_SHAPES": "any"} if dtype == "bfloat16" else {})), allwts=twin_wts)
    if dtype == "bfloat16":
        assert dl.tr_layers[3].c8_alone and dl.tr_layers[2].c8_fam.fwd == "tn_c8_dilconv_fwd"
    ulp = 2.0 ** -7
    te, te_d = dl.get_test_model(x, y, preds_feats=True)(0)[2], dense.get_test_model(x, y, preds_feats=True)(0)[2]
    rt, at = (0., ulp * np.abs(te_d).max()) if dtype == "bfloat16" else (1e-4, 1e-5)
    assert_close(te, te_d, rt, at, what="test logprob")
    fn, fd = dl.get_trin_model(x, y), dense.get_trin_model(x, y)
    (cost, _, lp), (cost_d, _, lp_d) = fn(0), fd(0)
    rt, at = (0., ulp * np.abs(lp_d).max()) if dtype == "bfloat16" else (1e-4, 1e-5)
    print("%s: cost %.6f twin %.6f, max |dlogprob| %.3g" % (dtype, cost, cost_d, np.abs(lp - lp_d).max()))
    assert_close(lp, lp_d, rt, at, what="logprob")
    assert_close(cost, cost_d, rt, at, what="cost")
    fn(1), fd(1)                                              # the first step's velocity lands
    for i, (a, d) in enumerate(zip(dl.tr_layers, dense.tr_layers)):
        for j, (w, v) in enumerate(zip(a.get_wts(), d.get_wts())):
            step = np.abs(v - twin_wts[i][j]).max()
            if i in DIL and j == 0:
                v = v[:, :, ::2, ::2]
                assert not np.array_equal(w, wts[i][0]), "the dilated filters did not move"
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - v).max(), np.abs(v).max()))
            assert_close(w, v, 2.0 ** -22, (ulp if dtype == "bfloat16" else 1e-4) * step, what="w %d %d" % (i, j))
    for s in range(2, 4):                                     # three steps after the first: the recorded step is entered
        assert np.isfinite(fn(s)[0])
