"""ConvLayers with narrow groups (4 and 2 maps a group) through NeuralNet on bfloat16, by the twin method of
tests/test_gpu_gconv_net.py: the grouped net against a dense net whose weights hold the groups' filters on the block
diagonal.  Agreement is that test's: one bf16 ulp (2^-7) of the largest logprob / of the largest step.

Without the feature the grouped net does not build: choose_conv refuses groups that are no whole cells."""
import copy

import numpy as np
import pytest

from tests.gpu_util import assert_close
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_dwconv_net import B, TP, _conv
from tests.test_gpu_gconv_net import _blocks, _dense

pytestmark = pytest.mark.gpu

GR = {2: 4, 4: 8}         # the grouped layers and their groups


def _layers(grouped):
    kw = (lambda g: {"groups": g}) if grouped else (lambda g: {})
    return [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, 3, "same"), _conv(16, 3, "same", **kw(4)),
            ("PoolLayer", {"pool_sz": 2}), _conv(16, 3, "valid", **kw(8)),
            ("HiddenLayer", {"n_out": 24, "pdrop": 0, "reg": {"maxnorm": 0}}), ("SoftmaxLayer", {"n_out": 10, "reg": {"maxnorm": 0}})]


def test_narrow_grouped_net_matches_its_dense_twin(monkeypatch):
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")          # one step at a time: a step's update has landed when it returns
    tp = dict(TP, DTYPE="bfloat16")
    rng = np.random.RandomState(3)
    x, y = rng.rand(4 * B, 3, 16, 16).astype(np.float32), rng.randint(0, 10, 4 * B).astype(np.int32)
    gr = NeuralNet(_layers(True), dict(tp))
    wts = [[w.copy() for w in l.get_wts()] for l in gr.tr_layers]
    assert [wts[i][0].shape for i in GR] == [(16, 4, 3, 3), (16, 2, 3, 3)]
    assert all(gr.tr_layers[i].c8_fam.fwd == "tn_c8_gconv_fwd" for i in GR)
    twin_wts = [[_dense(w[0], GR[i]), w[1]] if i in GR else w for i, w in enumerate(copy.deepcopy(wts))]
    # the dense twin must not fuse its 3x3 layer with the pool (tests/test_gpu_dwconv_net.py says why)
    monkeypatch.setattr(NeuralNet, "fuse_conv_pool", False)
    dense = NeuralNet(_layers(False), dict(tp, CONV_SHAPES="any"), allwts=twin_wts)
    fn, fd = gr.get_trin_model(x, y), dense.get_trin_model(x, y)
    (cost, _, lp), (cost_d, _, lp_d) = fn(0), fd(0)
    ulp = 2.0 ** -7
    print("cost %.6f twin %.6f, max |dlogprob| %.3g" % (cost, cost_d, np.abs(lp - lp_d).max()))
    assert_close(lp, lp_d, 0., ulp * np.abs(lp_d).max(), what="logprob")
    assert_close(cost, cost_d, 0., ulp * np.abs(lp_d).max(), what="cost")
    fn(1), fd(1)                                              # the first step's velocity lands
    for i, (a, d) in enumerate(zip(gr.tr_layers, dense.tr_layers)):
        for j, (w, v) in enumerate(zip(a.get_wts(), d.get_wts())):
            step = np.abs(v - twin_wts[i][j]).max()
            if i in GR and j == 0:
                v = _blocks(v, GR[i])
                assert not np.array_equal(w, wts[i][0]), "the grouped filters did not move"
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - v).max(), np.abs(v).max()))
            assert_close(w, v, 2.0 ** -22, ulp * step, what="w %d %d" % (i, j))
    for s in range(2, 4):                                     # three steps after the first: the recorded step is entered
        assert np.isfinite(fn(s)[0])
