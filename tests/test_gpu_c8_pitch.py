"""The 16-bit conv stack on maps whose side is not a power of two: c8 tensors of S x S maps stored at a pitch P > S
(theanet_amd/csrc/conv_c8.hip, "padded pitch"; device.C8Array).  Op by op through the C-ABI in both 16-bit dtypes --
conv forward (+ 2x2 max-pool and mask), input gradient (plain and gathered from a pooled gradient + mask) and weight
gradient on padded tensors, pack_pitch / crop / embed -- and whole nets against the stored-16-bit oracle.

Specification: tests/c8_util.py / tests/c8b_util.py applied to the LOGICAL (S x S) tensors; every pad cell of every
tensor an op writes is exactly zero (raw bits).  Tolerances those of tests/test_gpu_c8.py (fp16) and
tests/test_gpu_c8_bf16.py (bf16); nets those of tests/test_gpu_c8_mean.py; schedules bit for bit."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8_util as U
from tests import c8b_util as CB
from tests.gpu_util import assert_close, call, ctx, dev, load_prms
from tests.test_gpu_c8 import (ACTS, C8_CASES, LEAKY, SLOPE, WGRAD_RING_CASES, _act, _act_grad_from_out,
                               _assert_masks_equal_up_to_provable_near_ties, _rel, _wgrad_blas)
from tests.test_gpu_f16 import _inject_draws
from theanet_amd.device import DeviceArray
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

GS = {"float16": 1024.0, "bfloat16": 1024.0}
TOL16 = {"float16": 1e-3, "bfloat16": 1e-2}
GARBAGE = 0x5555


def _pitch(S):
    P = 8
    while P < S:
        P *= 2
    return P


# the cases of tests/test_gpu_c8.py with each power-of-two side H replaced by a smaller even side of the same pitch
# (S in {28, 24, 20} for 32, {14, 12, 10} for 16, 6 for 8, 48 for 64), and odd sides (7, 5) without pooling
_SIDES = {8: [6], 16: [14, 12, 10], 32: [28, 24, 20], 64: [48]}


def _padded(cases):
    out, k = [], 0
    for N, C, H, K in cases:
        if H in _SIDES:
            sides = _SIDES[H]
            out.append((N, C, sides[k % len(sides)], K))
            k += 1
    return out


PITCH_CASES = _padded(C8_CASES) + [(5, 24, 7, 40), (3, 1, 5, 16), (4, 3, 7, 32), (9, 8, 5, 8)]
PITCH_RING_CASES = _padded(WGRAD_RING_CASES)
GENERIC = ["tanh", "sigmoid"]


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request):
    ctx().set_matmul_dtype(request.param, GS[request.param])
    yield request.param
    ctx().set_matmul_dtype("float32")


def _R(dtype):
    return CB.rbf16 if dtype == "bfloat16" else U.r16


def _raw(a, dtype, P):
    """logical (N, C, S, S) -> raw bits of the c8 tensor at pitch P, pad zero."""
    N, C, S, _ = a.shape
    full = np.zeros((N, C, P, P), np.float64)
    full[:, :, :S, :S] = a
    return CB.to_c8(full) if dtype == "bfloat16" else U.to_c8(full).view(np.uint16)


def _garbage(N, C, P):
    return dev(np.full((N, (C + 7) // 8, P, P, 8), GARBAGE, np.uint16))


def _logical(arr, C, S, dtype, what):
    """raw c8 tensor at pitch P -> logical (N, C, S, S) float64, after asserting every pad cell is exactly zero."""
    raw = DeviceArray.get_value(arr)                  # (a C8Array's own get_value is the logical array)
    assert not raw[:, :, S:].any() and not raw[:, :, :, S:].any(), what + ": nonzero pad cells"
    raw = np.ascontiguousarray(raw[:, :, :S, :S])
    v = CB.from_c8(raw, C) if dtype == "bfloat16" else U.from_c8(raw.view(np.float16), C)
    return v.astype(np.float64)


def _conv_ops(case, name, dtype, wgrad):
    """Forward, forward + pool + mask, input gradient, pooled input gradient (S even) and -- wgrad -- the weight gradient
    (plain and gathered) of one padded shape, activation `name` in the epilogues."""
    N, C, S, K = case
    P, R, gs, tol = _pitch(S), _R(dtype), GS[dtype], TOL16[dtype]
    act, prm = ACTS[name]
    pool = S % 2 == 0
    rng = np.random.RandomState(S)
    x = R(rng.randn(N, C, S, S))
    W = (rng.randn(K, C, 3, 3) / np.sqrt(9 * C)).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    W16 = R(W)
    a = _act(name, U.conv_same(x, W16) + b[None, :, None, None])
    xd, Wd, bd = dev(_raw(x, dtype, P)), dev(W), dev(b)
    out = _garbage(N, K, P)
    call("tn_c8_conv_fwd", xd.ptr, Wd.ptr, bd.ptr, out.ptr, None, N, C, P, P, K, act, prm, 0, None)
    call("tn_c8_pad_zero", out.ptr, N, K, S, P)
    assert _rel(_logical(out, K, S, dtype, "forward"), R(a)) < tol
    if pool:
        Sp, Pp = S // 2, P // 2
        pm, bits = U.pool2(a)
        outp = _garbage(N, K, Pp)
        mk = dev(np.zeros((N, K // 8, Pp, Pp, 8), np.uint8))
        call("tn_c8_conv_fwd", xd.ptr, Wd.ptr, bd.ptr, outp.ptr, mk.ptr, N, C, P, P, K, act, prm, 1, None)
        call("tn_c8_pad_zero", outp.ptr, N, K, Sp, Pp)
        assert _rel(_logical(outp, K, Sp, dtype, "forward + pool"), R(pm)) < tol
        gotm = mk.get_value()[:, :, :Sp, :Sp].transpose(0, 1, 4, 2, 3).reshape(N, K, Sp, Sp)
        _assert_masks_equal_up_to_provable_near_ties(gotm, bits, a, x, W16, b, C, 0. if name == "leaky" else 2.0 ** -21)
    dz = R(gs * rng.randn(N, K, S, S) * 1e-3)
    if name == "leaky":
        prev = R(rng.randn(N, C, S, S))
        prev[0, 0, 0, :2] = 0
    else:
        prev = R(_act(name, 2 * rng.randn(N, C, S, S)))
    dzd, pd = dev(_raw(dz, dtype, P)), dev(_raw(prev, dtype, P))
    dxo = _garbage(N, C, P)
    call("tn_c8_conv_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, N, C, P, P, K, pd.ptr, act, prm, 0, None, None)
    call("tn_c8_pad_zero", dxo.ptr, N, C, S, P)
    dxw = U.conv_same_dgrad(dz, W16) * _act_grad_from_out(name, prev)
    assert _rel(_logical(dxo, C, S, dtype, "input gradient"), R(dxw)) < tol
    if pool:
        g = R(gs * rng.randn(N, K, Sp, Sp) * 1e-3)
        gd = dev(_raw(g, dtype, Pp))
        dzp = U.unpool_dz(g, gotm)
        dxo = _garbage(N, C, P)
        call("tn_c8_conv_dgrad", gd.ptr, Wd.ptr, dxo.ptr, N, C, P, P, K, pd.ptr, act, prm, 1, mk.ptr, None)
        call("tn_c8_pad_zero", dxo.ptr, N, C, S, P)
        dxw2 = U.conv_same_dgrad(dzp, W16) * _act_grad_from_out(name, prev)
        assert _rel(_logical(dxo, C, S, dtype, "pooled input gradient"), R(dxw2)) < tol
    if not wgrad:
        return
    gW, gb = dev(np.zeros((K, C, 3, 3), np.float32)), dev(np.zeros(K, np.float32))
    for pooled in ((0, 1) if pool else (0,)):
        src, dzz = (gd, dzp) if pooled else (dzd, dz)
        call("tn_c8_conv_wgrad", xd.ptr, src.ptr, gW.ptr, gb.ptr, N, C, P, P, K, pooled, mk.ptr if pooled else None)
        assert _rel(gW.get_value(), _wgrad_blas(x, dzz) / gs) < 2e-5
        assert _rel(gb.get_value(), dzz.sum(axis=(0, 2, 3)) / gs) < 2e-5


@pytest.mark.parametrize("case", PITCH_CASES)
def test_c8_pitch_conv_ops(case, dtype):
    """The five conv products of a layer on padded maps with the leaky-ReLU epilogue, against the logical statement."""
    N, C, S, K = case
    P = _pitch(S)
    assert S < P and ctx().lib.tn_c8_conv_supported(N, C, P, P, K, 3, 1, 1)
    _conv_ops(case, "leaky", dtype, True)


@pytest.mark.parametrize("name", GENERIC)
@pytest.mark.parametrize("case", PITCH_CASES)
def test_c8_pitch_conv_ops_generic_activation(case, name, dtype):
    _conv_ops(case, name, dtype, False)


@pytest.mark.parametrize("case", PITCH_RING_CASES)
def test_c8_pitch_wgrad_many_tiles(case, dtype):
    """The weight-gradient cases of tests/test_gpu_c8.py (rolling ring, slabs, tails) on padded inputs: plain and
    gathered from a pooled gradient with a random mask."""
    N, C, S, K = case
    P, Sp, Pp, R, gs = _pitch(S), S // 2, _pitch(S) // 2, _R(dtype), GS[dtype]
    rng = np.random.RandomState(11)
    x = R(rng.randn(N, C, S, S))
    dz = R(gs * rng.randn(N, K, S, S) * 1e-3)
    g = R(gs * rng.randn(N, K, Sp, Sp) * 1e-3)
    m = np.zeros((N, K, Pp, Pp), np.uint8)
    m[:, :, :Sp, :Sp] = 1 << rng.randint(0, 4, (N, K, Sp, Sp))
    mk = dev(np.ascontiguousarray(m.reshape(N, K // 8, 8, Pp, Pp).transpose(0, 1, 3, 4, 2)))
    xd, dzd, gd = dev(_raw(x, dtype, P)), dev(_raw(dz, dtype, P)), dev(_raw(g, dtype, Pp))
    gW, gb = dev(np.zeros((K, C, 3, 3), np.float32)), dev(np.zeros(K, np.float32))
    for pooled, src, dzz in ((0, dzd, dz), (1, gd, U.unpool_dz(g, m[:, :, :Sp, :Sp]))):
        call("tn_c8_conv_wgrad", xd.ptr, src.ptr, gW.ptr, gb.ptr, N, C, P, P, K, pooled, mk.ptr if pooled else None)
        assert _rel(gW.get_value(), _wgrad_blas(x, dzz) / gs) < 2e-5
        assert _rel(gb.get_value(), dzz.sum(axis=(0, 2, 3)) / gs) < 2e-5


def c8_pitch_launches():
    """Every padded conv call the tests above make, as (op, N, C, S, P, K, pool, act, prm): tests/test_c8_pitch_cpu.py
    checks that they reach every padded instantiation and every edge of each."""
    out = []
    for N, C, S, K in PITCH_CASES:
        P, pools = _pitch(S), ((0, 1) if S % 2 == 0 else (0,))
        for name in ["leaky"] + GENERIC:
            act, prm = ACTS[name]
            out += [(op, N, C, S, P, K, pool, act, prm) for op in (0, 1) for pool in pools]
        out += [(2, N, C, S, P, K, pool, 0, 0.) for pool in pools]
    for N, C, S, K in PITCH_RING_CASES:
        out += [(2, N, C, S, _pitch(S), K, pool, 0, 0.) for pool in (0, 1)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# pack / crop / embed
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,S", [(3, 1, 28), (5, 3, 24), (2, 12, 7), (4, 20, 48), (7, 8, 5), (3, 64, 3)])
def test_c8_pack_crop_embed(N, C, S, dtype):
    P = _pitch(S) if S > 4 else 4
    R = _R(dtype)
    rng = np.random.RandomState(N * S)
    data = rng.randn(N + 3, C, S, S).astype(np.float32)
    if S >= 5:     # (the pack feeds a conv layer: pitch >= 8)
        out = _garbage(N, C, P)
        call("tn_c8_pack_pitch", dev(data).ptr, 2, out.ptr, N, C, S, P, 0.5)
        np.testing.assert_array_equal(out.get_value(), _raw(R(0.5 * data[2:2 + N].astype(np.float64)), dtype, P))
    raw = _raw(R(rng.randn(N, C, S, S)), dtype, P)
    dense = dev(np.full((N, (C + 7) // 8, S, S, 8), GARBAGE, np.uint16))
    call("tn_c8_crop", dev(raw).ptr, dense.ptr, N, C, S, P)
    np.testing.assert_array_equal(dense.get_value(), raw[:, :, :S, :S])
    back = _garbage(N, C, P)
    call("tn_c8_embed", dense.ptr, back.ptr, N, C, S, P)
    np.testing.assert_array_equal(back.get_value(), raw)
    call("tn_c8_pad_zero", back.ptr, N, C, S, P)          # (a no-op on a zero pad)
    np.testing.assert_array_equal(back.get_value(), raw)
    junk = dev(np.full(raw.shape, GARBAGE, np.uint16))
    call("tn_c8_pad_zero", junk.ptr, N, C, S, P)
    j = junk.get_value()
    assert not j[:, :, S:].any() and not j[:, :, :, S:].any()
    assert (j[:, :, :S, :S] == GARBAGE).all()


def test_c8_array_pitch_roundtrip(dtype):
    from theanet_amd.device import C8Array
    rng = np.random.RandomState(3)
    a = C8Array(ctx(), 3, 12, 14, 14, pitch=16)
    assert a.shape == (3, 2, 16, 16, 8) and a.padded
    assert not a.get_value().any() and a.get_value().shape == (3, 12, 14, 14)       # allocated zeroed
    v = _R(dtype)(rng.randn(3, 12, 14, 14)).astype(np.float32)
    DeviceArray.set_value(a, np.full(a.shape, GARBAGE, np.uint16))
    a.set_value(v)
    np.testing.assert_array_equal(a.get_value(), v)
    raw = DeviceArray.get_value(a)
    assert not raw[:, :, 14:].any() and not raw[:, :, :, 14:].any() and not raw[:, 1, ..., 4:].any()


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
NET_GS = {"float16": 4096.0, "bfloat16": 1.0}
NET_TOL = {"float16": ((2e-3, 2e-4), 2e-6), "bfloat16": ((1.6e-2, 1.6e-3), 1.6e-5)}
R16 = O.r16


@pytest.fixture(params=["float16", "bfloat16"])
def net_dtype(request, monkeypatch):
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    yield request.param
    monkeypatch.setattr(O, "r16", R16)


def _mean_bwd_16(monkeypatch, ora):
    """The device's Mean backward in the oracle (tests/test_gpu_c8_mean.py)."""
    from tests.test_gpu_c8_mean import _mean_bwd_16 as patch
    if any(l.kind == "Mean" for l in ora.L):
        patch(monkeypatch, ora)


NETS = [("mnist_c16.prms", 28, 1, 16, 1), ("cifar_like.prms", 24, 3, 16, 1), ("cifar_gap.prms", 24, 3, 16, 1),
        ("wide6.prms", 48, 3, 4, 1)]
# Conv biases get 5x the weights' absolute tolerance: a bias moves by the sum of its map's gradient over every pixel,
# which cancels to ~1e-5, and one stored 16-bit gradient that rounds the other way (or one pooling near-tie that routes
# a pixel's gradient to its neighbour) moves that sum by a few 1e-6.  The MNIST-shaped net shows such a bias 3e-6 off
# at 32 x 32, unpadded, as well; a pad that leaked into the sums would move every bias of the layer.
BIAS_ATOL = 5


def _tr(prms, dtype):
    return dict(prms["training_params"], DTYPE=dtype, GRAD_SCALE=NET_GS[dtype])


@pytest.mark.parametrize("name,img,C,B,seed", NETS)
def test_padded_nets_match_16bit_oracle(net_dtype, name, img, C, B, seed, monkeypatch):
    """Two training steps of a net whose maps are not a power of two, against the stored-16-bit oracle (which knows
    nothing of pitches) -- and measurably closer to it than to the fp32 oracle."""
    from theanet_amd import NeuralNet
    dtype = net_dtype
    prms = load_prms(name, img, batch=B)
    tr = _tr(prms, dtype)
    rng = np.random.RandomState(seed)
    x = rng.rand(2 * B, C, img, img).astype(np.float32)
    y = rng.randint(0, 10, 2 * B).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    convs = [l for l in net.tr_layers if type(l).__name__ == "ConvLayer"]
    assert convs and all(l.f16 for l in convs) and convs[0].output.padded
    ora = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float32"), dtype=np.float64)
    _mean_bwd_16(monkeypatch, ora)
    (rt, at), wat = NET_TOL[dtype]
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, C, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:      # (the mode is not a no-op: the fp32 oracle is measurably further away)
            lp32 = ora32.forward(x[:B], True, draws)[0]
            assert np.abs(lp - lp_w).max() < .75 * np.abs(lp32 - lp_w).max() + 1e-6
        for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
            for j, w in enumerate(lyr.get_wts()):
                bias = j == 1 and type(lyr).__name__ == "ConvLayer"
                assert_close(w, ol.params[j], rt, wat * (BIAS_ATOL if bias else 1),
                             what="%s %s w %d %d step %d" % (name, dtype, i, j, s))
    # every padded tensor of the stack kept a zero pad through the steps
    for lyr in net.tr_layers:
        for t in (getattr(lyr, "output", None), getattr(lyr, "gin", None), getattr(lyr, "x16", None)):
            if getattr(t, "padded", False):
                raw = DeviceArray.get_value(t)
                S = t.c8[1]
                assert not raw[:, :, S:].any() and not raw[:, :, :, S:].any(), (name, type(lyr).__name__)


def test_padded_elastic_route_at_28(monkeypatch):
    """An active ElasticLayer under the first conv layer of a padded stack writes its fp32 output (no c8 prefill) and
    the conv layer packs it at pitch 32: the c8 input is the rounded distorted image, pad zero."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")          # (one net runs every step: its layers hold this step's tensors)
    prms = load_prms("mnist_c16.prms", 28, batch=8)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
    el, conv = net.tr_layers[0], net.tr_layers[1]
    assert el.active and conv.x16.padded and conv.x16.pitch == 32 and el._c8_consumer is None
    rng = np.random.RandomState(2)
    x = rng.rand(16, 1, 28, 28).astype(np.float32)
    fn = net.get_trin_model(x, rng.randint(0, 10, 16).astype(np.int32))
    fn(0)
    ctx().sync()
    want = CB.rbf16(el.output.get_value().astype(np.float64))
    assert np.abs(el.output.get_value() - x[:8]).max() > 1e-3          # (distorted)
    got = _logical(conv.x16, 1, 28, "bfloat16", "elastic -> pack")
    np.testing.assert_array_equal(got, want)


def test_padded_net_schedules_are_bit_identical(monkeypatch):
    """Two steps in flight against one at a time, and replayed (tn_net_plan_*) against interpreted steps, on the
    MNIST-shaped net at 28: costs, logprobs, a test-function result and the weights, bit for bit."""
    from theanet_amd import NeuralNet
    prms = load_prms("mnist_c16.prms", 28, batch=16)
    rng = np.random.RandomState(5)
    x = rng.rand(16 * 6, 1, 28, 28).astype(np.float32)
    y = rng.randint(0, 10, 16 * 6).astype(np.int32)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
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
        assert replayed == (plan == "1"), (pipe, plan, getattr(pl, "why", None))
        runs.append((outs, mids, [w.copy() for l in net.tr_layers for w in l.get_wts()]))
    ref = runs[0]
    for r in runs[1:]:
        for a, b in zip(ref[0], r[0]):
            for u, v in zip(a, b):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
        for (ta, wa), (tb, wb) in zip(ref[1], r[1]):
            for u, v in zip(ta, tb):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(wa, wb):
                np.testing.assert_array_equal(u, v)
        for u, v in zip(ref[2], r[2]):
            np.testing.assert_array_equal(u, v)


def test_padded_net_test_outputs_have_logical_shapes():
    from theanet_amd import NeuralNet
    prms = load_prms("mnist_c16.prms", 28, batch=8)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
    rng = np.random.RandomState(4)
    x = rng.rand(16, 1, 28, 28).astype(np.float32)
    te = net.get_data_test_model(get_output_of_layers=(0, 2, 4))
    res = te(x[:8])
    shapes = [np.asarray(r).shape for r in res[2:]]
    assert shapes == [(8, 1, 28, 28), (8, 32, 14, 14), (8, 64, 7, 7)], shapes
    assert np.abs(res[-1]).max() > 0 and res[0].shape[0] == 8


def _net(layers, img, C, dtype):
    from theanet_amd import NeuralNet
    tp = {"SEED": 1, "BATCH_SZ": 4, "INIT_LEARNING_RATE": .1, "EPOCHS_TO_HALF_RATE": 1, "DTYPE": dtype}
    return NeuralNet([("InputLayer", {"img_sz": img, "num_maps": C})] + layers + [("SoftmaxLayer", {"n_out": 10})], tp)


CONV = ("ConvLayer", {"num_maps": 16, "filter_sz": 3, "stride": 1, "mode": "same"})
POOL = ("PoolLayer", {"pool_sz": 2})


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_padded_refusals_name_the_limits(dt):
    try:
        with pytest.raises(AssertionError, match="at most 64 pixels"):
            _net([CONV, POOL, ("HiddenLayer", {"n_out": 64})], 80, 3, dt)                  # maps above 64
        with pytest.raises(AssertionError, match="2x2 on even maps"):
            _net([CONV, POOL, CONV, POOL, CONV, POOL, ("HiddenLayer", {"n_out": 64})], 28, 3, dt)   # pool on 7
        with pytest.raises(AssertionError, match="pitch of at least 8"):
            _net([CONV, POOL, CONV, POOL, CONV, ("HiddenLayer", {"n_out": 64})], 12, 3, dt)       # conv at pitch 4
        # ... and what these limits allow builds
        _net([CONV, POOL, ("ConvLayer", dict(CONV[1], num_maps=64)), POOL, ("HiddenLayer", {"n_out": 64})], 12, 3, dt)
    finally:
        ctx().set_matmul_dtype("float32")
