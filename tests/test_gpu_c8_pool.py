"""A stand-alone PoolLayer on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16'): the ops tn_c8_pool_fwd /
tn_c8_pool_bwd through the C-ABI, and nets whose PoolLayers no fused conv + pool block takes -- 3x3 windows, a pool above a
DropOutLayer or another PoolLayer, a window spanning the map, ignore_border on a map the window does not divide, and every
2x2 pool of a net built with fuse_conv_pool off.

Stored-16-bit semantics ("PoolLayer on the stack").  Forward: the maximum of the STORED values of the clipped
window, chosen and never rounded; the window is scanned row-major and replaced on strict >, so of equal values the first
one's pattern is kept.  Backward: every element whose value equals its window's maximum receives the whole gradient, bit
for bit (-0 == +0 ties); everything else, pad cells and channels past C included, is the all-zero pattern.  No act' is
applied: the layer looks through (PoolLayer.act_info), the producer of its incoming gradient has applied act' of the block
below from the pooled output and rounded once.

The oracle's stored-16-bit mode pools the UNROUNDED activation of the conv directly below (the fused block's rule) and
knows neither a pool above a DropOut or a Pool nor 1x1 convs under a pool, so the net tests teach it the layer from
outside (_teach_pool): a forward that takes the maximum and the ties of a stand-alone pool on the stored output of the
layer below, an _f16_down that finds the conv under chains of Pool and DropOut layers, and the device's Mean backward
(tests/test_gpu_c8_mean.py).  Dropout masks are injected on both sides.

Tolerances: the ops are equalities.  Nets: the bounds of tests/test_gpu_c8_mean.py, imported; schedules bit for bit."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import assert_close, call, ctx, dev, load_prms
from tests.test_gpu_c8_dropout import _from_raw, _to_raw, _value32
from tests.test_gpu_c8_mean import GS, R16, TOL, _bits
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

GARBAGE = 0x5555


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request, monkeypatch):
    """The element type; for bfloat16 the oracle's stored-16-bit mode rounds to bf16 (tests/test_gpu_bf16.py)."""
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    ctx().set_matmul_dtype(request.param, GS[request.param])
    yield request.param
    monkeypatch.setattr(O, "r16", R16)
    ctx().set_matmul_dtype("float32")


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
# (N, C, S, P, p, ignore_border).  Dense and padded inputs, odd maps in both border modes, a last window one pixel wide or
# dropped, a window of 4, a global maximum, a window larger than the map, an output at pitch 64 and a dense one above 64;
# the last four are the sides at which the kernels leave the shift for the division (tests/test_c8_pool_cpu.py): a dense
# input whose side is no power of two under the 3x3 and the run-time window, an output above 64 pixels under both.
CASES = [(1, 3, 4, 4, 2, False), (129, 8, 6, 8, 3, False), (37, 24, 7, 8, 2, False), (37, 24, 7, 8, 2, True),
         (5, 64, 16, 16, 3, False), (5, 64, 16, 16, 3, True), (300, 12, 32, 32, 3, False), (9, 12, 28, 32, 2, False),
         (33, 20, 14, 16, 4, False), (6, 8, 11, 16, 3, False), (6, 8, 11, 16, 3, True), (2, 40, 64, 64, 2, False),
         (3, 16, 8, 8, 8, False), (4, 8, 5, 8, 7, False), (2, 16, 128, 128, 3, False), (2, 8, 130, 130, 2, False),
         (2, 12, 6, 6, 3, False), (2, 8, 10, 10, 5, True), (1, 8, 195, 195, 3, False), (1, 5, 260, 260, 4, False)]


def pool_geom(case):
    """(N, C, S, P, p, So, Po) of a case: the output side of its border mode at the pitch rule of the layer."""
    from theanet_amd.device import c8_pool_pitch
    N, C, S, P, p, ib = case
    So = S // p if ib else -(-S // p)
    return N, C, S, P, p, So, c8_pool_pitch(So)


def _windows(a, p, So, fill):
    """(N, C, S, S) -> (N, C, So, So, p * p): the elements of every window in scan order, ``fill`` past the map edge."""
    N, C, S, _ = a.shape
    buf = np.full((N, C, So * p, So * p), fill, a.dtype)
    s = min(S, So * p)
    buf[:, :, :s, :s] = a[:, :, :s, :s]
    return buf.reshape(N, C, So, p, So, p).transpose(0, 1, 2, 4, 3, 5).reshape(N, C, So, So, p * p)


def _pool_input(rng, case, dtype):
    """Stored patterns with many ties: multiples of 0.5 in [-2, 2] and a sprinkle of +0, -0, 60000, -3e-6 and 6e-8; the
    first window of the first map holds -0 then +0 above negative values, the second one +0 then -0."""
    N, C, S, P, p, So, Po = pool_geom(case)
    v = rng.integers(-4, 5, (N, C, S, S)) * .5
    flat = v.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, k)] = rng.choice([0., -0., 60000., -3e-6, 6e-8], k)
    for j, pair in ((0, (-0., 0.)), (1, (0., -0.))):
        if j < So and min(S, (j + 1) * p) - j * p >= 2:
            v[0, 0, :min(S, p), j * p:min(S, (j + 1) * p)] = -1.
            v[0, 0, 0, j * p:j * p + 2] = pair
    return _bits(v, dtype).reshape(N, C, S, S)


@pytest.mark.parametrize("case", CASES, ids=["x".join(str(int(c)) for c in case) for case in CASES])
def test_c8_pool_ops_are_exact(dtype, case):
    N, C, S, P, p, So, Po = geom = pool_geom(case)
    ib, C8 = case[5], (C + 7) // 8
    rng = np.random.default_rng(CASES.index(case))
    xb = _pool_input(rng, case, dtype)
    xv = _value32(xb, dtype)
    wv, wb = _windows(xv, p, So, np.float32(-np.inf)), _windows(xb, p, So, np.uint16(0xffff))
    want = O.pool_fwd(xv, p, ib)
    assert want.shape == (N, C, So, So)
    # the inputs really tie: a tenth of all windows hold their maximum twice, one of them as +0 and -0
    tied = (wv == want[..., None]).sum(-1) >= 2
    assert tied.mean() >= .1, (case, tied.mean())
    zero = wv == 0
    assert (tied & (want == 0) & (zero & (wb == 0)).any(-1) & (zero & (wb == 0x8000)).any(-1)).any(), case
    # numpy's maximum of +0 and -0 has either sign: the pattern of a zero maximum is the first zero's of its window
    first_zero = np.take_along_axis(wb, zero.argmax(-1)[..., None], -1)[..., 0]
    want_bits = np.where(want == 0, first_zero, _bits(want.astype(np.float64), dtype).reshape(want.shape)).astype(np.uint16)
    assert (want_bits[want == 0] == 0x8000).any()                  # (-0 in front of +0: the first one's pattern)

    x = dev(_to_raw(xb, P))
    y = dev(np.full((N, C8, Po, Po, 8), GARBAGE, np.uint16))
    call("tn_c8_pool_fwd", x.ptr, y.ptr, *geom)
    np.testing.assert_array_equal(y.get_value(), _to_raw(want_bits, Po), err_msg="forward %s %s" % (dtype, case))

    gb = _bits(rng.standard_normal((N, C, So, So)), dtype).reshape(N, C, So, So)
    gb[gb == 0x8000] = 0                                           # (a gradient of -0 would make "selected" invisible)
    g = dev(_to_raw(gb, Po))
    gin = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
    call("tn_c8_pool_bwd", x.ptr, y.ptr, g.ptr, gin.ptr, *geom)
    got = _from_raw(gin.get_value())
    gwant = O.pool_bwd(xv, _value32(gb, dtype), p, ib)
    np.testing.assert_array_equal(_value32(got[:, :C, :S, :S], dtype), gwant, err_msg="backward %s %s" % (dtype, case))
    sel = O.pool_bwd(xv, np.ones((N, C, So, So), np.float32), p, ib) != 0
    assert sel.any()
    up = np.zeros((N, C, max(S, So * p), max(S, So * p)), np.uint16)
    up[:, :, :So * p, :So * p] = np.repeat(np.repeat(gb, p, 2), p, 3)
    # ... bit for bit where selected; unselected, uncovered and pad cells and channels past C the all-zero pattern
    np.testing.assert_array_equal(gin.get_value(), _to_raw(np.where(sel, up[:, :, :S, :S], 0).astype(np.uint16), P),
                                  err_msg="backward patterns %s %s" % (dtype, case))


def test_c8_pool_ops_refuse_bad_arguments():
    from theanet_amd import _lib
    ctx().set_matmul_dtype("float16", 4096.)
    try:
        x = dev(np.full((4, 1, 8, 8, 8), 0x3c00, np.uint16))
        out = dev(np.zeros((4, 1, 8, 8, 8), np.uint16))
        ok = (4, 8, 6, 8, 3, 2, 8)
        for args in ((None, out.ptr), (x.ptr, None)):
            with pytest.raises(_lib.BackendError, match="tn_c8_pool_fwd: bad arguments"):
                call("tn_c8_pool_fwd", *args, *ok)
        for args in ((None, x.ptr, x.ptr, out.ptr), (x.ptr, None, x.ptr, out.ptr), (x.ptr, x.ptr, None, out.ptr),
                     (x.ptr, x.ptr, x.ptr, None)):
            with pytest.raises(_lib.BackendError, match="tn_c8_pool_bwd: bad arguments"):
                call("tn_c8_pool_bwd", *args, *ok)
        bad = [(4, 8, 6, 8, 1, 6, 8),                # p = 1
               (4, 8, 6, 8, 65, 1, 8),               # p > 64
               (4, 8, 6, 8, 3, 3, 8),                # So neither S / p nor ceil(S / p)
               pool_geom((4, 8, 5, 8, 7, True)),     # So = 0
               (4, 8, 6, 8, 2, 3, 2),                # Po < So
               (4, 8, 6, 7, 3, 2, 8),                # P neither S nor a power of two
               (4, 8, 6, 8, 3, 2, 6),                # Po neither So nor a power of two
               (0, 8, 6, 8, 3, 2, 8), (4, 0, 6, 8, 3, 2, 8),
               (1 << 20, 64, 64, 64, 2, 32, 32)]     # 2^32 cells
        assert bad[3][5] == 0
        for geom in bad:
            assert not ctx().lib.tn_c8_pool_supported(*geom), geom
            with pytest.raises(_lib.BackendError, match="window %d" % geom[4]):
                call("tn_c8_pool_fwd", x.ptr, out.ptr, *geom)
            with pytest.raises(_lib.BackendError, match="maps of %d pixels at pitch %d" % geom[2:4]):
                call("tn_c8_pool_bwd", x.ptr, x.ptr, x.ptr, out.ptr, *geom)
        assert not out.get_value().any()                     # nothing was launched on the way
    finally:
        ctx().set_matmul_dtype("float32")


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
TP = {"SEED": 7, "BATCH_SZ": 6, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}
B = TP["BATCH_SZ"]


def _conv(k, act="relu10", f=3):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": 1, "mode": "same", "actvn": act})


def _hid(n, act="relu10"):
    return ("HiddenLayer", {"n_out": n, "actvn": act})


POOL2, POOL3 = ("PoolLayer", {"pool_sz": 2}), ("PoolLayer", {"pool_sz": 3})
POOL3_IB = ("PoolLayer", {"pool_sz": 3, "ignore_border": True})
DROP = ("DropOutLayer", {"pdrop": .25})
SOFTMAX = ("SoftmaxLayer", {"n_out": 10})
# name -> (image side, fuse_conv_pool, layers above the 3-map input, which PoolLayers stand alone)
NETS = {
    "a_pool3": (12, True, [_conv(16), POOL3, _hid(32), SOFTMAX], [True]),
    "b_1x1_drop_border": (14, True, [_conv(16), _conv(16, f=1), POOL3, DROP, _conv(24), POOL3_IB, _hid(32), SOFTMAX],
                          [True, True]),
    "c_pool_pool_mean": (18, True, [_conv(16), POOL3, POOL3, ("MeanLayer", {}), SOFTMAX], [True, True]),
    "d_fused_then_pool3": (16, True, [_conv(16), POOL2, POOL3, _hid(32), SOFTMAX], [False, True]),
    "e_unfused_28": (28, False, [_conv(16), POOL2, _conv(32), POOL2, _conv(32), POOL2, _hid(64), SOFTMAX],
                     [True, True, True]),
    "f_unfused_drop_pool": (16, False, [_conv(16, "relu"), DROP, POOL2, _hid(64, "relu"), SOFTMAX], [True]),
}


def _layers(name):
    img, fuse, lyrs, alone = NETS[name]
    return img, fuse, [("InputLayer", {"img_sz": img, "num_maps": 3})] + copy.deepcopy(lyrs), alone


def _tr(tp, dtype):
    return dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype])


def _data(img, n=3, seed=1, maps=3):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, maps, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _build(name, dtype, monkeypatch, **kw):
    """The net of NETS[name], its pools in the forms the table states (and the fused ones really fused)."""
    from theanet_amd import NeuralNet
    img, fuse, lyrs, alone = _layers(name)
    monkeypatch.setattr(NeuralNet, "fuse_conv_pool", fuse)
    net = NeuralNet(lyrs, _tr(TP, dtype), **kw)
    for graph in (net.tr_layers, net.te_layers):
        pools = [(i, l) for i, l in enumerate(graph) if type(l).__name__ == "PoolLayer"]
        assert [l.c8_alone for _, l in pools] == alone and all(l.f16 for _, l in pools)
        for i, l in pools:
            assert (l.fused_conv is None) == l.c8_alone and (getattr(graph[i - 1], "fused_pool", None) is l) == (not l.c8_alone)
    return net, lyrs, img


def _teach_pool(monkeypatch, ora, alone):
    """The stored-16-bit oracle taught the stand-alone PoolLayers ``alone`` (layer indices), from outside (module
    docstring)."""
    kinds = [l.kind for l in ora.L]
    stack = ("Conv", "Pool", "DropOut")

    def under(i):                                   # the Conv whose activation the block under layer i applies
        k = i - 1
        while kinds[k] in ("DropOut", "Pool"):
            k -= 1
        assert kinds[k] == "Conv"
        return ora.L[k].actvn

    def forward(x, train, draws=None, keep=False, aux=None):
        draws, dt, cache = draws or {}, ora.dtype, []
        h = np.asarray(x, dt)
        for i, l in enumerate(ora.L):
            c = {"in": h}
            if l.kind == "Conv":
                c["z"] = O.conv2d_fwd(h, l.params[0], l.params[1], l.stride, l.mode, f16=True)
                c["exact"] = O.activation(l.actvn)[0](c["z"])
                h = O.r16(c["exact"]).astype(dt)
            elif l.kind == "Pool":
                if i not in alone:
                    c["in"] = cache[-1]["exact"]            # a fused block: maximum and ties on the unrounded activation
                h = O.r16(O.pool_fwd(c["in"], l.p, l.ignore_border)).astype(dt)     # (alone: stored values, R changes nothing)
            elif l.kind == "Mean":
                h = O.mean_fwd(h)
            elif l.kind == "DropOut":
                if train:
                    c["mask"] = np.asarray(draws[i], dt).reshape(h.shape)
                    h = h * c["mask"]
                else:
                    h = h * dt.type(1 - l.pdrop)
            elif l.kind in ("Hidden", "Softmax"):
                h = h.reshape(h.shape[0], -1)
                c["in"], c["c8"] = h, kinds[i - 1] in stack
                c["z"] = ((O.r16(h) @ O.r16(l.params[0]) if c["c8"] else h @ l.params[0]) + l.params[1]).astype(dt)
                h = O.log_softmax(c["z"]) if l.kind == "Softmax" else O.activation(l.actvn)[0](c["z"])
            else:
                assert l.kind == "Input", l.kind
            c["out"] = h
            cache.append(c)
        return h, cache

    def down(g, i, cache):
        out = np.asarray(cache[i - 1]["out"], np.float64)
        g = np.asarray(g, np.float64).reshape(out.shape) * O.act_grad_from_out(under(i), out)
        if "mask" in cache[i - 1]:
            g = g * cache[i - 1]["mask"]
        return O.r16(g, ora.grad_scale)

    monkeypatch.setattr(ora, "forward", forward)
    monkeypatch.setattr(ora, "_f16_down", down)
    if "Mean" in kinds:
        actvn, orig, gs = under(kinds.index("Mean")), O.mean_bwd, ora.grad_scale

        def mean_bwd(x, dy):
            return O.r16(orig(x, dy) * O.act_grad_from_out(actvn, np.asarray(x, np.float64)), gs)

        monkeypatch.setattr(O, "mean_bwd", mean_bwd)


@pytest.mark.parametrize("name", sorted(NETS))
def test_pool_nets_match_16bit_oracle(dtype, name, monkeypatch):
    """Three training steps (cost, logprob, argmax; every dW / db through the weights after each update) with the oracle's
    dropout masks injected into both sides, then the test mode of the trained net, against the stored-16-bit oracle at the
    bounds of tests/test_gpu_c8_mean.py."""
    net, lyrs, img = _build(name, dtype, monkeypatch)
    x, y = _data(img)
    ora = O.OracleNet(copy.deepcopy(lyrs), dict(_tr(TP, dtype), DTYPE="float16"), dtype=np.float64)
    _teach_pool(monkeypatch, ora, {i for i, l in enumerate(net.tr_layers) if getattr(l, "c8_alone", False)})
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
    w0 = net.tr_layers[1].get_wts()[0].copy()
    for s in range(3):
        draws = _inject_draws(net, ora, B, 3, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        print("%s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (name, dtype, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
            for j, w in enumerate(lyr.get_wts()):
                print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
                assert_close(w, ol.params[j], rt, wat, what="%s %s w %d %d step %d" % (name, dtype, i, j, s))
    assert not np.array_equal(w0, net.tr_layers[1].get_wts()[0])       # the gradient reached the bottom through the pools
    tfn = net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
    print("%s %s test: max |dlogprob| %.3g" % (name, dtype, np.abs(feats[:B] - lp_w).max()))
    assert_close(feats[:B], lp_w, rt, at, what="%s %s test logprob" % (name, dtype))
    np.testing.assert_array_equal(preds[:B], preds_w)


def test_pool_net_schedules_are_bit_identical(dtype, monkeypatch):
    """Net b (device RNG for its DropOutLayer): two steps in flight against one at a time, and replayed (tn_net_plan_*)
    against interpreted steps -- the plan really taken: costs, logprobs, a test-function result and the weights in the
    middle of training, and the final weights, bit for bit."""
    _, _, lyrs, _ = _layers("b_1x1_drop_border")
    x, y = _data(14, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net, _, _ = _build("b_1x1_drop_border", dtype, monkeypatch)
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
        runs.append((outs, mids, [w for l in net.tr_layers for w in l.get_wts()]))
    for outs, mids, ws in runs[1:]:
        for a, b in zip(runs[0][0], outs):
            assert a[0] == b[0]
            np.testing.assert_array_equal(a[2], b[2])
        for (t0, w0), (t1, w1) in zip(runs[0][1], mids):
            for u, v in zip(t0, t1):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(w0, w1):
                np.testing.assert_array_equal(u, v)
        for a, b in zip(runs[0][2], ws):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("which", ["mnist_c16_28", "dense_16"])
def test_fused_and_standalone_pools_agree_in_test_mode(dtype, which, monkeypatch):
    """The same weights in test mode with fuse_conv_pool on (fused conv + 2x2 pool blocks: the maximum of the unrounded
    activations, rounded) and off (the conv stores its rounded activation, tn_c8_pool_fwd takes the maximum of the stored
    values): the same log-probs, bit for bit.  Rounding is monotone, R(max a) == max R(a), so the two could differ only
    through the fp32 summation order of the pooled and the unpooled instantiation of the conv product -- and these share
    their product loop: in c8_conv_kernel<E, FT, MODE, NS, LK, TK> (conv_c8.hip) MODE 0 / 1 differ in the epilogue alone,
    and c8_plan picks FT, NS, LK and TK from the geometry and the activation, never from the pool flag.  (Training is not
    compared: the fused block takes one argmax from the unrounded sums, the stand-alone pool hands the gradient to every
    tied stored maximum.)"""
    from theanet_amd import NeuralNet
    if which == "mnist_c16_28":
        prms = load_prms("mnist_c16.prms", 28, batch=B)
        lyrs, tp, img, maps = prms["layers"], prms["training_params"], 28, 1
    else:
        lyrs = [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16), POOL2, _conv(32), POOL2, _hid(64), SOFTMAX]
        tp, img, maps = TP, 16, 3
    x, y = _data(img, n=2, seed=11, maps=maps)
    feats, wts = [], None
    for fuse in (True, False):
        monkeypatch.setattr(NeuralNet, "fuse_conv_pool", fuse)
        net = NeuralNet(copy.deepcopy(lyrs), _tr(tp, dtype), allwts=wts)
        pools = [l for l in net.te_layers if type(l).__name__ == "PoolLayer"]
        assert len(pools) == 2 and all(l.c8_alone == (not fuse) for l in pools)
        wts = wts or net.get_init_params()["allwts"]
        feats.append(net.get_test_model(x, y, preds_feats=True)(1)[2][:B])
    print("%s %s: fused against stand-alone, max |dlogprob| %.3g" % (which, dtype, np.abs(feats[0] - feats[1]).max()))
    assert np.isfinite(feats[0]).all() and np.ptp(feats[0]) > 0
    np.testing.assert_array_equal(feats[1], feats[0], err_msg="%s %s stand-alone against fused" % (which, dtype))


def test_data_test_model_returns_the_pooled_maps(dtype, monkeypatch):
    """get_data_test_model on net b: the logical NCHW arrays of both stand-alone pools and of the 1x1 conv map under the
    first -- whose maximum over 3x3 windows the first pooled map is, exactly."""
    net, _, img = _build("b_1x1_drop_border", dtype, monkeypatch)
    fn = net.get_data_test_model(get_output_of_layers=(2, 3, 6))
    x = np.random.default_rng(7).random((B, 3, img, img), dtype=np.float32)
    _, preds, conv, pool, last = fn(x)
    assert conv.shape == (B, 16, 14, 14) and pool.shape == (B, 16, 5, 5) and last.shape == (B, 24, 1, 1) and preds.shape == (B,)
    assert np.abs(pool).max() > 0 and np.abs(last).max() > 0
    np.testing.assert_array_equal(pool, O.pool_fwd(conv, 3, False))
