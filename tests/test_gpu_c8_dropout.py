"""DropOutLayer on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16'): the ops tn_c8_dropout_fwd /
tn_c8_dropout_bwd / tn_c8_scale through the C-ABI, and nets with DropOutLayers between their conv blocks.

Stored-16-bit semantics.  Train forward y = x (.) m and backward gin = gout (.) m select stored values or
+0: exact.  The mask is the fp32 net's: element (n, c, h, w) of the LOGICAL (N, C, S, S) tensor is kept iff
tn_dropout_mask keeps element elem0 + ((n C + c) S + h) S + w for the same seed and step.  The backward applies no act':
the layer looks through (DropOutLayer.act_info), so the gradient is rounded once by its producer and a DropOutLayer
whose mask is all ones is the net without it, bit for bit.  Test version: y = R((1 - pdrop) x), product in fp32, one
nearest-even rounding.

The oracle's stored-16-bit mode does not know the layer, so the net tests adapt it from outside (_oracle_16): its
_f16_down multiplies by the DropOut's cached mask and by act' of the block under it before rounding (the oracle's own
DropOut branch then multiplies by the 0/1 mask once more, which changes nothing), a Hidden layer above a DropOut takes
16-bit operands like one above a Pool, and the Mean backward is the device's (tests/test_gpu_c8_mean.py).

Tolerances: the ops are equalities.  Nets: the bounds of tests/test_gpu_c8_mean.py (= tests/test_gpu_f16.py /
tests/test_gpu_bf16.py), imported; identity, schedules, sharding and the fp32 mask are bit for bit; the kept fraction is
within 4 standard deviations of 1 - pdrop."""
import copy

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8b_util as CB
from tests.gpu_util import assert_close, call, ctx, dev, load_prms
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
# (N, C, S, P): C < 8, C not a multiple of 8, dense S in {4, 8, 16, 32, 64}, padded S in {28, 14, 7, 6}, a dense side that
# is not a multiple of 4 and a 2 x 2 map
CASES = [(1, 3, 4, 4), (129, 8, 4, 4), (37, 24, 8, 8), (5, 64, 16, 16), (300, 12, 32, 32), (2, 40, 64, 64),
         (9, 12, 28, 32), (33, 20, 14, 16), (6, 8, 7, 8), (5, 5, 6, 8), (3, 16, 6, 6), (4, 8, 2, 2)]
ELEM0 = [0, 12345677, (1 << 33) + 8]          # aligned, not a multiple of 4, beyond 32 bits
SEED, STEP, DSTEP, PDROP = 424242, 3, 5, .3


def _to_raw(bits, P):
    """(N, C, S, S) uint16 patterns -> the raw c8 image (N, C8, P, P, 8), pad cells and channels past C zero."""
    N, C, S, _ = bits.shape
    C8 = (C + 7) // 8
    buf = np.zeros((N, C8 * 8, P, P), np.uint16)
    buf[:, :C, :S, :S] = bits
    return np.ascontiguousarray(buf.reshape(N, C8, 8, P, P).transpose(0, 1, 3, 4, 2))


def _from_raw(raw):
    """raw c8 image -> (N, 8 C8, P, P) uint16 patterns."""
    N, C8, P, _, _ = raw.shape
    return raw.transpose(0, 1, 4, 2, 3).reshape(N, C8 * 8, P, P)


def _unpack(m8):
    """(N, C8, P, P) mask bytes -> (N, 8 C8, P, P) 0/1."""
    N, C8, P, _ = m8.shape
    return np.unpackbits(m8[:, :, None], axis=2, bitorder="little").reshape(N, C8 * 8, P, P)


def _rand_bits(rng, shape, dtype):
    """Random stored values as patterns: normals, and a few zeros of both signs, large and tiny values."""
    v = rng.standard_normal(shape)
    flat = v.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, k)] = rng.choice([0., -0., 60000., -3e-6, 6e-8, 1.5], k)
    return _bits(v, dtype)


def _value32(bits, dtype):
    return CB.bf16_value(bits) if dtype == "bfloat16" else bits.view(np.float16).astype(np.float32)


def _ref_mask(N, C, S, pdrop, seed, step, d_step, elem0):
    """The mask tn_dropout_mask writes for the logical (N, C, S, S) tensor."""
    m = dev(np.full((N, C, S, S), 7, np.uint8))
    call("tn_dropout_mask", m.ptr, N * C * S * S, pdrop, seed, step, d_step.ptr if d_step is not None else None, elem0)
    return m.get_value()


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_c8_dropout_ops_are_exact(dtype, case):
    N, C, S, P = case
    C8 = (C + 7) // 8
    rng = np.random.default_rng(CASES.index(case))
    xb = _rand_bits(rng, (N, C, S, S), dtype)
    gb = _rand_bits(rng, (N, C, S, S), dtype)
    x, g = dev(_to_raw(xb, P)), dev(_to_raw(gb, P))
    d_step = dev(np.array([DSTEP], np.uint32))
    for elem0 in ELEM0:
        y = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
        m8 = dev(np.full((N, C8, P, P), 0xA5, np.uint8))
        call("tn_c8_dropout_fwd", x.ptr, y.ptr, m8.ptr, N, C, S, P, PDROP, SEED, STEP, d_step.ptr, elem0, 1)
        want = _ref_mask(N, C, S, PDROP, SEED, STEP, d_step, elem0)
        assert 0 < want.mean() < 1
        full = np.zeros((N, C8 * 8, P, P), np.uint8)
        full[:, :C, :S, :S] = want
        got = _unpack(m8.get_value())
        np.testing.assert_array_equal(got, full, err_msg="mask %s %s elem0 %d" % (dtype, case, elem0))   # pad, excess: 0
        xfull = _from_raw(x.get_value())
        np.testing.assert_array_equal(_from_raw(y.get_value()), np.where(full, xfull, 0).astype(np.uint16),
                                      err_msg="forward %s %s elem0 %d" % (dtype, case, elem0))
        # backward into a fresh tensor and in place
        gin = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
        call("tn_c8_dropout_bwd", g.ptr, m8.ptr, gin.ptr, N, C, S, P)
        gwant = np.where(full, _from_raw(g.get_value()), 0).astype(np.uint16)
        np.testing.assert_array_equal(_from_raw(gin.get_value()), gwant)
        g2 = dev(g.get_value())
        call("tn_c8_dropout_bwd", g2.ptr, m8.ptr, g2.ptr, N, C, S, P)
        np.testing.assert_array_equal(_from_raw(g2.get_value()), gwant)
    # the device step alone (step 0) and no device counter at all give the same numbers for the same sum
    ma, mb = dev(np.zeros((N, C8, P, P), np.uint8)), dev(np.zeros((N, C8, P, P), np.uint8))
    y = dev(np.zeros((N, C8, P, P, 8), np.uint16))
    call("tn_c8_dropout_fwd", x.ptr, y.ptr, ma.ptr, N, C, S, P, PDROP, SEED, 0, dev(np.array([8], np.uint32)).ptr, 0, 1)
    call("tn_c8_dropout_fwd", x.ptr, y.ptr, mb.ptr, N, C, S, P, PDROP, SEED, 8, None, 0, 1)
    np.testing.assert_array_equal(ma.get_value(), mb.get_value())
    # draw = 0: an injected mask (stray bits in pad cells and excess channels must not leak)
    inj = rng.integers(0, 256, (N, C8, P, P)).astype(np.uint8)
    m8 = dev(inj)
    y = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
    call("tn_c8_dropout_fwd", x.ptr, y.ptr, m8.ptr, N, C, S, P, PDROP, SEED, STEP, d_step.ptr, 0, 0)
    keep = np.zeros((N, C8 * 8, P, P), np.uint8)
    keep[:, :C, :S, :S] = _unpack(inj)[:, :C, :S, :S]
    np.testing.assert_array_equal(_from_raw(y.get_value()), np.where(keep, _from_raw(x.get_value()), 0).astype(np.uint16))
    np.testing.assert_array_equal(m8.get_value(), inj)
    # the test version: one nearest-even rounding of the fp32 product, bit patterns
    for scale in (1 - PDROP, .75, .5):
        y = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
        call("tn_c8_scale", x.ptr, y.ptr, N, C, S, P, scale)
        prod = _value32(_from_raw(x.get_value()), dtype) * np.float32(scale)             # fp32 product
        want = prod.astype(np.float16).view(np.uint16) if dtype == "float16" else CB.bf16_bits(CB.rbf16(prod.astype(np.float64)))
        np.testing.assert_array_equal(_from_raw(y.get_value()), want, err_msg="scale %s %s %g" % (dtype, case, scale))


def test_c8_dropout_ops_refuse_bad_arguments():
    ctx().set_matmul_dtype("float16", 4096.)
    try:
        x = dev(np.zeros((1, 1, 8, 8, 8), np.uint16))
        m = dev(np.zeros((1, 1, 8, 8), np.uint8))
        for geom in ((0, 8, 4, 4), (1, 0, 4, 4), (1, 8, 0, 4), (1, 8, 8, 4), (1, 8, 5, 6), (1 << 20, 64, 64, 64)):
            with pytest.raises(Exception):
                call("tn_c8_dropout_fwd", x.ptr, x.ptr, m.ptr, *geom, .5, 1, 0, None, 0, 1)
            with pytest.raises(Exception):
                call("tn_c8_dropout_bwd", x.ptr, m.ptr, x.ptr, *geom)
            with pytest.raises(Exception):
                call("tn_c8_scale", x.ptr, x.ptr, *geom, .5)
        for pdrop in (-.1, 1.5):
            with pytest.raises(Exception):
                call("tn_c8_dropout_fwd", x.ptr, x.ptr, m.ptr, 1, 8, 8, 8, pdrop, 1, 0, None, 0, 1)
        with pytest.raises(Exception):
            call("tn_c8_dropout_fwd", None, x.ptr, m.ptr, 1, 8, 8, 8, .5, 1, 0, None, 0, 1)
        with pytest.raises(Exception):
            call("tn_c8_dropout_fwd", x.ptr, x.ptr, None, 1, 8, 8, 8, .5, 1, 0, None, 0, 1)
        with pytest.raises(Exception):
            call("tn_c8_dropout_bwd", x.ptr, None, x.ptr, 1, 8, 8, 8)
        with pytest.raises(Exception):
            call("tn_c8_scale", x.ptr, None, 1, 8, 8, 8, .5)
        assert not x.get_value().any()                      # nothing was launched on the way
    finally:
        ctx().set_matmul_dtype("float32")


def test_c8_dropout_statistics_and_steps(dtype):
    """pdrop .25 on 2^20 elements: the kept fraction within 4 sigma of .75 (sigma = sqrt(.25 * .75 / n)), and the masks of
    two consecutive steps differ."""
    N, C, S = 64, 64, 16
    n = N * C * S * S
    assert n >= 10 ** 6
    x = dev(np.full((N, C // 8, S, S, 8), 0x3c00, np.uint16))
    d_step = dev(np.array([0], np.uint32))
    masks = []
    for step in (0, 1):
        d_step.set_value(np.array([step], np.uint32))
        m8 = dev(np.zeros((N, C // 8, S, S), np.uint8))
        y = dev(np.zeros((N, C // 8, S, S, 8), np.uint16))
        call("tn_c8_dropout_fwd", x.ptr, y.ptr, m8.ptr, N, C, S, S, .25, 99, 0, d_step.ptr, 0, 1)
        masks.append(_unpack(m8.get_value()))
        frac = masks[-1].mean()
        assert abs(frac - .75) <= 4 * np.sqrt(.25 * .75 / n), (step, frac)
    assert .3 < (masks[0] != masks[1]).mean() < .45          # independent draws differ on 2 * .25 * .75 of the elements


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
TP = {"SEED": 7, "BATCH_SZ": 8, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


def _conv(k, act):
    return ("ConvLayer", {"num_maps": k, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": act})


POOL = ("PoolLayer", {"pool_sz": 2})
DROP = ("DropOutLayer", {"pdrop": .25})


def _layers(head, act, img, drops=True):
    """hidden: Conv Pool [Drop] Conv Pool [Drop] Hidden Softmax (Drop -> Conv, Drop -> Hidden);
    mean: Conv Pool [Drop] Conv [Drop] Mean Softmax (Drop -> Conv, Drop on an unpooled conv -> Mean)."""
    d = [DROP] if drops else []
    L = [("InputLayer", {"img_sz": img, "num_maps": 3}), _conv(16, act), POOL] + d
    if head == "hidden":
        L += [_conv(32, act), POOL] + d + [("HiddenLayer", {"n_out": 64, "actvn": act})]
    else:
        L += [_conv(32, act)] + d + [("MeanLayer", {})]
    return L + [("SoftmaxLayer", {"n_out": 10})]


def _tr(tp, dtype):
    return dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype]) if dtype in GS else dict(tp, DTYPE=dtype)


def _data(B, img, n=4, seed=3):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, 3, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


def _drops(net):
    return [l for l in net.tr_layers if type(l).__name__ == "DropOutLayer" and l.drop is not None]


def _weights(net):
    return [w.copy() for l in net.tr_layers for w in l.get_wts()]


@pytest.mark.parametrize("img", [16, 24], ids=["dense", "padded"])
@pytest.mark.parametrize("act", ["relu10", "relu"])
@pytest.mark.parametrize("head", ["hidden", "mean"])
def test_all_ones_mask_is_the_net_without_the_layer(dtype, head, act, img):
    """Three training steps with every DropOutLayer's mask injected as all ones: the weights of the net built without
    those layers, bit for bit (single rounding of the gradient, act' taken through the layer)."""
    from theanet_amd import NeuralNet
    x, y = _data(8, img)
    plain = NeuralNet(_layers(head, act, img, False), _tr(TP, dtype))
    wts = plain.get_init_params()["allwts"]
    lyrs = _layers(head, act, img, True)
    it = iter(wts)
    allwts = [[] if name == "DropOutLayer" else next(it) for name, _ in lyrs]
    net = NeuralNet(lyrs, _tr(TP, dtype), allwts=allwts)
    drops = _drops(net)
    assert len(drops) == 2 and all(d.c8 is not None for d in drops)
    assert drops[0].output.padded == (img == 24)
    fa, fb = plain.get_trin_model(x, y), net.get_trin_model(x, y)
    for s in range(3):
        for d in drops:
            d.drop.inject(np.ones(d.drop.shape))
        ca, _, la = fa(s)
        cb, _, lb = fb(s)
        assert ca == cb
        np.testing.assert_array_equal(la, lb)
    moved = False
    for a, b, w0 in zip(_weights(plain), _weights(net), [w for l in wts for w in l]):
        np.testing.assert_array_equal(a, b)
        moved = moved or not np.array_equal(a, w0)
    assert moved


def _gap_drop(img, B):
    """cifar_gap.prms with a DropOutLayer (pdrop .25) after each pool: ... -> Drop -> Mean -> Softmax."""
    prms = load_prms("cifar_gap.prms", img, batch=B)
    out = []
    for name, args in prms["layers"]:
        out.append((name, args))
        if name == "PoolLayer":
            out.append(("DropOutLayer", {"pdrop": .25}))
    prms["layers"] = out
    return prms


def _oracle_16(monkeypatch, ora):
    """The stored-16-bit oracle taught the DropOutLayer on the stack, from outside (module docstring)."""
    kinds = [l.kind for l in ora.L]

    def under(i):                                   # the Conv whose activation the block under layer i applies
        k = i - 1
        while kinds[k] in ("DropOut", "Pool"):
            k -= 1
        assert kinds[k] == "Conv"
        return ora.L[k].actvn

    f16_down = ora._f16_down

    def down(g, i, cache):
        if kinds[i - 1] != "DropOut":
            return f16_down(g, i, cache)
        out = np.asarray(cache[i - 1]["out"], np.float64)            # x (.) m
        g = np.asarray(g, np.float64).reshape(out.shape) * O.act_grad_from_out(under(i), out)
        if "mask" in cache[i - 1]:
            g = g * cache[i - 1]["mask"]
        return O.r16(g, ora.grad_scale)

    monkeypatch.setattr(ora, "_f16_down", down)
    # a Hidden layer above a DropOut of the stack: 16-bit operands (its input is stored 16-bit already; its weights are
    # rounded for the forward product here, and cache["c8"] sends the backward down the oracle's own c8 branch)
    hid = [i for i, k in enumerate(kinds) if k == "Hidden" and kinds[i - 1] == "DropOut" and "Conv" in kinds[:i]
           and all(kk in ("DropOut", "Pool", "Conv", "Elastic", "Input") for kk in kinds[:i])]
    forward = ora.forward

    def fwd(x, train, draws=None, keep=False, aux=None):
        saved = [(i, ora.L[i].params[0]) for i in hid]
        for i, w in saved:
            ora.L[i].params[0] = np.asarray(O.r16(w), w.dtype)
        try:
            h, cache = forward(x, train, draws, keep, aux)
        finally:
            for i, w in saved:
                ora.L[i].params[0] = w
        for i in hid:
            cache[i]["c8"] = True
        return h, cache

    monkeypatch.setattr(ora, "forward", fwd)
    if "Mean" in kinds:
        i = kinds.index("Mean")
        actvn, orig, gs = under(i), O.mean_bwd, ora.grad_scale

        def mean_bwd(x, dy):
            return O.r16(orig(x, dy) * O.act_grad_from_out(actvn, np.asarray(x, np.float64)), gs)

        monkeypatch.setattr(O, "mean_bwd", mean_bwd)


ORACLE_NETS = [("cifar_drop.prms", 32, 8), ("cifar_gap_drop", 32, 8), ("cifar_drop.prms", 24, 8)]


@pytest.mark.parametrize("name,img,B", ORACLE_NETS)
def test_dropout_nets_match_16bit_oracle(dtype, name, img, B, monkeypatch):
    """Three training steps (cost, logprob, argmax; every dW / db through the weights after each update) with the
    oracle's elastic draws and dropout masks injected into both sides, then the test mode of the trained net, against
    the stored-16-bit oracle at the bounds of tests/test_gpu_c8_mean.py."""
    from theanet_amd import NeuralNet
    prms = _gap_drop(img, B) if name == "cifar_gap_drop" else load_prms(name, img, batch=B)
    tr = _tr(prms["training_params"], dtype)
    x, y = _data(B, img, n=3, seed=1)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(tr))
    assert len(_drops(net)) == 3 and all(d.c8 is not None for d in _drops(net))
    ora = O.OracleNet(copy.deepcopy(prms["layers"]), dict(tr, DTYPE="float16"), dtype=np.float64)
    _oracle_16(monkeypatch, ora)
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
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
    # test mode: (1 - pdrop) x, rounded once on the device, not in the oracle
    tfn = net.get_test_model(x, y, preds_feats=True)
    _, _, feats, preds = tfn(1)
    _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
    print("%s %s test: max |dlogprob| %.3g" % (name, dtype, np.abs(feats[:B] - lp_w).max()))
    assert_close(feats[:B], lp_w, rt, at, what="%s %s test logprob" % (name, dtype))
    np.testing.assert_array_equal(preds[:B], preds_w)


def test_mask_equals_the_fp32_nets(dtype, monkeypatch):
    """The same layers and SEED with DTYPE float32 and 16-bit, device RNG: after one training step every DropOutLayer's
    packed mask, unpacked, is the fp32 layer's byte mask (dense 16 x 16 / 8 x 8 maps and padded 12 x 12 / 6 x 6)."""
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", "0")
    for img in (32, 24):
        x, y = _data(8, img)
        masks = []
        for dt in ("float32", dtype):
            net = NeuralNet(_layers("hidden", "relu10", img), _tr(TP, dt))
            net.get_trin_model(x, y)(0)
            ds = _drops(net)
            assert len(ds) == 2 and all((d.c8 is not None) == (dt != "float32") for d in ds)
            masks.append([d.drop.unpacked() if d.c8 is not None else d.drop.mask.get_value() for d in ds])
        for a, b in zip(*masks):
            assert a.shape == b.shape and 0 < a.mean() < 1
            np.testing.assert_array_equal(a, b)


def test_sharded_nets_draw_the_unsharded_mask(dtype, monkeypatch):
    """Two nets built for rows [0, B/2) and [B/2, B) of a global batch draw, between them, the unsharded net's masks."""
    from theanet_amd import NeuralNet, comm
    B, img = 8, 24

    def masks(rank, size):
        monkeypatch.setattr(comm, "get_world", lambda: comm.World(rank, size, dry=True))
        net = NeuralNet(_layers("hidden", "relu", img), _tr(dict(TP, BATCH_SZ=B), dtype))
        out = []
        for d in _drops(net):
            assert d.drop.shape[0] == B // size and d.drop.elem0 == rank * (B // size) * int(np.prod(d.drop.shape[1:]))
            d.inpt.set_value(np.ones(d.drop.shape, np.float32))
            d.forward(True)
            out.append(d.drop.unpacked())
            np.testing.assert_array_equal(d.output.get_value(), out[-1])         # ones in: the output is the mask
        return out

    whole, lo, hi = masks(0, 1), masks(0, 2), masks(1, 2)
    for w, a, b in zip(whole, lo, hi):
        assert 0 < w.mean() < 1
        np.testing.assert_array_equal(w, np.concatenate([a, b]))


def test_dropout_net_schedules_are_bit_identical(dtype, monkeypatch):
    """cifar_drop.prms, device RNG: two steps in flight against one at a time, replayed (tn_net_plan_*) against
    interpreted steps -- the plan really taken -- and the 1-rank data-parallel step: costs, logprobs, a test-function
    result and the weights in the middle of training, and the final weights, bit for bit."""
    from theanet_amd import NeuralNet
    prms = load_prms("cifar_drop.prms", 32, batch=16)
    x, y = _data(16, 32, n=6, seed=5)
    runs = []
    for pipe, plan, dp in (("1", "1", "0"), ("0", "1", "0"), ("1", "0", "0"), ("0", "0", "0"), ("1", "1", "1"), ("0", "1", "1")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        monkeypatch.setenv("TN_DP_FORCE", dp)
        monkeypatch.setenv("TN_DP_PIPELINE", pipe)
        monkeypatch.setenv("TN_DP_OVERLAP", "0")
        net = NeuralNet(copy.deepcopy(prms["layers"]), _tr(prms["training_params"], dtype))
        assert len(_drops(net)) == 3
        fn = net.get_trin_model(x, y)
        te = net.get_test_model(x, y)
        outs, mids = [], []
        for s in range(40):
            if s in (30, 39):
                outs.append(fn(s % 6))
            else:
                fn.enqueue(s % 6)
            if s == 34:
                mids.append((te(1), _weights(net)))
        outs.append(fn.fetch())
        pl = getattr(fn, "_plan", None)
        replayed = pl is not None and pl.ready
        if fn.__class__.__name__ == "_PipeTrainFn" and fn._seq is not None:
            replayed = fn._seq._plan.ready
        if dp == "0":
            assert replayed == (plan == "1"), (pipe, plan, getattr(pl, "why", None))
        runs.append((outs, mids, _weights(net)))
        if dp == "1":
            assert net._dp
            net.ctx.call("tn_comm_destroy")
            net._dev_group = None
    for k, (outs, mids, ws) in enumerate(runs[1:]):
        dp = k + 1 >= 4
        for a, b in zip(runs[0][0], outs):
            if not dp:                      # (the data-parallel step sums its cost through the all-reduce buffer)
                assert a[0] == b[0]
            np.testing.assert_array_equal(a[2], b[2])
        for (t0, w0), (t1, w1) in zip(runs[0][1], mids):
            for u, v in zip(t0, t1):
                np.testing.assert_array_equal(np.asarray(u), np.asarray(v))
            for u, v in zip(w0, w1):
                np.testing.assert_array_equal(u, v)
        for a, b in zip(runs[0][2], ws):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_dropout_between_conv_and_its_pool_is_refused(dt):
    from theanet_amd import NeuralNet
    lyrs = [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, "relu"), DROP, POOL,
            ("HiddenLayer", {"n_out": 64}), ("SoftmaxLayer", {"n_out": 10})]
    try:
        with pytest.raises(AssertionError, match="between a ConvLayer and its PoolLayer breaks the fused"):
            NeuralNet(lyrs, _tr(TP, dt))
        # ... and what the stack admits builds: Drop over Drop, Drop with pdrop 0 (a pass-through)
        net = NeuralNet([lyrs[0], lyrs[1], POOL, DROP, ("DropOutLayer", {"pdrop": 0}), DROP] + lyrs[4:], _tr(TP, dt))
        d = [l for l in net.tr_layers if type(l).__name__ == "DropOutLayer"]
        assert d[1].output is d[1].inpt and d[1].drop is None and d[2].act_info()[0] is d[2].output
    finally:
        ctx().set_matmul_dtype("float32")


def test_dropout_seeds_travel_with_the_optimizer_state(dtype):
    """A checkpoint with optimizer / RNG state carries the 16-bit layers' stream seeds like the fp32 layers'."""
    from theanet_amd import NeuralNet
    net = NeuralNet(_layers("hidden", "relu", 16), _tr(TP, dtype))
    ck = net.get_init_params(with_opt_state=True)
    twin = NeuralNet(_layers("hidden", "relu", 16), _tr(TP, dtype), allwts=ck["allwts"])
    twin.load_opt_state(ck["opt_state"])
    seeds = [d.drop.seed for d in _drops(net)]
    assert len(seeds) == 2 and seeds == [d.drop.seed for d in _drops(twin)]
