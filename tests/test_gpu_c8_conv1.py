"""1x1 stride-1 ConvLayers on the 16-bit-resident conv stack (DTYPE 'float16' / 'bfloat16'): the ops tn_c8_conv1_fwd /
tn_c8_conv1_dgrad / tn_c8_conv1_wgrad through the C-ABI against numpy's stored-16-bit statement (a 1x1 product is one
einsum; tests/c8_util.py, tests/c8b_util.py), and nets with 1x1 layers against the unchanged stored-16-bit oracle.

Tolerances are the project's own for this arithmetic (operands rounded to the 16-bit type, exact products, fp32
accumulation, one rounding on store): stored 16-bit tensors 1e-3 of the largest entry for fp16 and 1e-2 for bf16
(tests/test_gpu_c8.py, tests/test_gpu_c8_bf16.py), fp32 results (dW, db) 2e-5 of the largest entry, nets TOL of
tests/test_gpu_c8_mean.py, schedules bit for bit.  Masks: bit for bit except at provable near-ties, the bound of
tests/test_gpu_c8.py with one tap, (C + 2) u (sum |x| |w| + |b|), u = 2^-24, and its cap (mismatches rarer than 1e-3)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import c8_util as U
from tests import c8b_util as CB
from tests.gpu_util import ROOT, act_code, assert_close, call, ctx, dev, empty, load_prms
from tests.test_gpu_c8_dropout import _oracle_16
from tests.test_gpu_c8_mean import GS, R16, TOL
from tests.test_gpu_f16 import _inject_draws
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

TOL16 = {"float16": 1e-3, "bfloat16": 1e-2}
SLOPE = .1


@pytest.fixture(params=["float16", "bfloat16"])
def dtype(request, monkeypatch):
    """The element type; for bfloat16 the oracle's stored-16-bit mode rounds to bf16 (tests/test_gpu_c8_mean.py)."""
    if request.param == "bfloat16":
        monkeypatch.setattr(O, "r16", CB.rbf16)
    ctx().set_matmul_dtype(request.param, GS[request.param])
    yield request.param
    monkeypatch.setattr(O, "r16", R16)


def _R(dtype):
    return CB.rbf16 if dtype == "bfloat16" else U.r16


def _rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)


def _c8(a, P, dtype):
    """(N, C, S, S) values -> device c8 tensor at pitch P (pad cells and channels past C zero)."""
    N, C, S, _ = a.shape
    buf = np.zeros((N, C, P, P))
    buf[:, :, :S, :S] = a
    return dev(CB.to_c8(buf) if dtype == "bfloat16" else U.to_c8(buf).view(np.uint16))


def _garbage(N, C, P):
    return dev(np.full((N, (C + 7) // 8, P, P, 8), 0x5555, np.uint16))


def _get(t, C, S, dtype):
    """Device c8 tensor -> its logical (N, C, S, S) values; every pad cell and every channel past C must be exactly 0."""
    raw = t.get_value()
    N, C8, P, _, _ = raw.shape
    bits = raw.transpose(0, 1, 4, 2, 3).reshape(N, C8 * 8, P, P)
    assert not bits[:, C:].any(), "channels past the last one must be written as 0"
    assert not bits[:, :, S:].any() and not bits[:, :, :, S:].any(), "pad cells must be written as 0"
    v = CB.bf16_value(bits) if dtype == "bfloat16" else bits.view(np.float16)
    return v[:, :C, :S, :S].astype(np.float64)


def _act(name, z):
    if name == "leaky":
        return U.leaky(z, SLOPE)
    if name == "linear":
        return z
    return np.tanh(z) if name == "tanh" else 1 / (1 + np.exp(-z))


def _act_grad_from_out(name, y):
    if name == "leaky":
        return U.leaky_grad_from_out(y, SLOPE)
    if name == "linear":
        return np.ones_like(y)
    return 1 - y * y if name == "tanh" else y * (1 - y)


def _code(name):
    return act_code({"leaky": "relu10"}.get(name, name))


def _assert_masks(gotm, bits, a, x, W16, b, C, fn_err):
    """tests/test_gpu_c8.py's _assert_masks_equal_up_to_provable_near_ties with one tap: (C + 2) u."""
    bad = gotm != bits
    print("mask bytes that differ: %d of %d" % (bad.sum(), bad.size))
    if not bad.any():
        return
    assert bad.mean() < 1e-3, "mask mismatches are not rare: %g" % bad.mean()
    absum = np.einsum("nchw,kc->nkhw", np.abs(x), np.abs(W16)) + np.abs(b)[None, :, None, None]
    tol = (C + 2) * 2.0 ** -24 * absum + fn_err
    N, K, H, _ = a.shape
    aw = a.reshape(N, K, H // 2, 2, H // 2, 2)
    tw = tol.reshape(N, K, H // 2, 2, H // 2, 2)
    m, tmax = aw.max(axis=(3, 5)), tw.max(axis=(3, 5))
    for n, k, i, j in zip(*np.nonzero(bad)):
        diff = int(gotm[n, k, i, j]) ^ int(bits[n, k, i, j])
        for e in range(4):
            if (diff >> e) & 1:
                gap = m[n, k, i, j] - aw[n, k, i, e >> 1, j, e & 1]
                assert gap <= 2 * tmax[n, k, i, j], ("window bit differs away from a tie", (n, k, i, j, e), gap)
        if diff & 0x30:
            assert abs(m[n, k, i, j]) <= tmax[n, k, i, j], ("sign bit differs away from zero", (n, k, i, j))
        assert diff & ~0x3f == 0, ("unused mask bits set", (n, k, i, j), gotm[n, k, i, j])


def _mask(mk, K, Sp):
    """Device mask (N, K8, Pp, Pp, 8) bytes -> (N, K, Sp, Sp); pad cells and channels past K must be 0."""
    raw = mk.get_value()
    N, K8, Pp, _, _ = raw.shape
    m = raw.transpose(0, 1, 4, 2, 3).reshape(N, K8 * 8, Pp, Pp)
    assert not m[:, K:].any() and not m[:, :, Sp:].any() and not m[:, :, :, Sp:].any()
    return np.ascontiguousarray(m[:, :K, :Sp, :Sp])


# (N, C, S, K), pitch (None: dense)
CASES = [((3, 16, 16, 32), None), ((2, 64, 64, 64), None), ((5, 24, 8, 40), None), ((2, 128, 32, 128), None),
         ((37, 3, 32, 32), None), ((9, 256, 16, 256), None), ((5, 1, 8, 40), None),
         ((6, 20, 28, 10), None), ((4, 192, 8, 10), None), ((2, 8, 16, 1), None),          # K % 8 != 0
         ((6, 20, 28, 10), 32), ((3, 16, 12, 24), 16), ((5, 24, 6, 40), 8),                 # padded pitch
         ((2100, 8, 16, 32), None), ((3, 100, 10, 70), None)]                               # many tiles, a partial last one
IDS = ["x".join(map(str, c)) + ("p%d" % p if p else "") for c, p in CASES]
GENERIC = [CASES[i] for i in (0, 2, 7, 10, 12)]
GENERIC_IDS = [IDS[i] for i in (0, 2, 7, 10, 12)]


def _ops(case, P, name, dtype, wgrad):
    (N, C, S, K), P = case, P or case[2]
    R, tol, gs = _R(dtype), TOL16[dtype], GS[dtype]
    act, prm = _code(name)
    assert ctx().lib.tn_c8_conv1_supported(N, C, S, P, K)
    rng = np.random.RandomState(0)
    x = R(rng.randn(N, C, S, S))
    W = (rng.randn(K, C) / np.sqrt(C)).astype(np.float32)
    b = (rng.randn(K) * .1).astype(np.float32)
    W16 = R(W)
    a = _act(name, np.einsum("nchw,kc->nkhw", x, W16) + b[None, :, None, None])
    xd, Wd, bd = _c8(x, P, dtype), dev(W.reshape(K, C, 1, 1)), dev(b)
    Sp, Pp = S // 2, P // 2
    # forward
    out = _garbage(N, K, P)
    call("tn_c8_conv1_fwd", xd.ptr, Wd.ptr, bd.ptr, out.ptr, None, N, C, S, P, K, act, prm, 0)
    e = _rel(_get(out, K, S, dtype), R(a))
    print("fwd: %.3g" % e)
    assert e < tol
    # forward + 2x2 max-pool + mask
    pm, bits = U.pool2(a)
    outp = _garbage(N, K, Pp)
    mk = dev(np.full((N, (K + 7) // 8, Pp, Pp, 8), 0x55, np.uint8))
    call("tn_c8_conv1_fwd", xd.ptr, Wd.ptr, bd.ptr, outp.ptr, mk.ptr, N, C, S, P, K, act, prm, 1)
    e = _rel(_get(outp, K, Sp, dtype), R(pm))
    print("fwd + pool: %.3g" % e)
    assert e < tol
    gotm = _mask(mk, K, Sp)
    _assert_masks(gotm, bits, a, x, W16, b, C, 0. if name in ("leaky", "linear") else 2.0 ** -21)
    outp2 = _garbage(N, K, Pp)
    call("tn_c8_conv1_fwd", xd.ptr, Wd.ptr, bd.ptr, outp2.ptr, None, N, C, S, P, K, act, prm, 1)      # mask NULL
    np.testing.assert_array_equal(outp2.get_value(), outp.get_value())
    # input gradient: prev_a given (exact zeros planted: the tie derivative) and NULL
    dz = R(gs * rng.randn(N, K, S, S) * 1e-3)
    if name in ("leaky", "linear"):
        prev = R(rng.randn(N, C, S, S))
        prev[0, 0, 0, :2] = 0
    else:
        prev = R(_act(name, 2 * rng.randn(N, C, S, S)))
    lin = np.einsum("nkhw,kc->nchw", dz, W16)
    dzd, pd = _c8(dz, P, dtype), _c8(prev, P, dtype)
    dxo = _garbage(N, C, P)
    call("tn_c8_conv1_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, N, C, S, P, K, pd.ptr, act, prm, 0, None)
    e = _rel(_get(dxo, C, S, dtype), R(lin * _act_grad_from_out(name, prev)))
    print("dgrad: %.3g" % e)
    assert e < tol
    dxo = _garbage(N, C, P)
    call("tn_c8_conv1_dgrad", dzd.ptr, Wd.ptr, dxo.ptr, N, C, S, P, K, None, act, prm, 0, None)
    assert _rel(_get(dxo, C, S, dtype), R(lin)) < tol
    # ... of a pooled block: dz = (window bit of the device's own mask) ? pooled gradient : 0
    g = R(gs * rng.randn(N, K, Sp, Sp) * 1e-3)
    gd = _c8(g, Pp, dtype)
    dzp = U.unpool_dz(g, gotm)
    dxo = _garbage(N, C, P)
    call("tn_c8_conv1_dgrad", gd.ptr, Wd.ptr, dxo.ptr, N, C, S, P, K, pd.ptr, act, prm, 1, mk.ptr)
    e = _rel(_get(dxo, C, S, dtype), R(np.einsum("nkhw,kc->nchw", dzp, W16) * _act_grad_from_out(name, prev)))
    print("dgrad pooled: %.3g" % e)
    assert e < tol
    if not wgrad:
        return
    # weight / bias gradient (fp32, the scale removed), plain and gathered; OVERWRITE
    x2 = x.transpose(1, 0, 2, 3).reshape(C, -1)
    for pooled, src, dzz in ((0, dzd, dz), (1, gd, dzp)):
        gW, gb = dev(np.full((K, C, 1, 1), 7., np.float32)), dev(np.full((K,), 7., np.float32))
        call("tn_c8_conv1_wgrad", xd.ptr, src.ptr, gW.ptr, gb.ptr, N, C, S, P, K, pooled, mk.ptr if pooled else None)
        eW = _rel(gW.get_value().reshape(K, C), dzz.transpose(1, 0, 2, 3).reshape(K, -1) @ x2.T / gs)
        eb = _rel(gb.get_value(), dzz.sum(axis=(0, 2, 3)) / gs)
        print("wgrad pooled %d: dW %.3g db %.3g" % (pooled, eW, eb))
        assert eW < 2e-5 and eb < 2e-5
    # the same input twice: the same bits
    g1, g2, b1, b2 = empty((K, C)), empty((K, C)), empty((K,)), empty((K,))
    call("tn_c8_conv1_wgrad", xd.ptr, dzd.ptr, g1.ptr, b1.ptr, N, C, S, P, K, 0, None)
    call("tn_c8_conv1_wgrad", xd.ptr, dzd.ptr, g2.ptr, b2.ptr, N, C, S, P, K, 0, None)
    np.testing.assert_array_equal(g1.get_value().view(np.uint32), g2.get_value().view(np.uint32))
    np.testing.assert_array_equal(b1.get_value().view(np.uint32), b2.get_value().view(np.uint32))


@pytest.mark.parametrize("case,P", CASES, ids=IDS)
def test_c8_conv1_ops_match_numpy(dtype, case, P):
    """Forward, forward + pool + mask, input gradient plain and pooled, weight gradient plain and pooled (and twice: the
    same bits) with the leaky-ReLU epilogue."""
    _ops(case, P, "leaky", dtype, True)


@pytest.mark.parametrize("name", ["tanh", "sigmoid", "linear"])
@pytest.mark.parametrize("case,P", GENERIC, ids=GENERIC_IDS)
def test_c8_conv1_ops_generic_activation(dtype, case, P, name):
    _ops(case, P, name, dtype, False)


def test_c8_conv1_planted_ties_set_every_window_bit(dtype):
    """A filter of zero weights (every window element is act(b)) and one all-equal input window: bits 0-3 all set."""
    N, C, S, K = 2, 16, 8, 16
    R = _R(dtype)
    rng = np.random.RandomState(3)
    x = R(rng.randn(N, C, S, S))
    x[1, :, 2:4, 4:6] = x[1, :, 2:3, 4:5]
    W = (rng.randn(K, C) / np.sqrt(C)).astype(np.float32)
    W[5] = 0
    b = (rng.randn(K) * .1).astype(np.float32)
    b[5] = .25
    act, prm = _code("leaky")
    out, mk = _garbage(N, K, S // 2), empty((N, K // 8, S // 2, S // 2, 8), np.uint8)
    call("tn_c8_conv1_fwd", _c8(x, S, dtype).ptr, dev(W).ptr, dev(b).ptr, out.ptr, mk.ptr, N, C, S, S, K, act, prm, 1)
    m = _mask(mk, K, S // 2)
    assert (m[:, 5] == 0x1f).all()
    assert ((m[1, :, 1, 2] & 0xf) == 0xf).all()
    a = U.leaky(np.einsum("nchw,kc->nkhw", x, R(W)) + b[None, :, None, None], SLOPE)
    _assert_masks(m, U.pool2(a)[1], a, x, R(W), b, C, 0.)
    assert (_get(out, K, S // 2, dtype)[:, 5] == .25).all()


def test_c8_conv1_ops_refuse_bad_arguments():
    ctx().set_matmul_dtype("float16", 4096.)
    x = dev(np.zeros((2, 1, 16, 16, 8), np.uint16))
    y = dev(np.full((2, 1, 16, 16, 8), 0x5555, np.uint16))
    m = dev(np.zeros((2, 1, 16, 16, 8), np.uint8))
    W, b = dev(np.zeros((8, 8), np.float32)), dev(np.zeros((8,), np.float32))
    assert not ctx().lib.tn_c8_conv1_supported(0, 8, 8, 8, 8) and not ctx().lib.tn_c8_conv1_supported(2, 8, 12, 24, 8)
    bad_geom = ((0, 8, 8, 8, 8), (2, 0, 8, 8, 8), (2, 8, 8, 8, 0), (2, 8, 12, 24, 8), (2, 8, 12, 8, 8), (2, 8, 0, 8, 8))
    for N, C, S, P, K in bad_geom:
        with pytest.raises(Exception):
            call("tn_c8_conv1_fwd", x.ptr, W.ptr, b.ptr, y.ptr, None, N, C, S, P, K, 0, 0., 0)
        with pytest.raises(Exception):
            call("tn_c8_conv1_dgrad", x.ptr, W.ptr, y.ptr, N, C, S, P, K, None, 0, 0., 0, None)
        with pytest.raises(Exception):
            call("tn_c8_conv1_wgrad", x.ptr, x.ptr, W.ptr, b.ptr, N, C, S, P, K, 0, None)
    g = (2, 8, 8, 8, 8)
    for args in ((None, W.ptr, b.ptr, y.ptr), (x.ptr, None, b.ptr, y.ptr), (x.ptr, W.ptr, None, y.ptr), (x.ptr, W.ptr, b.ptr, None)):
        with pytest.raises(Exception):
            call("tn_c8_conv1_fwd", *args, None, *g, 0, 0., 0)
    for args in ((None, W.ptr, y.ptr), (x.ptr, None, y.ptr), (x.ptr, W.ptr, None)):
        with pytest.raises(Exception):
            call("tn_c8_conv1_dgrad", *args, *g, None, 0, 0., 0, None)
    for args in ((None, x.ptr, W.ptr, b.ptr), (x.ptr, None, W.ptr, b.ptr), (x.ptr, x.ptr, None, b.ptr), (x.ptr, x.ptr, W.ptr, None)):
        with pytest.raises(Exception):
            call("tn_c8_conv1_wgrad", *args, *g, 0, None)
    odd = (2, 8, 7, 7, 8)
    with pytest.raises(Exception):
        call("tn_c8_conv1_fwd", x.ptr, W.ptr, b.ptr, y.ptr, m.ptr, *odd, 0, 0., 1)
    with pytest.raises(Exception):
        call("tn_c8_conv1_dgrad", x.ptr, W.ptr, y.ptr, *odd, None, 0, 0., 1, m.ptr)
    with pytest.raises(Exception):
        call("tn_c8_conv1_wgrad", x.ptr, x.ptr, W.ptr, b.ptr, *odd, 1, m.ptr)
    with pytest.raises(Exception):                    # a pooled gradient without its mask
        call("tn_c8_conv1_dgrad", x.ptr, W.ptr, y.ptr, *g, None, 0, 0., 1, None)
    with pytest.raises(Exception):
        call("tn_c8_conv1_wgrad", x.ptr, x.ptr, W.ptr, b.ptr, *g, 1, None)
    assert (y.get_value() == 0x5555).all()            # nothing was launched


def test_c8_conv1_cpu_backend_has_only_stubs():
    code = ("from theanet_amd.device import get_context\nc = get_context()\n"
            "assert c.lib.tn_c8_conv1_supported(2, 8, 8, 8, 8) == 0\n"
            "for name, args in (('tn_c8_conv1_fwd', (None,) * 5 + (2, 8, 8, 8, 8, 0, 0., 0)),\n"
            "                   ('tn_c8_conv1_dgrad', (None,) * 3 + (2, 8, 8, 8, 8, None, 0, 0., 0, None)),\n"
            "                   ('tn_c8_conv1_wgrad', (None,) * 4 + (2, 8, 8, 8, 8, 0, None))):\n"
            "    try:\n        c.call(name, *args)\n    except Exception as e:\n        print('STUB', name, e)\n"
            "    else:\n        raise SystemExit(name + ' ran')\n")
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.count("STUB") == 3, (r.stdout[-2000:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------------
# nets
# ---------------------------------------------------------------------------------------------------------------------
TP = {"SEED": 7, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}


def _conv(k, f, mode="same", act="relu10", stride=1):
    return ("ConvLayer", {"num_maps": k, "filter_sz": f, "stride": stride, "mode": mode, "actvn": act})


POOL = ("PoolLayer", {"pool_sz": 2})


def _nin(img=16):
    """Net (a): conv3(16) -> conv1(24) + pool -> DropOut -> conv3(32) -> conv1(32) -> conv1(10) -> Mean -> Softmax."""
    return [("InputLayer", {"img_sz": img, "num_maps": 3}), _conv(16, 3), _conv(24, 1, "valid"), POOL,
            ("DropOutLayer", {"pdrop": .25}), _conv(32, 3), _conv(32, 1), _conv(10, 1, "valid"), ("MeanLayer", {}),
            ("SoftmaxLayer", {"n_out": 10})]


def _first():
    """Net (c): conv1 as the first conv layer on 3x28x28 (pitch 32) + pool, conv3, a dense head (crop / embed)."""
    return [("InputLayer", {"img_sz": 28, "num_maps": 3}), _conv(12, 1, "valid"), POOL, _conv(16, 3),
            ("HiddenLayer", {"n_out": 64}), ("SoftmaxLayer", {"n_out": 10})]


def _net_prms(name, B):
    if name == "cifar_nin.prms":
        prms = load_prms(name, 32, batch=B)
        return prms["layers"], prms["training_params"], 32
    return (_nin(), dict(TP, BATCH_SZ=B), 16) if name == "nin" else (_first(), dict(TP, BATCH_SZ=B), 28)


def _tr(tp, dtype):
    return dict(tp, DTYPE=dtype, GRAD_SCALE=GS[dtype]) if dtype in GS else dict(tp, DTYPE=dtype)


def _data(B, img, n=2, seed=1):
    rng = np.random.RandomState(seed)
    return rng.rand(n * B, 3, img, img).astype(np.float32), rng.randint(0, 10, n * B).astype(np.int32)


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_c8_conv1_nets_build_16bit_resident(dt):
    """Fails on a build without the 1x1 route: construction asserts."""
    from theanet_amd import NeuralNet
    for layers in (_nin(), _first()):
        net = NeuralNet(copy.deepcopy(layers), _tr(TP, dt))
        convs = [l for l in net.tr_layers if type(l).__name__ == "ConvLayer"]
        assert convs and all(l.f16 for l in convs) and any(l.c8_1x1 for l in convs)
        assert all(l.f16 for l in net.te_layers if type(l).__name__ == "ConvLayer")
    assert NeuralNet(copy.deepcopy(_first()), _tr(TP, dt)).tr_layers[1].output.pitch == 32


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
@pytest.mark.parametrize("bad", [_conv(16, 1, "valid", stride=2), _conv(16, 5, "same"), _conv(16, 3, "valid")],
                         ids=["1x1-stride2", "5x5", "3x3-valid"])
def test_c8_conv1_other_shapes_still_refused_at_construction(dt, bad):
    from theanet_amd import NeuralNet
    layers = [("InputLayer", {"img_sz": 16, "num_maps": 3}), _conv(16, 3), bad, ("HiddenLayer", {"n_out": 32}),
              ("SoftmaxLayer", {"n_out": 10})]
    with pytest.raises(AssertionError):
        NeuralNet(copy.deepcopy(layers), _tr(TP, dt))
    net = NeuralNet(copy.deepcopy(layers), _tr(TP, "float32"))        # fp32 builds and runs as before
    x, y = _data(16, 16)
    cost = net.get_trin_model(x, y)(0)[0]
    assert np.isfinite(cost)


NETS = [("nin", 16), ("cifar_nin.prms", 16), ("first", 16)]


@pytest.mark.parametrize("name,B", NETS)
def test_c8_conv1_nets_match_16bit_oracle(dtype, name, B, monkeypatch):
    """Two training steps (forward, every gradient, momentum update, maxnorm) against the stored-16-bit oracle -- and
    measurably closer to it than to the fp32 oracle; net (a) then in test mode through get_test_model."""
    from theanet_amd import NeuralNet
    layers, tp, img = _net_prms(name, B)
    tr = _tr(tp, dtype)
    x, y = _data(B, img)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    convs = [l for l in net.tr_layers if type(l).__name__ == "ConvLayer"]
    assert convs and all(l.f16 for l in convs) and all(l.f16 for l in net.tr_layers if hasattr(l, "f16"))
    ora = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float16"), dtype=np.float64)
    ora32 = O.OracleNet(copy.deepcopy(layers), dict(tr, DTYPE="float32"), dtype=np.float64)
    _oracle_16(monkeypatch, ora)
    (rt, at), wat = TOL[dtype]
    fn = net.get_trin_model(x, y)
    for s in range(2):
        draws = _inject_draws(net, ora, B, 3, img)
        cost_w, lp_w, _ = ora.train_step(x[s * B:(s + 1) * B], y[s * B:(s + 1) * B], draws)
        cost, _, lp = fn(s)
        print("%s %s step %d: cost %.6f (oracle %.6f), max |dlogprob| %.3g" % (name, dtype, s, cost, cost_w, np.abs(lp - lp_w).max()))
        assert_close(lp, lp_w, rt, at, what="%s %s logprob step %d" % (name, dtype, s))
        assert_close(cost, cost_w, rt, at, what="%s %s cost step %d" % (name, dtype, s))
        np.testing.assert_array_equal(lp.argmax(1), lp_w.argmax(1))
        if s == 0:      # the mode is not a no-op: the fp32 oracle is measurably further away
            lp32 = ora32.forward(x[:B], True, draws)[0]
            assert np.abs(lp - lp_w).max() < .5 * np.abs(lp32 - lp_w).max() + 1e-6
    for i, (lyr, ol) in enumerate(zip(net.tr_layers, ora.L)):
        for j, w in enumerate(lyr.get_wts()):
            print("  w %d %d: max |d| %.3g of %.3g" % (i, j, np.abs(w - ol.params[j]).max(), np.abs(ol.params[j]).max()))
            assert_close(w, ol.params[j], rt, wat, what="%s %s w %d %d" % (name, dtype, i, j))
    if name == "nin":
        tfn = net.get_test_model(x, y, preds_feats=True)
        _, _, feats, preds = tfn(1)
        _, _, lp_w, preds_w = ora.test(x[B:2 * B], y[B:2 * B])
        assert_close(feats[:B], lp_w, rt, at, what="nin %s test logprob" % dtype)
        np.testing.assert_array_equal(preds[:B], preds_w)


def test_c8_conv1_net_schedules_are_bit_identical(dtype, monkeypatch):
    """Two steps in flight against one at a time, replayed (tn_net_plan_*) against interpreted steps: bit for bit."""
    from theanet_amd import NeuralNet
    B = 16
    x, y = _data(B, 16, n=6, seed=5)
    runs = []
    for pipe, plan in (("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")):
        monkeypatch.setenv("TN_PIPELINE", pipe)
        monkeypatch.setenv("TN_NET_PLAN", plan)
        net = NeuralNet(copy.deepcopy(_nin()), _tr(TP, dtype))
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
        assert replayed == (plan == "1"), (pipe, plan)
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


def test_c8_conv1_fp32_and_bf16_nets_share_weights():
    """The same net under DTYPE float32 and bfloat16: get_wts shapes agree ((K, C, 1, 1) for the 1x1 layers), and the
    fp32 net's weights, loaded into the bf16 net (allwts: the checkpoint route), give a first-step logprob within the
    bf16 net tolerance of the fp32 net's."""
    from theanet_amd import NeuralNet
    B = 16
    layers = [l for l in _nin() if l[0] != "DropOutLayer"]
    x, y = _data(B, 16)
    n32 = NeuralNet(copy.deepcopy(layers), _tr(TP, "float32"))
    other = NeuralNet(copy.deepcopy(layers), _tr(dict(TP, SEED=8), "bfloat16"))
    for a, b in zip(n32.tr_layers, other.tr_layers):
        assert [w.shape for w in a.get_wts()] == [w.shape for w in b.get_wts()]
    wts = n32.get_init_params()["allwts"]
    assert wts[2][0].shape == (24, 16, 1, 1)
    n16 = NeuralNet(copy.deepcopy(layers), _tr(dict(TP, SEED=8), "bfloat16"), allwts=wts)
    for a, b in zip(n32.tr_layers, n16.tr_layers):
        for u, v in zip(a.get_wts(), b.get_wts()):
            np.testing.assert_array_equal(u, v)
    lp32 = n32.get_trin_model(x, y)(0)[2]
    lp16 = n16.get_trin_model(x, y)(0)[2]
    (rt, at), _ = TOL["bfloat16"]
    print("max |dlogprob| bf16 - fp32: %.3g" % np.abs(lp16 - lp32).max())
    assert_close(lp16, lp32, rt, at, what="bf16 logprob against the fp32 net's")
