"""ElasticLayer per_image (tn_elastic_apply_img / tn_c8_elastic_apply_img: a distortion field for every image of the
minibatch, include/theanet_hip.h) -- per-op checks against the unchanged oracle run image by image on the draws the
device used, and whole nets on every training schedule.  tests/test_elastic_img_cpu.py runs the same cases against the
CPU backend.

The smoothing of this mode is the separable fp32 form of the reference's filter, so the coordinates differ from the
oracle's (2-D sum, float64 accumulation) by rounding.  The bound is derived, not tuned: with el = fl32(mag * noise) and
A(p) = (|el| correlated with elastic_filter(sigma)) in float64,
    b(p) = 2 (2 sigma + 1) 2^-23 A(p) + 2^-20        (two passes of 2 sigma + 1 fused multiply-adds whose partial sums
                                                      are bounded by A, the rounding of the 1-D filter values; 2^-20
                                                      covers the float64 chain and the rounding of the oracle's sum)
    tc = 2 max(zoom, 1 / zoom) max_p b(p)            (zoom scales an error, the rotation mixes the two: |c| + |s| <= 2)
"""
import functools

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from oracle import theanet_oracle as O
from tests.gpu_util import call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu
SEED = 0x51ED_1234_5678

# (N, C, h = w, sigma, magnitude, translation, zoom, angle)
CASES = [
    (5, 1, 9, 2, 8, 1, 1.2, 10),
    (3, 3, 12, 3, 20, 0, 1, 0),
    (4, 1, 10, 6, 25, 2, 1.1, 5),         # filter longer than the map
    (6, 1, 28, 15, 60, 2, 1.1, 5),
    (2, 3, 64, 4, 30, 2, 1.1, 5),         # more LDS than a launch gets by default
    (5, 2, 9, 1, 0, 2, 1, 0),             # translation only
    (5, 2, 9, 1, 0, 0, 1.2, 10),          # zoom + angle only
]
IDS = ["9s2", "12s3c3", "10s6", "28s15", "64s4c3", "transl", "zoomrot"]


def _args(case, nearest, invert, pflip=0.0, fm=None, step=3, d_step=None, rg0=7, draws_in=None, draws_out=None, target=None):
    N, C, hw, sigma, mag, tr, zoom, ang = case
    return (N, C, hw, hw, int(invert), int(nearest), float(tr), float(zoom), float(mag), int(sigma), float(ang), float(pflip),
            fm.ptr if fm is not None else None, SEED, step, d_step.ptr if d_step is not None else None, rg0,
            draws_in.ptr if draws_in is not None else None, draws_out.ptr if draws_out is not None else None,
            target.ptr if target is not None else None)


def _inputs(case):
    N, C, hw = case[:3]
    rng = np.random.RandomState(hw * 100 + N)
    x = rng.rand(N + 4, C, hw, hw).astype(np.float32)
    fm = (rng.rand(N, C, hw, hw) < .1).astype(np.uint8)
    return x, fm


def _device_run(case, nearest, invert):
    """Generated draws, an injected flip mask, x_row0 = 1, *d_row0 = 2, row_global0 = 7: (x rows used, mask, draws, target, out)."""
    N, C, hw = case[:3]
    x, fm = _inputs(case)
    nd = ctx().lib.tn_elastic_draws_count(hw, hw)
    draws, tgt, out = empty((N, nd)), empty((N, 2, hw, hw), np.float64), empty((N, C, hw, hw))
    d_row0, d_step = dev(np.array([2], np.int64)), dev(np.array([5], np.uint32))
    call("tn_elastic_apply_img", dev(x).ptr, 1, d_row0.ptr, out.ptr,
         *_args(case, nearest, invert, fm=dev(fm), d_step=d_step, draws_out=draws, target=tgt))
    return x[3:3 + N], fm, draws.get_value(), tgt.get_value(), out.get_value()


def _draws_of(d, hw):
    e = O.ElasticDraws()
    e.transln, e.origin_u, e.zoom_u = d[0:2].reshape(2, 1, 1), d[2:4].reshape(2, 1, 1), d[4:6].reshape(2, 1, 1)
    e.theta_u, e.noise = d[6], d[8:].reshape(2, hw, hw)
    return e


@functools.lru_cache(maxsize=None)
def _oracle(case, draws_bytes):
    """Per image: the oracle's un-clipped coordinates and the derived coordinate tolerance tc (module docstring)."""
    N, C, hw, sigma, mag, tr, zoom, ang = case
    draws = np.frombuffer(draws_bytes, np.float32).reshape(N, -1)
    prm = dict(translation=tr, zoom=zoom, magnitude=mag, sigma=sigma, angle=ang)
    targets, tcs = [], []
    for n in range(N):
        d = _draws_of(draws[n], hw)
        targets.append(O.elastic_field(hw, hw, prm, d))
        A = 0.0
        if mag:
            el = np.abs((O._tconst(mag) * d.noise).astype(np.float32)).astype(np.float64)
            pad = np.pad(el, ((0, 0), (sigma, sigma), (sigma, sigma)))
            win = sliding_window_view(pad, (2 * sigma + 1, 2 * sigma + 1), axis=(1, 2))
            A = np.einsum("chwuv,uv->chw", win, O.elastic_filter(sigma).astype(np.float64)).max()
        b = 2 * (2 * sigma + 1) * 2.0 ** -23 * A + 2.0 ** -20
        tcs.append(2 * max(zoom, 1 / zoom) * b)
    return np.stack(targets), np.array(tcs)


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("nearest", [True, False], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_per_image_fields_match_the_oracle_image_by_image(case, nearest, invert):
    N, C, hw = case[:3]
    x, fm, draws, target, out = _device_run(case, nearest, invert)
    assert np.isfinite(draws).all() and np.isfinite(target).all()
    want_t, tc = _oracle(case, draws.tobytes())
    err = np.abs(target - want_t).reshape(N, -1).max(axis=1)
    print("coordinates: max |target - oracle| per image", err, "tc", tc)
    assert (err <= tc).all(), (err, tc)
    xi = (np.float32(1) - x) if invert else x
    exempt = 0
    for n in range(N):
        want = O.elastic_apply(xi[n:n + 1], want_t[n], nearest, fm[n:n + 1].astype(np.float32))[0]
        if nearest:
            cy, cx = np.clip(want_t[n, 0], 0, hw - 1 - .001), np.clip(want_t[n, 1], 0, hw - 1 - .001)
            near = (np.abs(cy - np.floor(cy) - .5) <= tc[n]) | (np.abs(cx - np.floor(cx) - .5) <= tc[n])
            exempt += int(near.sum())
            np.testing.assert_array_equal(out[n][:, ~near], want[:, ~near], err_msg="image %d" % n)
        else:
            bound = 2 * tc[n] * float(xi[n].max() - xi[n].min()) + 4 * 2.0 ** -23 * float(np.abs(xi[n]).max())
            d = np.abs(out[n].astype(np.float64) - want.astype(np.float64)).max()
            print("image %d: max |out - oracle| %.3e, bound %.3e" % (n, d, bound))
            assert d <= bound, (n, d, bound)
    if nearest:
        share = exempt / float(N * hw * hw)
        print("exempted (a coordinate within tc of a rounding boundary): %.4f %%" % (100 * share))
        assert share <= .01


@pytest.mark.parametrize("nearest", [True, False], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_injected_draws_reproduce_the_generated_run(case, nearest):
    """draws_in = the first call's draws_out: the same output bit for bit (and the same draws_out, target)."""
    N, C, hw = case[:3]
    x, fm, draws, target, out = _device_run(case, nearest, 1)
    xs, fms = _inputs(case)
    d2, t2, o2 = empty(draws.shape), empty(target.shape, np.float64), empty(out.shape)
    call("tn_elastic_apply_img", dev(xs).ptr, 3, None, o2.ptr,
         *_args(case, nearest, 1, fm=dev(fms), step=99, rg0=0, draws_in=dev(draws), draws_out=d2, target=t2))
    np.testing.assert_array_equal(o2.get_value(), out)
    np.testing.assert_array_equal(d2.get_value(), draws)
    np.testing.assert_array_equal(t2.get_value(), target)


def test_every_image_has_its_own_field():
    """N = 5 with a magnitude: no two images share their coordinates (a field shared by the batch fails here), and the
    draws have the distributions of tn_elastic_draws."""
    case = (5, 1, 28, 15, 60, 2, 1.1, 5)
    _, _, draws, target, _ = _device_run(case, True, 0)
    for i in range(5):
        for j in range(i + 1, 5):
            assert not np.array_equal(target[i], target[j]), (i, j)
            assert not np.array_equal(draws[i, :8], draws[j, :8]) and not np.array_equal(draws[i, 8:], draws[j, 8:])
    assert np.all(np.abs(draws[:, 0:2]) <= 1) and np.all(np.abs(draws[:, 4:7]) <= 1)
    assert np.all((draws[:, 2:4] >= .25) & (draws[:, 2:4] <= .75))
    noise = draws[:, 8:].ravel()
    assert abs(noise.mean()) < .05 and abs(noise.std() - 1) < .05


@pytest.mark.parametrize("nearest", [True, False], ids=["nearest", "bilinear"])
def test_draws_follow_the_global_image_index_not_the_shard(nearest):
    """One call of N = 8 equals two calls of 4 with row_global0 0 and 4 (flip noise drawn on the device too), a repeat
    call is bit-identical, and another step value changes every image's draws."""
    case8, case4 = (8, 2, 12, 3, 20, 2, 1.1, 5), (4, 2, 12, 3, 20, 2, 1.1, 5)
    hw = 12
    x = np.random.RandomState(1).rand(8, 2, hw, hw).astype(np.float32)
    xd = dev(x)
    nd = ctx().lib.tn_elastic_draws_count(hw, hw)
    d_step = dev(np.array([11], np.uint32))

    def run(case, row0, rg0, step=3):
        N = case[0]
        draws, tgt, out = empty((N, nd)), empty((N, 2, hw, hw), np.float64), empty((N, 2, hw, hw))
        call("tn_elastic_apply_img", xd.ptr, row0, None, out.ptr,
             *_args(case, nearest, 1, pflip=.1, step=step, d_step=d_step, rg0=rg0, draws_out=draws, target=tgt))
        return draws.get_value(), tgt.get_value(), out.get_value()

    whole = run(case8, 0, 0)
    again = run(case8, 0, 0)
    lo, hi = run(case4, 0, 0), run(case4, 4, 4)
    for k in range(3):
        np.testing.assert_array_equal(again[k], whole[k])
        np.testing.assert_array_equal(np.concatenate([lo[k], hi[k]]), whole[k])
    plain = empty((8, 2, hw, hw))
    call("tn_elastic_apply_img", xd.ptr, 0, None, plain.ptr, *_args(case8, nearest, 1, step=3, d_step=d_step, rg0=0))
    assert .05 < np.mean(plain.get_value() != whole[2]) < .15           # the flips happened: about pflip of the elements
    other = run(case8, 0, 0, step=4)
    for n in range(8):
        assert not np.array_equal(other[0][n, :8], whole[0][n, :8]) and not np.array_equal(other[0][n, 8:], whole[0][n, 8:])


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("C,hw,nearest,invert,mode", [
    (3, 32, False, 0, "philox"), (3, 32, True, 1, "mask"), (1, 28, False, 1, "none"), (11, 16, True, 0, "mask"),
    (4, 64, False, 0, "philox"),
])
def test_c8_output_is_the_rounded_fp32_output(C, hw, nearest, invert, mode, dtype):
    """tn_c8_elastic_apply_img stores exactly the 16-bit rounding of tn_elastic_apply_img's value in the first conv
    layer's c8 cells, zero beyond C, for halfs and bf16."""
    N, rng = 5, np.random.RandomState(3)
    case = (N, C, hw, 4, 30, 2, 1.1, 5)
    x = rng.rand(N + 2, C, hw, hw).astype(np.float32)
    fm = dev((rng.rand(N, C, hw, hw) < .2).astype(np.uint8)) if mode == "mask" else None
    a = _args(case, nearest, invert, pflip=.15 if mode == "philox" else 0.0, fm=fm, step=3,
              d_step=dev(np.array([7], np.uint32)), rg0=40)
    xd, row0 = dev(x), dev(np.array([1], np.int64))
    out = empty((N, C, hw, hw))
    call("tn_elastic_apply_img", xd.ptr, 1, row0.ptr, out.ptr, *a)
    C8 = (C + 7) // 8
    out16 = empty((N, C8, hw * hw, 8), np.uint16)
    ctx().set_matmul_dtype(dtype)
    call("tn_c8_elastic_apply_img", xd.ptr, 1, row0.ptr, out16.ptr, *a)
    got = out16.get_value()
    want = np.zeros((N, C8 * 8, hw * hw), np.float32)
    want[:, :C] = out.get_value().reshape(N, C, hw * hw)
    want = want.reshape(N, C8, 8, hw * hw).transpose(0, 1, 3, 2)
    if dtype == "float16":
        np.testing.assert_array_equal(got.view(np.float16), want.astype(np.float16))
    else:
        u = np.ascontiguousarray(want).view(np.uint32)
        bf = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # round to nearest even
        np.testing.assert_array_equal(got, bf)
    assert np.ptp(out.get_value()) > .5                                    # (a picture, not a constant)


def test_bad_arguments_are_refused_and_the_predicate_has_its_edges():
    from theanet_amd._lib import BackendError
    lib = ctx().lib
    sup = lib.tn_elastic_img_supported
    for hw in (2, 9, 28, 64):
        for C in (1, 4):
            for sigma in (0, 1, 15, 32):
                assert sup(C, hw, hw, sigma)
    assert not sup(0, 28, 28, 4) and not sup(1, 1, 28, 4) and not sup(1, 28, 1, 4) and not sup(1, 28, 28, -1)

    def lds(h, w, s):            # the arithmetic of include/theanet_hip.h
        return 32 + 4 * (4 * h * (w | 1) + 2 * s + 2 + 8)
    assert lds(64, 64, 32) == 66888 > 64 * 1024
    assert lds(100, 100, 271) == 160 * 1024 and sup(3, 100, 100, 271) and not sup(3, 100, 100, 272)
    assert lds(102, 102, 0) > 160 * 1024 and not sup(1, 102, 102, 0) and sup(1, 101, 101, 0)

    case = (2, 1, 12, 3, 20, 2, 1.1, 5)
    x = dev(np.zeros((2, 1, 12, 12), np.float32))
    sentinel = np.full((2, 1, 12, 12), 7.0, np.float32)
    out = dev(sentinel)
    bad = [
        ("tn_elastic_apply_img", (None, 0, None, out.ptr) + _args(case, 1, 0)),                        # NULL x
        ("tn_elastic_apply_img", (x.ptr, 0, None, None) + _args(case, 1, 0)),                          # NULL out
        ("tn_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args((0,) + case[1:], 1, 0)),            # N = 0
        ("tn_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args((2, 1, 1) + case[3:], 1, 0)),       # 1 x 1 maps
        ("tn_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args(case[:3] + (0,) + case[4:], 1, 0)),  # magnitude, sigma 0
        ("tn_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args(case[:6] + (0.0, 5), 1, 0)),         # zoom 0
        ("tn_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args((2, 1, 102, 3) + case[4:], 1, 0)),   # too large for LDS
        ("tn_c8_elastic_apply_img", (x.ptr, 0, None, out.ptr) + _args((2, 1, 9) + case[3:], 1, 0)),     # 81 pixels: no c8 cells
    ]
    for name, args in bad:
        with pytest.raises(BackendError, match=r"rc=-2"):
            call(name, *args)
    np.testing.assert_array_equal(out.get_value(), sentinel)          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# whole nets: 12 x 12 x 1 (16 x 16 where the c8 tensor has to be unpadded), batch 8, Conv 8 'same' 3x3, Pool 2, Hidden 16
# without dropout, Softmax 5
# ---------------------------------------------------------------------------------------------------------------------
B = 8
EL = dict(translation=2, zoom=1.1, magnitude=20, sigma=3, pflip=.05, angle=5, nearest=False, invert_image=True)
REST = [("ConvLayer", {"num_maps": 8, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
        ("PoolLayer", {"pool_sz": 2}),
        ("HiddenLayer", {"n_out": 16, "pdrop": 0}),
        ("SoftmaxLayer", {"n_out": 5})]


def _tiny(img=12, dtype=None, first=None, **tp):
    import copy
    layers = [first or ("ElasticLayer", dict(EL, img_sz=img, per_image=True))] + copy.deepcopy(REST)
    tr = dict({"SEED": 7, "BATCH_SZ": B, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 1}, **tp)
    if dtype:
        tr["DTYPE"] = dtype
    return layers, tr


def _data(n_batches, img=12, seed=4):
    rng = np.random.RandomState(seed)
    return rng.rand(n_batches * B, 1, img, img).astype(np.float32), rng.randint(0, 5, n_batches * B).astype(np.int32)


def _weights(net):
    return [w.copy() for l in net.tr_layers for w in l.get_wts()]


def _replayed(fn):
    pl = getattr(fn, "_plan", None)
    if fn.__class__.__name__ == "_PipeTrainFn" and fn._seq is not None:
        pl = fn._seq._plan
    return pl is not None and pl.ready


@pytest.mark.parametrize("img,dtype", [(12, "float32"), pytest.param(12, "bfloat16", id="12-bf16-pitch"),
                                       pytest.param(16, "bfloat16", id="16-bf16-c8"), pytest.param(16, "float16", id="16-f16-c8")])
def test_training_on_per_image_fields_equals_training_on_the_recorded_batches(img, dtype):
    """Three steps with a per-image layer and injected draws, then an InputLayer net built with the first net's initial
    weights on the distorted batches the first net saw: the same weights bit for bit.  (16-bit stacks: 12 x 12 maps live
    at a padded pitch -- the stage writes fp32 and the conv layer packs it; 16 x 16 maps take tn_c8_elastic_apply_img.)"""
    import copy
    from theanet_amd import NeuralNet
    layers, tr = _tiny(img, None if dtype == "float32" else dtype)
    x, y = _data(3, img)
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    w0 = copy.deepcopy(net.get_init_params()["allwts"])
    first = net.tr_layers[0]
    assert first.img_field and first.fused_conv is None and not hasattr(first, "_maps")
    assert (first._c8_consumer is not None) == (dtype != "float32" and img == 16)
    fn = net.get_trin_model(x, y)
    rng, rec = np.random.RandomState(8), []
    for s in range(3):
        first.inject(transln=rng.uniform(-1, 1, (B, 2)), origin_u=rng.uniform(.25, .75, (B, 2)), zoom_u=rng.uniform(-1, 1, (B, 2)),
                     theta_u=rng.uniform(-1, 1, B), noise=rng.randn(B, 2, img, img), flipmask=rng.rand(B, 1, img, img) < .05)
        assert net._injecting()
        fn(s)
        rec.append(first._c8_consumer.x16.get_value() if first._c8_consumer is not None else first.output.get_value())
    rec = np.concatenate(rec)
    assert np.isfinite(rec).all() and np.abs(rec - (1 - x)).max() > .1           # distorted
    for n in range(1, B):                                                         # ... every image by draws of its own
        assert not np.array_equal(rec[n] - (1 - x[n]), rec[0] - (1 - x[0]))
    net2 = NeuralNet([("InputLayer", {"img_sz": img, "num_maps": 1})] + copy.deepcopy(layers[1:]), dict(tr), w0)
    fn2 = net2.get_trin_model(rec, y)
    for s in range(3):
        fn2(s)
    wa, wb = _weights(net), _weights(net2)
    assert len(wa) == len(wb) == 6
    for a, b, a0 in zip(wa, wb, [w for l in w0 for w in l]):
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(a, a0)                                          # (it trained)


def _run_schedule(monkeypatch, pipe, plan, steps=30, order=None, **tp):
    import copy
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", pipe)
    monkeypatch.setenv("TN_NET_PLAN", plan)
    layers, tr = _tiny(**tp)
    x, y = _data(6, tp.get("img", 12))
    if order is not None and order[0] == "physical":
        x, y = x[order[1]], y[order[1]]
    net = NeuralNet(copy.deepcopy(layers), dict(tr))
    fn = net.get_trin_model(x, y)
    if order is not None and order[0] == "device":
        fn.set_order(order[1])
    outs = []
    for s in range(steps):
        if s in (2, steps - 1):       # (a read right before step 6 would leave the first recorded step another state)
            outs.append(fn(s % 6))
        else:
            fn.enqueue(s % 6)
    return outs, _weights(net), _replayed(fn), net


def _same_runs(a, b):
    for u, v in zip(a[0], b[0]):
        assert np.float32(u[0]).view(np.uint32) == np.float32(v[0]).view(np.uint32), (u[0], v[0])
        np.testing.assert_array_equal(u[2], v[2])
    for u, v in zip(a[1], b[1]):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("tp", [{}, {"WT_AVG": .9}, pytest.param({"dtype": "bfloat16", "img": 16}, id="bf16")], ids=lambda t: "-".join(t) or "plain")
def test_per_image_net_is_the_same_on_every_schedule(tp, monkeypatch):
    """Generated draws: interpreted against recorded steps (tn_net_step) and one step at a time against two steps in
    flight, costs / log-probabilities / weights bit for bit (30 steps: a plan is recorded from step 6 on, 6 would never
    replay one)."""
    runs = {(p, r): _run_schedule(monkeypatch, p, r, **tp) for p in ("0", "1") for r in ("0", "1")}
    for p in ("0", "1"):
        assert runs[(p, "1")][2] and not runs[(p, "0")][2]
    ref = runs[("0", "0")]
    for k, run in runs.items():
        _same_runs(run, ref)
    if "WT_AVG" in tp:
        for (p, r), run in runs.items():
            for u, v in zip(run[3].get_avg_wts(), ref[3].get_avg_wts()):
                for a, b in zip(u, v):
                    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_per_image_net_on_a_shuffled_row_order(pipe, monkeypatch):
    """set_order (SHUFFLE): the draws follow the position in the minibatch, so a device-resident row order equals an
    in-order run on physically permuted data, bit for bit."""
    perm = np.random.RandomState(2).permutation(6 * B)
    a = _run_schedule(monkeypatch, pipe, "1", order=("device", perm))
    b = _run_schedule(monkeypatch, pipe, "1", order=("physical", perm))
    _same_runs(a, b)
    assert a[2] and b[2]


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_step_cost_and_fn_stay_equal_when_mixed(pipe, monkeypatch):
    """The cost ring with a per-image layer: c = step_cost, e = enqueue, f = fn(i), D = drain_costs -- between two
    drains every step_cost() step's cost arrives once, in order, equal to fn(i)'s of a reference run."""
    import copy
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_PIPELINE", pipe)
    layers, tr = _tiny()
    x, y = _data(6)
    ref_net, net = (NeuralNet(copy.deepcopy(layers), dict(tr)) for _ in range(2))
    ref_fn, fn = ref_net.get_trin_model(x, y), net.get_trin_model(x, y)
    want, got = [], {}
    for s, kind in enumerate("c" * 9 + "e" * 3 + "c" * 7 + "f" + "c" * 6 + "D" + "cccecc" + "D"):
        if kind == "D":
            for k, v in fn.drain_costs():
                assert k not in got
                got[k] = v
            assert sorted(got) == list(range(len(want)))
            np.testing.assert_array_equal(np.array([got[k] for k in range(len(want))], np.float32), np.array(want, np.float32))
            want, got = [], {}
            continue
        c = ref_fn(s % 6)[0]
        if kind == "c":
            want.append(c)
            for k, v in fn.step_cost(s % 6):
                assert k not in got
                got[k] = v
        elif kind == "e":
            fn.enqueue(s % 6)
        else:
            assert fn(s % 6)[0] == c
    for a, b in zip(_weights(ref_net), _weights(net)):
        np.testing.assert_array_equal(a, b)


def _calls_of_a_step(prms_name, monkeypatch):
    import ast
    import copy
    import os
    from tests.gpu_util import ROOT
    from theanet_amd import NeuralNet
    monkeypatch.setenv("TN_NET_PLAN", "0")
    with open(os.path.join(ROOT, "params", prms_name)) as fh:
        prms = ast.literal_eval(fh.read())
    prms["layers"][0][1]["img_sz"] = 28
    prms["training_params"].update(SEED=555555, BATCH_SZ=16)
    rng = np.random.RandomState(0)
    x, y = rng.rand(32, 1, 28, 28).astype(np.float32), rng.randint(0, 10, 32).astype(np.int32)
    net = NeuralNet(copy.deepcopy(prms["layers"]), dict(prms["training_params"]))
    fn = net.get_trin_model(x, y)
    for i in range(3):
        fn.enqueue(i % 2)
    c, calls = ctx(), []
    assert c.rec is None                 # (TN_NET_PLAN=0: nobody else is recording)
    c.rec = calls                        # Context.call appends (entry point, arguments) while it executes them
    try:
        fn.enqueue(1)
    finally:
        c.rec, c.rec_tainted = None, False
    names = [name for name, _ in calls]
    cost = fn.fetch()[0]
    assert np.isfinite(cost)
    return prms, net, names


def test_headline_net_with_per_image_fields_leaves_the_fused_block_alone(monkeypatch):
    """params/mnist_img.prms = mnist.prms + 'per_image' (28 x 28 x 1, the shape of the fused elastic + conv block): a
    step calls tn_elastic_apply_img and neither the fused entry point nor anything that builds a batch field."""
    import ast
    import os
    from tests.gpu_util import ROOT
    from theanet_amd import _lib
    prms, net, names = _calls_of_a_step("mnist_img.prms", monkeypatch)
    with open(os.path.join(ROOT, "params", "mnist.prms")) as fh:
        base = ast.literal_eval(fh.read())
    assert prms["layers"][0][1].pop("per_image") is True
    prms["layers"][0][1].pop("img_sz")
    assert prms["layers"] == base["layers"]
    assert names.count("tn_elastic_apply_img") == 1, names
    batch_field = {"tn_elastic_convpool_fwd_mask", "tn_rider_elastic_field", "tn_step_tail", "tn_elastic_field_gen",
                   "tn_elastic_field", "tn_elastic_apply", "tn_c8_elastic_apply"}
    assert not batch_field & set(names), names
    assert " Fields:PerImage" in net.tr_layers[0].representation
    if _lib.backend() == "hip":            # the shared-field net does take the fused block: the check above can fail
        _, _, shared = _calls_of_a_step("mnist.prms", monkeypatch)
        assert "tn_elastic_convpool_fwd_mask" in shared and "tn_elastic_apply_img" not in shared, shared


def test_refusals_and_what_stays_as_it_was(monkeypatch):
    import copy
    from theanet_amd import NeuralNet
    # (1) a shape the kernel does not take
    layers, tr = _tiny(first=("ElasticLayer", dict(EL, img_sz=128, per_image=True)))
    with pytest.raises(ValueError, match=r"per_image: 1 maps of 128 x 128 with sigma 3 do not fit.*tn_elastic_img_supported"):
        NeuralNet(layers, tr)
    # (2) in the middle of a net with a trainable layer below it
    mid = [("InputLayer", {"img_sz": 12, "num_maps": 1}),
           ("ConvLayer", {"num_maps": 4, "filter_sz": 3, "stride": 1, "mode": "same", "actvn": "relu10"}),
           ("ElasticLayer", dict(translation=2, per_image=True))] + copy.deepcopy(REST[1:])
    with pytest.raises(ValueError, match=r"per_image in the middle of a net with a trainable layer below it"):
        NeuralNet(mid, _tiny()[1])
    # ... the same layer with per_image and NO field (flip noise only) is today's layer
    mid[2] = ("ElasticLayer", dict(pflip=.1, per_image=True))
    assert not NeuralNet(mid, _tiny()[1]).tr_layers[2].img_field
    # (3) in the middle of a net with nothing trainable below it: fine, and every image is distorted by its own draws
    layers, tr = _tiny(first=("ColorLayer", {"img_sz": 12, "num_maps": 1, "balance": 1.2, "gamma": 1.2}))
    layers.insert(1, ("ElasticLayer", dict(translation=2, magnitude=20, sigma=3, per_image=True)))
    net = NeuralNet(layers, tr)
    x, y = _data(2)
    fn = net.get_trin_model(x, y)
    assert np.isfinite(fn(0)[0]) and np.isfinite(fn(1)[0])
    el = net.tr_layers[1]
    assert el.img_field and not hasattr(el, "_maps")
    # (4) debugout names the way to the coordinates
    with pytest.raises(AssertionError, match=r"tn_elastic_apply_img.*target"):
        el.debugout
    # (5) per_image without a field: accepted, today's path (same calls, same bits), only the representation says so
    outs = []
    for key in ({}, {"per_image": False}, {"per_image": True}):
        layers, tr = _tiny(first=("ElasticLayer", dict(img_sz=12, pflip=.1, invert_image=True, **key)))
        net = NeuralNet(layers, tr)
        fn = net.get_trin_model(x, y)
        fn(0)
        first = net.tr_layers[0]
        assert not first.img_field and hasattr(first, "_maps")
        outs.append((first.representation, first.output.get_value(), fn(1)[0]))
    assert outs[0][0] == outs[1][0] and "Fields" not in outs[0][0] and outs[2][0] == outs[0][0] + " Fields:PerImage"
    for o in outs[1:]:
        np.testing.assert_array_equal(o[1], outs[0][1])
        assert o[2] == outs[0][2]
    assert " Fields" not in str(NeuralNet(*_tiny(first=("ElasticLayer", dict(EL, img_sz=12)))))
    # the test version of a per-image layer is the shared one's
    net = NeuralNet(*_tiny())
    assert net.te_layers[0].representation == NeuralNet(*_tiny(first=("ElasticLayer", dict(EL, img_sz=12)))).te_layers[0].representation
