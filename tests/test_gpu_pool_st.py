"""PoolLayer ``stride`` on the device, op by op through the C-ABI: tn_c8_pool_st_fwd / tn_c8_pool_st_bwd (the 16-bit
conv stack, both element types) and tn_pool_st_fwd / tn_pool_st_bwd (fp32) against the numpy statement of
tests/test_pool_st_cpu.py.

Everything on the 16-bit ops is an equality of bit patterns.  Forward: the stored pattern that a row-major scan of the
clipped window keeps when it replaces on strict > (of equal values -- +0 and -0 included -- the first one's).  Backward:
the fp32 sum of the statement (row-major window order, started by its first term), rounded once to nearest even to the
element type; +0 patterns wherever there is no term, pad cells and channels past C included.  With stride = window the
new ops give the bits of tn_c8_pool_* / tn_pool_*.  The fp32 forward and linear backward are equalities too; with an
activation derivative riding on the backward the bounds are assert_close's defaults, as tests/test_gpu_kernels.py's
test_pool_fwd_bwd."""
import numpy as np
import pytest

from tests import test_gpu_c8_pool as GP
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.test_gpu_c8_dropout import _from_raw, _to_raw, _value32
from tests.test_gpu_c8_mean import _bits
from tests.test_gpu_c8_pool import dtype  # noqa: F401  (fixture: the element type, set on the context)
from tests.test_pool_st_cpu import covered, out_side, pool_st_bwd, pool_st_fwd
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

GARBAGE = 0x5555

# (N, C, S, P, p, st, ignore_border): the smallest with a ragged C; 3 against 2 outputs with a clipped last window; st > p:
# gaps and a one-pixel clipped window; nine windows on a pixel; a stride-1 window of two; the run-time loops; many blocks; a
# dense input pitch that is no power of two; an output of 65 pixels at a dense pitch -- and the (2, 1) and run-time
# instantiations on dense pitches that are no powers of two, input and output (tests/test_c8_pool_st_cpu.py).
CASES = [(1, 3, 5, 8, 3, 2, False), (37, 24, 6, 8, 3, 2, False), (37, 24, 6, 8, 3, 2, True), (5, 8, 7, 8, 2, 3, False),
         (5, 8, 7, 8, 2, 3, True), (3, 9, 6, 8, 3, 1, False), (2, 16, 12, 16, 2, 1, True), (2, 8, 11, 16, 5, 2, False),
         (129, 8, 6, 8, 3, 2, False), (1, 8, 66, 66, 3, 2, False), (1, 3, 131, 131, 3, 2, False),
         (1, 8, 67, 67, 2, 1, False), (1, 8, 70, 70, 4, 1, True)]
IDS = ["x".join(str(int(c)) for c in case) for case in CASES]


def pool_st_geom(case):
    """(N, C, S, P, p, st, So, Po) of a case: the output side of its border mode at the pitch rule of the layer."""
    from theanet_amd.device import c8_pool_pitch
    N, C, S, P, p, st, ib = case
    So = out_side(S, p, st, ib)
    return N, C, S, P, p, st, So, c8_pool_pitch(So)


def _inputs(case, dtype):
    """Stored patterns of x from a small grid with both zeros (ties inside and across windows are common) and of gout
    with mixed exponents and a few zeros of both signs (the order of the sum is visible)."""
    N, C, S, P, p, st, So, Po = pool_st_geom(case)
    rng = np.random.default_rng(100 + CASES.index(case))
    v = rng.integers(-4, 5, (N, C, S, S)) * .5
    flat = v.reshape(-1)
    k = max(1, flat.size // 12)
    flat[rng.integers(0, flat.size, k)] = rng.choice([0., -0.], k)
    xb = _bits(v, dtype).reshape(N, C, S, S)
    g = rng.standard_normal((N, C, So, So)) * 2.0 ** rng.integers(-6, 7, (N, C, So, So))
    flat = g.reshape(-1)
    k = max(1, flat.size // 16)
    flat[rng.integers(0, flat.size, k)] = rng.choice([0., -0.], k)
    return xb, _bits(g, dtype).reshape(N, C, So, So)


def _fwd_bits(xb, xv, p, st, So):
    """The pattern a row-major scan with strict > keeps: the first of the window's maxima (argmax returns the first)."""
    N, C, S, _ = xb.shape
    out = np.empty((N, C, So, So), np.uint16)
    for i in range(So):
        for j in range(So):
            sl = (slice(None), slice(None), slice(i * st, min(S, i * st + p)), slice(j * st, min(S, j * st + p)))
            wv, wb = xv[sl].reshape(N, C, -1), xb[sl].reshape(N, C, -1)
            out[:, :, i, j] = np.take_along_axis(wb, wv.argmax(-1)[..., None], -1)[..., 0]
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_c8_pool_st_ops_are_exact(dtype, case):
    N, C, S, P, p, st, So, Po = geom = pool_st_geom(case)
    ib, C8 = case[6], (C + 7) // 8
    assert ctx().lib.tn_c8_pool_st_supported(*geom)
    xb, gb = _inputs(case, dtype)
    xv, gv = _value32(xb, dtype), _value32(gb, dtype)
    want = pool_st_fwd(xv, p, st, ib)
    assert want.shape == (N, C, So, So)
    want_bits = _fwd_bits(xb, xv, p, st, So)
    np.testing.assert_array_equal(_value32(want_bits, dtype), want)

    x = dev(_to_raw(xb, P))
    y = dev(np.full((N, C8, Po, Po, 8), GARBAGE, np.uint16))
    call("tn_c8_pool_st_fwd", x.ptr, y.ptr, *geom)
    np.testing.assert_array_equal(y.get_value(), _to_raw(want_bits, Po), err_msg="forward %s %s" % (dtype, case))

    g = dev(_to_raw(gb, Po))
    gin = dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16))
    call("tn_c8_pool_st_bwd", x.ptr, y.ptr, g.ptr, gin.ptr, *geom)
    gsum = pool_st_bwd(xv, gv, p, st, ib)
    assert gsum.dtype == np.float32
    gwant = _bits(gsum.astype(np.float64), dtype).reshape(N, C, S, S)
    # ... bit for bit: the rounded sums, and the all-zero pattern in untied, uncovered and pad cells and channels past C
    np.testing.assert_array_equal(gin.get_value(), _to_raw(gwant, P), err_msg="backward %s %s" % (dtype, case))
    got = _from_raw(gin.get_value())
    assert not got[:, C:].any() and not got[:, :, S:].any() and not got[:, :, :, S:].any()


def test_the_cases_hold_what_they_are_for():
    """Conditions on the inputs, asserted on the statement's own result: over the case list a position is fed by two or
    more windows (and the order of its sum matters), a window holds its maximum twice, a zero maximum is held as +0 and
    as -0 in one window, a position lies in no window, and a -0 gradient arrives alone."""
    seen = dict(multi=False, order=False, tie_in_window=False, both_zeros=False, uncovered=False, neg_zero=False)
    for case in CASES:
        N, C, S, P, p, st, So, Po = pool_st_geom(case)
        xb, gb = _inputs(case, "float16")
        xv, gv = _value32(xb, "float16"), _value32(gb, "float16")
        cnt = pool_st_bwd(xv, np.ones((N, C, So, So), np.float32), p, st, case[6])
        seen["multi"] |= bool((cnt >= 2).any())
        fwd_sum = pool_st_bwd(xv, gv, p, st, case[6])
        rev = pool_st_bwd(xv[:, :, ::-1, ::-1], gv[:, :, ::-1, ::-1], p, st, case[6])[:, :, ::-1, ::-1] \
            if (S - p) % st == 0 else None                      # (the mirrored pool has the same windows: the reverse order)
        if rev is not None:
            seen["order"] |= bool((fwd_sum != rev).any())
        y = pool_st_fwd(xv, p, st, case[6])
        for i in range(min(So, 4)):
            for j in range(min(So, 4)):
                sl = (slice(None), slice(None), slice(i * st, min(S, i * st + p)), slice(j * st, min(S, j * st + p)))
                tie = xv[sl] == y[:, :, i:i + 1, j:j + 1]
                seen["tie_in_window"] |= bool((tie.sum((2, 3)) >= 2).any())
                zb = np.where(tie & (xv[sl] == 0), xb[sl], 1)
                seen["both_zeros"] |= bool(((zb == 0).any((2, 3)) & (zb == 0x8000).any((2, 3))).any())
        cov = covered(S, p, st, So)
        assert (cov == 0).any() == (st > p or (case[6] and (S - p) % st != 0)), case
        seen["uncovered"] |= bool(st > p and (cov[:(So - 1) * st] == 0).any())
        seen["neg_zero"] |= bool(((cnt == 1) & np.signbit(fwd_sum) & (fwd_sum == 0)).any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("case", GP.CASES, ids=["x".join(str(int(c)) for c in case) for case in GP.CASES])
def test_c8_stride_equal_to_window_gives_the_bits_of_the_old_ops(dtype, case):
    """tests/test_gpu_c8_pool.py's geometries: tn_c8_pool_st_* with st = p against tn_c8_pool_*, raw tensors bit for bit."""
    N, C, S, P, p, So, Po = GP.pool_geom(case)
    C8 = (C + 7) // 8
    rng = np.random.default_rng(GP.CASES.index(case))
    xb = GP._pool_input(rng, case, dtype)
    g = rng.standard_normal((N, C, So, So)) * 2.0 ** rng.integers(-6, 7, (N, C, So, So))
    g.reshape(-1)[::7] = -0.
    x, gd = dev(_to_raw(xb, P)), dev(_to_raw(_bits(g, dtype).reshape(N, C, So, So), Po))
    ys = [dev(np.full((N, C8, Po, Po, 8), GARBAGE, np.uint16)) for _ in range(2)]
    gs = [dev(np.full((N, C8, P, P, 8), GARBAGE, np.uint16)) for _ in range(2)]
    assert ctx().lib.tn_c8_pool_st_supported(N, C, S, P, p, p, So, Po)
    call("tn_c8_pool_fwd", x.ptr, ys[0].ptr, N, C, S, P, p, So, Po)
    call("tn_c8_pool_st_fwd", x.ptr, ys[1].ptr, N, C, S, P, p, p, So, Po)
    np.testing.assert_array_equal(ys[1].get_value(), ys[0].get_value())
    call("tn_c8_pool_bwd", x.ptr, ys[0].ptr, gd.ptr, gs[0].ptr, N, C, S, P, p, So, Po)
    call("tn_c8_pool_st_bwd", x.ptr, ys[1].ptr, gd.ptr, gs[1].ptr, N, C, S, P, p, p, So, Po)
    assert gs[0].get_value().any()
    np.testing.assert_array_equal(gs[1].get_value(), gs[0].get_value())


# (N C, H, W, p, st, ignore_border): H != W, overlap, gaps, nine windows on a pixel, a window larger than the map
F32_CASES = [(15, 7, 10, 3, 2, False), (15, 7, 10, 3, 2, True), (15, 10, 7, 2, 3, False), (15, 8, 5, 2, 3, True),
             (6, 6, 9, 3, 1, False), (700, 5, 4, 2, 1, True), (3, 4, 3, 5, 2, False), (2, 33, 17, 7, 3, False)]


def _f32_inputs(case):
    NC, H, W, p, st, ib = case
    rng = np.random.default_rng(F32_CASES.index(case))
    x = (rng.integers(-6, 7, (NC, 1, H, W)) * .25).astype(np.float32)          # (a grid: ties inside and across windows)
    x.reshape(-1)[::11] = -0.
    Ho, Wo = out_side(H, p, st, ib), out_side(W, p, st, ib)
    dy = (rng.standard_normal((NC, 1, Ho, Wo)) * 10.0 ** rng.integers(-3, 4, (NC, 1, Ho, Wo))).astype(np.float32)
    return x, dy, Ho, Wo


@pytest.mark.parametrize("case", F32_CASES, ids=["x".join(str(int(c)) for c in case) for case in F32_CASES])
def test_fp32_pool_st_ops(case):
    NC, H, W, p, st, ib = case
    x, dy, Ho, Wo = _f32_inputs(case)
    xd, dyd = dev(x), dev(dy)
    y = dev(np.full((NC, 1, Ho, Wo), 7e7, np.float32))
    call("tn_pool_st_fwd", xd.ptr, y.ptr, NC, H, W, p, st, Ho, Wo)
    want = pool_st_fwd(x, p, st, ib)
    np.testing.assert_array_equal(y.get_value(), want)
    dx = dev(np.full(x.shape, 7e7, np.float32))
    call("tn_pool_st_bwd", xd.ptr, y.ptr, dyd.ptr, dx.ptr, NC, H, W, p, st, Ho, Wo, 0, 0.0)
    gwant = pool_st_bwd(x, dy, p, st, ib)
    assert (pool_st_bwd(x, np.ones_like(dy), p, st, ib) >= 2).any() or p <= st or Ho * Wo == 1     # (overlap: real sums)
    np.testing.assert_array_equal(dx.get_value().view(np.uint32), gwant.view(np.uint32))
    kind, prm = act_code("relu05")
    call("tn_pool_st_bwd", xd.ptr, y.ptr, dyd.ptr, dx.ptr, NC, H, W, p, st, Ho, Wo, kind, prm)
    g = np.where(x > 0, 1.0, np.where(x < 0, .05, 1.05)).astype(np.float32)
    assert_close(dx.get_value(), gwant * g, what="pool_st bwd * act'")


@pytest.mark.parametrize("H,W,p,ib", [(7, 7, 2, False), (7, 10, 2, True), (9, 6, 3, False), (8, 8, 2, False), (5, 4, 7, False)])
def test_fp32_stride_equal_to_window_gives_the_bits_of_the_old_pair(H, W, p, ib):
    rng = np.random.default_rng(H * 10 + p)
    x = (rng.integers(-6, 7, (12, 1, H, W)) * .25).astype(np.float32)
    Ho, Wo = (H // p, W // p) if ib else (-(-H // p), -(-W // p))
    dy = rng.standard_normal((12, 1, Ho, Wo)).astype(np.float32)
    dy.reshape(-1)[::5] = -0.
    xd, dyd = dev(x), dev(dy)
    ys, dxs = [empty((12, 1, Ho, Wo)) for _ in range(2)], [empty(x.shape) for _ in range(4)]
    call("tn_pool_fwd", xd.ptr, ys[0].ptr, 12, H, W, p, Ho, Wo)
    call("tn_pool_st_fwd", xd.ptr, ys[1].ptr, 12, H, W, p, p, Ho, Wo)
    np.testing.assert_array_equal(ys[1].get_value().view(np.uint32), ys[0].get_value().view(np.uint32))
    for k, (kind, prm) in enumerate(((0, 0.0), act_code("relu05"))):
        call("tn_pool_bwd", xd.ptr, ys[0].ptr, dyd.ptr, dxs[2 * k].ptr, 12, H, W, p, Ho, Wo, kind, prm)
        call("tn_pool_st_bwd", xd.ptr, ys[1].ptr, dyd.ptr, dxs[2 * k + 1].ptr, 12, H, W, p, p, Ho, Wo, kind, prm)
        np.testing.assert_array_equal(dxs[2 * k + 1].get_value().view(np.uint32), dxs[2 * k].get_value().view(np.uint32))


def test_pool_st_ops_refuse_bad_arguments():
    from theanet_amd import _lib
    ctx().set_matmul_dtype("float16", 4096.)
    try:
        x = dev(np.full((4, 1, 8, 8, 8), 0x3c00, np.uint16))
        out = dev(np.zeros((4, 1, 8, 8, 8), np.uint16))
        ok = (4, 8, 6, 8, 3, 2, 3, 8)
        assert ctx().lib.tn_c8_pool_st_supported(*ok)
        for args in ((None, out.ptr), (x.ptr, None)):
            with pytest.raises(_lib.BackendError, match="tn_c8_pool_st_fwd: bad arguments"):
                call("tn_c8_pool_st_fwd", *args, *ok)
        for args in ((None, x.ptr, x.ptr, out.ptr), (x.ptr, None, x.ptr, out.ptr), (x.ptr, x.ptr, None, out.ptr),
                     (x.ptr, x.ptr, x.ptr, None)):
            with pytest.raises(_lib.BackendError, match="tn_c8_pool_st_bwd: bad arguments"):
                call("tn_c8_pool_st_bwd", *args, *ok)
        bad = [(4, 8, 6, 8, 1, 2, 3, 8),                # p = 1
               (4, 8, 6, 8, 65, 2, 1, 8),               # p > 64
               (4, 8, 6, 8, 3, 0, 3, 8),                # st = 0
               (4, 8, 6, 8, 3, 65, 1, 8),               # st > 64
               (4, 8, 6, 8, 3, 2, 4, 8),                # So neither of the two sides
               (4, 8, 6, 8, 3, 2, 0, 8),                # So = 0
               (4, 8, 5, 8, 7, 2, 0, 8),                # ignore_border with a window larger than the map: no side
               (4, 8, 6, 8, 3, 2, 3, 2),                # Po < So
               (4, 8, 6, 7, 3, 2, 3, 8),                # P neither S nor a power of two
               (4, 8, 6, 8, 3, 2, 3, 6),                # Po neither So nor a power of two
               (0, 8, 6, 8, 3, 2, 3, 8), (4, 0, 6, 8, 3, 2, 3, 8),
               (1 << 20, 64, 64, 64, 3, 2, 32, 32)]     # 2^32 cells
        for geom in bad:
            assert not ctx().lib.tn_c8_pool_st_supported(*geom), geom
            with pytest.raises(_lib.BackendError, match="window %d stride %d" % geom[4:6]):
                call("tn_c8_pool_st_fwd", x.ptr, out.ptr, *geom)
            with pytest.raises(_lib.BackendError, match="maps of %d pixels at pitch %d" % geom[2:4]):
                call("tn_c8_pool_st_bwd", x.ptr, x.ptr, x.ptr, out.ptr, *geom)
        assert not out.get_value().any()                     # nothing was launched on the way
    finally:
        ctx().set_matmul_dtype("float32")
    xf, of = dev(np.ones((2, 1, 6, 6), np.float32)), dev(np.zeros((2, 1, 6, 6), np.float32))
    for geom in ((2, 6, 6, 3, 2, 4, 3), (2, 6, 6, 3, 2, 3, 4), (2, 6, 6, 0, 2, 3, 3), (2, 6, 6, 3, 0, 3, 3), (0, 6, 6, 3, 2, 3, 3),
                 (2, 6, 6, 3, 2, 0, 3)):
        with pytest.raises(_lib.BackendError, match="tn_pool_st_fwd: bad arguments"):
            call("tn_pool_st_fwd", xf.ptr, of.ptr, *geom)
        with pytest.raises(_lib.BackendError, match="tn_pool_st_bwd: bad arguments"):
            call("tn_pool_st_bwd", xf.ptr, xf.ptr, xf.ptr, of.ptr, *geom, 0, 0.0)
    with pytest.raises(_lib.BackendError, match="tn_pool_st_fwd: bad arguments"):
        call("tn_pool_st_fwd", None, of.ptr, 2, 6, 6, 3, 2, 3, 3)
    with pytest.raises(_lib.BackendError, match="tn_pool_st_bwd: bad arguments"):
        call("tn_pool_st_bwd", xf.ptr, xf.ptr, None, of.ptr, 2, 6, 6, 3, 2, 3, 3, 0, 0.0)
    assert not of.get_value().any()
