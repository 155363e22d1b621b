"""tn_elastic_convpool_fwd_mask (ElasticLayer resampling fused into the first conv block's forward; the first launch
of every mnist.prms training step) against the oracle, over the case table of tests/elconv_cases.py -- which
tests/test_elconv_cases_cpu.py proves to reach every instantiation, operand form and loop edge of the kernel.

Per case: the resampled image against the oracle's ElasticLayer with injected draws; conv + activation + max-pool and
the pooling mask against float64, computed from the device's own resampled image (so this leg does not lean on
tn_convpool_fwd_mask); bit equality with tn_elastic_apply + tn_convpool_fwd_mask; and the operand forms that must not
change a bit (mask == NULL, row offset and step counter by value or through device memory)."""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests import elconv_cases as EC
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)
from tests.test_gpu_elastic import _pack

pytestmark = pytest.mark.gpu

LEAD, TAIL = 2, 2                   # rows of x before the batch / after it (no rows after it in an 'at_end' case)
SEED, STEP, ROW_GLOBAL0 = 99, 3, 40
ONE = np.float32(1)


class _Setup:
    """Operands of one case on the device, and the launches over them."""

    def __init__(self, c):
        self.c = c
        self.pad_lo, (self.Ho, self.Wo), (self.Hp, self.Wp), _ = EC.geometry(c)
        assert ctx().lib.tn_elastic_convpool_supported(c.h, c.w, c.K, EC.F, self.pad_lo, self.Ho, self.Wo, EC.P, self.Hp,
                                                       self.Wp)
        rng = np.random.RandomState(100 * c.h + c.w + c.K)
        # at_end: the batch is the last N rows of x, so a gather one row too far lands in the guard band (NaN)
        self.x = rng.rand(LEAD + c.N + (0 if c.at_end else TAIL), 1, c.h, c.w).astype(np.float32)
        self.batch = self.x[LEAD:LEAD + c.N]
        self.W = (rng.randn(c.K, 1, 3, 3) / 3).astype(np.float32)
        self.b = rng.randn(c.K).astype(np.float32)
        self.kind, self.prm = act_code(c.act)
        self.xd, self.Wd, self.bd = dev(self.x), dev(self.W), dev(self.b)
        self.d_row0, self.d_step = dev(np.array([1], np.int64)), dev(np.array([1], np.uint32))
        self.st, self.d = EC.oracle_stage(c)
        self.mi = self.fy = self.fx = None
        if c.map != "none":          # the sample map as test_elastic_field_and_apply_match_oracle builds it
            e, hw = EC.ELASTIC, c.h * c.w
            self.mi, self.fy, self.fx = empty((hw,), np.int32), empty((hw,)), empty((hw,))
            tgt = empty((2, c.h, c.w), np.float64)
            call("tn_elastic_field", dev(_pack(self.d, c.h, c.w)).ptr, c.h, c.w, float(e["translation"]), float(e["zoom"]),
                 float(e["magnitude"]), e["sigma"], float(e["angle"]), int(c.map == "nearest"), self.mi.ptr, self.fy.ptr,
                 self.fx.ptr, tgt.ptr)
            self.target = tgt.get_value()
        self.fm = dev(self.d.flipmask.astype(np.uint8)) if c.flip == "flipmask" else None

    def source(self, form):
        """x, x_row0, d_row0: the batch starts at row LEAD either way"""
        return (self.xd.ptr, LEAD, None) if form == "host" else (self.xd.ptr, LEAD - 1, self.d_row0.ptr)

    def sample(self, pflip, form):
        """invert .. row_global0 (the arguments tn_elastic_apply shares with the fused launch); the step is STEP either way"""
        c, p = self.c, lambda a: a.ptr if a is not None else None
        step = (STEP, None) if form == "host" else (STEP - 1, self.d_step.ptr)
        return (c.invert, int(c.map == "nearest"), p(self.mi), p(self.fy), p(self.fx), pflip, p(self.fm), SEED, *step,
                ROW_GLOBAL0)

    def geom(self):
        return (self.c.K, EC.F, self.pad_lo, self.Ho, self.Wo, EC.P, self.Hp, self.Wp, self.kind, self.prm)

    def outputs(self, mask):
        c = self.c
        return (empty((c.N, 1, c.h, c.w)), empty((c.N, c.K, self.Hp, self.Wp)),
                empty((c.N, c.K, self.Hp, self.Wp), np.uint8) if mask else None)

    def fused(self, pflip, mask, row0, step):
        c = self.c
        xd, y, m = self.outputs(mask)
        call("tn_elastic_convpool_fwd_mask", *self.source(row0), xd.ptr, c.N, c.h, c.w, *self.sample(pflip, step),
             self.Wd.ptr, self.bd.ptr, y.ptr, m.ptr if mask else None, *self.geom())
        return xd.get_value(), y.get_value(), m.get_value() if mask else None

    def separate(self, pflip, row0, step):
        c = self.c
        xd, y, m = self.outputs(True)
        call("tn_elastic_apply", *self.source(row0), xd.ptr, c.N, 1, c.h, c.w, *self.sample(pflip, step))
        call("tn_convpool_fwd_mask", xd.ptr, self.Wd.ptr, self.bd.ptr, y.ptr, m.ptr, c.N, 1, c.h, c.w, *self.geom())
        return xd.get_value(), y.get_value(), m.get_value()


def _check_resampled(s, got):
    """The resampled image (no Philox flips in it) against the oracle's stage; returns the share of pixels compared
    exactly (nearest-neighbour maps: 1 elsewhere)."""
    c = s.c
    assert np.isfinite(got).all(), "%s: %d resampled pixels are not finite (read outside x?)" % (
        c.name, (~np.isfinite(got)).sum())
    if c.map == "none":                                     # a copy: x or 1 - x, then the injected flips; exact
        want = ONE - s.batch if c.invert else s.batch
        if c.flip == "flipmask":
            want = np.where(s.d.flipmask != 0, ONE - want, want)
        np.testing.assert_array_equal(got, want)
        return 1.0
    want, target = s.st.forward(s.batch, s.d)
    # the smoothed-noise plane is a float32 sum in a different order
    np.testing.assert_allclose(s.target, target, rtol=0, atol=2e-4)
    if c.map == "nearest":
        # identical except where a coordinate sits within 5e-4 of a rounding boundary
        safe = EC.nearest_safe(target, c.h, c.w)
        assert safe.mean() > .99, "%.3f %% of the pixels excluded (within 5e-4 of a rounding boundary)" % (
            100 * (1 - safe.mean()))
        np.testing.assert_array_equal(got[:, :, safe], want[:, :, safe],
                                      err_msg="compared %.2f %% of the pixels" % (100 * safe.mean()))
        return float(safe.mean())
    assert_close(got, want, atol=2e-3, rtol=0, what="%s: bilinear" % c.name)
    assert np.abs(got - want).mean() < 2e-5
    return 1.0


def _check_conv_block(s, xd, y, m):
    """y and the pooling mask against conv -> act -> pool in float64 from the device's own resampled image; returns the
    largest |y - want|."""
    c, Ho, Wo, Hp, Wp = s.c, s.Ho, s.Wo, s.Hp, s.Wp
    fa, _ = O.activation(c.act)
    a = fa(O.conv2d_fwd(xd.astype(np.float64), s.W.astype(np.float64), s.b.astype(np.float64), 1, c.mode))
    assert a.shape == (c.N, c.K, Ho, Wo)
    want_y = O.pool_fwd(a, 2, False)
    assert_close(y, want_y, what="%s: convpool fwd (mask)" % c.name)
    # the mask marks exactly the window elements equal to the pooled value
    ap = np.full((c.N, c.K, 2 * Hp, 2 * Wp), -np.inf)
    ap[:, :, :Ho, :Wo] = a
    for r in range(4):
        sub = ap[:, :, (r >> 1)::2, (r & 1)::2]
        bit = (m >> r) & 1
        clear = np.abs(sub - want_y) > 1e-5          # away from float ties the bit is determined
        assert np.all(bit[clear] == 0), "%s: mask bit %d set off the maximum" % (c.name, r)
        outside = np.isneginf(sub)                   # an element past Ho x Wo (the partial last row) is never the maximum
        assert not bit[outside].any(), "%s: mask bit %d set for an element outside the conv output" % (c.name, r)
    assert np.all((m & 15) > 0) and np.all(m < 64)
    assert np.array_equal((m >> 4) & 1, y > 0) and np.array_equal((m >> 5) & 1, y < 0)
    return float(np.abs(y - want_y).max())


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_elastic_convpool_fused_against_the_oracle(case):
    c, s = case, _Setup(case)
    pflip = EC.PFLIP if c.flip == "philox" else 0.0
    xd, y, m = s.fused(pflip, c.mask, c.row0, c.step)

    # the resampled image against the oracle (Philox flips have none: the oracle sees the pflip = 0 launch)
    plain = s.fused(0.0, False, c.row0, c.step)[0] if c.flip == "philox" else xd
    share = _check_resampled(s, plain)
    if c.flip == "philox":
        flipped = xd != plain
        np.testing.assert_array_equal(xd[flipped], (ONE - plain)[flipped],
                                      err_msg="a pixel is neither v nor 1 - v of the launch without flips")
        p, n = EC.PFLIP, xd.size
        assert abs(flipped.mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), "%.4f of %d pixels flipped, pflip %.2f" % (
            flipped.mean(), n, p)

    # forms that must not change a bit: the other mask form (one of the two has the mask the rules below look at) ...
    xd_o, y_o, m_o = s.fused(pflip, not c.mask, c.row0, c.step)
    assert np.array_equal(xd_o, xd) and np.array_equal(y_o, y), "mask == NULL changes the outputs"
    m = m if c.mask else m_o
    # ... the row offset by value or through d_row0, the step by value or through d_step
    other = {"host": "device", "device": "host"}
    for what, got in (("d_row0", s.fused(pflip, True, other[c.row0], c.step)),
                      ("d_step", s.fused(pflip, True, c.row0, other[c.step]))):
        assert np.array_equal(got[0], xd) and np.array_equal(got[1], y) and np.array_equal(got[2], m), \
            "%s: the other form of %s changes the outputs" % (c.name, what)

    # conv + act + pool and the mask against float64, from the device's own resampled image
    err = _check_conv_block(s, xd, y, m)

    # bit equality with the separate ops (same seed, step and row_global0 under Philox flips)
    xd_s, y_s, m_s = s.separate(pflip, c.row0, c.step)
    assert np.array_equal(xd_s, xd), "%s: resampled image differs from tn_elastic_apply's" % c.name
    assert np.array_equal(y_s, y) and np.array_equal(m_s, m), "%s: y / mask differ from tn_convpool_fwd_mask's" % c.name

    print("elconv %-12s %s | compared exactly %.2f %% | max |y - want| %.3g" % (c.name, EC.describe(c), 100 * share, err))
