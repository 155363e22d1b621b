"""Per-op parity of the row and elementwise kernels around the conv / FC stack -- tn_head_rows (heads.hip),
tn_softmax_nll_cost (loss.hip), the colour ops, tn_elastic_apply_bwd, tn_aux_mix and tn_copy_cols (color.hip) --
each called through the C-ABI with inputs of its own and compared with the float64 oracle on the same float32
inputs, at the shapes where their loops take a second trip, their LDS carve-up grows and their block counts
leave one block.

Tolerances are the project's (tests/test_gpu_kernels.py): rtol 1e-4 / atol 1e-5 for fp32 values; atol 1e-7 for
gradients that carry inv_batch at B >= 1000; index outputs, untouched cells and exact-zero gradients bit-exact;
sums whose order the kernel does not fix (dcenters, the all-to-one-cell scatter) atol = max(1e-5, 2e-6 * scale).

Paths and the case that reaches each:
  * a lane loop's second trip (c += 64) in every head ........ test_head_rows / test_centered_head_rows, n > 64
  * ncls + 1 on both sides of 64 (RBF) ....................... test_centered_head_rows ncls 63 (64 columns), 64 (65)
  * wargmax with two maxima on one lane (c, c + 64) .......... the planted row 2 of test_head_rows, the duplicated
                                                               center of test_centered_head_rows
  * elastic bwd p += 256 with a ragged tail / at the LDS limit test_elastic_apply_bwd 28 x 28 / 128 x 128
  * the cost kernel's four-trip partial sum .................. test_softmax_nll_cost 'headline' (1024 blocks)
  * a second launch on a used workspace ...................... test_softmax_nll_cost, every case
  * label offsets through y_row0 and d_row0 .................. every head and cost case (3 + 2)
  * the NULL-output forms .................................... every head case (y NULL; only da NULL)"""
import numpy as np
import pytest

from oracle import theanet_oracle as O
from tests.gpu_util import act_code, assert_close, call, ctx, dev, empty
from tests.guard_util import device_guard  # noqa: F401  (autouse: guard bands and 0xFF poison on every device buffer)

pytestmark = pytest.mark.gpu

HEAD_SOFTMAX, HEAD_EXPLOSS, HEAD_HINGE, HEAD_LOGIT, HEAD_RBF = range(5)
LOSS_CODE = {"nll": 0, "nllsq": 1, "nlltrunc": 2, "hinge": 3, "exp": 4}
Y_ROW0, D_ROW0 = 3, 2          # the labels of row r sit at y[Y_ROW0 + D_ROW0 + r]


def filled(shape, dtype=np.float32):
    """A device array of 0xff bytes: a float the kernel forgets to write reads back as NaN, an index as -1."""
    a = empty(shape, dtype)
    a.fill_bytes(0xff)
    return a


def untouched(a):
    return a.view(np.uint8) == 0xff


def no_tile_to_refuse():
    """The C++ / OpenMP backend keeps class scores and scatter targets in host memory: it has no on-chip tile whose
    size it could refuse.  Every other backend must refuse what does not fit."""
    return ctx().backend == "cpu"


def labels(rng, B, n):
    """B + 5 labels of which the last B are used; they include class 0 and class n - 1."""
    y = rng.randint(0, n, B + Y_ROW0 + D_ROW0).astype(np.int32)
    lab = y[Y_ROW0 + D_ROW0:]
    lab[0], lab[-1] = 0, n - 1
    return y, lab


def check_pred(got, score, planted=()):
    """argmax is compared exactly.  A random row may be left out only if the float64 reference's two largest scores
    are closer than 1e-5 * max(1, |best|) (the rule of test_fc_softmax_nll_fused); with the committed seeds none is.
    Planted rows hold exact ties (also in the reference): the first index must win."""
    want = score.argmax(1)
    close = np.zeros(len(score), bool)
    if score.shape[1] > 1:
        top = np.sort(score, 1)[:, -2:]
        with np.errstate(invalid="ignore"):
            close = (top[:, 1] - top[:, 0]) < 1e-5 * np.maximum(1, np.abs(top[:, 1]))
    close[list(planted)] = False
    n_excluded = int(close.sum())
    assert n_excluded == 0
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ #
# 1. tn_head_rows
# ------------------------------------------------------------------------------------------------------------ #

DIRECT_HEADS = ["softmax-nll", "softmax-nllsq", "softmax-nll40", "softmax-hinge", "softmax-exp", "exploss", "hinge"]
# n = 1; one trip; exactly one trip (64); a second trip of one lane (65); a third trip (130); eight trips (457)
# B = 1; fewer than a block's four rows; a partial last block; many blocks
DIRECT_SHAPES = [(1, 1), (10, 6), (3, 64), (257, 65), (10, 130), (3, 457)]


def plant_rows(z, lab):
    """Rows with deliberate exact ties and exact-zero hinge margins; returns their indices."""
    B, n = z.shape
    planted = []
    if B >= 1:
        z[0, :] = 1.5                                   # all equal
        planted.append(0)
    if B >= 3 and n >= 2:
        c = n // 2                                      # two maxima 1 apart
        z[1, c] = z[1, c + 1 if c + 1 < n else c - 1] = np.abs(z[1]).max() + 1
        planted.append(1)
    if B >= 3 and n > 64:
        z[2, 0] = z[2, 64] = np.abs(z[2]).max() + 1     # two maxima exactly 64 apart: one lane, two trips
        planted.append(2)
    zero_margins = 0
    if B >= 10 and n >= 4:
        # hinge margins a[c] + 1 - a[y] that are exactly 0 (0.5 + 1 - 1.5): the rule t >= 0 is inclusive
        y = lab[3]
        cols = [c for c in range(0, n, 3) if c != y]
        z[3, cols] = 0.5
        z[3, y] = 1.5
        zero_margins = len(cols)
    return planted, zero_margins


def run_head(head, code, prm, a, y, B, n, ncol, centers=None, ncls=0, junk=0.0, act=(0, 0.0), inv=0.25,
             with_y=True, with_da=True, with_feat=False, dcent=None):
    o = dict(logprob=filled((B, ncol)), pred=filled((B,), np.int32),
             rowloss=filled((B,)) if with_y else None, rowstat=filled((B,)) if with_y else None,
             da=filled((B, n)) if with_y and with_da else None, feat=filled((B, n)) if with_feat else None)
    ptr = lambda d: d.ptr if d is not None else None
    call("tn_head_rows", head, code, prm, a.ptr, ptr(centers), ncls, y.ptr if with_y else None, Y_ROW0,
         dev(np.array([D_ROW0], np.int64)).ptr if with_y else None, ptr(o["feat"]), o["logprob"].ptr, ptr(o["rowloss"]),
         o["pred"].ptr, ptr(o["rowstat"]), ptr(o["da"]), ptr(dcent), B, n, inv, junk, act[0], act[1])
    return {k: v.get_value() for k, v in o.items() if v is not None}


def check_null_forms(full, run):
    """y = NULL (test graphs: no rowloss, rowstat, da) and da = NULL alone: what remains is bit-identical."""
    no_y = run(with_y=False)
    assert set(no_y) == set(full) - {"rowloss", "rowstat", "da"}
    for k, v in no_y.items():
        np.testing.assert_array_equal(v, full[k], err_msg="y = NULL: " + k)
    no_da = run(with_da=False)
    assert set(no_da) == set(full) - {"da"}
    for k, v in no_da.items():
        np.testing.assert_array_equal(v, full[k], err_msg="da = NULL: " + k)


@pytest.mark.parametrize("B,n", DIRECT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", DIRECT_HEADS)
def test_head_rows(kind, B, n):
    """SOFTMAX with its five losses, EXPLOSS and HINGE: logprob, feat, pred, rowloss, rowstat and da against the
    oracle's head; mean(rowloss) is its cost.  The hinge head's inclusive rule t >= 0 is pinned by planted exact-zero
    margins here, the truncated NLL's by test_head_rows_truncated_nll_kink_is_inclusive (its t depends on the rounding
    of logf, so no input alone places it); on the random rows the reference has no margin within 1e-6 of a kink."""
    rng = np.random.RandomState(1000 * DIRECT_HEADS.index(kind) + 7 * B + n)
    head, _, loss = kind.partition("-")
    z = (3 * rng.randn(B, n)).astype(np.float32)
    y, lab = labels(rng, B, n)
    if loss == "nll40" and n > 6:
        z[::2, :] -= 4                                  # both sides of the threshold P(label) = 0.4 with many classes
        z[np.arange(0, B, 2), lab[::2]] += 12
    planted, zero_margins = plant_rows(z, lab)
    z64, r = z.astype(np.float64), np.arange(B)
    feat_w = None
    if head == "softmax":
        lp_w, _, stat_w, cost_w, dz_w = O.softmax_head(z64, lab, loss)
        name, thr = O.parse_loss(loss)
        hd, code, prm = HEAD_SOFTMAX, LOSS_CODE[name], float(np.log(thr)) if thr else 0.0
        if name == "nlltrunc":
            assert np.abs(np.log(thr) - lp_w[r, lab]).min() >= 1e-6          # no row sits on the kink
            assert B < 10 or {True, False} == set(lp_w[r, lab] > np.log(thr))   # ... and both sides occur
    elif head == "exploss":
        lp_w, _, stat_w, cost_w, dz_w, feat_w = O.exploss_head(z64, lab)
        hd, code, prm = HEAD_EXPLOSS, LOSS_CODE["exp"], 0.0
    else:
        lp_w, _, stat_w, cost_w, dz_w = O.hinge_head(z64, lab)
        hd, code, prm = HEAD_HINGE, LOSS_CODE["hinge"], 0.0
        t = z64 + 1 - z64[r, lab][:, None]
        t[r, lab] = 1
        assert ((t != 0) & (np.abs(t) < 1e-6)).sum() == 0                    # no random margin near the kink
        assert (t == 0).sum() == zero_margins                                # the planted ones are exactly on it
    rl_w = O.head_rowloss(head, z64, lab, loss)
    assert abs(rl_w.mean() - cost_w) <= 1e-12 * max(1, abs(cost_w))
    inv = 0.25                                          # da is d cost / d a * (inv_batch * B); B-independent scale
    zd, yd = dev(z), dev(y)
    run = lambda **kw: run_head(hd, code, prm, zd, yd, B, n, n, inv=inv, with_feat=head == "exploss", **kw)
    got = run()
    what = "%s B=%d n=%d " % (kind, B, n)
    assert_close(got["logprob"], lp_w, what=what + "logprob")
    if feat_w is not None:
        assert_close(got["feat"], feat_w, what=what + "feat")
    check_pred(got["pred"], z64, planted)               # these heads take argmax of the input itself
    assert_close(got["rowloss"], rl_w, what=what + "rowloss")
    assert_close(got["rowloss"].astype(np.float64).mean(), cost_w, what=what + "cost")
    assert_close(got["rowstat"], stat_w, what=what + "rowstat")
    assert_close(got["da"], dz_w * B * inv, what=what + "da")
    check_null_forms(got, run)


@pytest.mark.parametrize("n", [6, 65])
def test_head_rows_truncated_nll_kink_is_inclusive(n):
    """t = loss_param - logprob[y] exactly 0: the threshold is the float32 logprob[y] that a first call returned (the
    kernel forms logprob[y] and the stored logprob by one expression), so t is 0 whatever the rounding of logf.  The
    rule t >= 0 is inclusive: the loss is 0 and the gradient is that of the plain NLL; one float32 step below the
    threshold the row is inactive and its gradient exactly 0."""
    rng = np.random.RandomState(n)
    z = (2 * rng.randn(1, n)).astype(np.float32)
    y, lab = labels(rng, 1, n)
    zd, yd = dev(z), dev(y)
    first = run_head(HEAD_SOFTMAX, LOSS_CODE["nlltrunc"], 0.0, zd, yd, 1, n, n, inv=1.0)
    lpy = first["logprob"][0, lab[0]]
    assert lpy < 0
    _, _, _, _, dz_nll = O.softmax_head(z.astype(np.float64), lab, "nll")
    on = run_head(HEAD_SOFTMAX, LOSS_CODE["nlltrunc"], float(lpy), zd, yd, 1, n, n, inv=1.0)
    assert on["rowloss"][0] == 0
    assert_close(on["da"], dz_nll, what="truncated NLL on the kink: the plain NLL gradient")
    assert np.abs(on["da"]).max() > 1e-3
    off = run_head(HEAD_SOFTMAX, LOSS_CODE["nlltrunc"], float(np.nextafter(lpy, np.float32(-np.inf))), zd, yd, 1, n, n,
                   inv=1.0)
    assert off["rowloss"][0] == 0 and not off["da"].any()


def test_head_rows_softmax_wide_range():
    """Logits of +-60: logprob stays finite and matches; a one-hot-like row has da = 0 within atol."""
    B, n = 10, 65
    rng = np.random.RandomState(60)
    z = rng.uniform(-60, 60, (B, n)).astype(np.float32)
    y, lab = labels(rng, B, n)
    z[0, :] = -60
    z[0, lab[0]] = 60
    lp_w, _, stat_w, cost_w, dz_w = O.softmax_head(z.astype(np.float64), lab, "nll")
    got = run_head(HEAD_SOFTMAX, 0, 0.0, dev(z), dev(y), B, n, n, inv=1.0 / B)
    assert np.isfinite(got["logprob"]).all()
    assert_close(got["logprob"], lp_w, what="wide logprob")
    assert_close(got["rowloss"], O.head_rowloss("softmax", z.astype(np.float64), lab), what="wide rowloss")
    assert_close(got["da"], dz_w, what="wide da")
    assert np.abs(got["da"][0]).max() <= 1e-5
    np.testing.assert_array_equal(got["pred"], z.argmax(1))


def distinct_codes(rng, ncls, nf):
    """ncls distinct rows of nf bits (two classes with one code would tie in every row)."""
    k = min(nf, 16)
    codes = rng.choice(2 ** k, ncls, replace=False)
    c = rng.randint(0, 2, (ncls, nf))
    c[:, :k] = (codes[:, None] >> np.arange(k)) & 1
    return c.astype(np.float32)


CENTERED = [
    # kind, B, n_features, ncls, junk_dist
    ("LOGIT", 1, 9, 6, 0.0), ("LOGIT", 10, 9, 2, 0.0), ("LOGIT", 3, 64, 63, 0.0), ("LOGIT", 257, 200, 64, 0.0),
    ("LOGIT", 10, 200, 100, 0.0),
    ("RBF", 1, 9, 2, 3.0), ("RBF", 10, 9, 6, np.inf), ("RBF", 3, 64, 63, np.inf),       # 64 columns: one full trip
    ("RBF", 257, 64, 64, 3.0e38), ("RBF", 10, 200, 64, 110.0),                          # 65 columns: a second trip
    # (200 features: squared distances to the centers of 80 to 165, the nearest below the junk distance 110 in 3 rows of 4)
    ("RBF", 257, 200, 100, 110.0), ("RBF", 10, 64, 100, np.inf), ("RBF", 257, 9, 6, 3.0),
]


@pytest.mark.parametrize("kind,B,nf,ncls,junk", CENTERED, ids=lambda v: str(v))
def test_centered_head_rows(kind, B, nf, ncls, junk):
    """LOGIT (sigmoid features in (0, 1), centers in {0, 1}) and RBF (scaled_tanh features, a junk column of finite
    or infinite distance; 3.0e38 is what the layer passes for inf): every output against the oracle, da =
    dv * act'(a), dcenters with and without the buffer, accumulated twice."""
    rng = np.random.RandomState(100 * ncls + nf + B)
    y, lab = labels(rng, B, ncls)
    if kind == "LOGIT":
        actn = "sigmoid"
        v = O.activation(actn)[0](2 * rng.randn(B, nf)).astype(np.float32)
        v[np.abs(v - .5) < 1e-3] = .45                  # keep every bit off the 'wrong bit' threshold (asserted below)
        cen = distinct_codes(rng, ncls, nf)
    else:
        actn = "scaled_tanh"
        v = O.activation(actn)[0]((.5 * rng.randn(B, nf)).astype(np.float32)).astype(np.float32)
        cen = rng.uniform(0, 1, (ncls, nf)).astype(np.float32)
    planted = []
    if B >= 3 and ncls > 64:
        # class 67 shares the center of class 3 and row 1 sits on it: two maxima exactly 64 apart
        cen[67] = cen[3]
        v[1] = np.where(cen[3] > .5, .999, .001) if kind == "LOGIT" else cen[3]
        planted = [1]
    jd = np.inf if junk > 1e38 else junk
    v64, c64 = v.astype(np.float64), cen.astype(np.float64)
    lp_w, _, stat_w, cost_w, dv_w, dc_w = O.centered_head(v64, c64, lab, kind, jd)
    if kind == "LOGIT":
        vp = v64 * .998 + .001
        assert np.abs(np.where(c64[lab] > .5, vp, 1 - vp) - .5).min() >= 1e-6    # no bit on the 'wrong bit' threshold
    rl_w = O.head_rowloss(kind, v64, lab, centers=c64, junk_dist=jd)
    assert abs(rl_w.mean() - cost_w) <= 1e-12 * max(1, abs(cost_w))
    ncol = ncls + (kind == "RBF")
    hd, inv, act = (HEAD_LOGIT if kind == "LOGIT" else HEAD_RBF), 0.25, act_code(actn)
    vd, yd, cd = dev(v), dev(y), dev(cen)
    run = lambda **kw: run_head(hd, 0, 0.0, vd, yd, B, nf, ncol, centers=cd, ncls=ncls, junk=junk, act=act, inv=inv, **kw)
    got = run()
    what = "%s B=%d nf=%d ncls=%d " % (kind, B, nf, ncls)
    fin = np.isfinite(lp_w)
    assert fin[:, :ncls].all() and fin[:, ncls:].all() == bool(np.isfinite(jd))
    assert_close(np.where(fin, got["logprob"], 0), np.where(fin, lp_w, 0), what=what + "logprob")
    assert (got["logprob"][~fin] < -1e30).all()          # the junk column of junk_dist = inf
    check_pred(got["pred"], lp_w, planted)
    assert_close(got["rowloss"], rl_w, what=what + "rowloss")
    assert_close(got["rowloss"].astype(np.float64).mean(), cost_w, what=what + "cost")
    assert_close(got["rowstat"], stat_w, what=what + "rowstat")
    assert_close(got["da"], dv_w * B * inv * O.act_grad_from_out(actn, v64), what=what + "da")
    check_null_forms(got, run)
    if kind == "RBF":
        # dcenters accumulates with float atomics over the rows (no fixed order): the weight-gradient tolerance
        dc_w = dc_w * B * inv
        atol = max(1e-5, 2e-6 * np.abs(dc_w).max())
        dcent = empty((ncls, nf))
        dcent.fill_bytes(0)
        with_dc = run(dcent=dcent)
        assert_close(dcent.get_value(), dc_w, atol=atol, what=what + "dcenters")
        for k, val in with_dc.items():                   # the buffer changes nothing else
            np.testing.assert_array_equal(val, got[k], err_msg="dcenters given: " + k)
        run(dcent=dcent)
        assert_close(dcent.get_value(), 2 * dc_w, atol=2 * atol, what=what + "dcenters, second call")


def test_head_rows_refuses_a_centered_head_without_centers():
    B, n = 2, 4
    a, y = dev(np.full((B, n), .5, np.float32)), dev(np.zeros(B + 5, np.int32))
    for head in (HEAD_LOGIT, HEAD_RBF):
        with pytest.raises(RuntimeError, match="centered heads need centers"):
            run_head(head, 0, 0.0, a, y, B, n, 3, centers=None, ncls=2)


def test_head_rows_refuses_more_classes_than_its_lds():
    """4 rows x (ncls + 1) scores of 4 bytes must fit 32 KB: 2047 classes do, 2048 do not (a host-side check)."""
    if no_tile_to_refuse():
        pytest.skip("this backend keeps the class scores in no on-chip tile")
    B, n = 1, 2
    rng = np.random.RandomState(0)
    a, y = dev(rng.rand(B, n).astype(np.float32)), dev(np.zeros(B + 5, np.int32))
    cen = dev(rng.rand(2048, n).astype(np.float32))
    got = run_head(HEAD_RBF, 0, 0.0, a, y, B, n, 2048, centers=cen, ncls=2047, junk=1.0)
    assert np.isfinite(got["logprob"]).all()
    with pytest.raises(RuntimeError, match="too many classes"):
        run_head(HEAD_RBF, 0, 0.0, a, y, B, n, 2049, centers=cen, ncls=2048, junk=1.0)


# ------------------------------------------------------------------------------------------------------------ #
# 2. tn_softmax_nll_cost
# ------------------------------------------------------------------------------------------------------------ #

COST_CASES = [(1, 1, None), (3, 10, None), (10, 65, 0.37), (1021, 457, None),
              (4096, 10, None),          # the headline step: 1024 blocks, the last block's i += 256 loop takes four trips
              (4099, 65, None)]          # 1025 blocks: a fifth, one-element trip and a block with one live row


@pytest.mark.parametrize("B,n,scale", COST_CASES, ids=["b1-n1", "b3-n10", "b10-n65-scaled", "b1021-n457", "headline",
                                                       "b4099-n65"])
def test_softmax_nll_cost(B, n, scale):
    """The cost variant: cost[0] = cost_scale * sum(rowloss) from the last block to finish, twice on one workspace
    (zeroed once) with bit-identical results; every other output bit-identical to tn_softmax_nll."""
    rng = np.random.RandomState(B + n)
    z = (3 * rng.randn(B, n)).astype(np.float32)
    y, lab = labels(rng, B, n)
    scale = 1.0 / B if scale is None else scale
    zd, yd, row0 = dev(z), dev(y), dev(np.array([D_ROW0], np.int64))
    ws = empty(((ctx().lib.tn_softmax_cost_ws_bytes(B) + 3) // 4,))
    ws.fill_bytes(0)
    sentinel = np.array([-777.0], np.float32)
    cost = dev(sentinel)
    costs = []
    for launch in range(2):
        o = [filled((B, n)), filled((B,)), filled((B,), np.int32), filled((B,)), filled((B, n))]
        call("tn_softmax_nll_cost", zd.ptr, yd.ptr, Y_ROW0, row0.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr,
             B, n, 1.0 / B, scale, cost.ptr, ws.ptr)
        costs.append(cost.get_value().copy())
        # a launch that never writes the cost (a ticket counter left standing) must not pass on the earlier value
        cost.set_value(sentinel)
    assert costs[1][0] != sentinel[0]
    np.testing.assert_array_equal(costs[0], costs[1])                 # fixed summation order, counter reset
    lp, rl, pred, rp, dz = [a.get_value() for a in o]
    p = [filled((B, n)), filled((B,)), filled((B,), np.int32), filled((B,)), filled((B, n))]
    call("tn_softmax_nll", zd.ptr, yd.ptr, Y_ROW0, row0.ptr, p[0].ptr, p[1].ptr, p[2].ptr, p[3].ptr, p[4].ptr, B, n,
         1.0 / B)
    for name, a, b in zip(("logprob", "rowloss", "pred", "rowp", "dz"), (lp, rl, pred, rp, dz), p):
        np.testing.assert_array_equal(a, b.get_value(), err_msg="cost variant vs tn_softmax_nll: " + name)
    want = O.log_softmax(z.astype(np.float64))
    r = np.arange(B)
    assert_close(lp, want, what="logprob")
    assert_close(rl, -want[r, lab], what="rowloss")
    assert_close(rp, np.exp(want[r, lab]), what="rowp")
    assert_close(dz, O.nll_dlogits(want, lab), atol=1e-7 if B >= 1000 else 1e-5, what="dz")
    np.testing.assert_array_equal(pred, z.argmax(1))
    assert_close(costs[0][0], scale * (-want[r, lab]).sum(), what="cost")


# ------------------------------------------------------------------------------------------------------------ #
# 3. colour
# ------------------------------------------------------------------------------------------------------------ #

COLOR_SHAPES = [(1, 1, 1), (5, 3, 144), (3, 4, 28 * 28), (2, 3, 64 * 64)]
COLOR_IDS = ["1x1x1", "5x3x12x12", "3x4x28x28", "2x3x64x64"]
X_ROW0 = 2


def color_factors(N, C, u, balance, gamma):
    fac = filled((N, C, 3))
    call("tn_color_factors", fac.ptr, N, C, balance, gamma, dev(u).ptr, 0, 0, None, 0)
    return fac


@pytest.mark.parametrize("maxval", [1.0, 255.0])
@pytest.mark.parametrize("N,C,hw", COLOR_SHAPES, ids=COLOR_IDS)
def test_color_apply(N, C, hw, maxval):
    """Forward with factors from injected draws and from an explicit table; the input holds exact zeros, negative
    values and values that clip at 1."""
    rng = np.random.RandomState(N * hw + int(maxval))
    balance, gamma = 1.4, 2.0
    st = O.ColorStage(1, num_maps=C, balance=balance, gamma=gamma, maxval=maxval)
    x = (rng.uniform(-.2, 1.3, (N + X_ROW0 + 1, C, hw)) * maxval).astype(np.float32)
    x[:, :, ::7] = 0
    u = rng.uniform(-1, 1, (3, N, C)).astype(np.float32)
    fac = color_factors(N, C, u, balance, gamma)
    f_w = np.stack([f[:, :, 0, 0] for f in st.factors(u)], axis=2)
    assert_close(fac.get_value(), f_w.astype(np.float32), rtol=1e-6, atol=0, what="factors from draws")
    xs = x[X_ROW0:X_ROW0 + N].astype(np.float64)[..., None]          # the oracle's stage takes (N, C, h, w)
    assert (xs == 0).any() and (xs < 0).any() or hw == 1
    out = filled((N, C, hw))
    xd = dev(x)
    call("tn_color_apply", xd.ptr, X_ROW0, fac.ptr, out.ptr, N, C, hw, maxval)
    want, saved = st.forward(xs, u)
    assert (saved[3] > 1).any() or hw == 1
    # maxval 255 needs more than atol 1e-5: the cancellation in 1 - (1 - o3) ** g2 leaves about eps of absolute error,
    # times 255.  Measured on these inputs: the formula in float32 numpy (as (x / m) * b and as x * (b / m)) misses the
    # float64 value by up to 1.36e-5 beyond rtol * |want| at maxval 255 (5.2e-8 at maxval 1); four times that.
    atol = 1e-5 if maxval == 1 else 5.5e-5
    assert_close(out.get_value(), want[..., 0], atol=atol, what="colour forward")
    # an explicit table: image 0 the identity (b = g1 = g2 = 1), the others arbitrary
    tab = rng.uniform(.6, 1.7, (N, C, 3)).astype(np.float32)
    tab[0] = 1
    call("tn_color_apply", xd.ptr, X_ROW0, dev(tab).ptr, out.ptr, N, C, hw, maxval)
    t64 = tab.astype(np.float64)[..., None, None]
    want, _ = st.apply(xs, t64[:, :, 0], t64[:, :, 1], t64[:, :, 2])
    assert_close(out.get_value(), want[..., 0], atol=atol, what="colour forward, explicit factors")


@pytest.mark.parametrize("prev", [None, "relu10", "tanh"])
@pytest.mark.parametrize("N,C,hw", COLOR_SHAPES, ids=COLOR_IDS)
def test_color_apply_bwd(N, C, hw, prev):
    """Gradient against ColorStage.backward.  Elements that clip (o1 < 0 or o1 > 1) give exactly 0.  The elements in
    range are built with o1 in [0.01, 0.99]: at o2 = 0 with g1 < 1 the derivative is infinite in the reference as
    well, and near o3 = 1 the fp32 value of 1 - o3 has no digits left -- neither is a property of the kernel."""
    rng = np.random.RandomState(N * hw + len(prev or ""))
    balance, gamma, maxval = 1.4, 2.0, 255.0
    st = O.ColorStage(1, num_maps=C, balance=balance, gamma=gamma, maxval=maxval)
    u = rng.uniform(-1, 1, (3, N, C)).astype(np.float32)
    fac = color_factors(N, C, u, balance, gamma)
    b = fac.get_value()[:, :, 0:1].astype(np.float64)
    o1 = rng.uniform(.012, .988, (N, C, hw))
    clip = rng.rand(N, C, hw) < .25
    o1[clip] = np.where(rng.rand(clip.sum()) < .5, rng.uniform(-.3, -.02, clip.sum()), rng.uniform(1.02, 1.3, clip.sum()))
    x = np.zeros((N + X_ROW0, C, hw), np.float32)
    x[X_ROW0:] = o1 * maxval / b
    g = rng.randn(N, C, hw).astype(np.float32)
    xs = x[X_ROW0:].astype(np.float64)[..., None]                    # the oracle's stage takes (N, C, h, w)
    _, saved = st.forward(xs, u)
    o1_w = saved[3][..., 0]
    inside = (o1_w >= .01) & (o1_w <= .99)
    outside = (o1_w < 0) | (o1_w > 1)
    assert (inside | outside).all() and (outside == clip).all()
    want = st.backward(g.astype(np.float64)[..., None], saved)[..., 0]
    args = (None, 0, 0.0)
    if prev:
        pa = rng.randn(N, C, hw).astype(np.float32)
        pa[:, :, ::5] = 0
        want = want * O.act_grad_from_out(prev, pa.astype(np.float64))
        args = (dev(pa).ptr,) + act_code(prev)
    dx = filled((N, C, hw))
    call("tn_color_apply_bwd", dev(x).ptr, X_ROW0, fac.ptr, dev(g).ptr, dx.ptr, N, C, hw, maxval, *args)
    got = dx.get_value()
    assert_close(got, want, what="colour backward")
    assert not got[outside].any()                                     # exactly zero where the clip is active


def test_color_factors_device_generator():
    """draws = NULL: factors within [1 / a, a]; the three of an image differ; keyed by the GLOBAL image index (a
    shard equals its rows of the whole batch bit for bit) and by step + *d_step."""
    C, balance, gamma, seed = 3, 1.5, 2.0, 0x1234567890abc

    def factors(N, row_global0, step, d_step=None):
        fac = filled((N, C, 3))
        call("tn_color_factors", fac.ptr, N, C, balance, gamma, None, seed, step,
             dev(np.array([d_step], np.uint32)).ptr if d_step is not None else None, row_global0)
        return fac.get_value()

    full = factors(8, 0, 3)
    assert ((full[..., 0] >= np.float32(1 / balance)) & (full[..., 0] <= np.float32(balance))).all()
    assert ((full[..., 1:] >= np.float32(1 / gamma)) & (full[..., 1:] <= np.float32(gamma))).all()
    assert (full[..., 0] != full[..., 1]).all() and (full[..., 1] != full[..., 2]).all() and \
        (full[..., 0] != full[..., 2]).all()
    assert len(np.unique(full)) == full.size                          # no image repeats another's draws
    np.testing.assert_array_equal(factors(4, 4, 3), full[4:8])
    np.testing.assert_array_equal(factors(8, 0, 1, d_step=2), full)
    assert not np.array_equal(factors(8, 0, 4), full)


# ------------------------------------------------------------------------------------------------------------ #
# 4. tn_elastic_apply_bwd
# ------------------------------------------------------------------------------------------------------------ #

ELASTIC_BWD = [
    # h = w, N, C, map, invert, flipmask, prev_a's activation
    (12, 1, 1, "identity", 0, False, None),            # one trip of p += 256 (144 pixels)
    (12, 2, 3, "bilinear", 1, True, "tanh"),
    (28, 3, 2, "bilinear", 0, True, "relu10"),         # 784 pixels: three full trips and one of 16
    (28, 1, 1, "nearest", 1, False, None),
    (28, 2, 2, "onecell", 0, False, None),             # every pixel gathers from one source cell
    (64, 4, 6, "bilinear", 0, True, None),             # N * C = 24
    (64, 2, 1, "nearest", 0, True, "tanh"),
    (128, 2, 1, "bilinear", 1, True, "tanh"),          # a 64 KB tile: exactly the limit
    (128, 1, 1, "identity", 0, False, None),
]


def sample_maps(rng, h, w, kind):
    """map_idx with rows <= h - 2 and columns <= w - 2 (the four taps stay inside), fractions in [0, 1)."""
    if kind == "identity":
        return None, None, None
    if kind == "onecell":
        idx = np.full(h * w, (h // 2) * w + w // 3, np.int32)
    else:
        idx = (rng.randint(0, h - 1, h * w) * w + rng.randint(0, w - 1, h * w)).astype(np.int32)
    assert (idx // w).max() <= h - 2 and (idx % w).max() <= w - 2
    if kind == "nearest":
        return idx, None, None
    fy, fx = rng.rand(h * w).astype(np.float32), rng.rand(h * w).astype(np.float32)
    assert fy.max() < 1 and fx.max() < 1
    return idx, fy, fx


@pytest.mark.parametrize("h,N,C,kind,invert,flip,prev", ELASTIC_BWD, ids=lambda v: str(v))
def test_elastic_apply_bwd(h, N, C, kind, invert, flip, prev):
    w = h
    rng = np.random.RandomState(h + 10 * N + C)
    idx, fy, fx = sample_maps(rng, h, w, kind)
    g = rng.randn(N, C, h, w).astype(np.float32)
    if kind == "onecell":
        g = np.abs(g)
    fm = (rng.rand(N, C, h, w) < .3).astype(np.uint8) if flip else None
    want = O.elastic_scatter(g, idx, fy, fx, w, fm, bool(invert))
    args = (None, 0, 0.0)
    if prev:
        pa = rng.randn(N, C, h, w).astype(np.float32)
        want = want * O.act_grad_from_out(prev, pa.astype(np.float64))
        args = (dev(pa).ptr,) + act_code(prev)
    ptr = lambda a: dev(a).ptr if a is not None else None
    dx = filled((N, C, h, w))
    call("tn_elastic_apply_bwd", dev(g).ptr, dx.ptr, N, C, h, w, invert, int(kind == "nearest"), ptr(idx), ptr(fy), ptr(fx),
         0.0, ptr(fm), 0, 0, None, 0, *args)
    atol = 1e-5
    if kind == "onecell":
        # all 784 contributions of an image meet in four LDS words, in no fixed order: the bound scales with sum |g|
        atol = max(1e-5, 2e-6 * np.abs(g).reshape(N * C, -1).sum(1).max())
    assert_close(dx.get_value(), want, atol=atol, what="elastic backward %s %dx%d" % (kind, h, w))


def test_elastic_apply_bwd_refuses_a_map_beyond_its_lds():
    """129 x 129 floats do not fit the 64 KB tile: a host-side check."""
    if no_tile_to_refuse():
        pytest.skip("this backend scatters into no on-chip tile")
    g = dev(np.zeros((1, 1, 129, 129), np.float32))
    dx = empty((1, 1, 129, 129))
    with pytest.raises(RuntimeError, match="too large"):
        call("tn_elastic_apply_bwd", g.ptr, dx.ptr, 1, 1, 129, 129, 0, 0, None, None, None, 0.0, None, 0, 0, None, 0,
             None, 0, 0.0)


@pytest.mark.parametrize("h,N", [(28, 64), (15, 8)], ids=["28x28", "15x15"])
def test_elastic_backward_regenerates_the_forward_flips(h, N):
    """The backward pass regenerates the flip noise instead of reading a mask: it must be the noise the forward pass
    drew, for the same seed, step, device counter and global row offset.  Forward on x = 0 with the identity map:
    the output IS the flip mask.  (28 x 28 takes the forward's four-pixel kernel, 15 x 15 its one-pixel kernel.)"""
    C, w, pflip, seed, step, row_global0 = 3, h, .15, 0xfeed5eed1234, 3, 7
    d_step = dev(np.array([2], np.uint32))
    x = np.zeros((N, C, h, w), np.float32)
    out = filled(x.shape)
    call("tn_elastic_apply", dev(x).ptr, 0, None, out.ptr, N, C, h, w, 0, 1, None, None, None, pflip, None, seed, step,
         d_step.ptr, row_global0)
    mask = out.get_value()
    assert set(np.unique(mask)) <= {0.0, 1.0}
    if N * C * h * w > 100000:
        assert abs(mask.mean() - pflip) < .003                        # the bound of test_gpu_elastic.py
    assert 0 < mask.mean() < 2 * pflip
    rng = np.random.RandomState(h)
    g = rng.randn(N, C, h, w).astype(np.float32)
    dx = filled(x.shape)
    call("tn_elastic_apply_bwd", dev(g).ptr, dx.ptr, N, C, h, w, 0, 1, None, None, None, pflip, None, seed, step,
         d_step.ptr, row_global0, None, 0, 0.0)
    want = O.elastic_scatter(g, None, None, None, w, mask, False)
    np.testing.assert_array_equal(dx.get_value(), want.astype(np.float32))     # a sign per element: exact
    # ... and it follows the counter: another step flips other elements
    call("tn_elastic_apply_bwd", dev(g).ptr, dx.ptr, N, C, h, w, 0, 1, None, None, None, pflip, None, seed, step + 1,
         d_step.ptr, row_global0, None, 0, 0.0)
    assert not np.array_equal(dx.get_value(), want.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ #
# 5. tn_aux_mix, tn_copy_cols
# ------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize("B", [1, 8, 300])
@pytest.mark.parametrize("d", [1, 2, 7])
def test_aux_mix(d, B):
    """Train mode with injected draws and test mode (the mean of the two candidates), boost and a row offset, against
    the input mix of the oracle's LocationInfoStage (whose perceptron, here of zero weights, plays no part)."""
    rng = np.random.RandomState(10 * d + B)
    row0, boost = 2, 2.5
    aux = rng.randn(B + row0 + 1, 2, d).astype(np.float32)
    u = rng.rand(B).astype(np.float32)
    st = O.LocationInfoStage([np.zeros((d, 1)), np.zeros(1), np.zeros((1, 1)), np.zeros(1)], None, (1, 1), boost,
                             np.dtype(np.float64))
    auxd = dev(aux)
    for train in (1, 0):
        out = filled((B, d))
        call("tn_aux_mix", auxd.ptr, row0, out.ptr, B, d, boost, train, dev(u).ptr if train else None, 0, 0, None, 0)
        _, (loc, _, _, _) = st.forward(aux[row0:row0 + B], u, bool(train))
        assert_close(out.get_value(), loc, what="aux mix train=%d" % train)


def test_aux_mix_device_generator():
    """u_inj = NULL: one U[0, 1) draw per row, shared by its columns, keyed by the GLOBAL row and step + *d_step.
    With candidates (1, 0) and a power-of-two boost the output is boost * u exactly."""
    d, boost, seed = 7, 2.0, 0xabcdef0123
    aux = np.zeros((300, 2, d), np.float32)
    aux[:, 0, :] = 1
    auxd = dev(aux)

    def mix(B, row0, step, d_step=None):
        out = filled((B, d))
        call("tn_aux_mix", auxd.ptr, row0, out.ptr, B, d, boost, 1, None, seed, step,
             dev(np.array([d_step], np.uint32)).ptr if d_step is not None else None, row0)
        return out.get_value()

    full = mix(300, 0, 3)
    u = (full / boost - aux[:, 1]) / (aux[:, 0] - aux[:, 1])
    assert ((u >= 0) & (u < 1)).all()
    assert (u == u[:, :1]).all()                                      # one draw per row
    assert len(np.unique(u[:, 0])) > 290 and abs(u.mean() - .5) < .1
    np.testing.assert_array_equal(mix(4, 4, 3), full[4:8])
    np.testing.assert_array_equal(mix(300, 0, 1, d_step=2), full)
    assert not np.array_equal(mix(300, 0, 4), full)


@pytest.mark.parametrize("prev", [None, "tanh"])
@pytest.mark.parametrize("col_src,col_dst,ncols", [(0, 0, 4), (3, 5, 4), (7, 9, 4), (0, 12, 1), (0, 1, 11)],
                         ids=["start", "middle", "end", "last-column", "whole-source"])
def test_copy_cols(col_src, col_dst, ncols, prev):
    """A column window of a (B, 11) matrix into a (B, 13) one.  prev_a is indexed at the DESTINATION position (the
    windows with col_src != col_dst pin that); columns outside the window keep their 0xff fill."""
    B, ld_src, ld_dst = 300, 11, 13
    rng = np.random.RandomState(col_src + 3 * col_dst + ncols)
    src = rng.randn(B, ld_src).astype(np.float32)
    want = src[:, col_src:col_src + ncols].astype(np.float64)
    args = (None, 0, 0.0)
    if prev:
        pa = rng.randn(B, ld_dst).astype(np.float32)
        want = want * O.act_grad_from_out(prev, pa[:, col_dst:col_dst + ncols].astype(np.float64))
        args = (dev(pa).ptr,) + act_code(prev)
    dst = filled((B, ld_dst))
    call("tn_copy_cols", dev(src).ptr, ld_src, col_src, dst.ptr, ld_dst, col_dst, ncols, B, *args)
    got = dst.get_value()
    window = np.zeros((B, ld_dst), bool)
    window[:, col_dst:col_dst + ncols] = True
    if prev:
        assert_close(got[window].reshape(B, ncols), want, what="copy_cols * act'")
    else:
        np.testing.assert_array_equal(got[window].reshape(B, ncols), want.astype(np.float32))
    assert untouched(got).reshape(B, ld_dst, 4).all(2)[~window].all()


def test_copy_cols_refuses_a_window_past_the_row():
    src, dst = dev(np.zeros((4, 11), np.float32)), empty((4, 13))
    for col_src, col_dst, ncols in [(8, 0, 4), (0, 10, 4)]:
        with pytest.raises(RuntimeError, match="tn_copy_cols"):
            call("tn_copy_cols", src.ptr, 11, col_src, dst.ptr, 13, col_dst, ncols, 4, None, 0, 0.0)
