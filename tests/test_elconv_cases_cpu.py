"""The case table of the fused elastic + conv1 forward (tests/elconv_cases.py) reaches every path of
elastic_convpool_fwd_kernel<ACT, KT> -- proved without a device, from ``branches()``.  Deleting a case from the table
fails ``test_the_table_covers_every_path``, which names the path that is no longer run; and no case is there for
nothing (``test_every_case_is_needed``)."""
import itertools

import pytest

from oracle import theanet_oracle as O
from tests import elconv_cases as EC


def _is(**want):
    return lambda b: all(b[k] == v for k, v in want.items())


# path of the kernel (or of its launcher) -> what the branches of a case that takes it look like
PATHS = {}
for leaky, KT in itertools.product((True, False), (4, 0)):
    PATHS["instantiation <%s, %d>" % ("TN_ACT_LEAKY" if leaky else "-1", KT)] = _is(inst=(leaky, KT))
for kind, inv in itertools.product(("none", "nearest", "bilinear"), (0, 1)):
    PATHS["map %s with invert = %d" % (kind, inv)] = _is(map=kind, invert=inv)
for kind in ("none", "flipmask", "philox"):
    PATHS["flip kind %s" % kind] = _is(flip=kind)
PATHS.update({
    "mask written": _is(mask=True),
    "mask == NULL": _is(mask=False),
    "x_row0 by value (d_row0 == NULL)": _is(row0="host"),
    "row offset through d_row0": _is(row0="device"),
    "step by value (d_step == NULL)": _is(step="host"),
    "step through d_step": _is(step="device"),
    "zero frame (Hx != h or Wx != w)": _is(zero_frame=True),
    "no zero frame (the tile is the image)": _is(zero_frame=False),
    "zero frame in rows only (Hx != h, Wx == w)": _is(frame_rows_only=True),
    "partial last pooling row (Ho odd), pad 0": _is(ho_odd=True, pad=0),
    "partial last pooling row (Ho odd), pad 1": _is(ho_odd=True, pad=1),
    "Ho even": _is(ho_odd=False),
    "non-square image": _is(nonsquare=True),
    "second trip of the resampling loop (h*w > 1024)": _is(trip2_resample=True),
    "second trip of the zero-frame loop (Hx*Wx > 1024)": _is(trip2_frame=True),
    "second trip of the window loop (Hp*Wp > 256)": _is(trip2_windows=True),
    "one-window image": _is(one_window=True),
    "K = 1": _is(K=1),
    "K = 16": _is(K=16),
    "N = 1": _is(N=1),
    # both neighbours of the K == 4 switch to the unrolled instantiation, in the generic leaky one
    "leaky, K = 3 (generic filter loop below the K == 4 switch)": _is(inst=(True, 0), K=3),
    "leaky, K = 5 (generic filter loop above the K == 4 switch)": _is(inst=(True, 0), K=5),
    "bilinear map on a batch that ends at the end of x": _is(end_bilinear=True),
})


def missing(cases):
    """The paths of PATHS that no case of ``cases`` takes."""
    bs = [EC.branches(c) for c in cases]
    return [name for name, takes in PATHS.items() if not any(takes(b) for b in bs)]


def test_the_table_covers_every_path():
    lost = missing(EC.CASES)
    assert not lost, "no case of tests/elconv_cases.py runs: " + "; ".join(lost)


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_every_case_is_needed(case):
    """Without the case at least one path is no longer run (so the coverage test above fails, naming it)."""
    assert missing([c for c in EC.CASES if c is not case]), "%s adds no path of its own" % case.name


@pytest.mark.parametrize("case", EC.CASES, ids=lambda c: c.name)
def test_case_is_well_formed_and_supported(case):
    c = case
    assert c.mode in ("valid", "same") and c.map in ("none", "nearest", "bilinear") and c.invert in (0, 1)
    assert c.flip in ("none", "flipmask", "philox") and c.row0 in ("host", "device") and c.step in ("host", "device")
    assert 1 <= c.N <= 9 and c.w % 4 == 0
    O.activation(c.act)
    pad_lo, (Ho, Wo), (Hp, Wp), _ = EC.geometry(c)
    assert EC.supported(c.h, c.w, c.K, EC.F, pad_lo, Ho, Wo, EC.P, Hp, Wp)
    assert len({k.name for k in EC.CASES}) == len(EC.CASES)


def test_the_restated_support_rule_rejects_what_the_kernel_cannot_take():
    ok = (28, 28, 4, 3, 0, 26, 26, 2, 13, 13)
    assert EC.supported(*ok)
    for i, v in ((1, 30), (2, 0), (2, 17), (3, 5), (7, 3), (4, 1), (8, 12), (9, 14)):
        bad = list(ok)
        bad[i] = v
        assert not EC.supported(*bad), bad
    assert EC.supported(108, 108, 1, 3, 1, 108, 108, 2, 54, 54)            # 110 x 110 floats: the largest tile in 48 KiB
    assert not EC.supported(112, 112, 1, 3, 1, 112, 112, 2, 56, 56)


def test_the_mandatory_shapes_are_in_the_table():
    have = {(c.h, c.w, c.mode) for c in EC.CASES}
    assert {(4, 4, "valid"), (13, 12, "valid"), (13, 12, "same"), (12, 20, "valid"), (36, 36, "same"),
            (28, 28, "valid")} <= have
    assert any((c.h, c.w, c.mode, c.K, c.N) == (4, 4, "valid", 1, 1) for c in EC.CASES)
    assert any((c.h, c.w, c.mode, c.N) == (36, 36, "same", 3) for c in EC.CASES)
    assert any((c.h, c.w, c.mode, c.K, c.act) == (28, 28, "valid", 4, "relu10") for c in EC.CASES)
    assert {(4, "tanh"), (16, "sigmoid"), (5, "relu05")} <= {(c.K, c.act) for c in EC.CASES}


@pytest.mark.parametrize("case", [c for c in EC.CASES if c.map == "nearest"], ids=lambda c: c.name)
def test_the_oracle_alone_leaves_nearly_every_nearest_pixel_comparable(case):
    """The GPU test compares a nearest-neighbour pixel exactly unless a coordinate lies within 5e-4 of a rounding
    boundary, and asserts that more than 99 % are compared.  Whether a seed allows that is decided by the oracle's field
    alone; a seed that does not is replaced here, not on the device."""
    st, d = EC.oracle_stage(case)
    target = O.elastic_field(case.h, case.w, st.prm, d)
    assert EC.nearest_safe(target, case.h, case.w).mean() > .99
