"""The case table of tn_elastic_convpool_fwd_mask (theanet_amd/csrc/elastic.hip, elastic_convpool_fwd_kernel<ACT, KT>:
ElasticLayer resampling fused into the first conv block's forward) and, per case, the kernel paths it takes.

No device code is imported here: tests/test_elconv_cases_cpu.py proves from ``branches()`` that the table reaches every
instantiation, operand form and loop edge of the kernel; tests/test_gpu_elastic_convpool.py runs the same table on the
device.  The oracle side of a case (its distortion stage with injected draws) is built here too, so that the CPU test
can check what only depends on the oracle: the share of nearest-neighbour pixels that can be compared exactly.
"""
import collections

import numpy as np

from oracle import theanet_oracle as O

Case = collections.namedtuple("Case", [
    "name", "N", "h", "w", "K",
    "mode", "act",              # conv mode ('valid' / 'same'), activation name
    "map",                      # 'none' (map_idx == NULL), 'nearest', 'bilinear'
    "invert",                   # 0 / 1
    "flip",                     # 'none', 'flipmask' (injected bytes), 'philox' (drawn on the device)
    "mask",                     # the case's own launch asks for the pooling mask (False: mask == NULL, the test graph's form)
    "row0", "step",             # 'host': x_row0 / step by value; 'device': through d_row0 / d_step
    "at_end",                   # the batch is the last N rows of the x allocation
    "seed",                     # of the oracle stage's draws (chosen on the CPU: see nearest_safe)
])

F, P = 3, 2                     # the only filter and pooling sizes the fused launch takes
PFLIP = .1
# one distortion for every case with a map: all four stages of the field (translation, smoothed noise, zoom, rotation)
ELASTIC = dict(translation=1, zoom=1.1, magnitude=20, sigma=3, angle=5)

CASES = [
    #    name           N   h   w   K  mode     act        map         inv flip        mask   row0      step      at_end seed
    Case("one_window",  1,  4,  4,  1, "valid", "relu",    "bilinear", 0, "none",     True,  "host",   "host",   True,  5),
    Case("odd_valid",   2, 13, 12,  3, "valid", "relu",    "nearest",  0, "flipmask", True,  "device", "host",   True,  5),
    Case("odd_same",    2, 13, 12,  2, "same",  "tanh",    "none",     1, "philox",   False, "host",   "device", False, 1),
    Case("nonsquare",   2, 12, 20,  2, "valid", "relu",    "bilinear", 1, "flipmask", True,  "device", "device", True,  8),
    Case("second_trip", 3, 36, 36,  2, "same",  "relu10",  "nearest",  1, "philox",   True,  "host",   "device", True,  5),
    Case("mnist_conv1", 9, 28, 28,  4, "valid", "relu10",  "nearest",  1, "philox",   True,  "device", "device", False, 5),
    Case("k4_tanh",     2,  8,  8,  4, "valid", "tanh",    "none",     0, "none",     False, "host",   "host",   False, 1),
    Case("k16_sigmoid", 2,  8,  8, 16, "same",  "sigmoid", "bilinear", 0, "philox",   True,  "host",   "host",   True,  5),
    Case("k5_relu05",   3,  8, 12,  5, "valid", "relu05",  "nearest",  0, "none",     True,  "device", "host",   False, 8),
]


def geometry(c):
    """pad_lo, (Ho, Wo), (Hp, Wp), (Hx, Wx): conv output, pooled output (partial windows kept) and the kernel's LDS tile."""
    pad_lo, _, Ho = O.conv_geometry(c.h, F, 1, c.mode)
    _, _, Wo = O.conv_geometry(c.w, F, 1, c.mode)
    Hp, Wp = O.pool_out_sz(Ho, P, False), O.pool_out_sz(Wo, P, False)
    return pad_lo, (Ho, Wo), (Hp, Wp), (2 * Hp + 2, 2 * Wp + 2)


def supported(h, w, K, f, pad_lo, Ho, Wo, p, Hp, Wp):
    """tn_elastic_convpool_supported (elastic.hip) restated, with the TN_ELASTIC_CONV knob at its default (on).  This is
    the ONLY logic of the library that the table duplicates; the GPU test asks the library itself for every case."""
    if f != 3 or p != 2 or K < 1 or K > 16 or w % 4 != 0:
        return False
    if h + 2 * pad_lo > 2 * Hp + 2 or w + 2 * pad_lo > 2 * Wp + 2:         # the image fits the tile
        return False
    if Hp != (Ho + 1) // 2 or Wp != (Wo + 1) // 2:
        return False
    return (2 * Hp + 2) * (2 * Wp + 2) * 4 <= 48 * 1024


def branches(c):
    """Which paths of elastic_convpool_fwd_kernel the case takes, from the case's own numbers.  Every predicate is the
    kernel's (or its launcher's), named after what it selects there."""
    pad_lo, (Ho, Wo), (Hp, Wp), (Hx, Wx) = geometry(c)
    leaky = O.leaky_slope(c.act) is not None and c.act != "linear"      # TN_ACT_LEAKY: relu, reluNN
    KT = 4 if c.K == 4 else 0                                          # launcher: K == 4 -> taps in registers
    zero_frame = Hx != c.h or Wx != c.w
    return dict(
        inst=(leaky, KT),
        map=c.map, invert=c.invert,
        invert_after=bool(c.invert and c.map != "bilinear"),           # invert && (!map_idx || nearest)
        invert_in_gather=bool(c.invert and c.map == "bilinear"),
        flip=c.flip, mask=c.mask, row0=c.row0, step=c.step,
        zero_frame=zero_frame,
        frame_rows_only=Hx != c.h and Wx == c.w,                       # image rows as wide as the tile's, one row short
        pad=pad_lo,                                                    # the image's offset in the tile
        ho_odd=Ho % 2 == 1,       # v10 false in the last pooling row (w % 4 == 0 keeps Wo even: v01 is always true)
        nonsquare=c.h != c.w,
        trip2_resample=c.h * c.w > 1024,                               # q4 += 256, four pixels each
        trip2_frame=zero_frame and Hx * Wx > 1024,                     # i += 1024
        trip2_windows=Hp * Wp > 256,                                   # q += 256
        one_window=Hp * Wp == 1, K=c.K, N=c.N,
        end_bilinear=c.at_end and c.map == "bilinear",                 # the 8-byte gather xi + m + w against the guard band
    )


def describe(c):
    """The branches of a case in one line (test output, summaries)."""
    b = branches(c)
    on = [k for k in ("zero_frame", "frame_rows_only", "ho_odd", "nonsquare", "trip2_resample", "trip2_frame", "trip2_windows",
                      "one_window", "end_bilinear") if b[k]]
    return "<%s,%d> map=%s invert=%d flip=%s mask=%s row0=%s step=%s%s" % (
        "leaky" if b["inst"][0] else "other", b["inst"][1], c.map, c.invert, c.flip, "yes" if c.mask else "NULL",
        c.row0, c.step, "".join(" " + k for k in on))


def oracle_stage(c):
    """(stage, draws) of the oracle's ElasticLayer for the case: ``stage.forward(x, draws)`` is what the resampled
    image must be.  Philox flips have no oracle (pflip = 0 here; the test checks them on their own).  The oracle draws
    its noise planes for square images: a non-square case takes the top-left h x w of them."""
    prm = dict(ELASTIC) if c.map != "none" else {}
    st = O.ElasticStage(max(c.h, c.w), num_maps=1, nearest=c.map == "nearest", invert_image=bool(c.invert),
                        pflip=PFLIP if c.flip == "flipmask" else 0, rand_gen=np.random.RandomState(c.seed), **prm)
    d = st.draw((c.N, 1, c.h, c.w))
    if d.noise is not None:
        d.noise = np.ascontiguousarray(d.noise[:, :c.h, :c.w])
    return st, d


def nearest_safe(target, h, w):
    """Pixels whose nearest-neighbour source is certain: both clipped coordinates further than 5e-4 from a rounding
    boundary (the device's field differs from the oracle's by a few 1e-4: float32 smoothing sums in another order)."""
    cy = np.clip(target[0], 0, h - 1.001)
    cx = np.clip(target[1], 0, w - 1.001)
    return (np.abs(cy - np.floor(cy) - .5) > 5e-4) & (np.abs(cx - np.floor(cx) - .5) > 5e-4)
