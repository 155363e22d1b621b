"""The general conv family of the 16-bit conv stack (CONV_SHAPES 'any'; theanet_amd/csrc/convg_c8.hip), the parts that
need no GPU: the coverage of its kernels and their edges by the op cases of tests/test_gpu_c8_convg.py (the scheme of
tests/test_c8_dispatch.py), and the host's decisions -- which family runs a ConvLayer and at which pitches
(c8.choose_conv), which PoolLayers stand alone (c8.pool_stands_alone / check_follows), the CONV_SHAPES param itself.

The launchers choose from host-only geometry: c8_convg_kernel<E, MODE> with MODE 0 (forward), 1 (input gradient, stride 1)
or 2 (input gradient, any stride), each with a leaky-ReLU or a generic epilogue, and c8_convg_wgrad_kernel<E>; E is the
element type, which the GPU tests run both of.  tn_c8_convg_plan runs that selection without a device.  A sweep over
ConvLayer geometries collects every reachable (kernel, epilogue) and every (kernel, edge) pair; the GPU cases must reach
all of them.

Edges (where the tiling goes wrong):
  one_octet / octets     the reduced maps (forward: channels, input gradient: filters; weight gradient: channels) fill one
                         octet -- two TAPS share an MFMA step -- or several
  half_step              the (tap, octet) cells are odd in number: the last step's second half is fed zeros
  ragged_octet           the reduced maps are no multiple of 8: the last octet's tail is zeros
  out_tail               the last block of 256 output pixels is partial (weight gradient: the last group of 8 column cells)
  row_tail               the last 32-row tile is partial (weight gradient: the last group of 64 filters)
  rows                   more than one 32-row tile (weight gradient: more than one column / filter group)
  one_slab / slabs       (weight gradient) one slab of partial sums or several
  pix_tail               (weight gradient) the last tile of 64 output pixels is partial"""
import ctypes
import functools
import os
import subprocess
import sys

import pytest

from tests import test_gpu_c8_convg as GC
from tests.gpu_util import ROOT, act_code


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 8)()

    def plan(op, geom, act=0, prm=0.):
        n = lib.tn_c8_convg_plan(op, *geom, act, prm, out, 8)
        return tuple(out[:n]) if n > 0 else None
    assert plan(0, (2, 8, 12, 16, 8, 3, 1, 0, 10, 16)), "tn_c8_convg_plan answers nothing (CPU backend loaded?)"
    return plan


def classify(op, geom, act, prm):
    p = _query()(op, geom, act, prm)
    if p is None:
        return None
    kernel, leaky, r8, steps, ragged_red, rows, blocks, ragged_out = p
    edges = {"one_octet" if r8 == 1 else "octets"}
    if kernel == 3:
        inst = ("wgrad",)
        edges.add("one_slab" if blocks == 1 else "slabs")
        edges |= {e for e, on in (("pix_tail", ragged_red), ("out_tail", ragged_out & 1), ("row_tail", ragged_out & 2),
                                  ("rows", rows > 1)) if on}
    else:
        inst = (("fwd", "dgrad1", "dgrads")[kernel], leaky)
        edges |= {e for e, on in (("half_step", ragged_red & 1), ("ragged_octet", ragged_red & 2), ("out_tail", ragged_out & 1),
                                  ("row_tail", ragged_out & 2), ("rows", rows > 1)) if on}
    return inst, edges


def _reach(launches):
    insts, pairs = set(), set()
    for op, geom, name in launches:
        r = classify(op, geom, *act_code({"leaky": "relu10"}.get(name, name)))
        if r is None:
            continue
        insts.add(r[0])
        pairs.update((r[0][0], e) for e in r[1])
    return insts, pairs


def _layer_geom(N, C, S, K, f, stride, mode):
    """What ConvLayer and c8.choose_conv make of a layer: the entry points' geometry, None where ConvLayer asserts."""
    from theanet_amd.device import c8_pool_pitch
    if mode == "same" and stride != 1:
        return None
    lo = GC.pad_lo(f, mode)
    hi = (f - 1) // 2 if mode == "same" else 0
    full = S + lo + hi - f + 1
    if full < 1 or full % stride:
        return None
    So = full // stride
    return N, C, S, c8_pool_pitch(S), K, f, stride, lo, So, c8_pool_pitch(So)


def _sweep():
    for S in (4, 8, 9, 12, 13, 28, 72):
        for N in (1, 2, 3, 70, 300):
            for C in (1, 3, 8, 9, 16, 20, 40):
                for K in (4, 8, 9, 20, 32, 72):
                    for f in (1, 2, 3, 4, 5):
                        for stride in (1, 2, 3):
                            for mode in ("valid", "same"):
                                g = _layer_geom(N, C, S, K, f, stride, mode)
                                if g is None:
                                    continue
                                for name in ("leaky", "tanh"):
                                    yield 0, g, name
                                    yield 1, g, name
                                yield 2, g, "leaky"


@functools.lru_cache(maxsize=None)
def sweep():
    return _reach(_sweep())


def test_plan_query_runs_the_launchers_selection():
    plan = _query()
    leaky, tanh = act_code("relu10"), act_code("tanh")
    mnist1 = (4096, 1, 28, 32, 4, 3, 1, 0, 26, 32)
    # forward: one octet, 9 taps = 9 cells = 5 steps with half a step of zeros, one row tile, N Po Po / 256 blocks
    assert plan(0, mnist1, *leaky) == (0, 1, 1, 5, 1 | 2, 1, 4096 * 32 * 32 // 256, 2)
    assert plan(0, mnist1, *tanh)[:2] == (0, 0)
    # input gradient: reduces over the filters, lanes over the input's pitch
    assert plan(1, mnist1, *leaky) == (1, 1, 1, 5, 1 | 2, 1, 4096 * 32 * 32 // 256, 2)
    assert plan(1, (2, 16, 10, 16, 8, 3, 2, 0, 4, 8), *leaky)[0] == 2
    # weight gradient: 9 column cells = 2 groups, one filter group: 256 slabs each, over N 26 26 / 64 pixel tiles
    assert plan(2, mnist1) == (3, 0, 1, 4096 * 26 * 26 // 64, 0, 2, 256, 1 | 2)
    assert plan(2, (2, 8, 4, 8, 16, 4, 1, 0, 1, 8))[6] == 1                  # two pixels: one tile, one slab
    assert plan(0, (2, 8, 12, 16, 8, 3, 1, 0, 11, 16)) is None and plan(3, mnist1) is None


def test_supported_geometries_have_a_plan_and_others_none():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    n = 0
    for op, g, name in _sweep():
        assert lib.tn_c8_convg_supported(*g), g
        assert _query()(op, g) is not None, (op, g)
        n += 1
    assert n > 10000
    for g in ((2, 8, 12, 16, 8, 3, 1, 0, 11, 16), (2, 8, 12, 24, 8, 3, 1, 0, 10, 16), (2, 8, 4, 8, 8, 7, 1, 0, 1, 8),
              (1 << 20, 64, 64, 64, 8, 3, 1, 0, 62, 64)):                      # So, pitch, f > S + padding, 2^32 cells
        assert not lib.tn_c8_convg_supported(*g) and all(_query()(op, g) is None for op in (0, 1, 2)), g


def test_gpu_cases_reach_every_instantiation():
    """The op cases of tests/test_gpu_c8_convg.py launch every kernel of the family with both epilogues."""
    insts, _ = sweep()
    assert insts == {(k, lk) for k in ("fwd", "dgrad1", "dgrads") for lk in (0, 1)} | {("wgrad",)}
    got, _ = _reach(GC.convg_launches())
    assert got == insts, "instantiations no case of tests/test_gpu_c8_convg.py launches: %s" % sorted(insts - got)


def test_gpu_cases_reach_every_edge_of_every_kernel():
    _, pairs = sweep()
    _, got = _reach(GC.convg_launches())
    assert not got - pairs, sorted(got - pairs)
    assert not pairs - got, "(kernel, edge) pairs no case of tests/test_gpu_c8_convg.py reaches: %s" % sorted(pairs - got)
    for k in ("fwd", "dgrad1", "dgrads", "wgrad"):
        assert {(k, "one_octet"), (k, "octets"), (k, "out_tail"), (k, "row_tail")} <= got, k
    assert {("fwd", "half_step"), ("fwd", "ragged_octet"), ("wgrad", "one_slab"), ("wgrad", "slabs"), ("wgrad", "pix_tail")} <= got


def test_the_case_list_is_what_convlayer_builds():
    """Every case's So, pitches and padding are ConvLayer's own for that layer (the stride divides S - f + 1)."""
    from theanet_amd.device import c8_pool_pitch
    for case in GC.CASES:
        N, C, S, P, K, f, stride, mode, So, Po = case
        g = _layer_geom(N, C, S, K, f, stride, mode)
        assert g is not None and g[7:9] == GC.geom(case)[7:9], case
        assert P in (S, c8_pool_pitch(S)) and Po in (So, c8_pool_pitch(So)), case


# ---- the host's decisions ---------------------------------------------------------------------------------------------
def _choose(shapes, c, side, in_pitch, k, f, stride, mode, n=16):
    from theanet_amd import _lib
    from theanet_amd.layer.c8 import choose_conv
    g = _layer_geom(n, c, side, k, f, stride, mode)
    return choose_conv(_lib.get_lib(), "bfloat16", shapes, n, c, side, in_pitch, k, f, stride, mode, g[7], g[8])


def test_family_choice_and_pitch_rule():
    # mnist conv1 / conv2: refused as today without the switch, the general family with it
    for args in ((1, 28, None, 4, 3, 1, "valid"), (4, 13, 16, 20, 3, 1, "valid"), (16, 16, 16, 16, 5, 1, "same"),
                 (16, 16, 16, 16, 1, 2, "valid"), (3, 80, None, 8, 3, 1, "same"), (8, 16, 16, 20, 3, 1, "same")):
        with pytest.raises(AssertionError, match="DTYPE bfloat16 needs 3x3 stride-1 'same' conv layers"):
            _choose("tiled", *args)
        fam, one, P, Po = _choose("any", *args)
        assert fam.fwd == "tn_c8_convg_fwd" and not (fam.tiles or fam.pad_zero or fam.pools or one), args
    fam, _, P, Po = _choose("any", 1, 28, None, 4, 3, 1, "valid")
    assert (P, Po) == (32, 32) and fam.geom == (16, 1, 28, 32, 4, 3, 1, 0, 26, 32)
    fam, _, P, Po = _choose("any", 4, 13, 16, 20, 3, 1, "valid")
    assert (P, Po) == (16, 16) and fam.geom == (16, 4, 13, 16, 20, 3, 1, 0, 11, 16)
    assert _choose("any", 3, 12, 16, 10, 5, 1, "valid")[2:] == (16, 8)                    # the pitch shrinks with the map
    assert _choose("any", 3, 80, None, 8, 3, 1, "same")[2:] == (80, 80)                   # dense above 64 pixels
    assert _choose("any", 3, 72, None, 8, 5, 1, "valid")[2:] == (72, 68)
    assert _choose("any", 8, 66, 66, 8, 3, 1, "valid")[2:] == (66, 64)
    assert _choose("any", 8, 4, 8, 16, 4, 1, "valid")[0].geom[-2:] == (1, 8)
    # shapes the tiled predicates accept keep their family, with or without the switch
    for args in ((3, 16, None, 16, 3, 1, "same"), (16, 12, 16, 32, 3, 1, "same"), (16, 16, 16, 20, 1, 1, "valid"),
                 (3, 28, None, 12, 1, 1, "same")):
        assert _choose("tiled", *args) == _choose("any", *args)
        fam, one, P, Po = _choose("any", *args)
        assert fam.pools and P == Po and fam.fwd == ("tn_c8_conv1_fwd" if one else "tn_c8_conv_fwd")
        assert fam.tiles == fam.pad_zero == (not one)


def _below(kind, out_sz=None, fam=None):
    return type(kind, (), {"out_sz": out_sz, "c8_fam": fam})()


def test_pool_decision():
    from theanet_amd.layer.c8 import check_follows, pool_stands_alone
    general = _choose("any", 4, 13, 16, 20, 3, 1, "valid")[0]
    tiled = _choose("any", 3, 16, None, 16, 3, 1, "same")[0]
    for out_sz in (11, 12):
        # a general-family layer is never fused; today's answer without the switch (construction has refused it before)
        assert pool_stands_alone(2, True, _below("ConvLayer", out_sz, general), True)
        check_follows("bfloat16", _below("ConvLayer", out_sz, general), "PoolLayer", 2, True, True)
    assert not pool_stands_alone(2, True, _below("ConvLayer", 16, tiled), True)             # the fused block stays
    assert pool_stands_alone(2, True, _below("ConvLayer", 13, tiled), True)                 # 2x2 on an odd map
    check_follows("bfloat16", _below("ConvLayer", 13, tiled), "PoolLayer", 2, True, True)
    assert not pool_stands_alone(2, True, _below("ConvLayer", 13, tiled), False)
    with pytest.raises(AssertionError, match="2x2 on even maps"):
        check_follows("bfloat16", _below("ConvLayer", 13, tiled), "PoolLayer", 2, True)
    for any_shapes in (False, True):
        assert pool_stands_alone(3, True, _below("ConvLayer", 16, tiled), any_shapes)
        assert pool_stands_alone(2, False, _below("ConvLayer", 16, tiled), any_shapes)
        assert not pool_stands_alone(2, True, _below("DropOutLayer"), any_shapes)          # refused by the grammar as today
        with pytest.raises(AssertionError, match="breaks the fused"):
            check_follows("bfloat16", _below("DropOutLayer"), "PoolLayer", 2, True, any_shapes)


def test_cpu_backend_has_only_stubs():
    from theanet_amd import _lib
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    h = ctypes.c_void_p()
    assert lib.tn_ctx_create(0, ctypes.byref(h)) == 0
    try:
        buf = (ctypes.c_uint16 * (16 * 16 * 8 * 2))()
        p = ctypes.addressof(buf)
        g = (2, 8, 12, 16, 8, 3, 1, 0, 10, 16)
        assert lib.tn_c8_convg_supported(*g) == 0
        assert lib.tn_c8_convg_fwd(h, p, p, p, p, *g, 0, 0.) != 0
        assert b"tn_c8_convg_fwd: not provided by the CPU backend" in lib.tn_last_error(h)
        assert lib.tn_c8_convg_dgrad(h, p, p, p, *g, None, 0, 0.) != 0
        assert b"tn_c8_convg_dgrad: not provided by the CPU backend" in lib.tn_last_error(h)
        assert lib.tn_c8_convg_wgrad(h, p, p, p, p, *g) != 0
        assert b"tn_c8_convg_wgrad: not provided by the CPU backend" in lib.tn_last_error(h)
        out = (ctypes.c_int * 8)()
        assert all(lib.tn_c8_convg_plan(op, *g, 0, 0., out, 8) < 0 for op in (0, 1, 2))
        assert not any(buf)
    finally:
        lib.tn_ctx_destroy(h)


CODE = """
import numpy as np
from theanet_amd import NeuralNet
layers = [("InputLayer", {"img_sz": 12, "num_maps": 1}),
          ("ConvLayer", {"num_maps": 4, "filter_sz": 3, "stride": 1, "mode": "valid", "actvn": "relu10"}),
          ("PoolLayer", {"pool_sz": 2}), ("HiddenLayer", {"n_out": 24, "actvn": "tanh"}), ("SoftmaxLayer", {"n_out": 10})]
tp = {"SEED": 3, "BATCH_SZ": 16, "NUM_EPOCHS": 1, "INIT_LEARNING_RATE": .05, "EPOCHS_TO_HALF_RATE": 2}
rng = np.random.RandomState(0)
x, y = rng.rand(32, 1, 12, 12).astype(np.float32), rng.randint(0, 10, 32).astype(np.int32)
try:
    NeuralNet(layers, dict(tp, CONV_SHAPES="all"))
except AssertionError as e:
    print("ASSERTED: %s" % e)
costs = []
for extra in ({}, {"CONV_SHAPES": "tiled"}, {"CONV_SHAPES": "any"}):
    net = NeuralNet(layers, dict(tp, **extra))
    assert net.tr_layers[1].args[-1] == extra.get("CONV_SHAPES", "tiled") == net.te_layers[1].args[-1]
    fn = net.get_trin_model(x, y)
    costs.append([float(fn(s)[0]) for s in range(2)])
assert costs[0] == costs[1] == costs[2] and np.isfinite(costs[0]).all(), costs
print("SAME BITS")
"""


def test_conv_shapes_param_on_a_float32_net():
    """On the CPU backend (a child process, tests/test_conv_param_cpu.py): an unknown value is an assertion that names the
    key; under DTYPE float32 'any' is accepted, reaches the conv layers of both graphs and changes no bit."""
    env = dict(os.environ, THEANET_BACKEND="cpu", OMP_NUM_THREADS="4", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CODE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ASSERTED: CONV_SHAPES must be 'tiled' or 'any'" in r.stdout and "SAME BITS" in r.stdout, r.stdout
