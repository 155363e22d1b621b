"""The stand-alone PoolLayer of the 16-bit conv stack, the parts that need no GPU: the output pitch rule, the stack's
grammar (c8.check_follows) over a table of spellings, the CPU backend's refusal of the ops, and the coverage of the
kernels' instantiations by the op cases of tests/test_gpu_c8_pool.py (the scheme of tests/test_c8_dispatch.py).

The launchers of theanet_amd/csrc/pool_c8.hip choose c8_pool_fwd_kernel<PW, SH> / c8_pool_bwd_kernel<PW, SH> from
host-only geometry: PW the window as a compile-time constant (2, 3) or 0 for the run-time loop, SH whether the pitch the
op's lanes are laid over (forward: the output's, backward: the input's) is a power of two (shifts) or not (divisions).
tn_c8_pool_plan runs that selection without a device; a sweep collects every instantiation it reaches, and the GPU cases
must reach exactly those."""
import ctypes
import functools

import pytest

from tests import test_gpu_c8_pool as GP


def test_pitch_rule():
    """c8_pitch(So) up to 64 pixels -- a 3x3 conv can follow a 4 x 4 result -- and dense above."""
    from theanet_amd.device import c8_pitch, c8_pool_pitch
    want = {1: 8, 2: 8, 4: 8, 5: 8, 11: 16, 32: 32, 43: 64, 64: 64, 65: 65}
    assert {s: c8_pool_pitch(s) for s in want} == want
    assert all(c8_pool_pitch(s) == c8_pitch(s) for s in range(1, 65)) and c8_pool_pitch(200) == 200


def _below(kind, out_sz=None):
    return type(kind, (), {"out_sz": out_sz})()


# (layer below, its map side, kind, pool_sz, fuse_conv_pool) -> None: accepted, or a fragment of the refusal
GRAMMAR = [
    (("ConvLayer", 8), "PoolLayer", 2, True, None),                        # the fused block
    (("ConvLayer", 7), "PoolLayer", 2, True, "2x2 on even maps"),          # pinned: tests/test_gpu_c8_pitch.py
    (("DropOutLayer", None), "PoolLayer", 2, True,
     "between a ConvLayer and its PoolLayer breaks the fused"),            # pinned: tests/test_gpu_c8_dropout.py
    (("PoolLayer", 8), "PoolLayer", 2, True, "must directly follow a ConvLayer"),
    (("ConvLayer", 8), "PoolLayer", 3, True, None),                        # stand-alone: any window but the fused 2x2 ...
    (("ConvLayer", 7), "PoolLayer", 3, True, None),
    (("ConvLayer", 8), "PoolLayer", 8, True, None),
    (("PoolLayer", 8), "PoolLayer", 3, True, None),                        # ... above a Pool or a DropOut layer
    (("DropOutLayer", None), "PoolLayer", 3, True, None),
    (("HiddenLayer", None), "PoolLayer", 3, True, "a stand-alone PoolLayer follows a Conv, Pool or DropOut layer"),
    (("ConvLayer", 7), "PoolLayer", 2, False, None),                       # without fusing every pool stands alone
    (("ConvLayer", 8), "PoolLayer", 2, False, None),
    (("DropOutLayer", None), "PoolLayer", 2, False, None),
    (("PoolLayer", 7), "PoolLayer", 2, False, None),
    (("PoolLayer", 4), "ConvLayer", None, True, None),                     # what may follow a pool
    (("PoolLayer", 4), "DropOutLayer", None, True, None),
    (("PoolLayer", 4), "MeanLayer", None, True, None),
    (("PoolLayer", 4), "HiddenLayer", None, True, None),
    (("PoolLayer", 4), "SoftmaxLayer", None, True, "a HiddenLayer must follow the conv stack"),
    (("PoolLayer", 4), "ElasticLayer", None, True, "only Conv / Pool / Mean / DropOut layers"),
]


@pytest.mark.parametrize("below,kind,pool_sz,fused,refusal", GRAMMAR)
def test_check_follows(below, kind, pool_sz, fused, refusal):
    from theanet_amd.layer.c8 import check_follows, pool_stands_alone
    if refusal is None:
        check_follows("bfloat16", _below(*below), kind, pool_sz, fused)
    else:
        with pytest.raises(AssertionError, match=refusal):
            check_follows("bfloat16", _below(*below), kind, pool_sz, fused)
    if kind == "PoolLayer":
        assert pool_stands_alone(pool_sz, fused) == (not fused or pool_sz != 2)


def test_cpu_backend_refuses_the_pool_ops():
    """The CPU backend answers the ops with its "not here" error, the capability query with 0 and the plan with an error."""
    from theanet_amd import _lib
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    h = ctypes.c_void_p()
    assert lib.tn_ctx_create(0, ctypes.byref(h)) == 0
    try:
        buf = (ctypes.c_uint16 * (8 * 8 * 8))()
        p = ctypes.addressof(buf)
        geom = (1, 8, 6, 8, 3, 2, 8)
        assert lib.tn_c8_pool_supported(*geom) == 0
        assert lib.tn_c8_pool_fwd(h, p, p, *geom) != 0
        assert b"tn_c8_pool_fwd: not provided by the CPU backend" in lib.tn_last_error(h)
        assert lib.tn_c8_pool_bwd(h, p, p, p, p, *geom) != 0
        assert b"tn_c8_pool_bwd: not provided by the CPU backend" in lib.tn_last_error(h)
        out = (ctypes.c_int * 8)()
        assert lib.tn_c8_pool_plan(0, *geom, out, 8) < 0 and lib.tn_c8_pool_plan(1, *geom, out, 8) < 0
        assert not any(buf)
    finally:
        lib.tn_ctx_destroy(h)


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 8)()

    def plan(op, geom):
        n = lib.tn_c8_pool_plan(op, *geom, out, 8)
        return tuple(out[:n]) if n > 0 else None
    assert plan(0, (2, 8, 6, 8, 3, 2, 8)), "tn_c8_pool_plan answers nothing (CPU backend loaded?)"
    return plan


def _reach(geoms):
    insts = set()
    for g in geoms:
        for op in (0, 1):
            pl = _query()(op, g)
            if pl is not None:
                insts.add((("fwd", "bwd")[op],) + pl[:2])
    return insts


def _sweep_geoms():
    from theanet_amd.device import c8_pitch, c8_pool_pitch
    for p in range(2, 9):
        for S in range(1, 300):
            for P in {S, c8_pitch(S)} if S <= 64 else {S}:
                for So in {S // p, -(-S // p)}:
                    yield 3, 12, S, P, p, So, c8_pool_pitch(So)


def test_plan_query_runs_the_launchers_selection():
    plan = _query()
    assert plan(0, (2048, 32, 32, 32, 3, 11, 16)) == (3, 1, 2048 * 4 * 16 * 16 // 256)
    assert plan(1, (2048, 32, 32, 32, 3, 11, 16)) == (3, 1, 2048 * 4 * 32 * 32 // 256)
    assert plan(0, (2, 8, 130, 130, 2, 65, 65))[:2] == (2, 0) and plan(1, (2, 8, 130, 130, 2, 65, 65))[:2] == (2, 0)
    assert plan(0, (2, 8, 10, 10, 5, 2, 8))[:2] == (0, 1) and plan(1, (2, 8, 10, 10, 5, 2, 8))[:2] == (0, 0)
    assert plan(0, (2, 8, 10, 10, 5, 3, 8)) is None and plan(0, (2, 8, 10, 10, 1, 10, 16)) is None     # So, p = 1
    assert plan(2, (2, 8, 10, 10, 5, 2, 8)) is None                                                    # no such op
    assert _query()(0, (2, 8, 5, 8, 7, 0, 8)) is None                                                  # So = 0


def test_supported_geometries_have_a_plan():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    n = 0
    for g in _sweep_geoms():
        ok = bool(lib.tn_c8_pool_supported(*g))
        assert ok == (g[5] >= 1), g
        assert (_query()(0, g) is not None) == ok and (_query()(1, g) is not None) == ok, g
        n += ok
    assert n > 1000


def test_gpu_cases_reach_every_instantiation():
    """The op cases of tests/test_gpu_c8_pool.py launch exactly the instantiations the sweep reaches: both ops, the three
    windows, shifts and divisions."""
    insts = _reach(_sweep_geoms())
    assert insts == {(op, pw, sh) for op in ("fwd", "bwd") for pw in (0, 2, 3) for sh in (0, 1)}
    got = _reach(GP.pool_geom(c) for c in GP.CASES)
    assert not got - insts, sorted(got - insts)
    assert not insts - got, "instantiations no case of tests/test_gpu_c8_pool.py launches: %s" % sorted(insts - got)
