"""The strided PoolLayer of the 16-bit conv stack, the parts that need no GPU: the capability query against the output-side
rule, the CPU backend's refusal of the ops, and the coverage of the kernels' instantiations by the op cases of
tests/test_gpu_pool_st.py (the scheme of tests/test_c8_pool_cpu.py).

The launchers of theanet_amd/csrc/pools_c8.hip choose c8_pool_st_fwd_kernel<PW, ST, SH> / c8_pool_st_bwd_kernel<E, PW,
ST, SH> from host-only geometry: (PW, ST) the window and stride as compile-time constants -- (3, 2), (2, 1) -- or (0, 0)
for the run-time loops, SH whether the pitch the op's lanes are laid over (forward: the output's, backward: the input's)
is a power of two.  tn_c8_pool_st_plan runs that selection without a device; a sweep collects every instantiation it
reaches, and the GPU cases must reach exactly those."""
import ctypes
import functools

from tests import test_gpu_pool_st as GS
from tests.test_pool_st_cpu import out_side


def test_cpu_backend_refuses_the_strided_pool_ops():
    """The CPU backend answers the ops with its "not here" error, the capability query with 0 and the plan with an error."""
    from theanet_amd import _lib
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    h = ctypes.c_void_p()
    assert lib.tn_ctx_create(0, ctypes.byref(h)) == 0
    try:
        buf = (ctypes.c_uint16 * (8 * 8 * 8))()
        p = ctypes.addressof(buf)
        geom = (1, 8, 6, 8, 3, 2, 3, 8)
        assert lib.tn_c8_pool_st_supported(*geom) == 0
        assert lib.tn_c8_pool_st_fwd(h, p, p, *geom) != 0
        assert b"tn_c8_pool_st_fwd: not provided by the CPU backend" in lib.tn_last_error(h)
        assert lib.tn_c8_pool_st_bwd(h, p, p, p, p, *geom) != 0
        assert b"tn_c8_pool_st_bwd: not provided by the CPU backend" in lib.tn_last_error(h)
        out = (ctypes.c_int * 8)()
        assert lib.tn_c8_pool_st_plan(0, *geom, out, 8) < 0 and lib.tn_c8_pool_st_plan(1, *geom, out, 8) < 0
        assert not any(buf)
    finally:
        lib.tn_ctx_destroy(h)


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    out = (ctypes.c_int * 8)()

    def plan(op, geom):
        n = lib.tn_c8_pool_st_plan(op, *geom, out, 8)
        return tuple(out[:n]) if n > 0 else None
    assert plan(0, (2, 8, 6, 8, 3, 2, 3, 8)), "tn_c8_pool_st_plan answers nothing (CPU backend loaded?)"
    return plan


def _reach(geoms):
    insts = set()
    for g in geoms:
        for op in (0, 1):
            pl = _query()(op, g)
            if pl is not None:
                insts.add((("fwd", "bwd")[op],) + pl[:3])
    return insts


def _sweep_geoms():
    from theanet_amd.device import c8_pitch, c8_pool_pitch
    for p in range(2, 7):
        for st in range(1, 8):
            for S in list(range(1, 80)) + [129, 131, 200]:
                for P in {S, c8_pitch(S)} if S <= 64 else {S}:
                    for So in {out_side(S, p, st, False)} | ({out_side(S, p, st, True)} if S >= p else set()):
                        yield 3, 12, S, P, p, st, So, c8_pool_pitch(So)


def test_supported_is_the_output_side_rule():
    """For every S, p, st of a sweep the query accepts exactly the two sides of Theano's rule (one where they coincide or
    the window does not fit), and the old family's answer at st = p."""
    from theanet_amd import _lib
    from theanet_amd.device import c8_pool_pitch
    lib = _lib.get_lib()
    for S in range(1, 41):
        for p in range(2, 8):
            for st in range(1, 9):
                sides = {out_side(S, p, st, False)} | ({out_side(S, p, st, True)} if S >= p else set())
                for So in range(0, S + 2):
                    got = bool(lib.tn_c8_pool_st_supported(5, 12, S, S, p, st, So, c8_pool_pitch(max(So, 1))))
                    assert got == (So in sides and So >= 1), (S, p, st, So)
                    if st == p:
                        assert got == bool(lib.tn_c8_pool_supported(5, 12, S, S, p, So, c8_pool_pitch(max(So, 1)))), (S, p, So)
    for bad in ((5, 12, 8, 8, 1, 1, 8, 8), (5, 12, 8, 8, 65, 2, 1, 8), (5, 12, 8, 8, 3, 0, 3, 8), (5, 12, 8, 8, 3, 65, 1, 8),
                (5, 12, 8, 12, 3, 2, 4, 8), (5, 12, 8, 8, 3, 2, 4, 6), (1 << 20, 64, 64, 64, 3, 2, 32, 32)):
        assert not lib.tn_c8_pool_st_supported(*bad), bad
    assert lib.tn_c8_pool_st_supported(5, 12, 200, 200, 64, 64, 4, 8) and lib.tn_c8_pool_st_supported(5, 12, 8, 8, 3, 2, 4, 8)


def test_plan_query_runs_the_launchers_selection():
    plan = _query()
    assert plan(0, (2048, 32, 32, 32, 3, 2, 16, 16)) == (3, 2, 1, 2048 * 4 * 16 * 16 // 256)
    assert plan(1, (2048, 32, 32, 32, 3, 2, 16, 16)) == (3, 2, 1, 2048 * 4 * 32 * 32 // 256)
    assert plan(0, (2, 8, 12, 12, 2, 1, 11, 16))[:3] == (2, 1, 1) and plan(1, (2, 8, 12, 12, 2, 1, 11, 16))[:3] == (2, 1, 0)
    assert plan(0, (2, 8, 12, 16, 3, 1, 10, 16))[:3] == (0, 0, 1) and plan(0, (2, 8, 12, 16, 2, 2, 6, 8))[:3] == (0, 0, 1)
    assert plan(0, (2, 8, 131, 131, 3, 2, 65, 65))[:3] == (3, 2, 0)
    assert plan(0, (2, 8, 10, 10, 5, 2, 5, 8)) is None and plan(0, (2, 8, 10, 10, 1, 1, 10, 16)) is None    # So, p = 1
    assert plan(2, (2, 8, 12, 12, 2, 1, 11, 16)) is None                                                   # no such op
    assert plan(0, (2, 8, 10, 10, 3, 0, 4, 8)) is None                                                     # st = 0


def test_supported_geometries_have_a_plan():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    n = 0
    for g in _sweep_geoms():
        ok = bool(lib.tn_c8_pool_st_supported(*g))
        assert ok == (g[6] >= 1), g
        assert (_query()(0, g) is not None) == ok and (_query()(1, g) is not None) == ok, g
        n += ok
    assert n > 1000


def test_gpu_cases_reach_every_instantiation():
    """The op cases of tests/test_gpu_pool_st.py launch exactly the instantiations the sweep reaches: both ops, the three
    (window, stride) forms, shifts and divisions."""
    insts = _reach(_sweep_geoms())
    assert insts == {(op, pw, st, sh) for op in ("fwd", "bwd") for pw, st in ((0, 0), (2, 1), (3, 2)) for sh in (0, 1)}
    got = _reach(GS.pool_st_geom(c) for c in GS.CASES)
    assert not got - insts, sorted(got - insts)
    assert not insts - got, "instantiations no case of tests/test_gpu_pool_st.py launches: %s" % sorted(insts - got)
