"""Coverage of the fp32 dense-layer kernels' instantiations by the GPU tests of tests/test_gpu_kernels.py, checked on
the CPU.

tn_fc_fwd, tn_fc_fwd_dropout, tn_fc_wgrad, tn_fc_dgrad, tn_fc_bwd, tn_fc_softmax_nll and tn_fc_softmax_train choose among
the kernels of theanet_amd/csrc/gemm.hip and fc_skinny.hip from the shape, the operands' alignment, the CU count and the
knobs.  tn_fc_plan runs that same selection (the plan functions the entry points themselves call) without a device.  A
sweep at 256 CUs over the shapes the configs use collects every reachable instantiation, and every (instantiation, edge)
pair; the launches the GPU tests make (test_gpu_kernels.fc_launches) must reach both sets exactly, so a new variant or a
dispatch change fails here until a GPU case covers it.

Instantiations:
  (kernel, AKC, BKC, BSUM, tile rows, stages)   the gemm_f32_* kernels; one product of a pair launch counts as one
  (kernel, NOUT, RB)                            the matrix-core skinny kernels
  (kernel,)                                     the scalar skinny kernels

Edges (where tiling goes wrong).  Gemm kernels, on the product's own M x N x K (forward B x n_out x n_in, weight
gradient n_in x n_out x B, input gradient B x n_in x n_out):
  M_tail      the last row tile is partial (tiles of 64 or 128 rows; deep: 32)
  N_tail      the last column tile is partial (64 columns; deep: 32)
  K_tail      the last slab's depth is not a multiple of 16
  slabs       more than one K slab (a finishing or reduction launch follows)
  short_slab  the last slab is shorter than the others
  c_scalar    the 16-byte epilogue is not taken
  few_cols    a forward of n_out <= 16 columns on the tiled route: a skinny layer that neither the matrix-core kernels
              (n_in % 4 != 0 or unaligned operands) nor the scalar kernel (W beyond its 60 KiB of LDS) can take
  mask / no_mask, prev / bare, drop
              the epilogue forms the op admits: forward with / without a dropout mask, input gradient with / without
              prev_a and mask, dropout drawn inline (a product split over K leaves them to its finishing kernel)
Skinny kernels:
  rows        a partial row block (16 rows forward, 8 rows input gradient; scalar: 8 forward, 16 input gradient)
  slab_tail   a partial row slab (128 rows; RB rows in softmax train; scalar weight gradient: 64)
  slabs       more than one row slab
  k_rem       n_in % 64 != 0: the last 64-wide weight-gradient block is partial and holds the db row (k = n_in)
  K_tail      forward: n_in % 16 != 0 (chunks of 16 per MFMA step; scalar: the 32 k-lanes)
  N_tail      input gradient: a partial column group (128 float4 columns; scalar: 256 columns)
  d_odd       pair: an odd number of 128-thread input-gradient blocks (the last block's second half is idle)
  passes      scalar forward: n_in > 512, several passes over x
  softmax     forward with the softmax / NLL tail (tn_fc_softmax_nll)
  mask / no_mask, prev / bare as above
"""
import ctypes
import functools

import pytest

from tests import test_gpu_kernels as G
from tests.test_abi import KNOB_DEFAULTS

CUS = 256
F_UNAL, F_BARE, F_RIDER, F_ELEM = 1, 2, 4, 8
OP_FWD, OP_DROP, OP_WGRAD, OP_DGRAD, OP_BWD, OP_NLL, OP_TRAIN = range(7)
NINTS = 17
KERNELS = ("generic", "fast", "dma", "deep", "pair", "pair_dma", "sc_fwd", "sc_wgrad", "sc_dgrad", "sk_fwd", "sk_wgrad",
           "sk_dgrad", "sk_pair", "sk_train")

# dense around the thresholds of the selection (64 / 128-row tiles, 16-deep K tiles, 256-deep DMA slabs, the split rules'
# 256 rows / 512 / 1024 / 2048 features, the skinny kernels' 8 / 16 / 128 rows and RB's 2048) and multiples of 4 .. 128,
# up to the largest shapes of the configs (8192 rows; wide6's 16384 x 1024)
BS = [1, 3, 4, 5, 8, 15, 16, 17, 32, 33, 37, 63, 64, 65, 100, 127, 128, 129, 133, 200, 255, 256, 257, 300, 511, 512, 513,
      1000, 1023, 1024, 1025, 1100, 2047, 2048, 2050, 4096, 8192, 8200]
N_INS = [1, 3, 4, 5, 7, 8, 12, 15, 16, 17, 30, 32, 33, 36, 63, 64, 65, 68, 100, 127, 128, 129, 252, 256, 260, 500, 511, 512,
         513, 516, 720, 1023, 1024, 1028, 1030, 2044, 2047, 2048, 2052, 2304, 4096, 4100, 4600, 5112, 16384]
N_OUTS = list(range(1, 18)) + [20, 30, 31, 32, 33, 36, 63, 64, 65, 70, 96, 100, 127, 128, 129, 130, 255, 256, 257, 260, 457,
                               500, 508, 511, 512, 513, 516, 520, 724, 1000, 1023, 1024]
OP_FLAGS = {OP_FWD: (0, F_BARE, F_UNAL, F_UNAL | F_BARE), OP_DROP: (0, F_UNAL, F_ELEM), OP_WGRAD: (0, F_UNAL),
            OP_DGRAD: (0, F_BARE, F_UNAL, F_UNAL | F_BARE), OP_BWD: (0, F_BARE, F_UNAL, F_UNAL | F_BARE, F_RIDER),
            OP_NLL: (0, F_UNAL), OP_TRAIN: (0, F_BARE, F_UNAL, F_UNAL | F_BARE)}


@functools.lru_cache(maxsize=None)
def _query():
    from theanet_amd import _lib
    lib = _lib.get_lib()
    buf = ctypes.create_string_buffer(4096)
    assert lib.tn_knobs(buf, len(buf)) == 0
    knobs = dict(kv.split("=") for kv in buf.value.decode().split())
    off = sorted(k for k, v in KNOB_DEFAULTS.items() if int(knobs[k]) != v)
    if off:
        pytest.skip("the dispatch coverage holds for the default selection only; unset " + ", ".join(off))
    out = (ctypes.c_int * (3 * NINTS))()
    f = lib.tn_fc_plan

    def plan(op, B, n_in, n_out, flags=0, cus=CUS):
        n = f(op, B, n_in, n_out, cus, flags, out, 3 * NINTS)
        if n <= 0:
            return None
        v = out[:n]
        return tuple(tuple(v[i:i + NINTS]) for i in range(0, n, NINTS))
    assert plan(OP_FWD, 64, 720, 500), "tn_fc_plan answers nothing (CPU backend loaded?)"
    return plan


def _classify_prod(op, B, n_in, n_out, flags, p):
    fam, ker, akc, bkc, bsum, tile_m, stages, c_vec, S, kchunk, MT, NT, finish, drop, nout, rb, rider = p
    name = KERNELS[ker]
    bare = bool(flags & F_BARE)
    e = {}
    if ker <= 5:                                           # the gemm kernels
        inst = (name, akc, bkc, bsum, tile_m, stages)
        M, N, K = (n_in, n_out, B) if bsum else (B, n_in, n_out) if bkc else (B, n_out, n_in)
        last = K - (S - 1) * kchunk
        assert 0 < last <= kchunk and MT == -(-M // tile_m) and NT == -(-N // (32 if name == "deep" else 64))
        assert finish == (S > 1) or (not bsum and finish and S == 1)
        e = {"M_tail": M % tile_m != 0, "N_tail": N % (32 if name == "deep" else 64) != 0, "K_tail": last % 16 != 0,
             "slabs": S > 1, "short_slab": S > 1 and last < kchunk, "c_scalar": not c_vec, "drop": bool(drop)}
        if not bsum and not bkc and not finish and not drop and op == OP_FWD:
            e["no_mask" if bare else "mask"] = True
        e["few_cols"] = not bsum and not bkc and n_out <= 16
        if bkc and not finish:
            e["bare" if bare else "prev"] = True
    elif name.startswith("sc_"):
        inst = (name,)
        if name == "sc_fwd":
            e = {"rows": B % 8 != 0, "K_tail": n_in % 32 != 0, "passes": n_in > 512, "softmax": op in (OP_NLL, OP_TRAIN)}
            if op == OP_FWD:
                e["no_mask" if bare else "mask"] = True
        elif name == "sc_wgrad":
            e = {"slab_tail": B % 64 != 0, "slabs": S > 1, "N_tail": n_in % 256 != 0}
        else:
            e = {"rows": B % 16 != 0, "N_tail": n_in % 256 != 0, "bare" if bare else "prev": True}
    else:
        inst = (name, nout, rb)
        assert nout == (0 if name in ("sk_fwd", "sk_wgrad") else n_out) and (rb > 0) == (name == "sk_train")
        if name == "sk_fwd":
            e = {"rows": B % 16 != 0, "K_tail": n_in % 16 != 0, "softmax": op in (OP_NLL, OP_TRAIN)}
            if op == OP_FWD:
                e["no_mask" if bare else "mask"] = True
        if name in ("sk_wgrad", "sk_pair"):
            e.update({"slab_tail": B % 128 != 0, "slabs": S > 1, "k_rem": n_in % 64 != 0})
        if name in ("sk_dgrad", "sk_pair"):
            e.update({"rows": B % 8 != 0, "N_tail": (n_in // 4) % 128 != 0, "bare" if bare else "prev": True})
        if name == "sk_pair":
            e["d_odd"] = (-(-(n_in // 4) // 128) * -(-B // 8)) % 2 == 1
        if name == "sk_train":
            e = {"slab_tail": B % rb != 0, "slabs": S > 1, "K_tail": n_in % 16 != 0, "k_rem": n_in % 64 != 0,
                 "bare" if bare else "prev": True}
    return inst, {k for k, on in e.items() if on}


def classify(op, B, n_in, n_out, flags=0):
    """[(instantiation, set of edges)] of the products one tn_fc_* call launches; [] where the call refuses."""
    plan = _query()(op, B, n_in, n_out, flags)
    return [_classify_prod(op, B, n_in, n_out, flags, p) for p in plan or ()]


def _reach(calls):
    insts, pairs = set(), set()
    for c in calls:
        for inst, edges in classify(*c):
            insts.add(inst)
            pairs.update((inst, e) for e in edges)
    return insts, pairs


def _sweep_calls():
    for op, flagset in OP_FLAGS.items():
        for B in BS:
            for n_in in N_INS:
                if B * n_in > 8192 * 1024 * 2:
                    continue
                for n_out in N_OUTS:
                    for fl in flagset:
                        yield op, B, n_in, n_out, fl


@functools.lru_cache(maxsize=None)
def sweep():
    return _reach(_sweep_calls())


@functools.lru_cache(maxsize=None)
def gpu_reach():
    return _reach(G.fc_launches())


def _fmt(s):
    return "\n  ".join(sorted(map(str, s)))


def _inst_edges(inst):
    """The edges an instantiation could have at all."""
    name = inst[0]
    if name in KERNELS[:6]:
        _, akc, bkc, bsum, tile_m, stages = inst
        e = ["M_tail", "N_tail", "K_tail", "slabs", "short_slab", "c_scalar"]
        if akc and not bkc and not name.startswith("pair"):
            e += ["mask", "no_mask", "drop", "few_cols"]
        if bkc:
            e += ["prev", "bare"]
        return e
    return {"sc_fwd": ["rows", "K_tail", "passes", "softmax", "mask", "no_mask"],
            "sc_wgrad": ["slab_tail", "slabs", "N_tail"],
            "sc_dgrad": ["rows", "N_tail", "prev", "bare"],
            "sk_fwd": ["rows", "K_tail", "softmax", "mask", "no_mask"],
            "sk_wgrad": ["slab_tail", "slabs", "k_rem"],
            "sk_dgrad": ["rows", "N_tail", "prev", "bare"],
            "sk_pair": ["slab_tail", "slabs", "k_rem", "rows", "N_tail", "d_odd", "prev", "bare"],
            "sk_train": ["slab_tail", "slabs", "K_tail", "k_rem", "prev", "bare"]}[name]


# Why an (instantiation, edge) pair cannot occur, or None.  test_unreachable_edges_are_the_documented_ones checks that
# these are exactly the pairs missing from the sweep, so each reason holds for the real selection (within the sweep's
# shapes, n_out <= 1024, and tn_fc_plan's flags, which misalign all operands together).
def _why_unreachable(inst, edge):
    name = inst[0]
    if name not in KERNELS[:6]:
        return None                                        # every edge of the skinny and scalar kernels occurs
    _, akc, bkc, bsum, tile_m, stages = inst
    if edge == "few_cols":
        # ... and what the scalar kernel cannot hold is a reduction of >= 904 features: split over K
        return None if name == "generic" else "x rows or operands that the skinny kernels refuse are not 16-byte aligned"
    if name == "deep":
        if edge in ("slabs", "short_slab"):
            return "the deep kernel splits K over its waves, never over slabs"
        if edge == "c_scalar":
            return "gemm_deep_ok asks for the 16-byte epilogue"
        return None
    if name == "generic":
        return "the inline dropout needs gemm_fast_ok" if edge == "drop" else None
    if edge == "c_scalar" and not bkc:
        # forward and weight gradient: B is row-contiguous, so gemm_fast_ok asks N % 4 == 0 of aligned operands -- all
        # the 16-byte epilogue asks (an elem0 % 4 != 0 sends tn_fc_fwd_dropout to the two-launch form, where elem0 is 0)
        return "a fast kernel with a row-contiguous B already has N % 4 == 0 and aligned operands"
    if edge == "c_scalar" and name.startswith("pair"):
        return "the pair needs the weight gradient on the fast kernel: n_in % 4 == 0, all the input gradient's epilogue asks"
    if edge in ("slabs", "short_slab") and bkc:
        if name.startswith("pair"):
            return "the pair launch runs an unsplit input gradient only"
        if name == "dma":
            return "a split input gradient has slabs of <= 144 (n_out <= 1024: S = min(8, n_out / 128)); the ring needs 256"
    if edge in ("slabs", "short_slab") and name == "dma" and akc and not bkc and stages == 4:
        return "a forward is split to reach two blocks per CU, never more: the 8-stage ring"
    return None


def test_plan_query_runs_the_launchers_selection():
    """Spot checks of the query against the documented selection."""
    plan = _query()
    fwd = plan(OP_FWD, 4096, 720, 500)[0]                  # the headline's fc1: 512 blocks = two per CU, the deep ring
    assert (KERNELS[fwd[1]], fwd[2:7], fwd[8]) == ("dma", (1, 0, 0, 64, 8), 1)
    assert plan(OP_FWD, 4100, 720, 500)[0][6] == 4         # more than two blocks per CU: four stages
    assert KERNELS[plan(OP_FWD, 512, 720, 500)[0][1]] == "deep"
    assert KERNELS[plan(OP_FWD, 512, 720, 500, F_UNAL)[0][1]] == "generic"
    assert plan(OP_FWD, 8192, 720, 500)[0][5] == 128       # 64 x 8 tiles of 128 x 64 = 2 per CU
    w = plan(OP_WGRAD, 4096, 720, 500)[0]
    assert w[2:5] == (0, 0, 1) and w[8] == 8 and w[9] == 512 and w[12] == 1
    d = plan(OP_DGRAD, 128, 16384, 1024)[0]                # wide6: split-K input gradient + finishing kernel
    assert d[2:5] == (1, 1, 0) and d[8] == 8 and d[12] == 1
    pair = plan(OP_BWD, 4096, 720, 500)
    assert len(pair) == 2 and {KERNELS[p[1]] for p in pair} == {"pair_dma"} and pair[0][16] == 0
    assert plan(OP_BWD, 4096, 720, 500, F_RIDER)[0][16] == 1
    assert plan(OP_BWD, 4096, 720, 500, F_RIDER | (255 << 8))[0][16] == 0      # a field beyond the ring's LDS does not ride
    assert [KERNELS[p[1]] for p in plan(OP_TRAIN, 4096, 500, 10)] == ["sk_train"] and plan(OP_TRAIN, 4096, 500, 10)[0][14:16] == (10, 16)
    assert plan(OP_TRAIN, 2047, 500, 10)[0][15] == 4
    # a wide head: forward, weight gradient, input gradient (both operands k-contiguous, n_out % 4 == 0: the fast kernel)
    assert [KERNELS[p[1]] for p in plan(OP_TRAIN, 21, 30, 40)] == ["generic", "generic", "fast"]
    assert [KERNELS[p[1]] for p in plan(OP_NLL, 19, 7, 5)] == ["sc_fwd"]
    assert plan(OP_DROP, 4096, 720, 500)[0][13] == 1 and plan(OP_DROP, 4096, 720, 500, F_ELEM)[0][13] == 0
    assert plan(OP_FWD, 0, 720, 500) is None and plan(7, 4, 4, 4) is None


def test_rider_changes_nothing_but_its_own_field():
    """A pending rider adds blocks to a pair launch; it never changes which kernels run the products."""
    plan = _query()
    for B in (64, 1024, 4096):
        for n_in in (100, 720, 2048):
            for n_out in (10, 96, 500):
                a, b = plan(OP_BWD, B, n_in, n_out), plan(OP_BWD, B, n_in, n_out, F_RIDER)
                assert [p[:16] for p in a] == [p[:16] for p in b]


def test_cpu_backend_has_no_plan():
    from theanet_amd import _lib
    import os
    if not os.path.isfile(_lib.CPU_LIB_PATH):
        pytest.skip("libtheanet_cpu.so not built")
    lib = _lib.bind(_lib.CPU_LIB_PATH, ctypes.RTLD_LOCAL)
    out = (ctypes.c_int * NINTS)()
    assert lib.tn_fc_plan(0, 64, 720, 500, 256, 0, out, NINTS) < 0


def test_gpu_cases_reach_every_instantiation():
    """The launches of tests/test_gpu_kernels.py reach exactly the instantiations the sweep reaches."""
    insts, _ = sweep()
    got, _ = gpu_reach()
    assert not got - insts, "GPU cases launch instantiations the sweep does not reach:\n  " + _fmt(got - insts)
    assert not insts - got, "instantiations no GPU case of tests/test_gpu_kernels.py launches:\n  " + _fmt(insts - got)


def test_gpu_cases_reach_every_edge_of_every_instantiation():
    _, pairs = sweep()
    _, got = gpu_reach()
    assert not got - pairs, "GPU cases reach pairs the sweep does not:\n  " + _fmt(got - pairs)
    missing = pairs - got
    assert not missing, "(instantiation, edge) pairs no GPU case of tests/test_gpu_kernels.py reaches:\n  " + _fmt(missing)


def test_unreachable_edges_are_the_documented_ones():
    insts, pairs = sweep()
    absent = {(i, e) for i in insts for e in _inst_edges(i) if (i, e) not in pairs}
    documented = {(i, e) for i in insts for e in _inst_edges(i) if _why_unreachable(i, e)}
    assert absent == documented, ("undocumented:\n  " + _fmt(absent - documented) +
                                  "\ndocumented but reachable:\n  " + _fmt(documented - absent))
