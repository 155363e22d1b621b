"""Reference of the multi-tensor momentum-SGD update (include/theanet_hip.h, the comment above tn_sgd_update_net), in
plain numpy, and the bound a correctly rounded implementation meets.

The library spells its roundings out (theanet_amd/csrc/common.h): with fl() = round to nearest float32,

    om   = fl(1 - m)
    gg   = fl(g * gscale)                               (PLAIN, LAZY, DELAYED; the pipelined forms take g as it is)
    g'   = fl(fl(gg + L1 * sign(p)) + 2 * L2 * p)       (L1 * sign(p) is exact: sign is -1, 0 or 1)
    v'   = fma(m, v, fl(om * g'))                       tn_vel
    step = fl(rate * lr)
    p'   = fma(-step, v_used, p_src)                    tn_stepped

Every rounding but the two fused multiply-adds (and the L2 term, below) is reproduced here bit for bit with float32
arithmetic.  A fused multiply-add is evaluated in float64: the product of two float32 values has 48 significant bits
and is exact there, so the float64 sum is within 2^-53 (relative) of the true value x, and a correctly rounded float32
result r = fl(x) has |r - x| <= ulp32(r) / 2.  The test is therefore

    |got - want64| <= 0.5 * ulp32(got) * (1 + 2^-20)                                        (check_rounded)

where the factor 1 + 2^-20 covers the float64 evaluation error (2^-53 |x| is below 2^-29 ulp32).  ulp32(r) is the
distance from |r| to the next float32 of larger magnitude, so the bound also holds where x rounds onto a power of two.

A segment with L2 != 0 is the one place where a compiler may or may not contract  g1 + (2*L2)*p  (g1 = fl(gg + L1*s),
t = 2*L2*p exact) into a fused multiply-add -- and, with L1 == 0, fold the product g * gscale into the sum instead.
Whichever it does, its g* satisfies, with M = max(|g1|, |t|) and the reference value g64 = g1 + t:

    not contracted:  g* = fl(g1 + fl(t)):            |g* - g64| <= ulp32(t)/2 + ulp32(g1 + fl(t))/2
    contracted:      g* = fl(g1 + t):                |g* - g64| <= ulp32(g1 + t)/2
    g * gscale fused g* = fl(g*gscale + fl(t)):      |g* - g64| <= ulp32(g1)/2 + ulp32(t)/2 + ulp32(.)/2

and a sum of two numbers of magnitude <= M has an ulp of at most 2 ulp32(M), so in every case
|g* - g64| <= sg := 2 * ulp32(M).  That slack is carried through the velocity: q* = fl(om * g*) has
|q* - om*g64| <= om*sg + ulp32(om*(|g64| + sg))/2, and v' = fl(m*v + q*) adds the final rounding ulp32(v')/2, so

    |got_v - (m*v + om*g64)| <= 0.5 * ulp32(got_v) * (1 + 2^-20) + om*sg + 0.5 * ulp32(om * (|g64| + sg)).

No bound here is taken from what a kernel computes.
"""
import numpy as np

PLAIN, LAZY, DELAYED, PIPE, PIPE_REG = range(5)         # the TN_UPD_* modes
F32 = np.float32


def ulp32(x):
    """Distance from |x| (rounded to float32) to the next float32 of larger magnitude, as float64."""
    return np.spacing(np.abs(np.asarray(x)).astype(F32)).astype(np.float64)


def sign(p):
    """-1, 0 or 1 as float32; both zeros have sign 0."""
    p = np.asarray(p, F32)
    return (p > 0).astype(F32) - (p < 0).astype(F32)


def reg_grad(gg, p, L1, L2):
    """g' = gg + L1*sign(p) + 2*L2*p for a float32 gradient ``gg`` already scaled: (value as float64, slack).  With
    L2 == 0 the value is an exact float32 and the slack is None."""
    gg = np.asarray(gg, F32)
    L1, L2 = F32(L1), F32(L2)
    if L1 != 0:
        gg = gg + L1 * sign(p)                          # float32 + float32 (an exact product): one rounding
    g64 = gg.astype(np.float64)
    if L2 == 0:
        return g64, None
    t = np.float64(F32(2) * L2) * np.asarray(p, F32).astype(np.float64)     # 2 * L2 is exact; the product is exact in float64
    return g64 + t, 2 * ulp32(np.maximum(np.abs(g64), np.abs(t)))


def velocity(v, g, m, gscale=None, p_terms=None, L1=0.0, L2=0.0):
    """v' = m*v + (1-m)*g': (want as float64, slack beyond half an ulp of the result).  gscale None: g is taken as it
    is (the pipelined forms); p_terms None: no L1 / L2 terms, else the weights they are taken at."""
    v, g, m = np.asarray(v, F32), np.asarray(g, F32), F32(m)
    om = F32(1) - m
    gg = g if gscale is None else g * F32(gscale)
    if p_terms is None:
        g64, sg = gg.astype(np.float64), None
    else:
        g64, sg = reg_grad(gg, p_terms, L1, L2)
    mv = np.float64(m) * v.astype(np.float64)           # exact
    if sg is None:
        q = om * g64.astype(F32)                        # g64 is an exact float32 here: fl(om * g') in float32
        return mv + q.astype(np.float64), None
    om64 = np.float64(om)
    return mv + om64 * g64, om64 * sg + 0.5 * ulp32(om64 * (np.abs(g64) + sg))


def stepped(p_src, v_used, rate, lr):
    """p' = p_src - fl(rate*lr) * v_used as float64 (the product is exact there)."""
    step = F32(rate) * F32(lr)
    return np.asarray(p_src, F32).astype(np.float64) - np.float64(step) * np.asarray(v_used, F32).astype(np.float64)


def check_rounded(got, want64, slack=None, what=""):
    """|got - want64| <= 0.5 * ulp32(got) * (1 + 2^-20) + slack, element by element; a NaN in ``got`` never passes."""
    got = np.asarray(got, F32)
    want64 = np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    tol = 0.5 * ulp32(got) * (1 + 2.0 ** -20)
    if slack is not None:
        tol = tol + slack
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want64)
        bad = ~(err <= tol)
    if bad.any():
        over = np.where(bad, np.where(np.isnan(err), np.inf, err / np.where(tol > 0, tol, 1)), 0)
        i = int(np.argmax(over.reshape(-1)))
        raise AssertionError("%s: %d/%d elements beyond the rounding bound, worst at %d: got %r want %r (|err| %.3g, bound %.3g)"
                             % (what, int(bad.sum()), bad.size, i, got.reshape(-1)[i], want64.reshape(-1)[i],
                                err.reshape(-1)[i], tol.reshape(-1)[i]))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_update(mode, flags, seg, got_p, got_v, lr, gscale=1.0, what=""):
    """One segment of one tn_sgd_update_net launch against the header's semantics.

    seg: dict with the segment's INPUTS p (for the pipelined forms: the stepping stream's own, old copy), psrc (pipelined
    forms only), v, g (float32 arrays) and momentum, rate, L1, L2.  got_p / got_v: what the launch left in p / v.
    A tensor the mode leaves alone must come back bit for bit; where p moves with the NEW velocity the stored (checked)
    velocity is what it is computed from."""
    p, v, g = (np.asarray(seg[k], F32) for k in ("p", "v", "g"))
    m, rate, L1, L2 = seg["momentum"], seg["rate"], seg.get("L1", 0.0), seg.get("L2", 0.0)
    got_p, got_v = np.asarray(got_p, F32), np.asarray(got_v, F32)
    if mode in (PLAIN, LAZY):
        want_v, slack = velocity(v, g, m, gscale, p, L1, L2)
        check_rounded(got_v, want_v, slack, what + " v")
        check_rounded(got_p, stepped(p, v, rate, lr), None, what + " p (moved by the OLD velocity)")
    elif mode == DELAYED:
        kind, terms = flags & 3, bool(flags & 4)
        assert kind in (1, 2, 3)
        if kind == 2:
            assert np.array_equal(bits(got_v), bits(v)), what + " v must stay"
        else:
            want_v, slack = velocity(v, g, m, gscale, p if terms else None, L1, L2)
            check_rounded(got_v, want_v, slack, what + " v")
        if kind == 3:
            assert np.array_equal(bits(got_p), bits(p)), what + " p must stay"
        else:
            check_rounded(got_p, stepped(p, got_v, rate, lr), None, what + " p (moved by the stored velocity)")
    elif mode in (PIPE, PIPE_REG):
        if flags & 1:
            terms = mode == PIPE_REG and (F32(L1) != 0 or F32(L2) != 0)
            want_v, slack = velocity(v, g, m, None, p if terms else None, L1, L2)
            check_rounded(got_v, want_v, slack, what + " v")
        else:
            assert np.array_equal(bits(got_v), bits(v)), what + " v must stay"
        check_rounded(got_p, stepped(seg["psrc"], got_v, rate, lr), None, what + " p_own (psrc moved by the stored velocity)")
    else:
        raise ValueError(mode)
    assert not np.isnan(got_p).any() and not np.isnan(got_v).any(), what + ": NaN"


def cost(rowloss, cost_scale):
    """cost_scale * sum(rowloss) in float64."""
    return np.float64(F32(cost_scale)) * np.asarray(rowloss, F32).astype(np.float64).sum()


def check_cost(got, rowloss, cost_scale, what=""):
    """rtol = nrow * 2^-24: nrow - 1 float32 additions of non-negative terms (in any fixed order every partial sum is at
    most the total, so each rounding is at most 2^-24 of it) and one multiplication."""
    rowloss = np.asarray(rowloss, F32)
    assert (rowloss >= 0).all()
    want = cost(rowloss, cost_scale)
    got = np.float64(np.asarray(got, F32).reshape(-1)[0])
    assert abs(got - want) <= rowloss.size * 2.0 ** -24 * abs(want), (what, got, want, rowloss.size)
