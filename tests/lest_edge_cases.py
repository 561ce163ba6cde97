"""Adversarial cases for the rank-weighted round: weights that are not robust, and the rank rule at its edges
(CPU only; the model is lest_cases.ref64_lest).

lest_cases runs beta_oracles data, on which every weight family keeps the pass-1 centre c1 inside the honest rows.
The rank-weighted estimator is as robust as its weights: under mean weights, a wide bell or a trimmed mean that
trims fewer ranks than there are outliers, the failing rows drag c1 away from the reliable ones.  Four families,
at one shape per lane-group width (SHAPES):

  A  displaced centre, moderate.  f rows at 0.5 +- M (M = 16, 1024 data units; 0.5 is the honest rows' centre).
     Pass 2 takes its power sums about c1, |c1 - reliable mean| / sd ~ 20 .. 10^4: the cancellation guard of
     consensus_fast_lest.hip (mean offset^2 > 16 variance -> the column is read again about the reliable mean) is
     all that keeps the skewness and the kurtosis.  displaced_case() proves on the CPU that a case bites:
     unguarded_fp32() -- the kernel's first-read arithmetic in numpy -- misses fast_cases.TOL["fp32"] on every
     displaced instance and meets it on the control, and the trigger holds (fails) with a factor 4 to spare.
  B  displaced centre, huge.  f rows (rows 0 .. f-1) at +-2^40 and +-2^80 under mean and wide-bell weights:
     c1 ~ (f / N) 2^e.  At 2^40 every honest y = x - c1 is -c1 and the first-read variance is exactly 0; at 2^80
     y^2 overflows fp32, so every qr is +inf and the first-read power sums are not finite.  (A re-read in fp32
     about c1 + dl fails both: dl carries the rounding of R terms ~ c1, more than the honest rows' spread unless
     every partial sum happens to be exact -- ZERO_VARIANCE at 2^40 -- and at 2^80 a guard that compares
     dl^2 with 16 mu2 = +inf never fires -- NaN moments committed with OK.  The CPU twin commits finite values.)
  C  extremes behind zero weights: fast_extreme_cases' tiers T0 .. T3, outlier counts, signs and row placement
     under trimmed_mean_weights(N, f) and median weights -- every outlier rank carries a zero weight.
  D  rank-cut ties: fast_cases.tie_case under bell and mean weights.

Bounds.  Nothing new: c1 and the constrained consensus -- lest_cases' (n + 2) 2^-24 max|x| over the n values
summed (family C: the n ranks with a non-zero weight; a zero weight contributes an exact zero and its value is not
read); qr, rel, skew, kurt -- fast_cases.TOL["fp32"]; the unconstrained consensus -- lest_cases.check_round's
N 2^-24 mean|x - c1| + 1 ulp, and in family C fast_extreme_cases' restatement of it over the R reliable rows (the
all-row mean of |x - c1| is ~ M there and would bound nothing).  The kernel's re-read takes the reliable rows' mean
and moments in fp64, as the CPU twin does: its error is far inside the bounds of the fp32 sum about c1, which stay.

qr = +inf is a legitimate output of families B and C (the fp64 value exceeds FLT_MAX).  split_overflow() asserts
+inf exactly there and finite elsewhere, then zeroes those entries on both sides so that lest_cases.check_round --
its isfinite assertion on every other output included -- runs unchanged.
"""
import functools
import math

import numpy as np
import torch

import fast_cases as fc
import fast_extreme_cases as fx
import lest_cases as lc
from helpers import beta_oracles
from svoc import estimators as est

# (N, D, f): one shape per lane-group width (1, 1, 2, 4 lanes per column), a partial slab and more than one slab
SHAPES = [(7, 6, 2), (64, 33, 8), (128, 64, 16), (256, 72, 32)]
LANES = {7: 1, 64: 1, 128: 2, 256: 4}
TOL = fc.TOL["fp32"]
MARGIN = 4.0            # to spare on either side of the guard's trigger dl^2 > 16 mu2


def weights_of(family, N, f):
    """w1 of a family over N ranks: lest_cases' families, ("trim", t): trimmed_mean_weights(N, t)."""
    if family[0] == "trim":
        return est.trimmed_mean_weights(N, family[1])
    return lc.weights_of(family, N, N - f)[0]


def _case(x, w1, w2, ref, constrained, ms, scale, shape, tag, active=None, **extra):
    """The dict lest_cases.check_round / run_lest take, plus the family's own fields."""
    N, D, f = shape
    active = torch.ones(x.shape[0], dtype=torch.uint8) if active is None else active
    return dict(x=x, w1=w1, w2=w2, weights=est.pack(w1, w2), ref=ref, constrained=constrained, max_spread=ms,
                scale=scale, N=N, D=D, f=f, tag=tag, active=active, **extra)


def run_case(ops, c, device, work=None):
    act = None if bool(c["active"].all()) else c["active"]
    return lc.run_lest(ops, c["x"].to(device), act, c["D"], c["f"], c["constrained"], c["max_spread"], c["weights"],
                       work)


def sub_batch(o, c, rows):
    """The instances `rows` of a case and of its outputs, for lest_cases.check_round over a part of the batch."""
    cut = lambda d: {k: v[rows] for k, v in d.items()}
    return cut(o), dict(c, x=c["x"][rows], ref=cut(c["ref"]), active=c["active"][rows])


# ------------------------------------------------------------------------------------- A: displaced, moderate
A_M = (16.0, 1024.0)
A_KINDS = ("all", "odd", "const", "neg", "inactive", "alt")     # instance b; const / inactive: lest_cases' indices
assert A_KINDS.index("const") == lc.CONSTANT and A_KINDS.index("inactive") == lc.INACTIVE and len(A_KINDS) == lc.B


def a_families(f):
    return [("mean",), ("bell", 1.0), ("trim", max(1, f // 4))]


def a_matrix():
    return [(s, M, fam, cons) for s in SHAPES for M in A_M for fam in a_families(s[2]) for cons in (True, False)]


def a_id(k):
    s, M, fam, cons = k
    return "%s-M%g-%s-%s" % (lc.shape_id(s), M, lc.family_id(fam), "cons" if cons else "unc")


def displaced_data(N, D, f, M):
    """Unit-scale fp64 data [B, N, D]: Beta(20, 20) rows; f rows (fast_extreme_cases.outlier_rows) at 0.5 + M in
    every column (all, const, inactive), in the odd columns only (odd), at 0.5 - M (neg), at 0.5 +- M alternating by
    row (alt: the control, c1 stays central).  Returns the data, the outlier rows and the displaced columns."""
    base, _ = beta_oracles(lc.B, N, D, 0, seed=N + D, dtype=torch.float64)
    x = base[:, :, :D].clone()
    g = torch.Generator().manual_seed(N + D + 1)
    outlier = torch.zeros(lc.B, N, dtype=torch.bool)
    displaced = torch.zeros(lc.B, D, dtype=torch.bool)
    odd = torch.arange(D) % 2 == 1
    for b, kind in enumerate(A_KINDS):
        cols = odd if kind == "odd" else torch.ones(D, dtype=torch.bool)
        for j, r in enumerate(fx.outlier_rows(N, f, "+", g)):
            neg = kind == "neg" or (kind == "alt" and j % 2 == 1)
            x[b, r, cols] = 0.5 - M if neg else 0.5 + M
            outlier[b, r] = True
        if kind != "alt":
            displaced[b] = cols
    x[lc.CONSTANT, :, 0] = 0.5
    return x, outlier, displaced


def _fma32(a, b, c):
    # the product of two fp32 values is exact in fp64; the sum is rounded to fp64, then to fp32
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def unguarded_fp32(x, mask, c1):
    """The kernel's pass 2 without its guard: x [N, D] fp32, mask [N] bool, c1 [D] fp32.  Per 64-row lane the fp32
    y = x - c1 and the sequential fp32 power sums (s3, s4 by fma), the lanes added in fp64, then the fp64 central
    moments about c1 and the sample-adjusted skewness / kurtosis (consensus_fast_lest.hip, the lines under
    "central moments from the shifted sums").  Returns fp64 (skew, kurt); NaN where the variance comes out <= 0."""
    xn, c1 = x.numpy().astype(np.float32), c1.numpy().astype(np.float32)
    N, D = xn.shape
    S = np.zeros((4, D), dtype=np.float64)
    for seg in range(0, N, 64):
        s1, s2, s3, s4 = (np.zeros(D, dtype=np.float32) for _ in range(4))
        for i in range(seg, min(seg + 64, N)):
            if not bool(mask[i]):
                continue                    # a masked row adds an exact zero
            y = xn[i] - c1
            y2 = y * y
            s1, s2 = s1 + y, s2 + y2
            s3, s4 = _fma32(y2, y, s3), _fma32(y2, y2, s4)
        assert s1.dtype == np.float32 and s2.dtype == np.float32
        S += np.stack([s1, s2, s3, s4]).astype(np.float64)
    n = float(int(mask.sum()))
    dl, e2, e3, e4 = S[0] / n, S[1] / n, S[2] / n, S[3] / n
    mu2 = e2 - dl * dl
    mu3 = e3 - 3.0 * dl * e2 + 2.0 * dl * dl * dl
    mu4 = e4 - 4.0 * dl * e3 + 6.0 * dl * dl * e2 - 3.0 * dl * dl * dl * dl
    with np.errstate(all="ignore"):
        m2 = np.where(mu2 > 0, mu2, np.nan)
        sk = (n * mu3 / (m2 * np.sqrt(m2))) * n / ((n - 1.0) * (n - 2.0))
        ku = ((n * mu4 / (m2 * m2)) * n * (n + 1.0) / (n - 1.0) - 3.0 * (n - 1.0) ** 2) / ((n - 2.0) * (n - 3.0))
    return torch.from_numpy(sk), torch.from_numpy(ku)


def misses_tol(got, want, key):
    """Per column: got is outside fast_cases' fp32 tolerance of want (NaN misses)."""
    rtol, atol = TOL[key]
    return ~((got - want).abs() <= atol + rtol * want.abs())


def trigger_ratio(x, mask, c1):
    """dl^2 / (16 mu2) per column in fp64: the guard fires where this exceeds 1.  x [N, D], c1 [D] fp64."""
    xr = x[mask]
    dl = xr.mean(0) - c1
    return dl * dl / (16.0 * xr.var(0, unbiased=False))


@functools.lru_cache(maxsize=None)
def displaced_case(key):
    shape, M, family, constrained = key
    N, D, f = shape
    R = N - f
    tag = "A-" + a_id(key)
    x1, outlier, displaced = displaced_data(N, D, f, M)
    w1, w2 = weights_of(family, N, f), est.rank_weights(R, 0.125)
    if constrained:
        # the scale from the model: the first reliability 1 - 2 sqrt(mean qr / D) is at least 1/2 in every instance
        q = lc.ref64_lest(fc._pad(x1, torch.float32)[:, :, :D], f, True, 1.0, w1, w2)["qr"]
        worst = math.sqrt(float(q.mean(1).max()) / D)
        scale = 2.0 ** math.floor(math.log2(0.25 / worst))
        ms = scale * math.sqrt(D)
    else:
        scale = 1.0
        ms = 2.0 * M * math.sqrt(D)          # above sqrt(mean qr) <= M sqrt(D): no reliability is clamped
    x = fc._pad(x1 * scale, torch.float32)
    ref = lc.ref64_lest(x[:, :, :D], f, constrained, ms, w1, w2)
    want = [lc.ST_ZERO_VARIANCE if k == "const" else lc.ST_OK for k in A_KINDS]
    assert ref["status"].tolist() == want, (tag, "ladder", ref["status"])
    assert bool(((ref["rel"] > 0) & (ref["rel"] < 1))[ref["status"] == 0].all()), (tag, "rel clamped", ref["rel"])
    lc.assert_cut_gap(ref, f, scale, tag)
    assert torch.equal(ref["reliable"], ~outlier), (tag, "the failing rows are the outliers")
    xd = x[:, :, :D].double()
    for b, kind in enumerate(A_KINDS):
        if kind in ("const", "inactive"):
            continue
        mask, dis = ref["reliable"][b], displaced[b]
        # the trigger, on the model's numbers, with MARGIN to spare on either side
        ratio = trigger_ratio(xd[b], mask, ref["c1"][b])
        assert bool((ratio[dis] > MARGIN).all()), (tag, kind, "guard must fire", float(ratio[dis].min()))
        assert bool((ratio[~dis] < 1.0 / MARGIN).all()), (tag, kind, "guard must not fire", float(ratio[~dis].max()))
        # the bite: without the guard the first-read arithmetic misses the tolerance (control: meets it)
        sk, ku = unguarded_fp32(x[b, :, :D], mask, ref["c1"][b].float())
        miss = misses_tol(sk, ref["skew"][b], "skew") | misses_tol(ku, ref["kurt"][b], "kurt")
        assert not bool(miss[~dis].any()), (tag, kind, "first read misses where c1 is central")
        assert kind == "alt" or bool(miss[dis].any()), (tag, kind, "the case does not bite")
    assert displaced[A_KINDS.index("odd")].any() and not displaced[A_KINDS.index("odd")].all()
    return _case(x, w1, w2, ref, constrained, ms, scale, shape, tag, active=lc.active_mask(), outlier=outlier,
                 displaced=displaced)


A_CONTROL = [A_KINDS.index("alt")]
A_MAIN = [b for b in range(lc.B) if b not in A_CONTROL]


def check_displaced(o, c):
    """lest_cases.check_round over the displaced, constant and inactive instances of a family-A batch."""
    return lc.check_round(*sub_batch(o, c, A_MAIN))


def check_control(o, c):
    """lest_cases.check_round over the control instance of the same launch (see test_displaced_control)."""
    o2, c2 = sub_batch(o, c, A_CONTROL)
    return lc.check_round(o2, dict(c2, tag=c["tag"] + "-control"))


# ------------------------------------------------------------------------------------------ B: displaced, huge
B_TIERS = (40, 80)
B_FAMILIES = [("mean",), ("bell", 1.0)]
B_SIGNS = ("+", "-")


def b_matrix():
    return [(s, e, fam) for s in SHAPES for e in B_TIERS for fam in B_FAMILIES]


def b_id(k):
    return "%s-2^%d-%s" % (lc.shape_id(k[0]), k[1], lc.family_id(k[2]))


def rank_rule(q, R):
    """The reliable mask of qr values q (a list): qr ascending, index descending, the first R."""
    order = sorted(range(len(q)), key=lambda i: (q[i], -i))
    m = torch.zeros(len(q), dtype=torch.bool)
    m[order[:R]] = True
    return m


@functools.lru_cache(maxsize=None)
def huge_case(key):
    """Rows 0 .. f-1 at +2^e (instance 0) and -2^e (instance 1); honest rows as fast_extreme_cases' (x 8 - 4);
    unconstrained with max_spread = 8 sqrt(D).  At 2^80 every fp32 qr is +inf and the rank rule drops the f lowest
    indices -- the outliers: the fp32 mask equals the model's."""
    shape, e, family = key
    N, D, f = shape
    R = N - f
    tag = "B-" + b_id(key)
    base, _ = beta_oracles(len(B_SIGNS), N, D, 0, seed=2000 + N + D + e, dtype=torch.float64)
    x = base[:, :, :D] * fx.SCALE - fx.SCALE / 2
    outlier = torch.zeros(len(B_SIGNS), N, dtype=torch.bool)
    for b, s in enumerate(B_SIGNS):
        x[b, :f] = 2.0 ** e if s == "+" else -(2.0 ** e)
        outlier[b, :f] = True
    x = fc._pad(x, torch.float32)
    w1, w2 = weights_of(family, N, f), est.mean_weights(R)
    ms = fx.SCALE * math.sqrt(D)
    ref = lc.ref64_lest(x[:, :, :D], f, False, ms, w1, w2)
    q = ref["qr"]
    assert (ref["status"] == 0).all() and (ref["rel"] == 0).all(), (tag, ref["status"], ref["rel"])
    assert torch.equal(ref["reliable"], ~outlier), (tag, "model mask")
    assert not ((q > fx.FLT_MAX / 4) & (q < fx.FLT_MAX * 4)).any(), (tag, "qr near FLT_MAX")
    assert bool((q > fx.FLT_MAX).all()) == (e == 80) and bool((q < fx.FLT_MAX).all()) == (e == 40), tag
    for b in range(len(B_SIGNS)):           # the rank rule over the fp32 view of the qr (+inf where it overflows)
        assert torch.equal(rank_rule(q[b].float().tolist(), R), ref["reliable"][b]), (tag, b, "fp32 mask")
        # the centre has left the honest rows by far more than their range
        assert bool((ref["c1"][b].abs() > 2.0 ** (e - 8)).all()), (tag, b, "c1")
    return _case(x, w1, w2, ref, False, ms, fx.SCALE, shape, tag, outlier=outlier)


def split_overflow(o, c):
    """qr must be +inf exactly where the model's fp64 value exceeds FLT_MAX and finite elsewhere.  Returns (o, c)
    with those entries zeroed on both sides, for lest_cases.check_round."""
    ref = c["ref"]
    over = ref["qr"] > fx.FLT_MAX
    ok = (ref["status"] == 0) & (c["active"] != 0)
    got = o["qr"]
    assert bool((got[over & ok[:, None]] == math.inf).all()), (c["tag"], "qr finite where the fp64 value overflows")
    assert bool(torch.isfinite(got[~over & ok[:, None]]).all()), (c["tag"], "qr not finite where the fp64 value fits")
    o2, ref2 = dict(o), dict(ref)
    o2["qr"] = torch.where(over & ok[:, None], torch.zeros_like(got), got)
    ref2["qr"] = torch.where(over, torch.zeros_like(ref["qr"]), ref["qr"])
    return o2, dict(c, ref=ref2)


def check_huge(o, c):
    """Status OK, rel == (0, 0) exactly (the clamp), qr = +inf where it overflows, then lest_cases.check_round."""
    assert (o["status"] == 0).all(), (c["tag"], "status", o["status"])
    assert bool((o["rel"] == 0).all()), (c["tag"], "rel", o["rel"])
    return lc.check_round(*split_overflow(o, c))


# --------------------------------------------------------------------------------- C: extremes, zero weights
C_TIERS = tuple(t for t, _ in fx.TIERS)


def c_families(f):
    return [("trim", f), ("median",)]


def c_matrix():
    return [(s, t, fam) for s in SHAPES for t in C_TIERS for fam in c_families(s[2])]


def c_id(k):
    return "%s-%s-%s" % (lc.shape_id(k[0]), k[1], lc.family_id(k[2]))


# fast_extreme_cases' seed (1000 + N + D) unless the rank-cut gap among the honest rows asks for another: at (256, 72)
# one T1 instance misses lest_cases.assert_cut_gap about the median centre, the next seed in steps of 1000 meets it
# for every tier and family
C_SEED = {(256, 72): 2328}


@functools.lru_cache(maxsize=None)
def zero_weight_case(key):
    """One tier of fast_extreme_cases.extreme_case (5 instances: k = 1 under +, -; k = f under +, -, alt) under a
    w1 whose f lowest and f highest ranks weigh nothing.  Unconstrained, as there: the constrained ladder cannot be
    OK (1 - 2 sqrt(mean qr / D) < 0 for every tier)."""
    shape, tier, family = key
    N, D, f = shape
    R = N - f
    tag = "C-" + c_id(key)
    xa, oa, inst = fx.extreme_case(N, D, f, C_SEED.get((N, D), fx.seed_of(N, D, "fp32")), torch.float32)
    rows = [b for b, (t, _, _, _) in enumerate(inst) if t == tier]
    assert len(rows) == 5
    x, outlier = xa[rows].clone(), oa[rows].clone()
    w1, w2 = weights_of(family, N, f), est.mean_weights(R)
    assert float(w1[:f].abs().sum()) == 0.0 and float(w1[N - f:].abs().sum()) == 0.0
    ms = fx.SCALE * math.sqrt(D)
    ref = lc.ref64_lest(x[:, :, :D], f, False, ms, w1, w2)
    assert (ref["status"] == 0).all(), (tag, ref["status"])
    lc.assert_cut_gap(ref, f, fx.SCALE, tag)
    expect = fx.constructed_mask(ref["qr"], outlier, f)
    assert torch.equal(ref["reliable"], expect) and (~expect).sum(1).eq(f).all(), (tag, "constructed mask")
    q = ref["qr"]
    assert not ((q > fx.FLT_MAX / 4) & (q < fx.FLT_MAX * 4)).any(), (tag, "qr near FLT_MAX")
    assert (ref["rel"][:, 0] == 0).all() and ((ref["rel"][:, 1] > 0) & (ref["rel"][:, 1] < 1)).all(), (tag, ref["rel"])
    # the largest |x| over the ranks that carry a weight: honest values only
    xs = torch.sort(x[:, :, :D].double(), dim=1).values
    wmax = xs[:, w1 != 0].abs().amax(1)                         # [B, D]
    assert bool((wmax <= fx.SCALE / 2).all()), (tag, "an outlier at a weighted rank")
    return _case(x, w1, w2, ref, False, ms, fx.SCALE, shape, tag, outlier=outlier, expect=expect, wmax=wmax,
                 n_weighted=int((w1 != 0).sum()), inst=[inst[b] for b in rows])


def check_zero_weight(o, c):
    """fast_extreme_cases.check_extreme's assertions with the c1 bound of a weighted sum: mask == constructed ==
    model, qr = +inf where the model says so, every other committed output finite and within its bound."""
    ref, N, D, tag = c["ref"], c["N"], c["D"], c["tag"]
    R = N - c["f"]
    assert (o["status"] == 0).all(), (tag, o["status"])
    for k in ("c1", "consensus", "skew", "kurt", "rel"):
        assert bool(torch.isfinite(o[k]).all()), (tag, k, "not finite")
    assert (o["reliable"] <= 1).all()
    mask = o["reliable"].bool()
    assert torch.equal(mask, c["expect"]), (tag, "reliable vs constructed mask")
    assert torch.equal(mask, ref["reliable"]), (tag, "reliable vs the fp64 model")
    frac = {}
    fx._worst(frac, "c1", (o["c1"].double() - ref["c1"]).abs(), (c["n_weighted"] + 2) * lc.U * c["wmax"])
    x = c["x"][:, :, :D].double()
    dev = ((x - ref["c1"][:, None, :]).abs() * mask[:, :, None]).sum(1) / R
    fx._worst(frac, "consensus", (o["consensus"].double() - ref["consensus"]).abs(),
              R * lc.U * dev + fc._ulp32(ref["consensus"]))
    for key in ("skew", "kurt", "rel"):
        rtol, atol = TOL[key]
        fx._worst(frac, key, (o[key].double() - ref[key]).abs(), atol + rtol * ref[key].abs())
    assert bool((o["rel"][:, 0] >= 0).all()), (tag, "rel1 < 0", o["rel"])
    fx.check_qr(o["qr"], ref["qr"], c["outlier"], "fp32", c["scale"], frac)
    print("FRAC %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(frac.items()))))
    for key, v in frac.items():
        assert v <= 1.0, (tag, key, "error / bound = %.3g" % v)
    return frac


# ------------------------------------------------------------------------------------------- D: rank-cut ties
D_FAMILIES = [("bell", 0.125), ("mean",)]


def tie_shapes():
    """The shapes at which fast_cases.tie_params yields a tie group the cut can split."""
    out = []
    for N, D, f in SHAPES:
        t, k = fc.tie_params(N, f)
        if 1 <= k < t and f - k >= 0 and D > 1:
            out.append((N, D, f))
    return out


def d_matrix():
    return [(s, signed, fam) for s in tie_shapes() for signed in (False, True) for fam in D_FAMILIES]


def d_id(k):
    return "%s-%s-%s" % (lc.shape_id(k[0]), "signed" if k[1] else "unsigned", lc.family_id(k[2]))


@functools.lru_cache(maxsize=None)
def tie_case(key):
    """fast_cases.tie_case: unsigned in a constrained round, signed (x 8 - 4) in an unconstrained one; w2 of the
    same family as w1.  The cut splits a group of bit-identical rows: the k lowest indices go."""
    shape, signed, family = key
    N, D, f = shape
    tag = "D-" + d_id(key)
    t, k = fc.tie_params(N, f)
    x, expect = fc.tie_case(lc.B, N, D, f, t, k, N + D, torch.float32, signed)
    scale, constrained = (8.0, False) if signed else (1.0, True)
    ms = scale * math.sqrt(D)
    w1, w2 = lc.weights_of(family, N, N - f)
    ref = lc.ref64_lest(x[:, :, :D], f, constrained, ms, w1, w2)
    assert (ref["status"] == 0).all(), (tag, ref["status"])
    assert bool(((ref["rel"] > 0) & (ref["rel"] < 1)).all()), (tag, ref["rel"])
    tie, outside = fc.tie_group_gap(ref, f)      # in place of assert_cut_gap: the cut gap is zero by construction
    assert (tie == 0).all(), (tag, tie)
    assert (outside > 0.01).all(), (tag, outside)
    assert torch.equal(ref["reliable"], expect), (tag, "constructed mask")
    assert (~expect).sum(1).eq(f).all() and not expect[:, 0].any() and expect[:, N - 1].all(), tag
    return _case(x, w1, w2, ref, constrained, ms, scale, shape, tag, expect=expect)


def check_tie(o, c):
    assert (o["status"] == 0).all(), (c["tag"], o["status"])
    assert torch.equal(o["reliable"].bool(), c["expect"]), (c["tag"], "reliable vs constructed mask")
    return lc.check_round(o, c)
