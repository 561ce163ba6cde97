"""Cases and an fp64 model for the rank-weighted (L-estimator) round, ``torch.ops.svoc.lest_round`` (CPU only).

ref64_lest is written from the round's formulas: per column the estimator L_w(x) = sum_k w[k] x(k) over the sorted
values (w1 over all N rows in pass 1, w2 over the R = N - f reliable rows in a constrained pass 2; an unconstrained
pass 2 takes their mean), qr about c1, the rank rule (qr ascending, index descending), the status ladder, the
population variance and the sample-adjusted skewness / excess kurtosis.  It works in fp64 over x.double() with a
Python sort for the rank rule and takes the weights as w.double() of the fp32 weights, so weight rounding is not
part of any error.  case() builds the data; check_round holds the assertions that test_lest.py (CPU twin) and
test_lest_gpu.py (HIP kernel) share.  Nothing here imports GPU code.

The bound on c1 and on the constrained consensus, per column:  (n + 2) * 2^-24 * max|x|  over the n values summed.
Derivation: the computed value is an fp32 dot product of n terms, each product and each addition rounded once (an
fma rounds once for both), in some order.  Every term passes through at most n roundings (a chain of at most 64
fused steps per lane plus at most 2 additions across the lanes of a column; a zero weight adds its exact zero), so
|computed - exact| <= gamma_n * sum_k |w_k x_k| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: the bound holds for any order of summation).  The weights are
non-negative fp32 roundings of an fp64 row that sums to 1, so sum_k |w_k x_k| <= (1 + u) max|x|, and for n <= 256
gamma_n (1 + u) < (n + 2) u.  It is derived from the number format alone, not measured.
"""
import functools
import math

import torch

import fast_cases as fc
from helpers import beta_oracles
from svoc import estimators as est

# (N, D, f): the smallest shapes that reach every instantiation and edge of the kernel
SHAPES = [(7, 6, 2), (2, 3, 0),              # tiny, one lane
          (64, 33, 8),                       # a full lane and a partial slab
          (65, 70, 8), (128, 64, 16),        # 2 lanes per column
          (129, 33, 32), (256, 72, 32),      # 4 lanes per column
          (256, 24, 0)]                      # no failing oracle
B = 6
INACTIVE = 4      # this instance is not active: every output stays untouched
CONSTANT = 2      # this instance has a constant column: ZERO_VARIANCE, every output but the status untouched
SIGMAS = (0.125, 0.03, 1.0)
# data variants: (name, scale, shift, constrained).  rel is scale-free with the spread bound in the data's units.
VARIANTS = [("cons", 1.0, 0.0, True), ("unc", 1.0, 0.0, False), ("signed", 8.0, -4.0, False)]

ST_OK, ST_INDEX_OOB, ST_RELIABILITY_INTERVAL, ST_USIZE_UNDERFLOW = 0, 5, 6, 8
ST_ZERO_VARIANCE, ST_TOO_FEW_RELIABLE = 32, 33

# seeds: N + D by default; the rank-cut gap assertion of case() decides whether a seed serves, and every seed in
# use here was checked on the CPU to pass it for every weight family of its shape
SEED_OVERRIDE = {}

U = 2.0 ** -24


def shape_id(s):
    return "%dx%dx%d" % s


def data(N, D, f, scale, shift):
    """beta_oracles mapped to x * scale + shift, rounded to fp32 last; [B, N, ld] with instance CONSTANT's column 0
    constant.  The same builder idea as fast_cases.signed_case."""
    seed = SEED_OVERRIDE.get((N, D, f), N + D)
    base, _ = beta_oracles(B, N, D, f, seed=seed, dtype=torch.float64)
    x = base[:, :, :D] * scale + shift
    x[CONSTANT, :, 0] = 0.5 * scale + shift
    return fc._pad(x, torch.float32)


def active_mask():
    a = torch.ones(B, dtype=torch.uint8)
    a[INACTIVE] = 0
    return a


def l_est(col_sorted, w):
    """sum_k w[k] x(k), fp64; col_sorted [n, D], w [n] (the fp32 weights, widened)."""
    return (w.double()[:, None] * col_sorted).sum(0)


def ref64_lest(x, f, constrained, max_spread, w1, w2):
    """One rank-weighted round per instance in fp64.  x [B, N, D] (any float dtype); w1 [N], w2 [N - f] fp32.
    Returns fp64 tensors, reliable as bool and status int [B]; the outputs of an instance whose status is not OK
    are meaningless (a reverted round writes nothing)."""
    x = x.double()
    Bn, N, D = x.shape
    R = N - f
    out = dict(c1=torch.zeros(Bn, D, dtype=torch.float64), qr=torch.zeros(Bn, N, dtype=torch.float64),
               reliable=torch.zeros(Bn, N, dtype=torch.bool), consensus=torch.zeros(Bn, D, dtype=torch.float64),
               rel=torch.zeros(Bn, 2, dtype=torch.float64), skew=torch.zeros(Bn, D, dtype=torch.float64),
               kurt=torch.zeros(Bn, D, dtype=torch.float64), status=torch.zeros(Bn, dtype=torch.int32))

    def rel_of(mean_qr):
        if constrained:
            return 1.0 - 2.0 * math.sqrt(mean_qr / D)
        return 1.0 - min(math.sqrt(mean_qr), max_spread) / max_spread

    for b in range(Bn):
        if f > N:
            out["status"][b] = ST_USIZE_UNDERFLOW
            continue
        if N < 2:
            out["status"][b] = ST_INDEX_OOB
            continue
        c1 = l_est(torch.sort(x[b], dim=0).values, w1)
        out["c1"][b] = c1
        qr = ((x[b] - c1) ** 2).sum(-1)
        out["qr"][b] = qr
        q = qr.tolist()
        order = sorted(range(N), key=lambda i: (q[i], -i))     # qr ascending, index descending
        keep = sorted(order[:R])
        out["reliable"][b, keep] = True
        rel1 = rel_of(sum(q) / N)
        out["rel"][b, 0] = rel1
        if not (0.0 <= rel1 <= 1.0):
            out["status"][b] = ST_RELIABILITY_INTERVAL
            continue
        if R < 2:
            out["status"][b] = ST_USIZE_UNDERFLOW if R <= 0 else ST_INDEX_OOB
            continue
        rel2 = rel_of(sum(q[i] for i in keep) / R)
        out["rel"][b, 1] = rel2
        if not (0.0 <= rel2 <= 1.0):
            out["status"][b] = ST_RELIABILITY_INTERVAL
            continue
        if R < 4:
            out["status"][b] = ST_TOO_FEW_RELIABLE
            continue
        xr = x[b, keep]
        if bool((xr.min(0).values == xr.max(0).values).any()):   # a constant reliable column, decided exactly
            out["status"][b] = ST_ZERO_VARIANCE
            continue
        mean = xr.sum(0) / R
        out["consensus"][b] = l_est(torch.sort(xr, dim=0).values, w2) if constrained else mean
        y = xr - mean
        m2, m3, m4 = (y ** 2).sum(0) / R, (y ** 3).sum(0) / R, (y ** 4).sum(0) / R
        n = float(R)
        out["skew"][b] = (n * m3 / m2 ** 1.5) * n / ((n - 1) * (n - 2))
        out["kurt"][b] = ((n * m4 / m2 ** 2) * n * (n + 1) / (n - 1) - 3 * (n - 1) ** 2) / ((n - 2) * (n - 3))
    return out


def qr_bound(q, scale):
    """fp32 error bound of a qr value: the tolerance fast_cases.check_round holds fp32 storage to."""
    rtol, atol = fc.TOL["fp32"]["qr"]
    return atol * scale ** 2 + rtol * abs(q)


def assert_cut_gap(ref, f, scale, tag):
    """fp32 cannot flip the rank cut: in every instance the gap between the R-th and (R+1)-th smallest qr exceeds
    the fp32 error bound of those two qr.  (f = 0: there is no cut.)  Fails the build of the case; never skips."""
    if f == 0:
        return
    s = torch.sort(ref["qr"], dim=1).values
    R = s.shape[1] - f
    for b in range(s.shape[0]):
        lo, hi = float(s[b, R - 1]), float(s[b, R])
        assert hi - lo > qr_bound(lo, scale) + qr_bound(hi, scale), (tag, b, "rank-cut gap", lo, hi)


def weights_of(family, N, R):
    """(w1, w2) of a weight family: ("bell", sigma), ("median",), ("mean",)."""
    if family[0] == "bell":
        return est.rank_weights(N, family[1]), est.rank_weights(R, family[1])
    if family[0] == "median":
        return est.median_weights(N), est.median_weights(R)
    if family[0] == "mean":
        return est.mean_weights(N), est.mean_weights(R)
    raise ValueError(family)


MODEL_FAMILIES = [("bell", s) for s in SIGMAS] + [("median",), ("mean",)]


def family_id(fam):
    return "-".join(str(v) for v in fam)


@functools.lru_cache(maxsize=None)
def case(shape, variant, family):
    """Data, weights, fp64 model and round arguments of one case (built once, shared, never modified)."""
    N, D, f = shape
    name, scale, shift, constrained = next(v for v in VARIANTS if v[0] == variant)
    x = data(N, D, f, scale, shift)
    w1, w2 = weights_of(family, N, N - f)
    ms = abs(scale) * math.sqrt(D)
    ref = ref64_lest(x[:, :, :D], f, constrained, ms, w1, w2)
    tag = "%s-%s-%s" % (shape_id(shape), variant, family_id(family))
    assert_cut_gap(ref, f, scale, tag)
    return dict(x=x, w1=w1, w2=w2, weights=est.pack(w1, w2), ref=ref, constrained=constrained, max_spread=ms,
                scale=scale, N=N, D=D, f=f, tag=tag, active=active_mask())


POISON = dict(c1=-7.25, consensus=-3.5, skew=11.0, kurt=-13.0, rel=-2.0, qr=-5.0, reliable=0xAB, status=-1)


def poisoned(Bn, N, D, device):
    """Outputs pre-filled with a value no round writes."""
    f32 = dict(dtype=torch.float32, device=device)
    return dict(c1=torch.full((Bn, D), POISON["c1"], **f32), consensus=torch.full((Bn, D), POISON["consensus"], **f32),
                skew=torch.full((Bn, D), POISON["skew"], **f32), kurt=torch.full((Bn, D), POISON["kurt"], **f32),
                rel=torch.full((Bn, 2), POISON["rel"], **f32), qr=torch.full((Bn, N), POISON["qr"], **f32),
                reliable=torch.full((Bn, N), POISON["reliable"], dtype=torch.uint8, device=device),
                status=torch.full((Bn,), POISON["status"], dtype=torch.int32, device=device))


def run_lest(ops, x, active, D, f, constrained, max_spread, weights, work=None):
    """lest_round over x on x's device into poisoned outputs; returns them as CPU tensors."""
    dev = x.device
    o = poisoned(x.shape[0], x.shape[1], D, dev)
    ops.lest_round(x, None if active is None else active.to(dev), D, f, constrained, max_spread, weights.to(dev),
                   o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"], work)
    return {k: v.cpu() for k, v in o.items()}


def run_case(ops, c, device):
    return run_lest(ops, c["x"].to(device), c["active"], c["D"], c["f"], c["constrained"], c["max_spread"],
                    c["weights"])


def untouched(o, b):
    """Every output of instance b but its status still holds the poison, bit for bit."""
    return all(bool((o[k][b] == POISON[k]).all()) for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable"))


def expected_status(c):
    st = c["ref"]["status"].clone()
    st[c["active"] == 0] = POISON["status"]
    return st


def check_round(o, c):
    """o: outputs of one round over case c (CPU tensors, from run_case).  Status against the model; reverted and
    inactive instances untouched; the committed ones against the model, each output within its bound.  Prints and
    returns the largest error of each toleranced output as a fraction of its bound."""
    ref, N, D, f, tag = c["ref"], c["N"], c["D"], c["f"], c["tag"]
    R = N - f
    x = c["x"][:, :, :D].double()
    want_st = expected_status(c)
    assert torch.equal(o["status"], want_st), (tag, "status", o["status"], want_st)
    frac = {}

    def worst(key, err, bound):
        # NaN must fail: `err <= bound` is False for a NaN error, and the folded fraction keeps a NaN (Python's
        # max() would drop it)
        assert bool((err <= bound).all()), (tag, key, "error / bound = %.3g" % float((err / bound).max()))
        v = float((err / bound).max())
        prev = frac.get(key, 0.0)
        frac[key] = v if (math.isnan(v) or v > prev) else prev

    for b in range(x.shape[0]):
        if int(want_st[b]) != ST_OK:
            assert untouched(o, b), (tag, b, "outputs of a reverted / inactive instance changed")
            continue
        for key in ("c1", "consensus", "skew", "kurt", "rel", "qr"):   # a sentinel that was multiplied in shows as NaN
            assert bool(torch.isfinite(o[key][b]).all()), (tag, b, key, "not finite")
        mask = o["reliable"][b].bool()
        assert torch.equal(mask, ref["reliable"][b]), (tag, b, "reliable vs the fp64 model")
        # c1: the derived dot-product bound over the column's N values (module docstring)
        worst("c1", (o["c1"][b].double() - ref["c1"][b]).abs(), (N + 2) * U * x[b].abs().max(0).values)
        xr = x[b][mask]
        err = (o["consensus"][b].double() - ref["consensus"][b]).abs()
        if c["constrained"]:
            worst("consensus", err, (R + 2) * U * xr.abs().max(0).values)
        else:
            # fast_cases.check_round: an fp32 sum of terms shifted by c1 + 1 ulp of the reference
            bound = N * U * (x[b] - ref["c1"][b]).abs().mean(0) + fc._ulp32(ref["consensus"][b])
            worst("consensus", err, bound)
        for key, (rtol, atol) in fc.TOL["fp32"].items():   # qr, rel, skew, kurt: fast_cases' fp32 tolerances
            if key == "qr":
                atol = atol * c["scale"] ** 2
            worst(key, (o[key][b].double() - ref[key][b]).abs(), atol + rtol * ref[key][b].abs())
    print("FRAC %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(frac.items()))))
    for key, v in frac.items():
        assert v <= 1.0, (tag, key, "error / bound = %.3g" % v)
    return frac


# ---------------------------------------------------------------------------------------------- one-hot weights
def hot_ranks(n, multi_lane):
    """The ranks a one-hot row is tried at over n values: the ends, the middle pair and, for the multi-lane shapes,
    both sides of every 64-rank lane boundary below n."""
    ks = {0, 1, n // 2 - 1, n // 2, n - 2, n - 1}
    if multi_lane:
        ks |= {k for k in (63, 64, 65, 127, 128, 191, 192) if k < n}
    return sorted(k for k in ks if 0 <= k < n)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_one_hot(ops, shape, device):
    """One-hot weights pin the rank-to-register mapping across lanes and the sentinel handling: the estimate must be
    the k-th order statistic of the fp32 column, bit for bit (torch.sort on the CPU).

    c1: w1 = one_hot(N, k) in an unconstrained round (its reliability never leaves [0, 1], whatever the centre), all
    N rows.  consensus: w2 = one_hot(R, k) in a constrained round about the median centre (w1 = median_weights),
    over the rows the round reports reliable -- equal to the fp64 model's mask.  Instances that revert (the constant
    column; R < 4) must stay untouched."""
    N, D, f = shape
    R = N - f
    multi = N > 64
    cm = case(shape, "cons", ("median",))          # the median-centred model: its mask serves every k of pass 2
    x = cm["x"]
    xs = torch.sort(x[:, :, :D], dim=1).values                 # [B, N, D] fp32
    ms = math.sqrt(D)
    xd = x.to(device)
    n_checked = 0
    for k in hot_ranks(N, multi):
        w = est.pack(est.one_hot(N, k), est.mean_weights(R))
        o = run_lest(ops, xd, cm["active"], D, f, False, ms, w)
        for b in range(B):
            ok = b != INACTIVE and b != CONSTANT and R >= 4
            if not ok:
                assert untouched(o, b), (shape, k, b, "untouched")
                continue
            assert int(o["status"][b]) == ST_OK, (shape, k, b, o["status"])
            assert same_bits(o["c1"][b], xs[b, k]), (shape, "c1 one-hot", k, b)
            n_checked += 1
    for k in hot_ranks(R, multi):
        w = est.pack(est.median_weights(N), est.one_hot(R, k))
        o = run_lest(ops, xd, cm["active"], D, f, True, ms, w)
        assert torch.equal(o["status"], expected_status(cm)), (shape, k, o["status"])
        for b in range(B):
            if int(o["status"][b]) != ST_OK:
                assert untouched(o, b), (shape, k, b, "untouched")
                continue
            mask = o["reliable"][b].bool()
            assert torch.equal(mask, cm["ref"]["reliable"][b]), (shape, k, b, "reliable")
            xr = torch.sort(x[b, :, :D][mask], dim=0).values
            assert same_bits(o["consensus"][b], xr[k]), (shape, "consensus one-hot", k, b)
            n_checked += 1
    return n_checked


def check_median_vs_fast(ops, shape, device):
    """Median weights: c1, the constrained consensus and the mask equal what fast_round writes for the same fp32
    input on the same device, bit for bit (the two non-zero products w x are exact halvings, so their sum is rounded
    once in any order)."""
    from helpers import run_fast
    N, D, f = shape
    c = case(shape, "cons", ("median",))
    o = run_case(ops, c, device)
    fo = run_fast(c["x"].to(device), D, f, True, c["max_spread"], active=c["active"].to(device))
    fo = {k: v.cpu() for k, v in fo.items()}
    n = 0
    for b in range(B):
        if b == INACTIVE:
            continue
        assert int(o["status"][b]) == int(fo["status"][b]), (shape, b, o["status"], fo["status"])
        if int(o["status"][b]) != ST_OK:
            continue
        assert same_bits(o["c1"][b], fo["c1"][b]), (shape, b, "c1 vs fast_round")
        assert same_bits(o["consensus"][b], fo["consensus"][b]), (shape, b, "consensus vs fast_round")
        assert torch.equal(o["reliable"][b], fo["reliable"][b]), (shape, b, "reliable vs fast_round")
        n += 1
    return n
