"""Signed and rank-cut-tie cases for the fast-mode kernels, with a plain fp64 reference (CPU only).

ref64 is written from the contract's formulas (svoc/ops/torch_ref.py docstring), in fp64 over
x.double(), with a Python sort for the rank rule (qr ascending, index descending): independent of the
fp32 reference and of any device.  signed_case / tie_case build the data; check_round holds the
assertions that test_fast_signed_ties.py (CPU engine) and test_fast_signed_ties_gpu.py (HIP kernels)
share.  Nothing here imports GPU code.
"""
import functools
import math

import torch

from helpers import beta_oracles

# (N, D, f): one dispatch path or lane-group width each
SMALL = [(7, 6, 2), (8, 5, 2), (9, 2, 2), (16, 3, 3), (16, 128, 3)]     # small kernel under hint 0 (bf16)
SMALL_SIGNED_ONLY = [(9, 1, 2)]                                         # D = 1 cannot carry tie_case
LANES = [(17, 40, 2), (63, 7, 1), (64, 33, 8),                          # 1 lane / column
         (65, 96, 8), (128, 64, 16),                                    # 2 lanes
         (129, 33, 32), (255, 40, 31), (256, 72, 32), (256, 24, 3),     # 4 lanes
         (100, 24, 40), (256, 40, 40),                                  # f > 32: two-network kernel
         (300, 24, 30), (600, 16, 64), (1100, 16, 100), (2100, 8, 64)]  # 8 / 16 / 32 / 64 lanes
SIGNED_MAPS = [(4.0, -1.5), (-4.0, 1.5), (8.0, -4.0)]
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def batch_of(N):
    return 6 if N <= 1024 else 3


def matrix():
    """Every (family, N, D, f, storage) the two test files run.  family: ("signed", scale, shift) or
    ("tie", signed).  The small-instance kernel exists for bf16 storage only."""
    out = []
    for storage in ("bf16", "fp32"):
        small = SMALL + SMALL_SIGNED_ONLY if storage == "bf16" else []
        for N, D, f in small + LANES:
            for sc, sh in SIGNED_MAPS:
                out.append((("signed", sc, sh), N, D, f, storage))
            if D > 1:
                out.append((("tie", False), N, D, f, storage))
                out.append((("tie", True), N, D, f, storage))
    return out


def case_id(c):
    fam, N, D, f, storage = c
    name = "signed%+g%+g" % fam[1:] if fam[0] == "signed" else ("tie_signed" if fam[1] else "tie")
    return "%s-%dx%dx%d-%s" % (name, N, D, f, storage)


def _pad(x, dtype):
    B, N, D = x.shape
    out = torch.zeros(B, N, (D + 7) // 8 * 8, dtype=dtype)
    out[:, :, :D] = x.to(dtype)            # round to the storage type last
    return out


def signed_case(B, N, D, f, scale, shift, seed, dtype):
    """beta_oracles data mapped to x * scale + shift; for (8, -4) and D >= 4 three structured columns."""
    base, _ = beta_oracles(B, N, D, f, seed=seed, dtype=torch.float64)
    base = base[:, :, :D]
    x = base * scale + shift
    if (scale, shift) == (8.0, -4.0) and D >= 4:
        g = torch.Generator().manual_seed(seed + 1)
        h, q = N // 2, N // 4
        for b in range(B):
            p = torch.randperm(N, generator=g)
            x[b, :, 0] = 1.0                       # median pair straddles zero: c1 = 0 exactly
            x[b, p[:h], 0] = -1.0
            p = torch.randperm(N, generator=g)
            z = N - 2 * q
            x[b, p[:q], 1] = -0.5                  # c1 = 0 by value among -0.0 / +0.0, variance > 0
            x[b, p[q:2 * q], 1] = 0.5
            x[b, p[2 * q:2 * q + z // 2], 1] = -0.0
            x[b, p[2 * q + z // 2:], 1] = 0.0
            x[b, :, 2] = -(4.0 * base[b, :, 2] + 1.0)   # all in [-5, -1]
    return _pad(x, dtype)


def tie_params(N, f):
    t = min(max(2, f + 1), 5, N - f - 3)
    k = min(max(1, min(f, t - 1)), t - 1)
    return t, k


def tie_case(B, N, D, f, t, k, seed, dtype, signed):
    """Honest Beta(20,20) rows; t identical rows (0.5 +- 0.3, sign alternating by column) of which the
    rank cut drops the k with the lowest indices; f - k far rows of alternating 0 / 1.  Returns the
    data and the expected reliable mask."""
    assert 1 <= k < t and f - k >= 0
    x, _ = beta_oracles(B, N, D, 0, seed=seed, dtype=torch.float64)
    x = x[:, :, :D].clone()
    g = torch.Generator().manual_seed(seed + 1)
    alt = (torch.arange(D) % 2).double()
    tied_row = 0.5 + 0.3 * (1.0 - 2.0 * alt)
    expect = torch.ones(B, N, dtype=torch.bool)
    for b in range(B):
        inner = (torch.randperm(N - 2, generator=g) + 1).tolist()      # rows 1 .. N-2, shuffled
        tied = sorted([0, N - 1] + inner[:t - 2])
        far = inner[t - 2:t - 2 + f - k]
        x[b, tied] = tied_row
        for j, r in enumerate(far):
            x[b, r] = alt if j % 2 == 0 else 1.0 - alt
        expect[b, far] = False
        expect[b, tied[:k]] = False
    if signed:
        x = x * 8.0 - 4.0
    return _pad(x, dtype), expect


def _smooth_median(col_sorted, count):
    m = count // 2
    return 0.5 * (col_sorted[m - 1] + col_sorted[m])


def ref64(x, f, constrained, max_spread, legacy=False):
    """One fast round per instance in fp64.  x: [B, N, D] of any float dtype.  Returns fp64 tensors
    (reliable: bool).  legacy: the obsolete contracts' round (svoc/reference.py consensus_round): the
    constrained reliability without the / D, skewness and kurtosis zero."""
    x = x.double()
    B, N, D = x.shape
    R = N - f
    c1 = torch.empty(B, D, dtype=torch.float64)
    qr = torch.empty(B, N, dtype=torch.float64)
    reliable = torch.zeros(B, N, dtype=torch.bool)
    cons = torch.empty(B, D, dtype=torch.float64)
    rel = torch.empty(B, 2, dtype=torch.float64)
    skew = torch.empty(B, D, dtype=torch.float64)
    kurt = torch.empty(B, D, dtype=torch.float64)

    def rel_of(mean_qr):
        if constrained:
            return 1.0 - 2.0 * math.sqrt(mean_qr / (1 if legacy else D))
        return 1.0 - min(math.sqrt(mean_qr), max_spread) / max_spread

    for b in range(B):
        xs = torch.sort(x[b], dim=0).values
        c1[b] = _smooth_median(xs, N)
        qr[b] = ((x[b] - c1[b]) ** 2).sum(-1)
        q = qr[b].tolist()
        order = sorted(range(N), key=lambda i: (q[i], -i))     # qr ascending, index descending
        keep = sorted(order[:R])
        reliable[b, keep] = True
        xr = x[b, keep]
        if constrained:
            cons[b] = _smooth_median(torch.sort(xr, dim=0).values, R)
        else:
            cons[b] = xr.sum(0) / R
        rel[b, 0] = rel_of(sum(q) / N)
        rel[b, 1] = rel_of(sum(q[i] for i in keep) / R)
        y = xr - xr.sum(0) / R
        m2, m3, m4 = (y ** 2).sum(0) / R, (y ** 3).sum(0) / R, (y ** 4).sum(0) / R
        n = float(R)
        safe = m2 > 0
        m2s = torch.where(safe, m2, torch.ones_like(m2))
        z3 = n * m3 / m2s ** 1.5
        z4 = n * m4 / m2s ** 2
        skew[b] = torch.where(safe, z3 * n / ((n - 1) * (n - 2)), torch.zeros_like(z3))
        kurt[b] = torch.where(safe, (z4 * n * (n + 1) / (n - 1) - 3 * (n - 1) ** 2) / ((n - 2) * (n - 3)),
                              torch.zeros_like(z4))
        if legacy:
            skew[b], kurt[b] = 0.0, 0.0
    return dict(c1=c1, qr=qr, reliable=reliable, consensus=cons, rel=rel, skew=skew, kurt=kurt)


@functools.lru_cache(maxsize=None)
def make(case):
    """Data, reference and round arguments of one matrix() entry (built once, shared, never modified)."""
    fam, N, D, f, storage = case
    B, dtype, seed = batch_of(N), DTYPES[storage], N + D
    if fam[0] == "signed":
        scale, constrained, expect = fam[1], False, None
        x = signed_case(B, N, D, f, fam[1], fam[2], seed, dtype)
    else:
        scale, constrained = (8.0, False) if fam[1] else (1.0, True)
        t, k = tie_params(N, f)
        x, expect = tie_case(B, N, D, f, t, k, seed, dtype, fam[1])
    # rel is scale-free with the spread bound in the data's units
    ms = abs(scale) * math.sqrt(D)
    ref = ref64(x[:, :, :D], f, constrained, ms)
    return dict(x=x, ref=ref, expect=expect, constrained=constrained, max_spread=ms, scale=scale,
                structured=fam == ("signed", 8.0, -4.0) and D >= 4, N=N, D=D, f=f, storage=storage, family=fam[0])


def cut_gap(ref, f):
    """Relative qr gap between sorted ranks R-1 and R, per instance."""
    s = torch.sort(ref["qr"], dim=1).values
    R = s.shape[1] - f
    return (s[:, R] - s[:, R - 1]) / s[:, R]


def tie_group_gap(ref, f):
    """tie_case: (|qr[R-1] - qr[R]|, smallest relative distance from the tie group to any other qr)."""
    s = torch.sort(ref["qr"], dim=1).values
    R = s.shape[1] - f
    q = s[:, R:R + 1]
    d = ((s - q).abs() / q)
    d = torch.where(s == q, torch.full_like(d, float("inf")), d)
    return (s[:, R] - s[:, R - 1]).abs(), d.min(dim=1).values


# Borrowed fast-mode tolerances against a reference: (rtol, atol).  bf16: test_ops_gpu._cmp_fast;
# fp32: test_f32_gpu.test_f32_kernel_vs_torch.  The qr atol is in squared data units (x scale^2);
# rel, skew and kurt are scale-free.
TOL = {"bf16": dict(qr=(2e-4, 1e-5), rel=(1e-4, 1e-4), skew=(2e-3, 2e-3), kurt=(2e-3, 5e-3)),
       "fp32": dict(qr=(2e-5, 1e-6), rel=(1e-5, 1e-6), skew=(1e-3, 5e-4), kurt=(1e-3, 5e-4))}


def _ulp32(v):
    a = v.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def check_round(o, c, tag=""):
    """o: outputs of one fast round over case c (CPU tensors).  Asserts mask / c1 / consensus / moments
    against ref64 and returns the largest error of each toleranced output as a fraction of its bound."""
    ref, x, N, D = c["ref"], c["x"][:, :, :c["D"]].double(), c["N"], c["D"]
    assert (o["status"] == 0).all(), (tag, o["status"])
    mask = o["reliable"].bool()
    assert torch.equal(mask, ref["reliable"]), (tag, "reliable vs ref64")
    if c["expect"] is not None:
        assert torch.equal(mask, c["expect"]), (tag, "reliable vs constructed mask")
    # c1 / constrained consensus: one correctly rounded fp32 add of two storage values and an exact
    # halving == the fp64 value rounded to fp32.  Compared by value (-0.0 == +0.0).
    assert (o["c1"].double() == ref["c1"].float().double()).all(), (tag, "c1")
    if c["structured"]:
        assert (o["c1"][:, :2] == 0).all(), (tag, "structured c1")
    frac = {}
    if c["constrained"]:
        assert (o["consensus"].double() == ref["consensus"].float().double()).all(), (tag, "consensus")
    else:
        # fp32 sum of terms shifted by c1: |err| <= N * 2^-24 * mean_i |x_i - c1| + 1 ulp(reference)
        bound = N * 2.0 ** -24 * (x - ref["c1"][:, None, :]).abs().mean(1) + _ulp32(ref["consensus"])
        err = (o["consensus"].double() - ref["consensus"]).abs()
        frac["consensus"] = float((err / bound).max())
    for key, (rtol, atol) in TOL[c["storage"]].items():
        if key == "qr":
            atol = atol * c["scale"] ** 2
        err = (o[key].double() - ref[key]).abs()
        frac[key] = float((err / (atol + rtol * ref[key].abs())).max())
    print("FRAC %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(frac.items()))))
    for key, v in frac.items():
        assert v <= 1.0, (tag, key, "error / bound = %.3g" % v)
    return frac
