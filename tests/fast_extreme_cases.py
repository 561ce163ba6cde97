"""Fast rounds whose failing oracles send huge finite values, against fast_cases.ref64 (CPU only).

The fast tier promises the honest consensus while at most n_failing rows are garbage.  Here the garbage is
finite but enormous: every component of k <= f rows is +-M with M a power of two (exact in bf16), in four tiers:

    T0  M = 2^20    nothing overflows in fp32; the all-rows-minus-removed power sums cancel completely
    T1  M = 2^40    d^4 overflows, d^2 does not
    T2  M = 2^80    d^2 overflows: qr = +inf in fp32
    T3  M = 2^126   the sum of f >= 4 outliers' first powers overflows

The batch axis of one case carries tier x outlier count (1, f) x sign pattern (+, -, alternating by row; the
alternating pattern of one row is the + one and is left out): 20 instances, one kernel launch.  Honest rows are
Beta(20, 20) mapped to x * 8 - 4 as fast_cases.signed_case does; rounds are unconstrained with max_spread =
8 sqrt(D).  Outlier rows: row 0 and row N - 1 always (a single outlier takes row 0 under +, row N - 1 under -),
then one row in every further 64-row segment while k allows, the rest drawn from a seeded permutation.

make() builds a case once (shared, never modified) and asserts what the data must meet (test_fast_extreme.py runs
it for every case): the rank-cut gap, the constructed mask == the ref64 mask, no ref64 qr within a factor 4 of
FLT_MAX, and a first reliability of exactly 0 (clamped).  check_extreme holds the assertions the CPU twin and the
HIP kernels share; shard_round runs a case as two unequal column shards (mode 1, fp32 sum of the qr partials, mode
2 with the global rel_dim) and expects slices of the whole-instance ref64.  Nothing here imports GPU code.
"""
import functools
import math

import numpy as np
import torch

import fast_cases as fc
import fast_shard_cases as sc
from helpers import beta_oracles

TIERS = (("T0", 20), ("T1", 40), ("T2", 80), ("T3", 126))
SIGNS = ("+", "-", "alt")
SCALE = 8.0
FLT_MAX = 3.4028234663852886e38

# (N, D, f)
SMALL = [(7, 6, 2), (16, 128, 3)]                                       # small kernel (bf16, hint 0)
WINDOW = [(17, 40, 2), (64, 33, 8), (65, 96, 8), (128, 64, 16), (255, 40, 31), (256, 24, 3)]
WINDOW_ROUTE = {(17, 40, 2): (1, 5), (64, 33, 8): (1, 5), (65, 96, 8): (2, 5), (128, 64, 16): (2, 17),
                (255, 40, 31): (4, 17), (256, 24, 3): (4, 5)}           # (lane groups, half-width H)
TWO_ONLY = [(100, 24, 40), (300, 24, 30), (2100, 8, 64)]                # two-network kernel under hint 0
TWO_GROUPS = {(100, 24, 40): 2, (300, 24, 30): 8, (2100, 8, 64): 64}
SPLIT = [(128, 64, 16, 23), (300, 24, 30, 9)]                           # (N, D, f, cut): T2 and T3 instances only
CLAMP_SHAPES = [(7, 6, 2, "bf16"), (64, 33, 8, "bf16"), (64, 33, 8, "fp32")]
# fp32 max_spread values ms with fl32(ms * fl32(1 / ms)) != 1 (found with clamp_search(): the product is 1 - 2^-24
# for each; no fp32 value gives a product above 1, see test_clamp_constants), between the honest rows' spread and
# the outliers'
CLAMP_MS = (41.0, 47.0, 55.0, 83.0)
# ... and values whose fp32 reciprocal is rounded UP: the rounded product is 1, the exact one 1 + (1 .. 6) x 2^-26.
# A fused multiply-subtract 1 - ms * fl32(1 / ms) sees that excess (a reliability below 0: RELIABILITY_INTERVAL where
# the contract's 1 - ms / ms is 0).  0.3 and 3 lie below the honest rows' spread: the second reliability clamps too.
CLAMP_MS_UP = (24.0, 30.0, 63.0, 3.0, 0.3)


def matrix():
    """Every (N, D, f, storage); the small-instance kernel exists for bf16 storage only."""
    out = []
    for storage in ("bf16", "fp32"):
        for shape in (SMALL if storage == "bf16" else []) + WINDOW + TWO_ONLY:
            out.append(shape + (storage,))
    return out


def split_matrix():
    return [s + (storage,) for storage in ("bf16", "fp32") for s in SPLIT]


def case_id(c):
    return "x".join(str(v) for v in c[:3]) + "".join("-%s" % v for v in c[3:])


def instances(f):
    """(tier, log2 M, k, sign pattern) of every instance of a batch."""
    out = []
    for tier, e in TIERS:
        for k in (1, f):
            for s in SIGNS:
                if not (k == 1 and s == "alt"):
                    out.append((tier, e, k, s))
    return out


def outlier_rows(N, k, sign, g):
    if k == 1:
        return [N - 1 if sign == "-" else 0]
    rows = [0, N - 1]
    for seg in range(1, (N + 63) // 64):
        r = 64 * seg + 31
        if len(rows) < k and r < N - 1:
            rows.append(r)
    for r in torch.randperm(N, generator=g).tolist():
        if len(rows) < k and r not in rows:
            rows.append(r)
    return sorted(rows)


# the default seed misses the rank-cut gap of 1e-4 in one instance of these: the next seed meets it
RESEEDED = {(300, 24, "bf16"): 1000, (2100, 8, "bf16"): 1000}


def seed_of(N, D, storage):
    return 1000 + N + D + RESEEDED.get((N, D, storage), 0)


def extreme_case(N, D, f, seed, dtype):
    """The storage tensor [B, N, ld], the outlier mask [B, N] and the instance list."""
    inst = instances(f)
    B = len(inst)
    base, _ = beta_oracles(B, N, D, 0, seed=seed, dtype=torch.float64)
    x = base[:, :, :D] * SCALE - SCALE / 2
    g = torch.Generator().manual_seed(seed + 1)
    out = torch.zeros(B, N, dtype=torch.bool)
    for b, (_, e, k, sign) in enumerate(inst):
        assert 1 <= k <= f
        for j, r in enumerate(outlier_rows(N, k, sign, g)):
            neg = sign == "-" or (sign == "alt" and j % 2 == 1)
            x[b, r] = -(2.0 ** e) if neg else 2.0 ** e
            out[b, r] = True
    return fc._pad(x, dtype), out, inst


def constructed_mask(qr, outlier, f):
    """Reliable = everything but the outliers and the f - k honest rows with the largest qr."""
    expect = ~outlier
    for b in range(qr.shape[0]):
        drop = f - int(outlier[b].sum())
        if drop:
            q = torch.where(outlier[b], torch.full_like(qr[b], -1.0), qr[b])
            expect[b, torch.topk(q, drop).indices] = False
    return expect


@functools.lru_cache(maxsize=None)
def make(case):
    N, D, f, storage = case
    x, outlier, inst = extreme_case(N, D, f, seed_of(N, D, storage), fc.DTYPES[storage])
    ms = SCALE * math.sqrt(D)
    ref = fc.ref64(x[:, :, :D], f, False, ms)
    c = dict(x=x, ref=ref, outlier=outlier, inst=inst, expect=constructed_mask(ref["qr"], outlier, f),
             max_spread=ms, scale=SCALE, constrained=False, N=N, D=D, f=f, storage=storage)
    preconditions(c)
    return c


def preconditions(c):
    ref, f, N, D = c["ref"], c["f"], c["N"], c["D"]
    x = c["x"]
    assert x.shape[0] == len(c["inst"]) and torch.isfinite(x).all() and (x[:, :, D:] == 0).all()
    assert (c["outlier"].sum(1) == torch.tensor([k for _, _, k, _ in c["inst"]])).all()
    assert c["outlier"][:, 0].any() and c["outlier"][:, N - 1].any()
    for b, (_, e, k, sign) in enumerate(c["inst"]):
        rows = c["outlier"][b].nonzero().flatten().tolist()
        assert (x[b, rows, :D].double().abs() == 2.0 ** e).all()
        if k > 1:
            assert 0 in rows and N - 1 in rows
            segs = {r // 64 for r in rows}
            assert len(segs) == min(k, (N + 63) // 64), (N, k, rows)
            assert (x[b, rows, 0] < 0).any() == (sign != "+") and (x[b, rows, 0] > 0).any() == (sign != "-")
    gap = fc.cut_gap(ref, f)                       # for k < f: among the honest rows
    assert (gap >= 1e-4).all(), gap
    assert torch.equal(ref["reliable"], c["expect"]) and (~c["expect"]).sum(1).eq(f).all()
    assert not (c["outlier"] & ref["reliable"]).any()
    q = ref["qr"]
    assert not ((q > FLT_MAX / 4) & (q < FLT_MAX * 4)).any()
    assert (ref["rel"][:, 0] == 0).all()
    assert ((ref["rel"][:, 1] > 0) & (ref["rel"][:, 1] < 1)).all()


def _worst(frac, key, err, bound):
    # a non-finite error becomes inf and stays (NaN <= 1 must not pass, and max() would drop a NaN)
    v = float((err / bound).max()) if err.numel() else 0.0
    frac[key] = max(frac.get(key, 0.0), v if math.isfinite(v) else math.inf)


def check_qr(got, want64, outlier, storage, scale, frac, key="qr"):
    """Honest rows within TOL; outlier rows +inf exactly where the fp64 value rounds to +inf in fp32, otherwise
    within TOL's rtol."""
    rtol, atol = fc.TOL[storage]["qr"]
    got = got.double()
    hon = ~outlier
    _worst(frac, key, (got[hon] - want64[hon]).abs(), atol * scale ** 2 + rtol * want64[hon].abs())
    w32 = want64.float()
    inf = outlier & torch.isinf(w32)
    assert (got[inf] == math.inf).all(), (key, "finite where the fp64 value overflows fp32", got[inf])
    fin = outlier & ~torch.isinf(w32)
    assert torch.isfinite(got[fin]).all(), (key, "not finite where the fp64 value fits fp32", got[fin])
    _worst(frac, key + "_out", (got[fin] - want64[fin]).abs(), rtol * want64[fin].abs())


def check_extreme(o, c, tag="", cols=None, rows=None):
    """o: outputs of one fast round over case c (CPU tensors).  cols = (lo, hi): o is a column shard's (c1,
    consensus, skew and kurt are the slices; qr, rel and the mask are the whole instance's).  rows: the instances
    of the batch that o holds.  Asserts every output of every instance and returns the largest error of each
    toleranced output as a fraction of its bound."""
    N, D, storage = c["N"], c["D"], c["storage"]
    lo, hi = cols or (0, D)
    sel = slice(None) if rows is None else rows
    ref = {k: v[sel] for k, v in c["ref"].items()}
    x, outlier, expect = c["x"][sel][:, :, lo:hi].double(), c["outlier"][sel], c["expect"][sel]
    assert (o["status"] == 0).all(), (tag, o["status"])
    for k in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
        assert not torch.isnan(o[k]).any(), (tag, k, "NaN")
    assert (o["reliable"] <= 1).all()
    mask = o["reliable"].bool()
    assert torch.equal(mask, ref["reliable"]), (tag, "reliable vs ref64")
    assert torch.equal(mask, expect), (tag, "reliable vs constructed mask")
    # c1: fast_cases.check_round's rule (the fp64 value rounded to fp32, compared by value)
    assert (o["c1"].double() == ref["c1"][:, lo:hi].float().double()).all(), (tag, "c1")
    frac = {}
    # fp32 sum over the R reliable rows of terms shifted by c1: check_round's forward bound, restated over the
    # reliable rows (the all-row mean of |x - c1| is ~ M here and would bound nothing)
    R = N - c["f"]
    dev = ((x - ref["c1"][:, None, lo:hi]).abs() * mask[:, :, None]).sum(1) / R
    want = ref["consensus"][:, lo:hi]
    _worst(frac, "consensus", (o["consensus"].double() - want).abs(), R * 2.0 ** -24 * dev + fc._ulp32(want))
    tol = fc.TOL[storage]
    for key in ("skew", "kurt"):
        rtol, atol = tol[key]
        want = ref[key][:, lo:hi]
        _worst(frac, key, (o[key].double() - want).abs(), atol + rtol * want.abs())
    rtol, atol = tol["rel"]
    want = ref["rel"][:, 1]
    _worst(frac, "rel2", (o["rel"][:, 1].double() - want).abs(), atol + rtol * want.abs())
    # the first reliability: exactly 0 in ref64 wherever the spread is clamped, and never below 0
    clamped = ref["rel"][:, 0] == 0
    r1 = o["rel"][:, 0].double()
    assert (r1[clamped] >= 0).all(), (tag, "rel1 < 0", r1)
    _worst(frac, "rel1", (r1 - ref["rel"][:, 0]).abs(), atol + rtol * ref["rel"][:, 0].abs())
    check_qr(o["qr"], ref["qr"], outlier, storage, c["scale"], frac)
    print("FRAC %s %s" % (tag, " ".join("%s=%.3g" % kv for kv in sorted(frac.items()))))
    for key, v in frac.items():
        assert v <= 1.0, (tag, key, "error / bound = %.3g" % v)
    return frac


# ------------------------------------------------------------------------------------------------ split modes
def split_rows(c):
    """The T2 and T3 instances of a case."""
    return [b for b, (tier, _, _, _) in enumerate(c["inst"]) if tier in ("T2", "T3")]


@functools.lru_cache(maxsize=None)
def make_split(case):
    """case: (N, D, f, cut, storage).  The shards as the engine stores them and the fp64 qr partial of each."""
    N, D, f, cut, storage = case
    c = make((N, D, f, storage))
    rows = split_rows(c)
    x = c["x"][rows][:, :, :D].double()
    bounds = [(0, cut), (cut, D)]
    assert cut != D - cut
    parts = sc._storage_parts(x, cut, fc.DTYPES[storage])
    c1 = c["ref"]["c1"][rows]
    partial = [((x[:, :, lo:hi] - c1[:, None, lo:hi]) ** 2).sum(-1) for lo, hi in bounds]
    return dict(c=c, rows=rows, bounds=bounds, parts=parts, partial=partial, cut=cut)


def shard_round(s, launch, tag=""):
    """One round of make_split()'s case as two column shards.  launch(part, x, args, mode, bufs) is
    fast_shard_cases.sharded_round's: one half on shard `part` with the output buffers prefilled from `bufs`,
    returning them as CPU tensors.  Returns the mode-2 outputs per shard."""
    c, rows = s["c"], s["rows"]
    N, B = c["N"], len(rows)
    outlier = c["outlier"][rows]
    frac = {}
    first = []
    for i, (lo, hi) in enumerate(s["bounds"]):
        a = dict(D=hi - lo, f=c["f"], constrained=False, max_spread=c["max_spread"], active=None, rel_dim=c["D"])
        o = launch(i, s["parts"][i], a, 1, sc.fresh_outputs(B, N, hi - lo))
        t = (tag, "mode 1", "shard %d" % i)
        assert (o["status"] == 0).all(), (t, o["status"])
        assert (o["c1"].double() == c["ref"]["c1"][rows][:, lo:hi].float().double()).all(), (t, "c1")
        assert not torch.isnan(o["qr"]).any(), (t, "NaN")
        check_qr(o["qr"], s["partial"][i], outlier, c["storage"], c["scale"], frac, "qr1")
        for k in sc.PASS2_OUTS:
            assert sc._is_sentinel(o, k), (t, k, "written by mode 1")
        first.append(o)
    assert all(v <= 1.0 for v in frac.values()), (tag, frac)       # (pass 2 would run on it)
    qr = first[0]["qr"] + first[1]["qr"]                            # the all-reduce: an fp32 sum
    second = []
    for i, (lo, hi) in enumerate(s["bounds"]):
        a = dict(D=hi - lo, f=c["f"], constrained=False, max_spread=c["max_spread"], active=None, rel_dim=c["D"])
        inp = sc._clone(first[i])
        inp["qr"] = qr.clone()
        o = launch(i, s["parts"][i], a, 2, sc._clone(inp))
        t = "%s mode 2 shard %d" % (tag, i)
        assert sc._same_bits(o["c1"], inp["c1"]), (t, "c1 changed")
        assert sc._same_bits(o["qr"], inp["qr"]), (t, "qr != the summed input")
        check_extreme(o, c, t, cols=(lo, hi), rows=rows)
        second.append(o)
    return second


# ------------------------------------------------------------------------------------------------ the clamp alone
def clamp_search(lo=20.0, hi=100.0):
    """fp32 integers ms in [lo, hi] with fl32(ms * fl32(1 / ms)) != 1, and whether any product exceeds 1."""
    ms = np.arange(lo, hi + 1, dtype=np.float32)
    prod = (ms * (np.float32(1) / ms).astype(np.float32)).astype(np.float32)
    return [float(v) for v in ms[prod != 1]], bool((prod > 1).any())


def reciprocal_excess(ms):
    """ms * fl32(1 / ms) - 1 exactly (fp64 holds the 48-bit product of two fp32 values)."""
    m = np.float32(ms)
    return float(m) * float(np.float32(np.float32(1) / m)) - 1.0


def clamp_rows(c):
    """The T0 (no overflow) and T2 instances of a case."""
    return [b for b, (tier, _, _, _) in enumerate(c["inst"]) if tier in ("T0", "T2")]


def clamp_spreads(D):
    return (SCALE * math.sqrt(D),) + CLAMP_MS + CLAMP_MS_UP


def check_clamp(o, c, ms, tag=""):
    """Status 0 and 0 <= rel1 <= atol; the mask does not depend on max_spread."""
    atol = fc.TOL[c["storage"]]["rel"][1]
    rows = clamp_rows(c)
    assert (o["status"] == 0).all(), (tag, ms, o["status"])
    r1 = o["rel"][:, 0].double()
    assert ((r1 >= 0) & (r1 <= atol)).all(), (tag, ms, r1)
    assert torch.equal(o["reliable"].bool(), c["expect"][rows]), (tag, ms, "reliable")
    r2 = o["rel"][:, 1].double()
    assert ((r2 >= 0) & (r2 <= 1)).all(), (tag, ms, r2)
