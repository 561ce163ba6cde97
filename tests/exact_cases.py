"""Cases that pin every exact-round engine to the Python golden model (CPU only; nothing here touches a GPU).

The expected values of a case come from svoc.reference.round_status alone -- the pure-integer model that
tests/test_reference.py ties to the contract's goldens -- never from the CPU engine or a kernel.  make(case) builds
the int64 [B, N, D] values, runs the model once per instance and returns the eight output tensors an engine must
produce over outputs prefilled with PATTERN: the model's integers as an int64 holds them (reference.wrap_i64), and
the untouched pattern on every output but `status` where the model reverts.  test_exact_model.py runs the CPU
engine against it, test_exact_model_gpu.py every kernel route.

One batch mixes roles, so that a hand-off or a revert sits beside committed neighbours:
  plain     Beta(20,20) honest rows and f uniform ones (helpers.beta_oracles in fp64, scaled to wsad);
  tie       t identical rows at indices 0, 63, 64, N - 1 (both sides of a 64-row lane segment) whose equal qr
            straddles the rank cut: the cut drops the k lowest-indexed of them (qr ascending, index descending);
  dups      a column of three distinct values with an equal median pair, and one whose median pair has an odd sum
            (the halving truncates; toward zero where the unconstrained map makes the sum negative);
  outlier   a reliable row far out in one column only (|z| large: the int64 z-power forms);
  revert    a zero-variance column, a variance of exactly 1 (wsqrt(1) divides by zero), rel1 < 0, or rel1 < 0
            together with a zero-variance column (the stage order decides the code), rotating over the matrix.
Reverts that follow from the round's arguments (R = 3, 2, 1, n_failing > N, max_spread = 0) are whole cases (`arg`).
Unconstrained batches rotate the two moment reverts only: W - wsad_div(min(ms, sd), ms) saturates at 0 once
sd >= ms and cannot leave [0, 1] for ms > 0, so no data gives an unconstrained reliability fault.

Unconstrained families map the same unit data through v = centre[c] + (x - 500000) k with an odd k:
  narrow_a  k = 17, centres within int32 (also run with int32 storage): deviations below 2^25;
  narrow_b  k = 513, centres up to 2^51 of both signs and 0: deviations past 2^25, still within 2^30 of row 0;
  wide      k = 60001 (2^30 <= spread < 2^37), centres of both signs up to 2^52: the wide-column kernel (N <= 256);
  wide_n    the same values at N > 256, and past37 (k = 2000001): the i128 kernel's domain;
  past64    values uniform in +-2^62: the model says OK with qr near 2^106 and the engines hold it wrapped;
  overflow  one instance whose pass-1 deviation squared passes 2^127: the model raises OVERFLOW.
"""
import collections
import functools

import torch

from fixtures import GOLDEN
from helpers import beta_oracles
from svoc import reference as ref
from svoc.status import Status
from wsadx_cases import MS, OUTS, PATTERN

Case = collections.namedtuple("Case", "family N D f bf legacy storage arg")
# family: con | narrow_a | narrow_b | wide | wide_n | past37 | past64 | overflow; f: the round's n_failing; bf: the
# failing rows the data is built with; arg: None or the argument-level revert (R3, R2, R1, fgtN, ms0)

CON = [(7, 6, 2), (33, 70, 4), (64, 33, 20), (65, 64, 8), (128, 40, 30), (129, 33, 3), (256, 24, 32), (256, 24, 100),
       (300, 16, 30), (600, 8, 64), (1100, 8, 100), (2100, 4, 64), (4096, 4, 64)]
NARROW = [(7, 6, 2), (33, 70, 4), (65, 64, 8), (256, 24, 32), (300, 16, 30), (1100, 8, 100), (4096, 4, 64)]
WIDE = [(16, 64, 3), (64, 33, 8), (100, 24, 10), (200, 24, 20), (256, 24, 32)]
LEGACY = [(7, 1, 2), (64, 33, 8)]
# (family, N, D, f, bf, arg)
ARG = [("con", 64, 33, 61, 8, "R3"), ("con", 300, 16, 297, 30, "R3"), ("con", 65, 64, 63, 8, "R2"),
       ("con", 7, 6, 5, 2, "R2"), ("con", 129, 33, 128, 3, "R1"), ("con", 600, 8, 599, 64, "R1"),
       ("con", 33, 70, 34, 4, "fgtN"), ("con", 256, 24, 257, 32, "fgtN"), ("con", 7, 6, 8, 2, "fgtN"),
       ("narrow_a", 64, 33, 8, 8, "ms0"), ("wide", 64, 33, 61, 8, "R3"), ("narrow_b", 33, 70, 32, 4, "R1"),
       ("narrow_a", 65, 64, 66, 8, "fgtN")]
# the window half-width and lanes per column the constrained shapes claim to reach (check_routes)
CLAIM = {(7, 6, 2): (1, 5), (33, 70, 4): (1, 5), (64, 33, 20): (1, 0), (65, 64, 8): (2, 5), (128, 40, 30): (2, 17),
         (129, 33, 3): (4, 5), (256, 24, 32): (4, 17), (256, 24, 100): (4, 0), (300, 16, 30): (8, 0),
         (600, 8, 64): (16, 0), (1100, 8, 100): (32, 0), (2100, 4, 64): (64, 0), (4096, 4, 64): (64, 0)}

K = {"con": 1, "narrow_a": 17, "narrow_b": 513, "wide": 60001, "wide_n": 60001, "past37": 2000001, "overflow": 17}
CENTRES = {"con": [500000],
           "narrow_a": [0, -300_000_000, 500_000_000, 3_000_001], "overflow": [0, -300_000_000, 500_000_000],
           "narrow_b": [60_000_000_001, -3_000_000_000, 0, -(1 << 51)],
           "wide": [60_000_000_001, -60_000_000_000, (1 << 52) + 12345, -(1 << 52) - 999, 0],
           "wide_n": [60_000_000_001, -60_000_000_000, (1 << 52) + 12345, -(1 << 52) - 999, 0],
           "past37": [0, 60_000_000_001, -(1 << 55)]}
FAMILY_SEED = {"con": 0, "narrow_a": 1, "narrow_b": 2, "wide": 3, "wide_n": 4, "past37": 5, "past64": 6, "overflow": 7}
REVERTS_CON = ["zero_var", "var_one", "rel1_neg", "two_faults"]
REVERTS_UNC = ["zero_var", "var_one"]
INTENDED = {"zero_var": Status.DIV_BY_ZERO, "var_one": Status.DIV_BY_ZERO, "rel1_neg": Status.RELIABILITY_INTERVAL,
            "two_faults": Status.RELIABILITY_INTERVAL}
INT32_MAX = (1 << 31) - 1


# --------------------------------------------------------------------------------------------------- the matrix
def batch_of(N):
    return 6 if N < 2048 else 3


def matrix(storage=("int64", "int32")):
    out = []
    for N, D, f in CON:
        out.append(Case("con", N, D, f, f, False, "int64", None))
    for N, D, f in LEGACY:
        out.append(Case("con", N, D, f, f, True, "int64", None))
    for i, (N, D, f) in enumerate(NARROW):
        out.append(Case("narrow_a" if i % 2 == 0 else "narrow_b", N, D, f, f, False, "int64", None))
    for N, D, f in WIDE:
        out.append(Case("wide", N, D, f, f, False, "int64", None))
    out.append(Case("past37", 9, 3, 2, 2, False, "int64", None))
    out.append(Case("wide_n", 300, 16, 30, 30, False, "int64", None))
    out.append(Case("past64", 9, 3, 2, 2, False, "int64", None))
    out.append(Case("overflow", 9, 3, 2, 2, False, "int64", None))
    for fam, N, D, f, bf, arg in ARG:
        out.append(Case(fam, N, D, f, bf, False, "int64", arg))
    # int32 storage: every constrained case, and every unconstrained one whose values fit
    out += [c._replace(storage="int32") for c in out if c.family in ("con", "narrow_a")]
    return [c for c in out if c.storage in storage]


def case_id(c):
    return "%s%s-%dx%dx%d%s-%s" % (c.family, "_legacy" if c.legacy else "", c.N, c.D, c.f,
                                   "-" + c.arg if c.arg else "", c.storage)


def constrained(c):
    return c.family == "con"


def exact_win_h(N, f):
    """csrc/include/svoc/launch.hpp exact_win_h, restated."""
    if N < 4 or N > 256 or f < 0 or f > N - 2:
        return 0
    R = N - f
    a = N // 2 - R // 2
    need = max(a + 1, f - a + 1)
    return 5 if need <= 5 else (17 if need <= 17 and N > 64 else 0)


def lanes(N):
    """Lanes per column of the column kernels (consensus_wsad.hip / consensus_wsadx.hip dispatch)."""
    return next(g for g, top in ((1, 64), (2, 128), (4, 256), (8, 512), (16, 1024), (32, 2048), (64, 4096)) if N <= top)


def roles(c):
    if c.family == "past64":
        return ["uniform"] * batch_of(c.N)
    if c.family == "overflow":
        return ["overflow"] + ["plain"] * 5
    if batch_of(c.N) == 6:
        return ["plain", "tie", "revert", "dups", "outlier", "golden" if (c.N, c.D, c.family) == (7, 6, "con") else "revert"]
    return ["tie", ["dups", "outlier", "plain"][(c.N + c.f) % 3], "revert"]


def revert_kind(c, slot):
    kinds = REVERTS_CON if constrained(c) else REVERTS_UNC
    kind = kinds[(c.N + c.D + c.bf + slot) % len(kinds)]
    return "zero_var" if kind == "two_faults" and c.D < 3 else kind


# --------------------------------------------------------------------------------------------- unit data builders
def _plain(N, D, f, seed):
    x, _ = beta_oracles(1, N, D, f, seed=seed, dtype=torch.float64)
    return (x[0, :, :D] * 1e6).round().to(torch.int64)


def _far_row(D, j):
    alt = (torch.arange(D) % 2) * 1_000_000
    return alt if j % 2 == 0 else 1_000_000 - alt


def tie_rows(N, f):
    """(tied row indices, k): the rows on both sides of a lane-segment edge where N allows; the cut drops k."""
    tied = sorted({i for i in (0, 63, 64, N - 1) if i < N})
    return tied, min(f, len(tied) // 2)


def _tie(N, D, f, seed):
    tied, k = tie_rows(N, f)
    x = _plain(N, D, 0, seed)
    g = torch.Generator().manual_seed(seed + 1)
    others = [i for i in torch.randperm(N, generator=g).tolist() if i not in tied]
    x[tied] = 500_000 + 300_000 * (1 - 2 * (torch.arange(D) % 2))
    for j, r in enumerate(others[:f - k]):
        x[r] = _far_row(D, j)
    return x


def _dups(N, D, f, seed):
    x = _plain(N, D, f, seed)
    if D < 3:
        return x
    g = torch.Generator().manual_seed(seed + 1)
    p, q = torch.randperm(N, generator=g), max(2, N // 4)
    x[:, 0] = 500_000                       # {0, 500000, 1000000}: the median pair is equal
    x[p[:q], 0] = 0
    x[p[q:2 * q], 0] = 1_000_000
    p, mid = torch.randperm(N, generator=g), N // 2
    x[p[:mid], 1] = 250_001                 # {250001, 750000, 1000000}: the median pair sums to an odd number
    x[p[mid:], 1] = 750_000
    x[p[N - 2:], 1] = 1_000_000
    return x


def outlier_at(N, D, f, seed):
    g = torch.Generator().manual_seed(seed + 1)
    p = torch.randperm(N, generator=g).tolist()
    return p[:f], p[f], seed % D            # far rows, the outlier's row, its column


def _outlier(N, D, f, seed):
    x = _plain(N, D, 0, seed)
    if D < 2:
        return x
    far, r, col = outlier_at(N, D, f, seed)
    for j, i in enumerate(far):
        x[i] = _far_row(D, j)
    x[:, col] = 500_000 + torch.div(x[:, col] - 500_000, 2, rounding_mode="trunc")   # a tight column: |z| > 5.79
    for j, i in enumerate(far):
        x[i, col] = _far_row(D, j)[col]
    x[r, col] = 1_000_000
    return x


def _rel1_neg(N, D, seed, const_col):
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.full((N, D), 1_000_000, dtype=torch.int64)
    x[torch.randperm(N, generator=g)[:N // 2 + 1]] = 0      # c1 = 0 and half the rows one unit away: rel1 < 0
    if const_col:
        x[:, 0] = 500_000
    return x


def build(c):
    """values [B, N, D] int64, and per instance (role, revert kind, the outlier's (row, column))."""
    B = batch_of(c.N)
    g = torch.Generator().manual_seed(77 + c.N + c.D)
    if c.family == "past64":
        return torch.randint(-(1 << 62), (1 << 62) + 1, (B, c.N, c.D), generator=g, dtype=torch.int64), \
            [("uniform", None, None)] * B
    fam = c.family
    k, centres = K[fam], CENTRES[fam]
    centre = torch.tensor([centres[d % len(centres)] for d in range(c.D)], dtype=torch.int64)
    vals, tags = [], []
    for slot, role in enumerate(roles(c)):
        seed = 1000 * slot + c.N + 7 * c.D + c.bf + 100_000 * FAMILY_SEED[fam]
        kind = revert_kind(c, slot) if role == "revert" else None
        if role == "golden":
            x = torch.tensor(GOLDEN["constrained_6d"][0], dtype=torch.int64)
        elif role == "tie":
            x = _tie(c.N, c.D, c.bf, seed)
        elif role == "dups":
            x = _dups(c.N, c.D, c.bf, seed)
        elif role == "outlier":
            x = _outlier(c.N, c.D, c.bf, seed)
        elif kind in ("rel1_neg", "two_faults"):
            x = _rel1_neg(c.N, c.D, seed, kind == "two_faults")
        else:
            x = _plain(c.N, c.D, c.bf, seed)
        if c.legacy and c.D > 1:   # no / D in the obsolete reliability: a quarter of the spread keeps rel1 >= 0
            x = 500_000 + torch.div(x - 500_000, 4, rounding_mode="trunc")
        v = centre + (x - 500_000) * k
        col = seed % c.D
        if kind == "zero_var":
            v[:, col] = centre[col] - 200_000 * k
        if kind == "var_one":      # every deviation from the mean within 1000 +- 200: each qdev is exactly 1
            v[:, col] = centre[col] + 1000 * (1 - 2 * (torch.arange(c.N) % 2))
        if role == "overflow":     # c1 = -2^63, and x - c1 = 2^64 - 1 squares past 2^127
            v[:, col] = torch.iinfo(torch.int64).max
            v[:c.N // 2 + 1, col] = torch.iinfo(torch.int64).min
        vals.append(v)
        at = outlier_at(c.N, c.D, c.bf, seed)[1:] if role == "outlier" and c.D >= 2 else None
        tags.append((role, kind, at))
    return torch.stack(vals).contiguous(), tags


def domain(v):
    """Which kernel's value domain one unconstrained instance [N, D] is in, from the kernels' header contracts:
    narrow (consensus_wsad.hip: |B| < 2^52, every value within [-2^30, 2^30) of its column's row 0, B), wide
    (consensus_wsadx.hip: |B| < 2^61, |x - B| < 2^37, N <= 256), else i128."""
    N = v.shape[0]
    base = [int(b) for b in v[0]]
    lo = [int(m) - b for m, b in zip(v.min(0).values, base)]
    hi = [int(m) - b for m, b in zip(v.max(0).values, base)]
    if all(abs(b) < (1 << 52) for b in base) and all(l >= -(1 << 30) for l in lo) and all(h < (1 << 30) for h in hi):
        return "narrow"
    if N <= 256 and all(abs(b) < (1 << 61) for b in base) and all(max(-l, h) < (1 << 37) for l, h in zip(lo, hi)):
        return "wide"
    return "i128"


# ------------------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model(c):
    assert c.storage == "int64"
    values, tags = build(c)
    B, N, D = values.shape
    ms = 0 if c.arg == "ms0" else MS
    exp = {k: torch.full((B, D), PATTERN[k], dtype=torch.int64) for k in ("c1", "consensus", "skew", "kurt")}
    exp["rel"] = torch.full((B, 2), PATTERN["rel"], dtype=torch.int64)
    exp["qr"] = torch.full((B, N), PATTERN["qr"], dtype=torch.int64)
    exp["reliable"] = torch.full((B, N), PATTERN["reliable"], dtype=torch.uint8)
    exp["status"] = torch.zeros(B, dtype=torch.int32)
    results, wrapped = [], False
    for b in range(B):
        st, r = ref.round_status(values[b].tolist(), c.f, constrained(c), ms, c.legacy)
        results.append(r)
        exp["status"][b] = int(st)
        if r is None:
            continue
        rows = {"c1": r.c1, "consensus": r.consensus, "skew": r.skewness, "kurt": r.kurtosis, "rel": [r.rel1, r.rel2],
                "qr": r.qr}
        for k, row in rows.items():
            w = [ref.wrap_i64(x) for x in row]
            wrapped = wrapped or w != list(row)
            exp[k][b] = torch.tensor(w, dtype=torch.int64)
        exp["reliable"][b] = torch.tensor(r.reliable, dtype=torch.uint8)
    # the engines hold int64: only the designated case may need the wrap
    assert wrapped == (c.family == "past64"), case_id(c)
    doms = [None if constrained(c) else domain(values[b]) for b in range(B)]
    ok = [r is not None for r in results]
    # Decided by the column kernel alone (consensus_wsad.hip), committed or reverted.  Constrained: every instance
    # over [0, 1e6] but R < 2 with f <= N once rel1 passed (the kernel hands the smooth median's error code to the
    # i128 kernel: its `fb` flag); the staged moments are int32, which make() asserts they fit.  Unconstrained: the
    # narrow domain.  Reverts included: a reliable column of variance 0 or 1 is the kernel's own DIV_BY_ZERO.
    if constrained(c):
        assert int(values.min()) >= 0 and int(values.max()) <= 1_000_000
        for r in results:
            assert r is None or all(abs(x) <= INT32_MAX for x in r.skewness + r.kurtosis)
        handed = 0 <= c.f <= N and N - c.f < 2
        column = [not handed or int(s) == Status.RELIABILITY_INTERVAL for s in exp["status"]]
        n_x = 0
    else:
        column = [d == "narrow" for d in doms]
        n_x = sum(1 for d, o in zip(doms, ok) if d == "wide" and o)
    return dict(values=values, f=c.f, constrained=constrained(c), legacy=c.legacy, ms=ms, exp=exp, tags=tags,
                results=results, domains=doms, column=column, stats=[n_x, column.count(False) - n_x])


def make(c):
    """The case: values in the case's storage type, the round's arguments, `exp` (the eight expected tensors),
    `column` (per instance: the column kernel decides it alone), `stats` (the dispatcher's [wide-column, i128]
    counters) and the model's results."""
    m = dict(_model(c._replace(storage="int64")))
    if c.storage == "int32":
        v = m["values"]
        assert int(v.min()) >= -(1 << 31) and int(v.max()) < (1 << 31), case_id(c)
        m["values"] = v.to(torch.int32)
    return m


# ----------------------------------------------------------------------------------------------- self-checks
def check_routes():
    """The matrix reaches what it claims: windows {5, none} at 1 lane, {5, 17} at 2, {5, 17, none} at 4, lane groups
    8 .. 64, the wide-column kernel at 1 / 2 / 4 lanes, the i128-only domains."""
    got = {}
    for N, D, f in CON:
        assert CLAIM[(N, D, f)] == (lanes(N), exact_win_h(N, f)), (N, D, f)
        got.setdefault(lanes(N), set()).add(exact_win_h(N, f))
    assert got[1] == {5, 0} and got[2] == {5, 17} and got[4] == {5, 17, 0}, got
    assert all(got[g] == {0} for g in (8, 16, 32, 64)), got
    assert any(D % (4 * 64 // lanes(N)) != 0 for N, D, f in CON)          # a partial last slab
    assert {lanes(N) for N, D, f in WIDE} == {1, 2, 4}
    assert {lanes(N) for N, D, f in NARROW} == {1, 2, 4, 8, 32, 64}
    fams = {c.family for c in matrix()}
    assert {"past37", "wide_n", "past64", "overflow"} <= fams


def check_case(c):
    """What the builders intended holds in the model: value domains, the tie straddles the cut, the outlier is
    reliable and far out, the plain roles commit, each revert gives its code."""
    m = make(c)
    N, D, R = c.N, c.D, c.N - c.f
    status = [Status(int(s)) for s in m["exp"]["status"]]
    if not constrained(c):
        want = {"narrow_a": "narrow", "narrow_b": "narrow", "wide": "wide", "overflow": None}.get(c.family, "i128")
        assert all(d == want for d in m["domains"]) or want is None, (case_id(c), m["domains"])
    arg_code = {None: None, "R3": Status.DIV_BY_ZERO, "R2": Status.DIV_BY_ZERO, "fgtN": Status.USIZE_UNDERFLOW,
                "ms0": Status.DIV_BY_ZERO, "R1": Status.INDEX_OOB if constrained(c) else Status.DIV_BY_ZERO}[c.arg]
    for b, (role, kind, at) in enumerate(m["tags"]):
        r = m["results"][b]
        if kind in ("rel1_neg", "two_faults"):
            assert status[b] == INTENDED[kind], (case_id(c), b, kind, status[b])
        elif arg_code is not None:
            assert status[b] == arg_code, (case_id(c), b, role, status[b])
        elif role == "overflow":
            assert status[b] == Status.OVERFLOW
        elif role == "revert":
            assert status[b] == (Status.OK if c.legacy else INTENDED[kind]), (case_id(c), b, kind, status[b])
        else:
            assert status[b] == Status.OK, (case_id(c), b, role, status[b])
        if arg_code is not None or r is None:
            continue
        if role == "tie":
            tied, k = tie_rows(N, c.bf)
            q = r.qr[tied[0]]
            assert all(r.qr[i] == q for i in tied)
            below = sum(1 for x in r.qr if x < q)
            assert sum(1 for x in r.qr if x == q) == len(tied) and R - below == len(tied) - k and 1 <= k < len(tied)
            assert [r.reliable[i] for i in tied] == [False] * k + [True] * (len(tied) - k), case_id(c)
        if at is not None:
            row, col = at
            assert r.reliable[row], case_id(c)
            rel_col = [int(m["values"][b, i, col]) for i in range(N) if r.reliable[i]]
            mean = ref.average(rel_col)
            z = ref.wdiv(int(m["values"][b, row, col]) - mean, ref.wsqrt(ref.variance(rel_col, mean)))
            if R >= 64 and not c.legacy:      # z^2 >= 2^25 wsad: the column kernel's int64 z-power forms
                assert ref.wmul(z, z) >= (1 << 25), (case_id(c), z)
        if role == "dups" and D >= 3 and not c.legacy:
            s = sorted(int(x) for x in m["values"][b, :, 1])
            assert (s[N // 2 - 1] + s[N // 2]) % 2 == 1
            s = sorted(int(x) for x in m["values"][b, :, 0])
            assert s[N // 2 - 1] == s[N // 2] and len(set(s)) == 3


def compare(out, exp, rows=None, keys=OUTS):
    """Every output of `out` equals the model's on the instances `rows` (all by default); returns the mismatches."""
    bad = []
    for k in keys:
        got, want = out[k], exp[k]
        for b in (range(want.shape[0]) if rows is None else rows):
            if not torch.equal(got[b].to(want.dtype), want[b]):
                bad.append((k, b))
    return bad


def sharded_round(m, cut, launch):
    """The round as two unequal column shards: mode 1 on each, the qr partials summed in int64, mode 2 with the
    global D on each.  Instances the model commits: the concatenation is the model's whole round.  Instances it
    reverts: some shard reports the model's code, every other shard that code or OK (a shard cannot see another's
    columns), and a reverting shard leaves its outputs alone."""
    v, exp = m["values"], m["exp"]
    B, N, D = v.shape
    parts = [v[:, :, :cut].contiguous(), v[:, :, cut:].contiguous()]
    assert parts[0].shape[2] != parts[1].shape[2]
    first = [launch(dict(m, values=s), mode=1, rel_dim=D) for s in parts]
    ok = [b for b in range(B) if int(exp["status"][b]) == 0]
    assert ok and len(ok) < B
    for h in first:
        assert (h["status"] == 0).all()
        for k in ("consensus", "skew", "kurt", "rel", "reliable"):
            assert (h[k] == PATTERN[k]).all(), k
    assert torch.equal(torch.cat([h["c1"] for h in first], 1)[ok], exp["c1"][ok])
    qr = first[0]["qr"] + first[1]["qr"]
    assert torch.equal(qr[ok], exp["qr"][ok])
    second = [launch(dict(m, values=s), mode=2, rel_dim=D, inp={"c1": h["c1"], "qr": qr, "status": h["status"]})
              for s, h in zip(parts, first)]
    for k in ("c1", "consensus", "skew", "kurt"):
        assert torch.equal(torch.cat([h[k] for h in second], 1)[ok], exp[k][ok]), k
    for h in second:
        for k in ("rel", "qr", "reliable", "status"):
            assert torch.equal(h[k][ok].to(exp[k].dtype), exp[k][ok]), k
    for b in set(range(B)) - set(ok):
        codes = [int(h["status"][b]) for h in second]
        assert int(exp["status"][b]) in codes and set(codes) <= {0, int(exp["status"][b])}, (b, codes)
        for h in second:
            if int(h["status"][b]) != 0:
                for k in ("consensus", "skew", "kurt", "rel", "reliable"):
                    assert (h[k][b] == PATTERN[k]).all(), (b, k)
    return first, second


SHARDED = [(Case("wide", 100, 24, 10, 10, False, "int64", None), 9),
           (Case("con", 600, 8, 64, 64, False, "int64", None), 3)]
