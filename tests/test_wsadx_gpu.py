"""Exact unconstrained rounds over wide columns (csrc/kernels/consensus_wsadx.hip; VERDICT r5 missing item 1).

Columns whose values spread more than 2^30 wsad around their row-0 value used to leave the column kernel for the
i128 kernel (~100x slower).  The int64 wide-column kernel now takes them up to |x - B| < 2^37 (and |x| < 2^62);
every round it commits must equal the i128 kernel and the CPU golden engine bit for bit (contract.cairo:370-434,
signed_decimal.cairo:52-116, math.cairo:113-398), and every round it cannot take (out of its domain, or a revert)
must still come out right through the i128 kernel.  The routing counters (engine.exact_routing) say which kernel
ran.
"""
import pytest
import torch

from wsadx_cases import DEV, DIV_BY_ZERO, MS, OUTS, UNIT, _honest, _prices, _run

pytestmark = pytest.mark.gpu


def _check(v, f, expect_wide, ms=MS):
    cpu = _run(v, f, ms=ms)
    i128 = _run(v.to(DEV), f, {"SVOC_EXACT_I128": "1"}, ms=ms)
    got = _run(v.to(DEV), f, {"SVOC_EXACT_WSAD_MIN_D": "1"}, ms=ms)
    for k in OUTS:
        assert torch.equal(got[k], cpu[k]), k
        assert torch.equal(i128[k], cpu[k]), k
    assert got["stats"][0] == expect_wide, got["stats"]
    return got


@pytest.mark.parametrize("N,D,f", [(64, 96, 8), (64, 300, 20), (33, 70, 5), (16, 64, 3), (7, 70, 2)])
def test_wide_price_columns_bit_exact(N, D, f):
    """60,000 +- 20,000 real units (values ~2^35 wsad apart): the wide-column kernel commits every round."""
    B = 8
    v = _prices(B, N, D, f, seed=N * 7 + D)
    got = _check(v, f, expect_wide=B if N >= 4 else 0)
    assert got["stats"][1] == 0 and (got["status"] == 0).all()


def test_wide_int32_storage_spanning_2_31():
    """int32 storage over the whole int32 range (columns spread past 2^30 around their base)."""
    B, N, D, f = 6, 64, 80, 8
    v = _prices(B, N, D, f, seed=3, centre=0.0, spread=2000.0).clamp(-(2 ** 31), 2 ** 31 - 1)
    cpu = _run(v, f)
    got = _run(v.to(DEV, torch.int32), f, {"SVOC_EXACT_WSAD_MIN_D": "1"})
    for k in OUTS:
        assert torch.equal(got[k], cpu[k]), k
    assert got["stats"] == [B, 0]


def test_wide_domain_boundaries():
    """Instances at the kernels' boundaries: spread just below 2^30 (column kernel), 2^30 .. 2^37 (wide-column
    kernel), past 2^37 from the base and |x| >= 2^62 (i128 kernel) -- every one equal to the CPU engine."""
    B, N, D, f = 8, 64, 64, 8
    base = _prices(B, N, D, f, seed=11, centre=1000.0, spread=100.0)
    v = base.clone()
    v[0, 5, 3] = v[0, 0, 3] + (1 << 30) - 1             # column kernel: just inside 2^30
    v[1, 5, 3] = v[1, 0, 3] + (1 << 30)                 # wide-column kernel: just past 2^30
    v[2, 9, 7] = v[2, 0, 7] - (1 << 37) + 1             # wide-column: just inside 2^37
    v[3, 9, 7] = v[3, 0, 7] + (1 << 37)                 # i128: at 2^37
    v[4, :, 2] += (1 << 62) - (1 << 33)                 # i128: a column at |x| >= 2^62 - 2^33 ... (below)
    v[4, 0, 2] = (1 << 62)                              #   ... with one value at 2^62
    v[5] += (1 << 52)                                   # wide bases (|B| ~ 2^52): column kernel's limit, wide takes it
    v[5, 3, 1] = v[5, 0, 1] + (1 << 31)
    v[6, :, 4] = -(1 << 40)                             # a constant wide column: variance 0 -> DIV_BY_ZERO (i128)
    v[6, 1, 4] = -(1 << 40) + (1 << 31)
    v[6, 2:, 4] = -(1 << 40)
    cpu = _run(v, f)
    got = _run(v.to(DEV), f, {"SVOC_EXACT_WSAD_MIN_D": "1"})
    for k in OUTS:
        assert torch.equal(got[k], cpu[k]), k
    assert cpu["status"][:6].eq(0).all() and cpu["status"][7].item() == 0
    # wide-column rounds: instances 1, 2, 5 (and 6 is a wide revert, left to the i128 kernel)
    assert got["stats"][0] == 3, got["stats"]
    assert got["stats"][1] >= 3, got["stats"]          # 3, 4 out of domain; 6 reverts


def test_wide_reverts_match_cpu():
    """Wide rounds the contract reverts (R < 4: the kurtosis divides by zero; max_spread 0: the reliability
    divides by zero) are left to the i128 kernel, which reports the contract's status; a max_spread below the
    qr's root clamps both reliabilities to 0 -- a valid round the wide-column kernel commits."""
    B, N, D, f = 4, 64, 64, 8
    v = _prices(B, N, D, f, seed=21)
    got = _check(v, f, expect_wide=B, ms=10 ** 9)       # 1,000 units: rel1 = rel2 = 0 (min(ms, sd) = ms)
    assert got["rel"].eq(0).all() and got["status"].eq(0).all()
    got = _check(v, 61, expect_wide=0)                  # R = 3
    assert got["status"].ne(0).all()
    got = _check(v, f, expect_wide=0, ms=0)             # wsad_div by max_spread = 0
    assert got["status"].ne(0).all()


def test_engine_reports_routing():
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    B, N, D, f = 4, 64, 128, 8
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=False,
                          unconstrained_max_spread=1e6)
    e = ConsensusEngine(cfg, B, device=DEV, mode="exact")
    e.values.copy_(_prices(B, N, D, f, seed=5).to(DEV))
    e.enabled.fill_(1); e.n_active.fill_(N); e.touched.fill_(1)
    e.run_round()
    r = e.exact_routing()
    assert r == {"processed": B, "wide_column": B, "i128": 0}, r
    assert (e.status == 0).all()


# ---------------------------------------------------------------------------------------------------------
# Edges of the wide-column kernel's arithmetic (csrc/include/svoc/wsad_wide.hpp): inputs the Beta(20,20) price
# data never produces.  Every test asserts, from the CPU engine's result, the condition that makes it reach the
# branch it is about, then compares the wide-column kernel, the i128 kernel and the CPU engine bit for bit.
# ---------------------------------------------------------------------------------------------------------
def _column_z(v, cpu, b, c):
    """(exact |x - mean| per row, an upper bound of the reliable rows' sd) of column c of instance b, in wsad:
    the variance is floor(mean of floor((d^2 + 500000) / 1e6)) <= mean(d^2) / 1e6 + 1 and the contract's Newton
    sqrt ends within 1 of sqrt(variance 1e6)."""
    import math
    mean = int(cpu["consensus"][b, c])
    rel = [int(r) for r in cpu["reliable"][b]]
    d = [abs(int(x) - mean) for x in v[b, :, c]]
    dr = [x for x, r in zip(d, rel) if r]
    var = sum((x * x + 500000) // UNIT for x in dr) // len(dr)
    return d, var, math.isqrt((var + 1) * UNIT) + 2


@pytest.mark.parametrize("N,D,f", [(64, 70, 8), (33, 70, 5), (7, 64, 2)])
def test_far_outlier_on_a_masked_row(N, D, f):
    """One oracle 137,000 units off in one column, either side, in row 0, a middle row or the last row: the row
    is not reliable and its z-score is far past 2^31 (around 10^13), which the kernel's z division must never
    see -- it divides the reliable rows only.  With N < 64 and the outlier in row 0 the padding rows carry it too."""
    B = 8
    v = _honest(B, N, D, seed=100 + N)
    where = []
    for b in range(B):
        row = (0, N // 2, N - 1)[b % 3]
        col = (b * 11 + 3) % D
        sign = 1 if b % 2 == 0 else -1
        if row == 0:
            v[b, 0, col] += sign * ((1 << 37) - (1 << 20))      # (every |x - B| stays below 2^37)
        else:
            v[b, row, col] = v[b, 0, col] + sign * ((1 << 37) - 1)
        where.append((row, col))
    assert {(r == 0, b % 2) for b, (r, _) in enumerate(where)} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    got = _check(v, f, expect_wide=B)
    cpu = _run(v, f)
    assert cpu["status"].eq(0).all()
    for b, (row, col) in enumerate(where):
        assert int(cpu["reliable"][b, row]) == 0
        d, _, sd_up = _column_z(v, cpu, b, col)
        assert d[row] * UNIT // sd_up > (1 << 31), (b, d[row], sd_up)
    assert got["stats"] == [B, 0]


@pytest.mark.parametrize("f,off", [(8, 1000), (0, 1100)])
def test_large_reliable_z(f, off):
    """A reliable row with |z| > 5.8 (z^2 >= 2^25 wsad): the int64 branch of the z^4 step.  f = 8: the failing
    rows sit 30,000 units out in every column and one honest row 1000 units out in one column (z = sqrt(55) =
    7.416); f = 0: one row 1100 units out (past the column kernel's 2^30), z near sqrt(63)."""
    B, N, D = 4, 64, 64
    v = _honest(B, N, D, seed=200 + f)
    if f:
        v[:, N - f:, :] += 30_000 * UNIT
    where = [((b * 13 + 1) % (N - f), (b * 17 + 2) % D) for b in range(B)]
    for b, (row, col) in enumerate(where):
        v[b, row, col] += off * UNIT
    got = _check(v, f, expect_wide=B)
    cpu = _run(v, f)
    assert cpu["status"].eq(0).all()
    for b, (row, col) in enumerate(where):
        assert int(cpu["reliable"][b, row]) == 1
        d, _, sd_up = _column_z(v, cpu, b, col)
        z = d[row] * UNIT // sd_up                              # (a lower bound of |z| in wsad)
        assert z > 5_800_000 and z * z // UNIT >= (1 << 25), (b, z)
    assert got["stats"] == [B, 0]


@pytest.mark.parametrize("D,lo,hi,wide", [(192, 0, 1 << 62, True), (256, 1 << 62, 1 << 63, False),
                                          (1024, 1 << 64, 1 << 65, False)],
                         ids=["D192-below-2^62", "D256-past-2^62", "D1024-past-2^64"])
def test_qr_sum_hand_offs(D, lo, hi, wide):
    """One row 2^37 - 1 wsad above row 0 in every column: its qr sum stays below 2^62 at D = 192 (the wide-column
    kernel commits), reaches 2^62 at D = 256 and carries out of uint64 at D = 1024 (both handed to the i128
    kernel).  The int64 qr output is the i128 sum truncated, in the CPU engine and the i128 kernel alike."""
    B, N, f = 2, 8, 2
    v = _honest(B, N, D, seed=300 + D)
    rows = (3, 7)
    for b in range(B):
        v[b, rows[b], :] = v[b, 0, :] + (1 << 37) - 1
    got = _check(v, f, expect_wide=B if wide else 0)
    cpu = _run(v, f)
    for b in range(B):
        qr = sum(((int(x) - int(c)) ** 2 + 500000) // UNIT for x, c in zip(v[b, rows[b]], cpu["c1"][b]))
        assert lo <= qr < hi, (qr / 2 ** 62, D)
        trunc = (qr + (1 << 63)) % (1 << 64) - (1 << 63)
        assert int(cpu["qr"][b, rows[b]]) == trunc
    assert got["stats"] == ([B, 0] if wide else [0, B])


def test_many_qr_sums_past_2_62_hand_off():
    """N = 64: rows 0 and 1 equal, half of the others 2^37 - 1 above row 0 and half below it in all 640 columns.
    c1 is row 0, each far row's qr sum is 2^63.39 (no carry out of uint64) and the mean of the 64 sums 2^63.35 --
    negative as int64, outside the Newton sqrt's domain: the instance is flagged before the reliabilities are
    computed and the i128 kernel takes it."""
    B, N, D, f = 2, 64, 640, 8
    v = _honest(B, N, D, seed=350)
    v[:, 1, :] = v[:, 0, :]
    v[:, 2::2, :] = v[:, :1, :] + (1 << 37) - 1
    v[:, 3::2, :] = v[:, :1, :] - (1 << 37) + 1
    cpu = _run(v, f)
    for b in range(B):
        assert torch.equal(cpu["c1"][b], v[b, 0])
        qr = [sum(((int(x) - int(c)) ** 2 + 500000) // UNIT for x, c in zip(v[b, r], cpu["c1"][b])) for r in range(N)]
        assert all((1 << 62) <= q < (1 << 64) for q in qr[2:]), [q / 2 ** 62 for q in qr[2:]]
        assert (1 << 63) <= sum(qr) // N < (1 << 64), sum(qr) / N / 2 ** 63
    got = _check(v, f, expect_wide=0)
    assert got["stats"] == [0, B]


@pytest.mark.parametrize("amp,var", [(1000, 1), (1500, 2)])
def test_variance_one_and_two(amp, var):
    """A column of a wide instance whose reliable rows alternate +-amp wsad around 1e9: amp = 1000 gives variance
    1, whose sqrt divides by zero in the contract (the round reverts: left to the i128 kernel, status
    DIV_BY_ZERO); amp = 1500 gives variance 2, the smallest the wide-column kernel commits (sd = 1414)."""
    B, N, D, f = 2, 16, 64, 2
    v = _honest(B, N, D, seed=400 + amp)
    v[:, N - f:, :] += 30_000 * UNIT                            # the two failing rows: a wide instance
    cols = (5, 40)
    alt = torch.tensor([amp if i % 2 == 0 else -amp for i in range(N)], dtype=torch.int64)
    for b in range(B):
        v[b, :, cols[b]] = 10 ** 9 + alt
    got = _check(v, f, expect_wide=B if var == 2 else 0)
    cpu = _run(v, f)
    assert (amp * amp + 500000) // UNIT == var                  # each reliable row's qdev, hence their mean
    # a reverted round leaves no outputs to read: the rows and the mean are read from the same instances with the
    # column at +-1500 (the variance-2 case itself), which differ from the variance-1 ones in that column only
    v2 = v.clone()
    for b in range(B):
        v2[b, :, cols[b]] = 10 ** 9 + alt // amp * 1500
    ok = _run(v2, f)
    assert ok["status"].eq(0).all()
    for b in range(B):
        assert ok["reliable"][b].tolist() == [1] * (N - f) + [0] * f
        assert int(ok["consensus"][b, cols[b]]) == 10 ** 9
        assert _column_z(v2, ok, b, cols[b])[1] == 2
    if var == 1:
        assert cpu["status"].eq(DIV_BY_ZERO).all() and got["stats"] == [0, B]
    else:
        assert cpu["status"].eq(0).all() and got["stats"] == [B, 0]


@pytest.mark.parametrize("N,D,f,storage", [(33, 70, 5, torch.int64), (7, 70, 2, torch.int64), (33, 70, 5, torch.int32)],
                         ids=["N33-int64", "N7-int64", "N33-int32"])
def test_mixed_sign_columns_below_64_rows(N, D, f, storage):
    """Columns around zero (+-2000 units) with N < 64: means and medians that truncate toward zero on either side
    of the sign change, through the row-masked instantiations in int64 and in int32 storage."""
    B = 8
    v = _prices(B, N, D, f, seed=500 + N, centre=0.0, spread=2000.0)
    if storage == torch.int32:
        v = v.clamp(-(2 ** 31), 2 ** 31 - 1)
    cpu = _run(v, f)
    i128 = _run(v.to(DEV, storage), f, {"SVOC_EXACT_I128": "1"})
    got = _run(v.to(DEV, storage), f, {"SVOC_EXACT_WSAD_MIN_D": "1"})
    for k in OUTS:
        assert torch.equal(got[k], cpu[k]), k
        assert torch.equal(i128[k], cpu[k]), k
    assert cpu["status"].eq(0).all()
    assert ((v - v[:, :1]).abs().amax((1, 2)) > (1 << 30)).all()   # every instance past the column kernel's domain
    assert (cpu["consensus"] < 0).any() and (cpu["consensus"] > 0).any()
    assert (cpu["c1"] < 0).any() and (cpu["c1"] > 0).any()
    assert got["stats"] == [B, 0]


def test_qr_ties_at_the_rank_cut():
    """Three identical far rows with f = 2: equal qr across the cut.  The contract's order is (qr ascending, index
    descending), so the highest index of the three is the one that stays reliable."""
    B, N, D, f = 4, 16, 64, 2
    v = _honest(B, N, D, seed=600)
    trios = [(2, 5, 11), (0, 1, 2), (13, 14, 15), (0, 7, 15)]
    for b, t in enumerate(trios):
        v[b, list(t), :] = v[b, t[0], :] + 30_000 * UNIT
    got = _check(v, f, expect_wide=B)
    cpu = _run(v, f)
    assert cpu["status"].eq(0).all()
    for b, t in enumerate(trios):
        assert len({int(cpu["qr"][b, r]) for r in t}) == 1
        assert [int(cpu["reliable"][b, r]) for r in t] == [0, 0, 1]
        assert int(cpu["reliable"][b].sum()) == N - f
    assert got["stats"] == [B, 0]
