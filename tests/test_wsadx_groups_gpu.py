"""Exact unconstrained rounds over wide columns with 64 < N <= 256 oracles: the lane-group form of the int64
wide-column kernel (csrc/kernels/consensus_wsadx.hip; NSEG = 2 lanes per column for N <= 128, 4 for N <= 256).

Every case compares three results bit for bit on all eight outputs -- the new path, the i128 kernel
(SVOC_EXACT_I128=1) and the CPU engine -- and asserts the routing counters (stats[0]: rounds the wide-column kernel
committed, stats[1]: rounds left to the i128 kernel).  A test about a branch first asserts, from the CPU result or
the input, that the input reaches it.
"""
import pytest
import torch

from svoc import ops as svops
from wsadx_cases import DEV, DIV_BY_ZERO, MS, OUTS, PATTERN, UNIT, _column_z, _honest, _prices, _run, _tdiv

pytestmark = pytest.mark.gpu


def _check(v, f, expect, ms=MS, storage=torch.int64, active=None, prefill=False):
    """The three results, bit for bit; `expect` = [wide-column rounds, i128 rounds] of the new path.  Returns
    (new path, CPU engine)."""
    cpu = _run(v, f, ms=ms, active=active, prefill=prefill)
    i128 = _run(v.to(DEV, storage), f, {"SVOC_EXACT_I128": "1"}, ms=ms, active=active, prefill=prefill)
    got = _run(v.to(DEV, storage), f, {"SVOC_EXACT_WSAD_MIN_D": "1"}, ms=ms, active=active, prefill=prefill)
    for k in OUTS:
        assert torch.equal(got[k], cpu[k]), k
        assert torch.equal(i128[k], cpu[k]), k
    assert got["stats"] == list(expect), got["stats"]
    assert i128["stats"] == [0, 0], i128["stats"]       # (the forced i128 run has no column kernel to count)
    return got, cpu


# ---------------------------------------------------------------------------------------------------------------
# 1. price columns
@pytest.mark.parametrize("N,D,f", [(65, 70, 8), (128, 96, 16), (129, 70, 16), (200, 130, 25), (256, 64, 32),
                                   (256, 300, 32)])
def test_price_columns_bit_exact(N, D, f):
    """60,000 +- 20,000 real units: one real row in the second lane (65), a full NSEG = 2 group (128), the first
    NSEG = 4 shape (129), a masked NSEG = 4 group (200), full groups (256), several slabs with a partial one
    (D = 300).  The wide-column kernel commits every round (before this kernel: stats[0] == 0)."""
    B = 8
    v = _prices(B, N, D, f, seed=N * 7 + D)
    assert ((v - v[:, :1]).abs().amax((1, 2)) >= (1 << 30)).all()
    got, _ = _check(v, f, [B, 0])
    assert (got["status"] == 0).all()


# 2. int32 storage
@pytest.mark.parametrize("N", [128, 256])
def test_int32_storage_over_the_whole_range(N):
    B, D, f = 6, 80, N // 8
    v = _prices(B, N, D, f, seed=3 + N, centre=0.0, spread=2000.0).clamp(-(2 ** 31), 2 ** 31 - 1)
    assert v.min() < -1_990_000_000 and v.max() > 1_990_000_000     # (+-2,000 units: 93% of the int32 range)
    got, _ = _check(v, f, [B, 0], storage=torch.int32)
    assert (got["status"] == 0).all()


# 3. domain boundaries
@pytest.mark.parametrize("row", [5, 70, 135, 255])
def test_domain_boundaries(row):
    """The special value in one row of each lane of the group: just inside 2^30 (column kernel), at 2^30 and just
    inside 2^37 (this kernel), at 2^37 and at 2^62 (i128), bases near 2^52, a constant wide column (DIV_BY_ZERO
    through the i128 kernel)."""
    B, N, D, f = 8, 256, 64, 32
    v = _prices(B, N, D, f, seed=11 + row, centre=1000.0, spread=100.0)
    v[0, row, 3] = v[0, 0, 3] + (1 << 30) - 1           # column kernel: just inside 2^30
    v[1, row, 3] = v[1, 0, 3] + (1 << 30)               # wide-column kernel: at 2^30
    v[2, row, 7] = v[2, 0, 7] - (1 << 37) + 1           # wide-column: just inside 2^37
    v[3, row, 7] = v[3, 0, 7] + (1 << 37)               # i128: at 2^37
    v[4, :, 2] += (1 << 62) - (1 << 33)                 # i128: a column next to 2^62 with one value at 2^62
    v[4, row, 2] = (1 << 62)
    v[5] += (1 << 52)                                   # bases near 2^52
    v[5, row, 1] = v[5, 0, 1] + (1 << 31)
    v[6, :, 4] = -(1 << 40)                             # a constant wide column: variance 0 -> DIV_BY_ZERO (i128)
    v[6, row, 4] = -(1 << 40) + (1 << 31)
    assert ((v[[0, 7]] - v[[0, 7], :1]).abs().amax((1, 2)) < (1 << 30)).all()
    got, cpu = _check(v, f, [3, 3])                     # 1, 2, 5 wide; 3, 4 out of the domain; 6 reverts; 0, 7 narrow
    assert cpu["status"][:6].eq(0).all() and cpu["status"][7].item() == 0
    assert cpu["status"][6].item() == DIV_BY_ZERO


# 4. a far outlier on a masked row
@pytest.mark.parametrize("N,D,f", [(65, 70, 8), (200, 70, 25), (256, 70, 32)])
def test_far_outlier_on_a_masked_row(N, D, f):
    """One oracle 2^37 - 1 wsad off in one column, either side, in row 0, a middle row or the last row: the row is
    not reliable and its z-score is around 10^13, which the z division must never see.  With N = 65 and the outlier
    in row 0 the padding rows of the second lane re-read it too."""
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
    got, cpu = _check(v, f, [B, 0])
    assert cpu["status"].eq(0).all()
    for b, (row, col) in enumerate(where):
        assert int(cpu["reliable"][b, row]) == 0
        _, sd, _ = _column_z(v, cpu, b, col)
        d = abs(int(v[b, row, col]) - int(cpu["consensus"][b, col]))
        assert d * UNIT // sd > (1 << 40), (b, d, sd)             # far past wdiv_z's |z| < 2^31


# 5. large reliable z
def test_large_reliable_z():
    """N = 256, f = 0.  Column `ca`: one row 1,100 units out, z near sqrt(255) 1e6 -- z^2 z passes 2^51 (the int64
    z^3).  Column `cb`: every row equal but one 27,600 wsad out: the variance is exactly 2 (sd = 1414, the
    smallest committed) and z = 1.94e7, so the kurtosis dividend s4 n (n + 1) passes 2^53.  (At 25,300 wsad the
    variance is 2 as well but the dividend is 6.6e15, short of 2^53 = 9.0e15; 27,305 .. 27,800 passes it.)"""
    B, N, D, f = 4, 256, 64, 0
    v = _honest(B, N, D, seed=200)
    where = [((b * 67 + 1) % N, (b * 17 + 2) % D, (b * 17 + 9) % D, (b * 89 + 70) % N) for b in range(B)]
    for b, (ra, ca, cb, rb) in enumerate(where):
        v[b, ra, ca] += 1100 * UNIT
        v[b, :, cb] = 1000 * UNIT
        v[b, rb, cb] += 27_600 * (1 if b % 2 else -1)
    got, cpu = _check(v, f, [B, 0])
    assert cpu["status"].eq(0).all() and cpu["reliable"].eq(1).all()
    for b, (ra, ca, cb, rb) in enumerate(where):
        _, _, z = _column_z(v, cpu, b, ca)
        za = abs(z[ra])
        assert za > 15_000_000 and (za * za + 500000) // UNIT * za >= (1 << 51), (b, za)
        var, sd, z = _column_z(v, cpu, b, cb)
        assert var == 2 and sd == 1414
        s4 = sum(((x * x + 500000) // UNIT) ** 2 // UNIT for x in z)      # (a lower bound: each term floored)
        assert s4 * N * (N + 1) > (1 << 53), (b, s4)


# 6. qr hand-offs
@pytest.mark.parametrize("D,lo,hi,wide", [(192, 0, 1 << 62, True), (256, 1 << 62, 1 << 63, False),
                                          (1024, 1 << 64, 1 << 65, False)],
                         ids=["D192-below-2^62", "D256-past-2^62", "D1024-past-2^64"])
def test_qr_sum_hand_offs(D, lo, hi, wide):
    """One row of the second lane 2^37 - 1 wsad above row 0 in every column: its qr sum stays below 2^62 at
    D = 192 (committed), reaches 2^62 at D = 256 and carries out of uint64 at D = 1024 (both handed off)."""
    B, N, f = 2, 128, 16
    v = _honest(B, N, D, seed=300 + D)
    rows = (100, 127)
    for b in range(B):
        v[b, rows[b], :] = v[b, 0, :] + (1 << 37) - 1
    got, cpu = _check(v, f, [B, 0] if wide else [0, B])
    for b in range(B):
        qr = sum(((int(x) - int(c)) ** 2 + 500000) // UNIT for x, c in zip(v[b, rows[b]], cpu["c1"][b]))
        assert lo <= qr < hi, (qr / 2 ** 62, D)
        trunc = (qr + (1 << 63)) % (1 << 64) - (1 << 63)
        assert int(cpu["qr"][b, rows[b]]) == trunc


def test_many_qr_sums_past_2_62_hand_off():
    """Half the rows 2^37 - 1 below row 0 and half above it in every column: the low rows' qr sums reach 2^62
    together (their mean stays below it), the instance is flagged before the reliabilities are computed and the
    i128 kernel takes it."""
    B, N, D, f = 2, 128, 128, 16
    v = _honest(B, N, D, seed=350)
    v[:, 1::2, :] = v[:, :1, :] + (1 << 37) - 1
    v[:, 2::2, :] = v[:, :1, :] - (1 << 37) + 1
    got, cpu = _check(v, f, [0, B])
    for b in range(B):
        qr = [sum(((int(x) - int(c)) ** 2 + 500000) // UNIT for x, c in zip(v[b, r], cpu["c1"][b])) for r in (2, 4, 126)]
        assert all((1 << 62) <= q < (1 << 63) for q in qr), [q / 2 ** 62 for q in qr]


# 7. ties at the rank cut across lanes
def test_qr_ties_at_the_rank_cut_across_lanes():
    """Three identical far rows with f = 2, in three lanes of the group and around a lane boundary: equal qr across
    the cut; the order is (qr ascending, index descending), so only the highest index stays reliable."""
    N, D, f = 256, 64, 2
    trios = [(10, 100, 250), (63, 64, 65), (0, 128, 255), (191, 192, 193)]
    B = len(trios)
    v = _honest(B, N, D, seed=600)
    for b, t in enumerate(trios):
        v[b, list(t), :] = v[b, t[0], :] + 30_000 * UNIT
    got, cpu = _check(v, f, [B, 0])
    assert cpu["status"].eq(0).all()
    for b, t in enumerate(trios):
        assert len({int(cpu["qr"][b, r]) for r in t}) == 1
        assert [int(cpu["reliable"][b, r]) for r in t] == [0, 0, 1]
        assert int(cpu["reliable"][b].sum()) == N - f


# 8. medians
@pytest.mark.parametrize("N,f", [(129, 16), (200, 25)])
def test_medians_truncating_and_tied(N, f):
    """Mixed-sign columns around 0 (+-2,000 units: medians and means that truncate toward zero on either side);
    columns whose two middle values sit in different lanes of the group; columns with more than N / 2 identical
    values."""
    B, D = 6, 70
    v = _prices(B, N, D, f, seed=500 + N, centre=0.0, spread=2000.0)
    g = torch.Generator().manual_seed(N)
    split, tied = [], []
    for b in range(B):
        # the two middle values in rows of different lanes: rows (3, 64 + 5) and, where they exist, (130, 70)
        for c, (ra, rb) in ((5 + b, (3, 69)), (40 + b, (N - 1, 70) if N <= 192 else (130, 199))):
            s = v[b, :, c].sort().values
            rows = [r for r in torch.randperm(N, generator=g).tolist() if r not in (ra, rb)]
            rows[N // 2 - 1:N // 2 - 1] = [ra, rb]          # rank N/2 - 1 -> row ra, rank N/2 -> row rb
            v[b, rows, c] = s
            assert ra // 64 != rb // 64
            split.append((b, c, int(s[N // 2 - 1]), int(s[N // 2])))
        # N / 2 + 3 identical values in random rows (of every lane)
        c = 20 + b
        val = int(v[b, 0, c]) if b % 2 else -777_777_777
        v[b, torch.randperm(N, generator=g)[:N // 2 + 3], c] = val
        tied.append((b, c, val))
    got, cpu = _check(v, f, [B, 0])
    assert cpu["status"].eq(0).all()
    assert ((v - v[:, :1]).abs().amax((1, 2)) > (1 << 30)).all()
    assert (cpu["consensus"] < 0).any() and (cpu["consensus"] > 0).any()
    assert (cpu["c1"] < 0).any() and (cpu["c1"] > 0).any()
    # an odd sum of the middle pair on either side of zero: the truncation toward zero is exercised
    mids = v.sort(1).values[:, N // 2 - 1:N // 2 + 1].sum(1)
    odd = mids[mids % 2 != 0]
    assert (odd < 0).any() and (odd > 0).any()
    for b, c, lo, hi in split:
        assert int(cpu["c1"][b, c]) == _tdiv(lo + hi, 2)
    for b, c, val in tied:
        assert int(cpu["c1"][b, c]) == val


# 9. a mixed batch with an active mask
def test_mixed_batch_with_active_mask():
    """Narrow instances (column kernel), wide ones (this kernel), one out of the domain and one zero-variance revert
    (i128 kernel), one inactive: the outputs of the reverted and the inactive instances keep a pre-filled pattern,
    and the counters equal the per-instance expectation."""
    B, N, D, f = 8, 256, 96, 32
    v = _prices(B, N, D, f, seed=900, centre=1000.0, spread=100.0)          # narrow: 0, 6
    for b in (1, 4, 5, 7):
        v[b] = _prices(1, N, D, f, seed=901 + b)[0]                         # wide: 1, 5, 7 (4: inactive)
    v[2, 200, 11] = v[2, 0, 11] + (1 << 37) + 5                             # out of the domain
    v[3, :, 50] = 7 * UNIT                                                  # a wide zero-variance column
    v[3, 131, 50] = 7 * UNIT + (1 << 32)
    active = torch.tensor([1, 1, 1, 1, 0, 1, 1, 1], dtype=torch.uint8)
    got, cpu = _check(v, f, [3, 2], active=active, prefill=True)
    assert cpu["status"].tolist() == [0, 0, 0, DIV_BY_ZERO, -1, 0, 0, 0]
    for k in OUTS:
        assert (got[k][4] == PATTERN[k]).all(), k                            # inactive: nothing written
    for k in ("c1", "consensus", "skew", "kurt"):
        assert (got[k][3] == PATTERN[k]).all(), k                            # reverted: no output of the round
    for b in (0, 1, 2, 5, 6, 7):
        for k in ("c1", "consensus", "skew", "kurt", "qr"):
            assert not (got[k][b] == PATTERN[k]).any(), (k, b)


# 10. the gate
def test_gate_above_256_and_at_64():
    """N = 300 wide price columns still go to the i128 kernel; N = 64 still to the one-lane wide-column kernel."""
    B = 4
    got, _ = _check(_prices(B, 300, 70, 37, seed=1000), 37, [0, B])
    assert (got["status"] == 0).all()
    got, _ = _check(_prices(B, 64, 70, 8, seed=1001), 8, [B, 0])
    assert (got["status"] == 0).all()


# 11. the engine
def test_engine_routing_and_updates():
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    B, N, D, f = 4, 256, 128, 32
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=False,
                          unconstrained_max_spread=1e6)
    v = _prices(B, N, D, f, seed=5)
    e = ConsensusEngine(cfg, B, device=DEV, mode="exact")
    e.values.copy_(v.to(DEV))
    e.enabled.fill_(1); e.n_active.fill_(N); e.touched.fill_(1)
    e.run_round()
    assert e.exact_routing() == {"processed": B, "wide_column": B, "i128": 0}, e.exact_routing()
    assert (e.status == 0).all()

    # a second engine fed update by update, and its CPU twin: the same statuses, previews included
    inst = torch.arange(B).repeat_interleave(N)
    orc = torch.arange(N).repeat(B)
    vals = v.reshape(B * N, D)
    more_i = torch.arange(B)
    more_o = torch.tensor([3, 70, 135, 255])
    more_v = v[more_i, more_o].clone()
    more_v[1] += 10_000 * UNIT                          # still inside 2^37 of the column bases
    more_v[2, :] = v[2, 0, :] + (1 << 38)               # out of the wide-column domain: the i128 kernel judges it
    res = {}
    for dev in ("cpu", DEV):
        g = ConsensusEngine(cfg, B, device=dev, mode="exact")
        st = g.apply_updates(inst, orc, vals.to(dev))
        g.run_round()
        before = g.exact_routing()
        pv = g.preview_updates(more_i, more_o, more_v.to(dev))
        sp = g.step(more_i, more_o, more_v.to(dev))              # the exact stream: one transaction per update
        res[dev] = (st.cpu().tolist(), pv.cpu().tolist(), sp.cpu().tolist(), g.status.cpu().tolist(),
                    g.consensus.cpu(), g.kurt.cpu(), before, g.exact_routing())
    assert res["cpu"][:4] == res[DEV][:4]
    assert res[DEV][1] == res[DEV][2]                            # the preview names the step's statuses
    assert torch.equal(res["cpu"][4], res[DEV][4]) and torch.equal(res["cpu"][5], res[DEV][5])
    before, after = res[DEV][6], res[DEV][7]
    assert before == {"processed": B, "wide_column": B, "i128": 0}, before
    # the stream's rounds went through the same dispatch: three wide instances more, the out-of-domain one on i128
    assert after["wide_column"] >= before["wide_column"] + 3 and after["i128"] >= 1, after

    # the verdict op (what a preview's wave runs) over the wide values: routed to the wide-column kernel as well
    rel = torch.full((B, 2), -7, dtype=torch.int64, device=DEV)
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    xs = torch.zeros(2, dtype=torch.int32, device=DEV)
    svops.ops().exact_verdict(v.to(DEV), None, f, False, MS, rel, status, False, xs, None)
    assert xs.tolist() == [B, 0] and status.tolist() == [0] * B
    assert torch.equal(rel, e.rel)
