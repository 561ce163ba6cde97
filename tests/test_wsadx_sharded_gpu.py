"""D-sharded exact unconstrained rounds on the int64 wide-column kernel (csrc/kernels/consensus_wsadx.hip, N <= 256):
mode 1 (this shard's c1 and qr partials) and mode 2 (pass 2 from the all-reduced qr).

Every case compares three results bit for bit on all eight outputs -- the default path, the i128 kernel
(SVOC_EXACT_I128=1) and the CPU engine -- over outputs prefilled with a pattern (an unwanted write shows), and asserts
the routing counters of the launch (stats[0]: instances whose half a wide-column kernel took, stats[1]: instances left
to the i128 kernel).  A test about a branch first asserts, from the CPU result or the input, that the input reaches it.
Shapes: the smallest that reach every lane layout (N <= 64, two lanes per column to 128, four to 256; full and masked
groups) and a slab edge (256 / 128 / 64 columns), D split into two unequal contiguous shards.
"""
import os
import tempfile

import pytest
import torch

from wsadx_cases import DEV, DIV_BY_ZERO, OK, OUTS, OVERFLOW, PATTERN, UNIT, _prices, _run

pytestmark = pytest.mark.gpu
# (N, D, f) and where D is cut: the first shard ends one or two columns past a slab edge
SHAPES = [(7, 300, 1), (64, 520, 8), (100, 140, 12), (128, 260, 16), (200, 70, 24), (256, 130, 32)]
CUT = {7: 257, 64: 300, 100: 129, 128: 129, 200: 65, 256: 66}


def _check(v, f, mode, expect, rel_dim=0, inp=None, storage=torch.int64, active=None):
    """The three results, bit for bit; `expect` = [wide-column halves, i128 halves] of the default path.  Returns
    (default path, CPU engine)."""
    kw = dict(mode=mode, rel_dim=rel_dim, inp=inp, prefill=True, active=active)     # (an unwanted write shows)
    cpu = _run(v, f, **kw)
    i128 = _run(v.to(DEV, storage), f, {"SVOC_EXACT_I128": "1"}, **kw)
    got = _run(v.to(DEV, storage), f, {"SVOC_EXACT_WSAD_MIN_D": "1"}, **kw)
    print(f"mode {mode} N {v.shape[1]} D {v.shape[2]} {storage}: stats {got['stats']} (expected {list(expect)}), "
          f"status {cpu['status'].tolist()}")
    for k in OUTS:
        assert torch.equal(i128[k], cpu[k]), (k, "i128")
        assert torch.equal(got[k], cpu[k]), k
    assert got["stats"] == list(expect), got["stats"]
    assert i128["stats"] == [0, 0], i128["stats"]       # (the forced i128 run has no column kernel to count)
    return got, cpu


def _shards(v, cut):
    return [v[:, :, :cut].contiguous(), v[:, :, cut:].contiguous()]


def _mode2_inputs(B, N, D, seed, lo=10 ** 12, hi=2 * 10 ** 12):
    """Inputs of a second half the test makes up: any c1 (the unconstrained pass 2 does not read it), a qr per oracle
    in [lo, hi) (the rank cut follows it, whatever the values are), status OK."""
    g = torch.Generator().manual_seed(seed)
    return {"c1": torch.randint(-10 ** 9, 10 ** 9, (B, D), generator=g, dtype=torch.int64),
            "qr": torch.randint(lo, hi, (B, N), generator=g, dtype=torch.int64),
            "status": torch.zeros(B, dtype=torch.int32)}


def _sharded_round(v, f, cut, storage=torch.int64, expect1=None, expect2=None):
    """Both halves over two column shards, each checked three ways; the partials summed on the host; the
    concatenated result against the CPU engine's whole round."""
    B, N, D = v.shape
    expect1 = [B, 0] if expect1 is None else expect1
    expect2 = [B, 0] if expect2 is None else expect2
    parts = _shards(v, cut)
    assert parts[0].shape[2] != parts[1].shape[2]
    first = [_check(s, f, 1, expect1, D, storage=storage)[0] for s in parts]
    for h in first:
        assert (h["status"] == OK).all()
        for k in ("consensus", "skew", "kurt", "rel", "reliable"):
            assert (h[k] == PATTERN[k]).all(), k              # the first half writes c1, qr and status only
    qr = first[0]["qr"] + first[1]["qr"]
    second = [_check(s, f, 2, expect2, D, {"c1": h["c1"], "qr": qr, "status": h["status"]}, storage=storage)[0]
              for s, h in zip(parts, first)]
    whole = _run(v, f, prefill=True)                          # the CPU engine, unsharded
    assert (whole["status"] == OK).all()
    for k in ("c1", "consensus", "skew", "kurt"):
        assert torch.equal(torch.cat([second[0][k], second[1][k]], 1), whole[k]), k
    for h in second:
        for k in ("rel", "qr", "reliable", "status"):
            assert torch.equal(h[k], whole[k]), k
    return second, whole


# ---------------------------------------------------------------------------------------------------------------
# 1. price columns, both halves
@pytest.mark.parametrize("N,D,f", SHAPES)
def test_price_columns_both_halves(N, D, f):
    """60,000 +- 20,000 real units in int64: every half of every shard runs on a wide-column kernel ([B, 0]; before
    these kernels took the halves: [0, B])."""
    B = 4
    v = _prices(B, N, D, f, seed=N * 7 + D)
    for s in _shards(v, CUT[N]):
        assert ((s - s[:, :1]).abs().amax((1, 2)) >= (1 << 30)).all()
    _sharded_round(v, f, CUT[N])


@pytest.mark.parametrize("N,D,f", [(64, 520, 8), (200, 70, 24)])
def test_int32_storage_spread_past_2_30(N, D, f):
    """int32 storage, every column spread between 2^30 and 2^31 wsad around its row 0.  (The column kernel must
    flag the second half for int32 storage too: it has no pass 1 there to stage the columns' bases, and committing
    without them once put uninitialised words into the consensus.)"""
    B = 3
    v = _prices(B, N, D, f, seed=3 + N, centre=0.0, spread=1000.0)
    for s in _shards(v, CUT[N]):
        m = (s - s[:, :1]).abs().amax((1, 2))
        assert (m >= (1 << 30)).all() and (m < (1 << 31)).all()
    _sharded_round(v, f, CUT[N], storage=torch.int32)


# 2. narrow int64 columns
@pytest.mark.parametrize("N,D,f", [(64, 520, 8), (200, 70, 24)])
def test_narrow_int64_columns(N, D, f):
    """60,000 +- 200 units: inside 2^30, so the column kernel takes the first half itself ([0, 0]); it flags every
    int64 second half (no pass 1 has validated the high words) and the wide-column kernel takes it ([B, 0])."""
    B = 4
    v = _prices(B, N, D, f, seed=40 + N, spread=200.0)
    assert ((v - v[:, :1]).abs().amax((1, 2)) < (1 << 30)).all()
    _sharded_round(v, f, CUT[N], expect1=[0, 0])


# 3. second halves whose inputs the test makes up
def test_mode2_qr_ties_at_the_rank_cut_across_lanes():
    """Three equal, largest qr with f = 2, in three lanes of a group and around a lane boundary: the order is (qr
    ascending, index descending), so only the highest index stays reliable."""
    N, D, f = 256, 70, 2
    trios = [(10, 100, 250), (63, 64, 65), (0, 128, 255), (191, 192, 193)]
    B = len(trios)
    v = _prices(B, N, D, f, seed=600)
    inp = _mode2_inputs(B, N, D, seed=601)
    for b, t in enumerate(trios):
        inp["qr"][b, list(t)] = 3 * 10 ** 12
    got, cpu = _check(v, f, 2, [B, 0], 2 * D, inp)
    assert cpu["status"].eq(OK).all()
    for b, t in enumerate(trios):
        assert [int(cpu["reliable"][b, r]) for r in t] == [0, 0, 1]
        assert int(cpu["reliable"][b].sum()) == N - f


@pytest.mark.parametrize("N,D,f", [(64, 70, 8), (200, 70, 24)])
def test_mode2_qr_at_2_62_hands_off(N, D, f):
    """A global qr of 2^62 - 1 is taken; 2^62, and one that is negative as int64, go to the i128 kernel."""
    B = 3
    v = _prices(B, N, D, f, seed=610 + N)
    inp = _mode2_inputs(B, N, D, seed=611)
    inp["qr"][0, N - 1] = (1 << 62) - 1
    inp["qr"][1, N - 1] = 1 << 62
    inp["qr"][2, N // 2] = -5
    _check(v, f, 2, [1, 2], 2 * D, inp)


def test_mode2_failed_first_half_writes_nothing():
    """status != OK on entry (some shard's first half failed): nothing written, nothing counted."""
    B, N, D, f = 3, 100, 70, 12
    v = _prices(B, N, D, f, seed=620)
    inp = _mode2_inputs(B, N, D, seed=621)
    inp["status"].fill_(OVERFLOW)
    got, _ = _check(v, f, 2, [0, 0], 2 * D, inp)
    for k in ("consensus", "skew", "kurt", "rel", "reliable"):
        assert (got[k] == PATTERN[k]).all(), k
    for k in ("c1", "qr", "status"):
        assert torch.equal(got[k], inp[k]), k
    inp["status"][1] = OK                                   # one instance passed: it alone runs
    got, _ = _check(v, f, 2, [1, 0], 2 * D, inp)
    assert got["status"].tolist() == [OVERFLOW, OK, OVERFLOW]
    assert (got["consensus"][[0, 2]] == PATTERN["consensus"]).all() and (got["consensus"][1] != PATTERN["consensus"]).all()


@pytest.mark.parametrize("mode", [1, 2])
def test_active_mask(mode):
    B, N, D, f = 5, 130, 70, 16
    v = _prices(B, N, D, f, seed=630)
    active = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    got, _ = _check(v, f, mode, [3, 0], 2 * D, _mode2_inputs(B, N, D, seed=631) if mode == 2 else None, active=active)
    for k in OUTS if mode == 1 else ("consensus", "skew", "kurt", "rel", "reliable"):
        assert (got[k][[1, 4]] == PATTERN[k]).all(), k       # inactive: nothing written
    assert got["status"][[0, 2, 3]].eq(OK).all()


# 4. hand-offs: the i128 kernel names the status
@pytest.mark.parametrize("N,f", [(64, 8), (200, 24)])
def test_mode1_partial_at_2_58_is_overflow(N, f):
    """One row 2^37 - 1 wsad above row 0 in 16 columns (instance 0) and in 15 (instance 1): each such term is about
    2^54.07, so the row's partial passes 2^58 with 16 of them (OVERFLOW, by the i128 kernel, nothing written) and
    stays below with 15 (taken here)."""
    B, D = 2, 70
    row = N - 3
    v = 1000 * UNIT + torch.randint(-20_000, 20_001, (B, N, D), generator=torch.Generator().manual_seed(700 + N))
    v[0, row, :16] = v[0, 0, :16] + (1 << 37) - 1
    v[1, row, :15] = v[1, 0, :15] + (1 << 37) - 1
    s = v.sort(1).values
    c1 = [[(int(s[b, N // 2 - 1, c]) + int(s[b, N // 2, c])) // 2 for c in range(D)] for b in range(B)]   # (positive)
    part = [sum(((int(x) - c) ** 2 + 500000) // UNIT for x, c in zip(v[b, row], c1[b])) for b in range(B)]
    assert (1 << 58) <= part[0] < (1 << 62) and part[1] < (1 << 58), [p / 2 ** 58 for p in part]
    got, cpu = _check(v, f, 1, [1, 1], 2 * D)
    assert cpu["status"].tolist() == [OVERFLOW, OK]
    for k in ("c1", "qr"):
        assert (got[k][0] == PATTERN[k]).all(), k
    assert int(got["qr"][1, row]) == part[1]


@pytest.mark.parametrize("N,f,rows", [(7, 1, (3, 2, 6)), (100, 12, (70, 30, 99)), (200, 24, (150, 70, 199))])
def test_mode2_domain_hand_offs(N, f, rows):
    """The second half has no pass 1, so pass 2a checks the domain over every row itself.  A value 2^37 from its
    column's row 0 on a row the rank cut removes (instance 0), on a reliable row (1), on the last row before the
    padding (2); 2^37 - 1 on a removed row is still taken (3); a column whose base is 2^61 (4)."""
    B, D = 5, 70
    r_out, r_in, r_last = rows
    v = _prices(B, N, D, f, seed=710 + N)
    inp = _mode2_inputs(B, N, D, seed=711)
    inp["qr"][:, r_out] = 3 * 10 ** 12                      # the largest: not reliable
    inp["qr"][:, r_in] = 10 ** 11                           # the smallest: reliable
    v[0, r_out, 5] = v[0, 0, 5] + (1 << 37)
    v[1, r_in, 66] = v[1, 0, 66] - (1 << 37)
    v[2, r_last, 9] = v[2, 0, 9] + (1 << 37)
    v[3, r_out, 5] = v[3, 0, 5] + (1 << 37) - 1
    v[4, :, 33] += (1 << 61)
    assert N % 64 != 0 and r_last == N - 1
    got, cpu = _check(v, f, 2, [1, 4], 2 * D, inp)
    assert cpu["status"].eq(OK).all()
    assert cpu["reliable"][:, r_out].eq(0).all() and cpu["reliable"][:, r_in].eq(1).all()


@pytest.mark.parametrize("N,D,f", [(64, 520, 8), (130, 140, 16)])
def test_zero_variance_column_in_one_shard(N, D, f):
    """A constant column in the first shard of one instance: that shard's second half reverts with DIV_BY_ZERO (the
    i128 kernel names it) and leaves the pattern; the other shard, which cannot see the column, runs the instance."""
    B = 3
    v = _prices(B, N, D, f, seed=720 + N)
    v[1, :, 5] = 7 * UNIT
    cut = CUT.get(N, 129)
    parts = _shards(v, cut)
    first = [_check(s, f, 1, [B, 0], D)[0] for s in parts]
    qr = first[0]["qr"] + first[1]["qr"]
    for i, (s, h) in enumerate(zip(parts, first)):
        got, cpu = _check(s, f, 2, [B - 1, 1] if i == 0 else [B, 0], D, {"c1": h["c1"], "qr": qr, "status": h["status"]})
        assert cpu["status"].tolist() == ([OK, DIV_BY_ZERO, OK] if i == 0 else [OK] * B)
        if i == 0:
            for k in ("consensus", "skew", "kurt", "rel", "reliable"):
                assert (got[k][1] == PATTERN[k]).all(), k


# 5. the engine
def _engine(cfgd, v, dev=DEV):
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    e = ConsensusEngine(ConsensusConfig(**cfgd), v.shape[0], device=dev, mode="exact")
    e.values.copy_(v.to(dev, e.values.dtype))
    e.enabled.fill_(1); e.n_active.fill_(v.shape[1]); e.touched.fill_(1)
    return e


STATE = ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status", "consensus_active", "touched",
         "metrics_fx")


@pytest.mark.parametrize("N,D,f", [(64, 520, 8), (130, 140, 16)])
def test_engine_sharded_world1_equals_whole_round(N, D, f):
    from svoc.parallel.dshard import run_round_sharded
    B = 4
    v = _prices(B, N, D, f, seed=800 + N)
    cfgd = dict(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=False, unconstrained_max_spread=1e6)
    ref, e = _engine(cfgd, v), _engine(cfgd, v)
    ref.run_round()
    run_round_sharded(e, D, world=1)
    assert (ref.status == OK).all()
    for k in STATE:
        assert torch.equal(getattr(e, k), getattr(ref, k)), k
    assert e.rounds == ref.rounds
    # a sharded round counts once (its second half): no instance on the i128 kernel
    assert e.exact_routing() == {"processed": B, "wide_column": B, "i128": 0}, e.exact_routing()
    assert ref.exact_routing() == e.exact_routing()


# 6. two ranks on one GPU (gloo)
def _worker(rank, world, port, outdir, x, cfgd):
    from test_dist_gpu import _init
    _init(rank, world, port)
    import torch.distributed as dist
    from svoc.parallel.dshard import run_round_sharded, shard_bounds
    lo, hi = shard_bounds(cfgd["dimension"], rank, world)
    e = _engine({**cfgd, "dimension": hi - lo}, x[:, :, lo:hi])
    run_round_sharded(e, cfgd["dimension"], world=world)
    torch.save({k: getattr(e, k).cpu() for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status")}
               | dict(lo=lo, hi=hi, routing=e.exact_routing()), os.path.join(outdir, f"wx{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu():
    import torch.multiprocessing as mp
    from test_dist_gpu import _free_port
    B, N, D, f = 4, 130, 140, 16
    v = _prices(B, N, D, f, seed=900)
    cfgd = dict(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=False, unconstrained_max_spread=1e6)
    ref = _engine(cfgd, v)
    ref.run_round()
    assert (ref.status == OK).all()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, _free_port(), d, v, cfgd), nprocs=2, join=True)
        r = [torch.load(os.path.join(d, f"wx{i}.pt"), weights_only=True) for i in range(2)]
    for s in r:
        for k in ("rel", "qr", "reliable", "status"):
            assert torch.equal(s[k], getattr(ref, k).cpu()), k
        for k in ("c1", "consensus", "skew", "kurt"):
            assert torch.equal(s[k], getattr(ref, k).cpu()[:, s["lo"]:s["hi"]]), k
        assert s["routing"] == {"processed": B, "wide_column": B, "i128": 0}, s["routing"]
