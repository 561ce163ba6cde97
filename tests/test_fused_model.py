"""The fused-round model (fused_cases.py) is pinned before it judges a kernel: its cases hold what they
claim, the routes are the claimed ones, and the model agrees with the CPU engine's generic transactional
path (update, round, restore) over the same batches.  No GPU."""
import pytest
import torch

import fast_cases
import fused_cases as fc
from fused_cases import INTERVAL_INPUT, NOT_ORACLE, OK, ZERO_VARIANCE
from svoc import ops as svops
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine

CASES = [pytest.param(s, id=fc.shape_id(s)) for s in fc.SHAPES]


def test_every_instantiation_is_listed():
    """Lane groups 1 / 2 / 4 x half-widths 5 / 17, each fused and deferred, and both wide forms."""
    fused = {(s.nseg, s.h) for s in fc.SHAPES if not s.wide}
    defer = {(s.nseg, s.h) for s in fc.SHAPES if fc.deferred(s)}
    wide = {(s.nseg, s.h) for s in fc.SHAPES if s.wide}
    every = {(g, h) for g in (1, 2, 4) for h in (5, 17)}
    assert fused == every and defer == every and wide == {(4, 5), (4, 17)}
    assert any(s.D % 4 and not fc.deferred(s) for s in fc.SHAPES) and any(s.D > 4096 for s in fc.SHAPES)


@pytest.mark.parametrize("s", CASES)
def test_route_is_the_claimed_one(s):
    r = svops.fast_route("fp32", s.N, s.D, (s.D + 7) // 8 * 8, s.f, True)
    assert r.kernel == svops.KERNEL_WINDOW and (r.lane_groups, r.win_h) == (s.nseg, s.h)
    assert r.fused_max_u == 256 and r.defer_max_u == (127 if s.D % 4 == 0 else 0)
    assert r.pruned == (s.N == 256 and s.h == 17)
    assert s.wide == (s.U > 255) and fc.deferred(s) == (s.U <= r.defer_max_u)


@pytest.mark.parametrize("s", CASES)
def test_cut_gap(s):
    """The reference alone: every instance's rank cut is at least 100 x the fp32 qr rtol wide at every step."""
    c = fc.build(s)
    assert fc.MIN_CUT_GAP == 100 * fast_cases.TOL["fp32"]["qr"][0]
    for step, m in enumerate(c["steps"]):
        gap = fast_cases.cut_gap(m["ref"], s.f)
        assert float(gap.min()) >= fc.MIN_CUT_GAP, (step, gap.tolist())
        assert torch.equal(m["ref"]["reliable"], ~c["far"]), step


@pytest.mark.parametrize("s", CASES)
def test_case_holds_its_situations(s):
    """Read off the model's statuses (and the batches): what fused_cases._batch says each role plants."""
    c = fc.build(s)
    N, D, U, B = s.N, s.D, s.U, c["B"]
    st = [m["upd_status"] for m in c["steps"]]
    rs = [m["status"] for m in c["steps"]]
    orc = [o for o, _ in c["batches"]]
    rows = [r for _, r in c["batches"]]
    neg0 = lambda t: (fc.bits(t) == -(1 << 31))
    accepted = lambda step, b: {o for o, x in zip(orc[step][b].tolist(), st[step][b].tolist()) if x == OK}

    b = fc.role_inst(c, fc.INVALID)
    for step in range(fc.STEPS):
        u = U - 2 if step == 0 else U - 1
        assert st[step][b, u] == INTERVAL_INPUT and int((st[step][b] == OK).sum()) == U - 1 and rs[step][b] == OK
        row = rows[step][b, u]
        assert not (0 <= row[D - 1] <= 1) and bool(((row[:D - 1] >= 0) & (row[:D - 1] <= 1)).all())
    assert U < 34 or U - 2 >= 32                                    # a slot past the first 32-bit word of bad slots
    # ... accepted at step 0 (the end of the instance's batch, a distinctive last column), invalid at step 1
    assert orc[0][b, U - 1] == N - 1 and st[0][b, U - 1] == OK and st[1][b, U - 1] == INTERVAL_INPUT
    assert c["steps"][0]["values"][b, N - 1, D - 1] == 0.875 == c["steps"][2]["values"][b, N - 1, D - 1]
    assert bool(neg0(rows[0][b, 0, 0])) and st[0][b, 0] == OK and bool(neg0(c["steps"][0]["values"][b, orc[0][b, 0], 0]))
    kinds = {int(fc.bits(rows[step][b, U - 2 if step == 0 else U - 1, D - 1])) for step in range(fc.STEPS)}
    assert len(kinds) == 3

    b = fc.role_inst(c, fc.ZV_SEQUENCE)
    assert rs[0][b] == OK and rs[1][b] == ZERO_VARIANCE and rs[2][b] == OK
    assert (st[0][b] == OK).all() and (st[1][b] == ZERO_VARIANCE).all()          # a plain zero-variance revert
    assert torch.equal(orc[0][b], orc[1][b])                                      # ... while its rows pend
    assert torch.equal(c["steps"][1]["values"][b], c["steps"][0]["values"][b])
    assert not torch.equal(c["steps"][0]["values"][b], c["x0"][b])
    if B == 2:
        return

    b = fc.role_inst(c, fc.VALID)
    for step in range(fc.STEPS):
        assert (st[step][b] == OK).all() and rs[step][b] == OK
        assert orc[step][b, U - 1] == N - 1
        assert c["steps"][step]["values"][b, N - 1, D - 1] == rows[step][b, U - 1, D - 1] == (0.875, 0.8125, 0.90625)[step]
        assert bool(neg0(c["steps"][step]["values"][b, orc[step][b, 0], 0]))
    a0, a1, a2 = accepted(0, b), accepted(1, b), accepted(2, b)
    assert a0 & a1 and (a0 - a1 or U == N) and (a1 - a2 or U == N)  # accepted in s and s + 1; in s only

    b = fc.role_inst(c, fc.THREE_INVALID)
    for step in range(fc.STEPS):
        bad = (st[step][b] == INTERVAL_INPUT).nonzero().flatten().tolist()
        assert bad == [0, U // 2, U - 1] and rs[step][b] == OK
        assert orc[step][b, 0] // 64 == orc[step][b, U // 2] // 64
        assert int((st[step][b] == OK).sum()) == U - 3
    assert U == 3 or (bool(neg0(rows[0][b, 1, 1])) and st[0][b, 1] == OK)

    b = fc.role_inst(c, fc.ZV_AFTER_DROP)
    assert rs[0][b] == ZERO_VARIANCE and st[0][b, 1] == INTERVAL_INPUT
    assert (st[0][b, [u for u in range(U) if u != 1]] == ZERO_VARIANCE).all()
    assert not c["far"][b, orc[0][b, 1]]
    zc = fc.bits(c["x0"][b, ~c["far"][b], fc.ZCOL])
    assert set(zc.tolist()) == {0, -(1 << 31)}                     # constant by value, not by bits
    # ... the column is constant only once that row is dropped: stored regardless, the round would not revert
    x = c["x0"][b].clone()
    x[orc[0][b]] = rows[0][b].nan_to_num(0.5, 0.5, 0.5).clamp(0, 1)
    assert not bool((x[~c["far"][b]] == x[~c["far"][b]][0]).all(0).any())
    assert torch.equal(c["steps"][0]["values"][b], c["x0"][b]) and rs[1][b] == OK and (st[1][b] == OK).all()

    b = fc.role_inst(c, fc.NO_ORACLE)
    ids, nan_no = set(), 0
    for step in range(fc.STEPS):
        for u, o in enumerate(orc[step][b].tolist()):
            if not 0 <= o < N:
                ids.add(o)
                isnan = bool(rows[step][b, u].isnan().any())
                nan_no += isnan
                assert st[step][b, u] == (INTERVAL_INPUT if isnan else NOT_ORACLE)
        assert rs[step][b] == OK
    assert ids == set(fc.OUTSIDE_IDS(N)) and nan_no >= 1

    if fc.deferred(s):
        # the lagging state differs from the exact one after some launch, and the last batch's commit closes it
        lag = c["lag"]
        assert any(not torch.equal(lag[k], c["steps"][k - 1]["values"]) for k in range(1, fc.STEPS))
        last = fc.STEPS - 1
        done = fc.update_cases.model_commit(lag[last], rows[last].reshape(B * U, D), orc[last].reshape(-1),
                                            st[last].reshape(-1), U)
        assert torch.equal(fc.bits(done), fc.bits(c["steps"][last]["values"]))


OUT = ("c1", "consensus", "rel", "reliable", "skew", "kurt", "qr")


@pytest.mark.parametrize("s", CASES)
def test_model_matches_cpu_engine(s):
    """step() of the CPU engine (fp32 storage; update, round, restore) over the same batches: statuses, ``values``
    and ``reliable`` equal, c1 and consensus equal by value, the rest within TOL["fp32"] (fast_cases.check_round);
    a reverted instance keeps every output of the step before."""
    c = fc.build(s)
    N, D, f, U, B = s.N, s.D, s.f, s.U, c["B"]
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    e = ConsensusEngine(cfg, batch=B, device="cpu", mode="fast", storage="fp32")
    e.randomize(seed=1)
    e.run_round()
    e.values[:, :, :D] = c["x0"]
    e.run_round(only_touched=False)     # (step() skips the round of an instance whose updates were all rejected)
    inst = torch.arange(B).repeat_interleave(U)
    for step, ((orc, rows), m) in enumerate(zip(c["batches"], c["steps"])):
        before = {k: getattr(e, k).clone() for k in OUT}
        st = e.step(inst, orc.reshape(-1), rows.reshape(B * U, D))
        tag = "%s step %d" % (fc.shape_id(s), step)
        fc.same(st.view(B, U), m["upd_status"], tag, "upd_status [instance, slot]")
        fc.same(e.status, m["status"], tag, "status [instance]")
        fc.same(e.values[:, :, :D], m["values"], tag, "values [instance, oracle, column]")
        ok = (m["status"] == OK).nonzero().flatten()
        o = {k: getattr(e, k)[ok] for k in OUT}
        o["status"] = e.status[ok]
        fast_cases.check_round(o, fc.round_case(c, step, ok), tag)
        for b in (m["status"] != OK).nonzero().flatten().tolist():
            for k in OUT:
                fc.same(getattr(e, k)[b], before[k][b], tag, "reverted instance %d wrote %s" % (b, k))
