"""The saved-batch transactional fast round on the CPU ops against the sequential model of txn_cases.py:
apply_updates with save, fast_round, restore_updates (the CPU fast_round refuses rst_saved, so the restore op
follows it explicitly).  Pins the CPU twin's generic path, and proves every case and its conditions before
any GPU run."""
import pytest
import torch

import txn_cases as tc
from svoc import ops as svops
from txn_cases import OK, RELIABILITY_INTERVAL, TOO_FEW_RELIABLE, ZERO_VARIANCE

CASES = [pytest.param(c, id=tc.case_id(c)) for c in tc.CASES]


@pytest.mark.parametrize("c", CASES)
def test_case_conditions(c):
    """Cut gap, reliabilities clear of the interval's ends, variance of the reliable columns, each role's
    verdict: for every instance, from the model alone."""
    m = tc.build(c)
    codes = tc.conditions(m)
    assert 5 <= m["U"] <= min(c.N, 40)
    if c.legacy and not c.constrained:
        assert set(codes.values()) == {OK, tc.STATUS_PREFILL}      # no valid data reverts such a round
    elif c.N - c.f < 4:
        assert codes["VALID"] == TOO_FEW_RELIABLE and codes["REL_AND_ZV"] == RELIABILITY_INTERVAL
    else:
        want = RELIABILITY_INTERVAL if c.legacy else ZERO_VARIANCE
        assert codes["VALID"] == codes["ACTIVATE_OK"] == codes["REJECTED_OK"] == OK
        assert codes["ZV"] == codes["ACTIVATE_REVERT"] == codes["REJECTED_REVERT"] == want
        assert codes.get("REL_AND_ZV", RELIABILITY_INTERVAL) == RELIABILITY_INTERVAL and codes.get("ZV2", want) == want
    assert codes["INACTIVE"] == tc.STATUS_PREFILL


def test_case_list_covers_the_roll_back_forms():
    """Both forms of the roll-back, every lane-group width and half-width of the in-kernel one, duplicates on
    each form, and what the model does with a reverted activation and with rejected updates."""
    inker = {(c.nseg, c.h) for c in tc.CASES if c.rollback and c.constrained and not c.legacy}
    assert inker == {(g, h) for g in (1, 2, 4) for h in (5, 17)}
    assert {c.rollback for c in tc.CASES if c.dup} == {0, 1}
    assert {(c.kernel, c.storage) for c in tc.CASES if not c.rollback} == {
        (tc.SMALL, "bf16"), (tc.TWO_NET, "bf16"), (tc.WINDOW, "fp32"), (tc.TWO_NET, "fp32")}
    m = tc.build(tc.CASES[0])
    c, U, model = m["case"], m["U"], m["model"]
    b = m["roles"].index(tc.ACTIVATE_REVERT)
    dis = m["disabled"][b]
    assert len(dis) >= 2 and int(m["state"]["n_active"][b]) == c.N - len(dis)
    assert int(model["post"]["n_active"][b]) == c.N and int(model["final"]["n_active"][b]) == c.N - len(dis)
    assert model["final"]["enabled"][b, dis].tolist() == [0] * len(dis)
    assert torch.equal(model["final"]["values"][b].view(torch.int16), m["state"]["values"][b].view(torch.int16))
    b = m["roles"].index(tc.REJECTED_REVERT)
    st = model["final"]["upd_status"].view(tc.B, U)[b].tolist()
    assert set(st) == {2, 3, ZERO_VARIANCE}                        # INTERVAL_INPUT, NOT_ORACLE, the round's code
    assert [st[u] for u in (0, 2, U - 1)] == [3, 3, 3] and st[1] == 2 and st[3] == 2
    b = m["roles"].index(tc.INACTIVE)
    assert set(model["final"]["upd_status"].view(tc.B, U)[b].tolist()) == {OK}
    assert not torch.equal(model["final"]["values"][b].view(torch.int16), m["state"]["values"][b].view(torch.int16))


@pytest.mark.parametrize("c", CASES)
def test_cpu_ops_match_model(c):
    m = tc.build(c)
    tc.conditions(m)
    o = svops.ops()
    r = tc.Run(m, "cpu")
    r.apply(o)
    active = r.active()
    assert torch.equal(active.bool(), m["model"]["active"])
    r.round(o, active)
    r.restore(o, active)
    tc.check(r, "cpu")
