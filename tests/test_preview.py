"""Preview of update_prediction (a simulated call): ConsensusEngine.preview_updates, ConsensusService.preview_batch,
OracleConsensus.simulate_update_prediction and the exact_verdict op on the CPU -- the statuses equal the ones the
committing calls return, and nothing changes."""
import pytest
import torch

import auth_cases as ac
import verdict_cases as vc
from svoc import ops as svops
from svoc import reference as ref
from svoc.api import OracleConsensus
from svoc.config import ConsensusConfig
from svoc.status import ConsensusRevert, Status

pytestmark = pytest.mark.skipif(not svops.available(), reason="svoc/_C.so not built")

N, D, F = 7, 3, 2


def test_preview_equals_step():
    seen = vc.run_preview_stream("cpu", N, D, F)
    assert {Status.OK, Status.NOT_ACTIVE, Status.DIV_BY_ZERO, Status.INTERVAL_INPUT, Status.NOT_ORACLE} <= seen, seen


# ---- a verdict that depends on an earlier update of the same batch -----------------------------------------
# 8 oracles x 4 columns, f = 2: oracles 6 and 7 are far out in columns 1 .. 3 (always masked); column 0 of the
# reliable oracles 0 .. 5 holds 500000 except oracle 0 (450000) and oracle 1 (550000).  Moving both to 500000
# leaves the reliable column 0 without variance: whichever of the two updates comes second reverts.
N2, D2, F2 = 8, 4, 2
ROWS = [[450_000, 480_000, 510_000, 520_000], [550_000, 505_000, 490_000, 470_000],
        [500_000, 520_000, 530_000, 480_000], [500_000, 470_000, 495_000, 515_000],
        [500_000, 510_000, 460_000, 530_000], [500_000, 495_000, 525_000, 490_000],
        [500_000, 100_000, 100_000, 100_000], [500_000, 900_000, 900_000, 900_000]]
UPD_A = (0, [500_000, 480_000, 510_000, 520_000])
UPD_B = (1, [500_000, 505_000, 490_000, 470_000])


def _bootstrapped_engine():
    e = vc.engine(N2, D2, F2, 1, "cpu")
    st = e.step(torch.zeros(N2, dtype=torch.int64), torch.arange(N2), torch.tensor(ROWS))
    assert st.tolist() == [int(Status.NOT_ACTIVE)] * (N2 - 1) + [vc.OK]
    assert e.reliable[0].tolist() == [1] * 6 + [0, 0]
    return e


def test_preview_sees_accepted_updates_of_the_batch():
    e = _bootstrapped_engine()
    for order in ((UPD_A, UPD_B), (UPD_B, UPD_A)):
        inst = torch.zeros(2, dtype=torch.int64)
        orc = torch.tensor([order[0][0], order[1][0]])
        vals = torch.tensor([order[0][1], order[1][1]])
        for K in (None, 2):
            snap = vc.snapshot(e)
            p = e.preview_updates(inst, orc, vals, updates_per_instance=K)
            vc.assert_unchanged(e, snap)
            assert p.tolist() == [vc.OK, int(Status.DIV_BY_ZERO)], order   # the second one completes the column
    # each alone is accepted: so A is OK before B and DIV_BY_ZERO after it (and the other way round)
    for o, v in (UPD_A, UPD_B):
        assert e.preview_updates(torch.tensor([0]), torch.tensor([o]), torch.tensor([v])).tolist() == [vc.OK]


def test_simulate_update_prediction_abi():
    admins, oracles = [11, 12, 13], [100 + i for i in range(N2)]
    c = OracleConsensus(admins, True, 2, F2, True, 0, D2, oracles)
    for o, row in zip(oracles, ROWS):
        c.update_prediction(o, row)
    assert c.consensus_active()
    assert c.update_prediction(oracles[UPD_A[0]], UPD_A[1]) == Status.OK

    def getters():
        return (c.get_consensus_value(), c.get_reliability(), c.get_skewness(), c.get_kurtosis(),
                c.get_oracle_value_list(admins[0]), c.consensus_active())
    before = getters()
    st = c.simulate_update_prediction(oracles[UPD_B[0]], UPD_B[1])      # would revert: returned, not raised
    assert st == Status.DIV_BY_ZERO and isinstance(st, Status)
    assert c.simulate_update_prediction(oracles[2], ROWS[3]) == Status.OK
    assert c.simulate_update_prediction(99, ROWS[3]) == Status.NOT_ORACLE
    assert c.simulate_update_prediction(oracles[2], [1_000_001] + ROWS[3][1:]) == Status.INTERVAL_INPUT
    assert getters() == before
    with pytest.raises(ConsensusRevert) as err:
        c.update_prediction(oracles[UPD_B[0]], UPD_B[1])
    assert err.value.status == Status.DIV_BY_ZERO
    assert getters() == before


def test_preview_batch_authenticates_like_update_batch():
    book = ac.oracle_book(N2, 2)
    svc = ac.service("cpu", n=N2, d=D2, f=F2, batch=2, book=book)
    boot = [(b, book[b][o], ROWS[o]) for b in range(2) for o in range(N2)]
    assert svc.update_batch(*ac.tensors(boot, "cpu", "exact")).tolist() == ([1] * (N2 - 1) + [0]) * 2
    codes, applied = svc.governance([("propose", 1, ac.ADMINS[0], (4, ac.new_oracle(1))), ("vote", 1, ac.ADMINS[1], 0, True)])
    assert codes == [Status.OK] * 2 and applied == [False, True]
    items = [(1, book[1][4], ROWS[4]),            # the replaced oracle's old address
             (1, ac.new_oracle(1), ROWS[4]),      # its new one
             (0, book[0][4], ROWS[4]),            # instance 0 kept its oracle
             (0, ac.UNKNOWN, [1_000_001, 0, 0, 0]),
             (5, book[0][0], ROWS[0])]
    want = [Status.NOT_ORACLE, Status.OK, Status.OK, Status.INTERVAL_INPUT, Status.NOT_ORACLE]
    snap = vc.snapshot(svc.engine)
    got = svc.preview_batch(*ac.tensors(items, "cpu", "exact"))
    vc.assert_unchanged(svc.engine, snap)
    assert [Status(s) for s in got.tolist()] == want
    assert [Status(s) for s in svc.update_batch(*ac.tensors(items, "cpu", "exact")).tolist()] == want


def test_legacy_simulate_update_prediction():
    """The obsolete contract's ABI (legacy rounds: exact_verdict runs the full round into scratch outputs)."""
    from svoc.api import LegacyOracleConsensus
    oracles = [100 + i for i in range(N2)]
    c = LegacyOracleConsensus([11, 12, 13], True, 2, F2, True, 0, D2, oracles, variant="nd_legacy")
    for o, row in zip(oracles[:-1], ROWS):
        c.update_prediction(o, row)
    assert c.simulate_update_prediction(oracles[0], ROWS[1]) == Status.NOT_ACTIVE
    assert not c.consensus_active()
    # the last oracle's commit would run the first round: its verdict is the one update_prediction then gets
    st = c.simulate_update_prediction(oracles[-1], ROWS[-1])
    assert st == Status.OK and not c.consensus_active() and int(c.engine.n_active[0]) == N2 - 1
    assert c.update_prediction(oracles[-1], ROWS[-1]) == Status.OK and c.consensus_active()
    before = (c.get_consensus_value(), c.get_reliability(), c.get_oracle_value_list(11))
    assert c.simulate_update_prediction(oracles[2], [2_000_000] + ROWS[2][1:]) == Status.INTERVAL_INPUT
    assert c.simulate_update_prediction(99, ROWS[2]) == Status.NOT_ORACLE
    assert c.simulate_update_prediction(oracles[2], ROWS[3]) == Status.OK
    assert (c.get_consensus_value(), c.get_reliability(), c.get_oracle_value_list(11)) == before


def test_preview_predictions_fast_mode_raises():
    svc = ac.service("cpu", mode="fast", n=N2, d=D2, f=F2, batch=1, book=ac.oracle_book(N2, 1))
    with pytest.raises(NotImplementedError, match="exact"):
        svc.preview_predictions([(0, svc.gov.oracle_list(0)[0], [0.5] * D2)])


def test_preview_needs_exact_mode():
    from svoc.engine import ConsensusEngine
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=F, constrained=True)
    e = ConsensusEngine(cfg, batch=1, device="cpu", mode="fast")
    with pytest.raises(NotImplementedError, match="exact"):
        e.preview_updates(torch.tensor([0]), torch.tensor([0]), torch.zeros(1, D))


# ---- the op ------------------------------------------------------------------------------------------------

def _golden(x, f):
    st, res = ref.round_status(x.tolist(), f, True)
    return Status(st), res


def _assert_recipes_against_the_golden_model(n, d, f):
    """The recipes give the statuses of the table, for the reasons it names (svoc/reference.py)."""
    for name in vc.RECIPES:
        x = vc.recipe(name, n, d, f)
        st, res = _golden(x, f)
        if name in vc.EXPECTED:
            assert st == vc.EXPECTED[name], name
        if name in ("plain", "plain_b", "out_of_domain"):
            assert st == Status.OK and res.reliable == [False] * f + [True] * (n - f), name
    # "variance 1": the reliable rows of the last column have variance exactly 1
    x = vc.recipe("variance_one", n, d, f)
    col = x[f:, d - 1].tolist()
    assert ref.variance(col, ref.average(col)) == 1
    col = vc.recipe("zero_variance", n, d, f)[f:, d - 1].tolist()
    assert ref.variance(col, ref.average(col)) == 0
    assert _golden(vc.recipe("plain", n, d, f), n - 3)[0] == Status.DIV_BY_ZERO        # R < 4


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_exact_verdict_op_cpu(dtype):
    n, d, f = 8, 4, 2
    _assert_recipes_against_the_golden_model(n, d, f)
    x = vc.batch(n, d, f)
    want = [int(_golden(x[b], f)[0]) for b in range(len(vc.RECIPES))]
    assert want[:4] == [int(vc.EXPECTED[k]) for k in vc.RECIPES[:4]]
    st_r, rel_r = vc.run_round(x.to(dtype), f)
    assert st_r.tolist() == want
    st_v, rel_v, _ = vc.run_verdict(x.to(dtype), f)
    vc.same_verdict(st_v, rel_v, st_r, rel_r)
    # R < 4 (f = N - 3): the kurtosis divides by zero wherever the reliabilities pass
    st_r, rel_r = vc.run_round(x.to(dtype), n - 3)
    assert st_r.tolist()[0] == int(Status.DIV_BY_ZERO) == int(_golden(x[0], n - 3)[0])
    st_v, rel_v, _ = vc.run_verdict(x.to(dtype), n - 3)
    vc.same_verdict(st_v, rel_v, st_r, rel_r)
    # inactive instances keep their status and rel
    act = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.uint8)
    rel = torch.full((6, 2), -7, dtype=torch.int64)
    status = torch.full((6,), -1, dtype=torch.int32)
    svops.ops().exact_verdict(x.to(dtype), act, f, True, 0, rel, status, False)
    assert status.tolist() == [want[0], -1, want[2], -1, want[4], -1]
