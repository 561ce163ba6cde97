"""Authenticated update_prediction at batch scale: the batched address lookup (find_oracle_index,
contract.cairo:505-518), ``ConsensusService.update_batch`` against one ``ReferenceContract`` per instance, the
device table as the only source of truth, and the pending-batch row marks with unauthenticated entries.
All checks are equalities on integers or bit patterns."""
import pytest
import torch

import auth_cases as ac
from svoc import ops as svops
from svoc.codec import addresses_to_limbs
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine, _PendingBatches
from svoc.status import Status

pytestmark = pytest.mark.skipif(not svops.available(), reason="svoc/_C.so not built")


@pytest.mark.parametrize("M", ac.LOOKUP_M)
def test_find_address_matches_first_match_loop(M):
    table, inst, addr, want = ac.lookup_case(M)
    out = torch.full_like(inst, 77)
    svops.ops().find_address(table, inst, addr, out)
    assert out.tolist() == want.tolist()
    if M >= 3:
        assert int((want == 1).sum()) >= 2           # both copies of the in-chunk duplicate name the lower index
    if M > 64:
        assert int((want == 5).sum()) >= 2           # ... and of the cross-chunk one
    assert int((want == M - 1).sum()) >= 1 and int((want == -1).sum()) >= 8


def test_find_address_empty_batch_and_checks():
    table, inst, addr, _ = ac.lookup_case(7)
    out = torch.empty(0, dtype=torch.int64)
    svops.ops().find_address(table, inst[:0], addr[:0], out)      # K = 0
    with pytest.raises(RuntimeError):
        svops.ops().find_address(table, inst, addr, torch.empty(3, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        svops.ops().find_address(table, inst.int(), addr, torch.empty_like(inst))
    with pytest.raises(RuntimeError):
        svops.ops().find_address(table[:, :, :3], inst, addr, torch.empty_like(inst))


def test_addresses_to_limbs_and_resolvers():
    svc = ac.service("cpu")
    book = ac.oracle_book()
    assert addresses_to_limbs([]).shape == (0, 4)
    inst = [b for b in range(ac.B) for _ in range(ac.N)] + [0, ac.B]
    callers = [a for r in book for a in r] + [ac.UNKNOWN, book[0][0]]
    got = svc.gov.resolve_oracles(inst, addresses_to_limbs(callers))
    assert got.tolist() == list(range(ac.N)) * ac.B + [-1, -1]
    out = torch.empty(2, dtype=torch.int64)
    assert svc.gov.resolve_admins([1, 1], addresses_to_limbs([ac.ADMINS[2], book[1][0]]), out=out) is out
    assert out.tolist() == [2, -1]
    assert svc.gov.oracle_index(3, book[3][6]) == 6 and svc.gov.oracle_index(3, book[2][6]) is None
    assert svc.gov.oracle_index(ac.B, book[0][0]) is None and svc.gov.oracle_index(0, -1) is None
    assert svc.gov.admin_index(0, ac.ADMINS[1]) == 1 and svc.gov.admin_index(0, book[0][0]) is None


def test_update_batch_matches_reference_contracts():
    stream = ac.Stream()
    contracts, want = stream.replay_reference()
    svc = ac.service("cpu")
    got = ac.run_exact_stream(svc, stream)
    assert got == want
    # the stream covers what it is meant to cover
    assert want["phase1"].count(Status.OK) == ac.B and set(want["phase1"]) == {Status.OK, Status.NOT_ACTIVE}
    p3 = want["phase3"]
    assert p3[1] == Status.NOT_ORACLE and p3[2] == Status.OK and p3[3] == Status.INTERVAL_INPUT
    assert p3[4] == Status.NOT_ORACLE and p3[6].is_revert and p3[6] not in (Status.NOT_ORACLE, Status.INTERVAL_INPUT)
    assert Status.NOT_ORACLE in want["phase4"] and Status.INTERVAL_INPUT in want["phase4"]
    ac.check_against_contracts(svc, contracts)


def test_update_batch_fast_equals_step_with_python_indices():
    stream = ac.Stream()
    auth, plain = ac.service("cpu", "fast", "fp32"), ac.service("cpu", "fast", "fp32")
    replaced = False
    for name, items, _ in stream.batches():
        if name == "gov":
            for s in (auth, plain):
                assert s.governance(items)[1] == [False, True, False, True]
            replaced = True
            continue
        inst, caller, vals = ac.tensors(items, "cpu", "fast")
        st_a = auth.update_batch(inst, caller, vals)
        st_p = plain.engine.step(inst, torch.tensor(stream.resolve(items, replaced)), vals)
        assert torch.equal(st_a, st_p), name
    assert int(Status.NOT_ORACLE) in st_a.tolist()
    for k in ac.STATE:
        assert torch.equal(getattr(auth.engine, k), getattr(plain.engine, k)), k
    assert bool(auth.engine.consensus_active.all())


def test_direct_table_write_is_seen_by_the_next_call():
    svc = ac.service("cpu")
    book = ac.oracle_book()
    v = [400_000, 600_000]
    assert svc.update_predictions([(1, book[1][3], v)]) == [Status.NOT_ACTIVE]
    new = ac.new_oracle(9)
    svc.gov.oracle_addr[1, 3] = ac.limbs(new)        # no governance call: the device table is the only truth
    assert svc.update_predictions([(1, book[1][3], v), (1, new, v)]) == [Status.NOT_ORACLE, Status.NOT_ACTIVE]
    assert svc.gov.oracle_index(1, new) == 3 and svc.gov.oracle_index(1, book[1][3]) is None


def test_update_predictions_keeps_its_status_order():
    svc = ac.service("cpu")
    book = ac.oracle_book()
    with pytest.raises(ValueError):
        svc.update_predictions([(0, book[0][0], [1, 2, 3])])
    got = svc.update_predictions([
        (0, ac.UNKNOWN, [1 << 200, 5]),              # arbitrary-size ints: the interval pre-check comes first
        (0, ac.UNKNOWN, [5, 5]),
        (ac.B, book[0][0], [5, 5]),
        (0, book[0][2], [5, 5]),
        (0, 1 << 300, [5, 5]),                       # not an address at all
        (-2, book[0][0], [-1, 5]),
    ])
    assert got == [Status.INTERVAL_INPUT, Status.NOT_ORACLE, Status.NOT_ORACLE, Status.NOT_ACTIVE,
                   Status.NOT_ORACLE, Status.INTERVAL_INPUT]


def test_unauthenticated_entry_keeps_the_valid_mark_of_its_cell():
    """A folded batch holding (b, oracle 0, valid) then (b, oracle -1): the round that reverts restores every
    row of b, row 0 included (the -1 entry clamps onto row 0's cell and must not erase its mark)."""
    N, D, b = 16, 8, 1
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=2, constrained=True)
    e = ConsensusEngine(cfg, batch=3, device="cpu", mode="fast", storage="fp32")
    e.randomize(seed=4)
    e.run_round()
    before = {k: getattr(e, k).clone() for k in ac.STATE}
    row = torch.full((1, D), 0.5)
    st0 = e.apply_updates(torch.tensor([b, b]), torch.tensor([0, -1]), row.expand(2, D))
    assert st0.tolist() == [int(Status.OK), int(Status.NOT_ORACLE)]
    for o in range(1, N):                            # one batch per oracle: more than FOLD_AT pending batches
        e.apply_updates(torch.tensor([b]), torch.tensor([o]), row)
    assert N > _PendingBatches.FOLD_AT and e._pending.dense is not None
    e.run_round()                                    # every oracle of b at one point: zero variance, revert
    assert e.status[b].item() == int(Status.ZERO_VARIANCE)
    assert st0.tolist() == [int(Status.ZERO_VARIANCE), int(Status.NOT_ORACLE)]
    for k in ac.STATE:
        if k != "status":
            assert torch.equal(getattr(e, k), before[k]), k
