"""The CPU governance ops against the golden contract (tests/gov_cases.py), and, from the golden alone, the
conditions that keep the cases from passing empty.  The same cases run on the GPU in
tests/test_governance_gpu.py."""
import pytest
import torch

import gov_cases as gc
from svoc.governance import Governance
from svoc.reference import ReferenceContract
from svoc.status import Status


def _gov(built, device="cpu"):
    return Governance(built.B, built.A, built.N, device, True, built.majority)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_random_case_cpu_matches_golden(shape):
    built = gc.random_case(shape)
    gc.check_ordered(_gov(built), built)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_random_cases_are_not_empty(shape):
    """From the golden alone: a replacement applies and every status code is met; an instance's run is several
    hundred actions long (more than one 256-lane workgroup of the sorted batch)."""
    built = gc.random_case(shape)
    stage = built.stages[0]
    assert int(stage.applied.sum()) >= 1
    need = {Status.OK, Status.NOT_ADMIN, Status.WRONG_ORACLE_INDEX, Status.ALREADY_ORACLE, Status.WRONG_ADMIN_INDEX,
            Status.UNWRAP_NONE}
    assert {int(s) for s in need} <= set(stage.status.tolist())
    assert 3 <= built.B <= 8 and stage.status.numel() == gc.K_RANDOM
    assert int(torch.bincount(stage.actions["inst"]).min()) > 256
    acts = built.action_list[0]
    # a non-admin caller one limb away from an admin, a new address one limb away from an oracle (accepted)
    near = {x for row in built.addr.near_admins for x in row}
    assert all(stage.status[k] == int(Status.NOT_ADMIN) for k, a in enumerate(acts) if a.caller in near)
    assert sum(a.caller in near for a in acts) > 50
    near_o = {x for row in built.addr.spares for x in row[gc.N_SPARES:]}
    assert any(a.kind == gc.PROPOSE and a.arg0 and a.addr in near_o and stage.status[k] == 0
               for k, a in enumerate(acts))
    if built.A == 64 and built.majority > 2:   # bit 63 of a vote column is set at the end (a negative int64 column)
        assert bool((stage.state["votes"] < 0).any())


def test_addresses_are_what_the_cases_claim():
    ad = gc.random_case(gc.SHAPES[2]).addr
    for b in range(len(ad.admins)):
        everyone = ad.admins[b] + ad.oracles[b] + ad.spares[b] + ad.near_admins[b]
        assert len(set(everyone)) == len(everyone)
        for x in everyone:
            assert x.bit_length() == 251 and all(l >> 63 for l in gc.limbs(x)[:3])     # negative int64 limbs 0-2
        pool = ad.admins[b] + ad.oracles[b] + ad.spares[b][:gc.N_SPARES]
        for i in range(len(pool) - 4):      # entries i and i + 4 differ in limb i % 4 alone
            assert [p != q for p, q in zip(gc.limbs(pool[i]), gc.limbs(pool[i + 4]))] == [L == i % 4 for L in range(4)]
        for L in range(4):
            a, o = ad.near_admins[b][L], ad.spares[b][gc.N_SPARES + L]
            assert a not in ad.admins[b] and min(gc.n_limbs_differing(a, x) for x in ad.admins[b]) == 1
            assert o not in ad.oracles[b] and min(gc.n_limbs_differing(o, x) for x in ad.oracles[b]) == 1
            assert gc.limbs(a)[L] != gc.limbs(ad.admins[b][L % len(ad.admins[b])])[L]
            assert gc.limbs(o)[L] != gc.limbs(ad.oracles[b][L % len(ad.oracles[b])])[L]


def _same(x, y):
    for s, t in zip(x.stages, y.stages):
        assert torch.equal(s.status, t.status) and torch.equal(s.applied, t.applied)
        assert all(torch.equal(s.state[k], t.state[k]) for k in s.state)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_cheap_rollback_is_the_golden_contract(shape):
    """gov_cases.Contract changes how ReferenceContract rolls a transaction back, not what it does: the
    unmodified contract gives the same answers (every action for A <= 5, the first 400 beyond: it takes
    milliseconds per action there)."""
    K = gc.K_RANDOM if shape.A <= 5 else 400
    _same(gc.random_case(shape, K, gc.Contract), gc.random_case(shape, K, ReferenceContract))


def test_directed_case_golden_and_cpu():
    """A = 64, majority 64: what the golden says about each scenario, then the CPU op against it."""
    built = gc.directed_case()
    _same(built, gc.directed_case(ReferenceContract))
    stage, acts = built.stages[0], built.action_list[0]
    st, ap = stage.status.tolist(), stage.applied.tolist()
    run = lambda b: [k for k, a in enumerate(acts) if a.inst == b]     # noqa: E731
    OK, NA = int(Status.OK), int(Status.NOT_ADMIN)
    for b in (0, 1):        # the 64th vote applies, and not before; the last emitter is 62 / 63
        r = run(b)
        assert len(r) == 64 and [st[k] for k in r] == [OK] * 64 and [ap[k] for k in r] == [0] * 63 + [1]
    assert acts[run(1)[-1]].caller == built.addr.admins[1][63]
    r = run(2)              # ..., withdraw, admin 1 (63 votes: nothing applies), emitter 63 again (64: applies)
    assert [st[k] for k in r] == [OK] * len(r) and [ap[k] for k in r] == [0] * (len(r) - 1) + [1]
    assert acts[r[-3]].arg1 == 0 and acts[r[-3]].caller == acts[r[-1]].caller == built.addr.admins[2][63]
    r = run(3)              # Some, None, 62 stored votes, the 64th vote reverts, a new proposition
    assert [st[k] for k in r] == [OK] * 64 + [int(Status.UNWRAP_NONE), OK] and not any(ap[k] for k in r)
    vm = stage.lists[3][2]
    assert [vm[e][5] for e in range(64)] == [e == 5 for e in range(64)]            # the column was cleared
    assert stage.lists[3][1][5] == (1, built.addr.spares[3][3])
    r = run(4)
    assert [st[k] for k in r] == [OK] * 4 + [int(Status.ALREADY_ORACLE)] * 7 + [NA] * 4
    assert stage.lists[4][0] == built.addr.oracles[4]
    out = [k for k, a in enumerate(acts) if not 0 <= a.inst < built.B]
    assert len(out) == 6 and all(st[k] == NA and ap[k] == 0 for k in out)
    assert stage.lists[5][1] == [None] * 64 and not any(any(row) for row in stage.lists[5][2])
    assert [len(set(l[0]) - set(o)) for l, o in zip(stage.lists, built.addr.oracles)] == [1, 1, 1, 0, 0, 0]
    gc.check_ordered(_gov(built), built)


def test_unwrap_none_vote_bit_is_not_stored():
    """Directed scenario 3 without the closing proposition: the reverted 64th vote leaves bit 63 of column 5 clear."""
    built = gc.directed_case()
    acts = [a for a in built.action_list[0] if a.inst == 3][:-1]
    cut = gc.build("directed-3", 64, 7, 64, built.addr, [acts])
    vm = cut.stages[0].lists[3][2]
    assert cut.stages[0].status.tolist()[-1] == int(Status.UNWRAP_NONE)
    assert [vm[e][5] for e in range(64)] == [e != 63 for e in range(64)]
    assert int(cut.stages[0].state["votes"][3, 5]) == (1 << 63) - 1
    gc.check_ordered(_gov(cut), cut)


def test_empty_batch():
    built = gc.empty_case()
    gc.check_ordered(_gov(built), built)
    gc.check_unordered(_gov(built), built)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_unique_slice_cpu_matches_golden(shape):
    """The unordered op's cases (one action per instance, two launches) on the CPU, through both ops; from the
    golden alone: the vote decides wherever the proposition stood (A >= 2)."""
    built = gc.slice_case(shape)
    first, second = built.stages
    assert first.actions["inst"].numel() == gc.SLICE_B > 2 * 256
    assert not torch.equal(first.actions["inst"], torch.arange(gc.SLICE_B))        # shuffled
    codes = set(first.status.tolist())
    assert {int(Status.OK), int(Status.NOT_ADMIN), int(Status.WRONG_ORACLE_INDEX), int(Status.ALREADY_ORACLE)} <= codes
    assert {int(Status.OK), int(Status.NOT_ADMIN), int(Status.WRONG_ADMIN_INDEX)} <= set(second.status.tolist())
    assert int(second.applied.sum()) > (gc.SLICE_B // 5 if shape.A >= 2 else -1)
    assert (int(second.applied.sum()) == 0) == (shape.A == 1)
    gc.check_unordered(_gov(built), built)
    gc.check_ordered(_gov(built), built)
