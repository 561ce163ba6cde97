"""Cases for the admin voting ops (csrc/include/svoc/governance.hpp, csrc/kernels/governance.hip) with the golden
contract ``svoc.reference.ReferenceContract`` as the reference: one contract per instance, the status is the
revert's code (0 otherwise), ``applied`` is what ``vote_for_a_proposition`` returns.

Imports no svoc code except svoc.reference, svoc.codec and svoc.status; CPU only.  tests/test_governance_model.py
runs the cases through the CPU ops (and checks from the golden alone that they are not empty);
tests/test_governance_gpu.py runs them through the HIP kernels.

Addresses are full width.  Every instance draws a 251-bit base whose limbs 0-2 have bit 63 set (negative int64
limbs); every admin, oracle and spare is the base with ONE limb changed, and which limb cycles with the entry, so
entries i and i + 4 differ in one limb only and each of the four limbs alone decides some comparison.  Four more
spares equal an oracle, and four non-admin callers equal an admin, in three limbs (one per limb).
"""
from __future__ import annotations

import functools
import random
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from svoc.codec import address_to_limbs
from svoc.reference import ReferenceContract
from svoc.status import ConsensusRevert, Status

M64 = (1 << 64) - 1
PROPOSE, VOTE = 0, 1
N_SPARES = 6


# ------------------------------------------------------------------------------------------------ the golden
class Contract(ReferenceContract):
    """ReferenceContract with a cheaper rollback.  The parent deep-copies its whole state before every
    transaction (64 x 64 votes, 300 oracles: milliseconds per action, and a case has thousands); this one saves
    what the governance transactions can write.  The rules (``_update_proposition``, ``_vote``) are the parent's,
    and tests/test_governance_model.py runs the unmodified parent next to it."""

    def _transaction(self, fn, *args):
        votes = [row[:] for row in self.vote_matrix]
        props = list(self.propositions)
        addrs = [o.address for o in self.oracles]
        try:
            return fn(*args)
        except ConsensusRevert:
            self.vote_matrix, self.propositions = votes, props
            for o, a in zip(self.oracles, addrs):
                o.address = a
            raise


def new_contract(cls, admins: Sequence[int], oracles: Sequence[int], majority: int) -> ReferenceContract:
    return cls(list(admins), True, majority, 0, True, 0, 1, list(oracles))


class Action(NamedTuple):
    inst: int
    caller: int
    kind: int            # PROPOSE / VOTE
    arg0: int            # propose: 1 Some / 0 None;  vote: which_admin
    arg1: int            # propose: old oracle index; vote: support
    addr: int            # propose: new address


def apply_golden(contracts: List[ReferenceContract], a: Action) -> Tuple[int, int]:
    """-> (status, applied) of one action; an instance outside [0, B) is nobody's admin."""
    if not 0 <= a.inst < len(contracts):
        return int(Status.NOT_ADMIN), 0
    c = contracts[a.inst]
    try:
        if a.kind == PROPOSE:
            c.update_proposition(a.caller, (a.arg1, a.addr) if a.arg0 else None)
            return int(Status.OK), 0
        return int(Status.OK), int(bool(c.vote_for_a_proposition(a.caller, a.arg0, bool(a.arg1))))
    except ConsensusRevert as e:
        return int(e.status), 0


# ------------------------------------------------------------------------------------------------ addresses
def limbs(x: int) -> List[int]:
    return [(x >> (64 * i)) & M64 for i in range(4)]


def xor_limb(x: int, L: int, v: int) -> int:
    return x ^ (v << (64 * L))


def n_limbs_differing(x: int, y: int) -> int:
    return sum(p != q for p, q in zip(limbs(x), limbs(y)))


class Addresses(NamedTuple):
    admins: List[List[int]]        # [B][A]
    oracles: List[List[int]]       # [B][N]
    spares: List[List[int]]        # [B][N_SPARES + 4]: the last four equal an oracle in three limbs
    near_admins: List[List[int]]   # [B][4]: equal an admin in three limbs; not admins


def make_addresses(rng: random.Random, B: int, A: int, N: int) -> Addresses:
    out = Addresses([], [], [], [])
    for _ in range(B):
        base = 0
        for L in range(3):
            base |= (rng.getrandbits(64) | (1 << 63)) << (64 * L)
        base |= (rng.getrandbits(58) | (1 << 58)) << 192           # bit 250: a 251-bit value
        pool = [xor_limb(base, i % 4, i // 4 + 1) for i in range(A + N + N_SPARES)]
        admins, oracles, spares = pool[:A], pool[A:A + N], pool[A + N:]
        spares = spares + [xor_limb(oracles[L % N], L, 1 << 40) for L in range(4)]
        near = [xor_limb(admins[L % A], L, 1 << 41) for L in range(4)]
        out.admins.append(admins); out.oracles.append(oracles); out.spares.append(spares); out.near_admins.append(near)
    return out


# ------------------------------------------------------------------------------------------------ built cases
class Stage(NamedTuple):
    """One launch: the actions as the ops take them, what the golden answers, and its state afterwards."""
    actions: Dict[str, torch.Tensor]     # inst, caller, kind, arg0, arg1, addr
    status: torch.Tensor                 # int32 [K]
    applied: torch.Tensor                # uint8 [K]
    state: Dict[str, torch.Tensor]       # oracle_addr, votes, prop_tag, prop_idx, prop_addr (idx / addr: tag 1 only)
    lists: Optional[list]                # per instance (oracle_list, propositions, vote_matrix), small B only


class Built(NamedTuple):
    name: str
    A: int
    N: int
    majority: int
    B: int
    addr: Addresses
    stages: List[Stage]
    action_list: List[List[Action]]


def wrap(x: int) -> int:
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def action_tensors(actions: Sequence[Action]) -> Dict[str, torch.Tensor]:
    K = len(actions)
    return dict(
        inst=torch.tensor([a.inst for a in actions], dtype=torch.int64).reshape(K),
        caller=torch.tensor([address_to_limbs(a.caller) for a in actions], dtype=torch.int64).reshape(K, 4),
        kind=torch.tensor([a.kind for a in actions], dtype=torch.int32).reshape(K),
        arg0=torch.tensor([a.arg0 for a in actions], dtype=torch.int32).reshape(K),
        arg1=torch.tensor([a.arg1 for a in actions], dtype=torch.int64).reshape(K),
        addr=torch.tensor([address_to_limbs(a.addr) for a in actions], dtype=torch.int64).reshape(K, 4))


def state_tensors(contracts: List[ReferenceContract], A: int, N: int) -> Dict[str, torch.Tensor]:
    """The golden state in the device layout: 4 int64 limbs per address, one vote column per receiving admin
    with bit e = vote_matrix[e][receiver]."""
    B = len(contracts)
    oracle_addr = torch.tensor([[address_to_limbs(a) for a in c.get_oracle_list()] for c in contracts],
                               dtype=torch.int64).reshape(B, N, 4)
    votes = torch.tensor([[wrap(sum(int(c.vote_matrix[e][r]) << e for e in range(A))) for r in range(A)]
                          for c in contracts], dtype=torch.int64).reshape(B, A)
    tag = torch.tensor([[0 if p is None else 1 for p in c.propositions] for c in contracts], dtype=torch.int8)
    idx = torch.tensor([[0 if p is None else p[0] for p in c.propositions] for c in contracts], dtype=torch.int32)
    paddr = torch.tensor([[address_to_limbs(0 if p is None else p[1]) for p in c.propositions] for c in contracts],
                         dtype=torch.int64).reshape(B, A, 4)
    return dict(oracle_addr=oracle_addr, votes=votes, prop_tag=tag.reshape(B, A), prop_idx=idx.reshape(B, A),
                prop_addr=paddr)


def build(name: str, A: int, N: int, majority: int, addr: Addresses, launches: List[List[Action]],
          cls=Contract, with_lists: bool = True) -> Built:
    B = len(addr.admins)
    contracts = [new_contract(cls, addr.admins[b], addr.oracles[b], majority) for b in range(B)]
    stages = []
    for actions in launches:
        res = [apply_golden(contracts, a) for a in actions]
        lists = None
        if with_lists:
            lists = [(c.get_oracle_list(), list(c.propositions), [row[:] for row in c.vote_matrix]) for c in contracts]
        stages.append(Stage(action_tensors(actions), torch.tensor([r[0] for r in res], dtype=torch.int32),
                            torch.tensor([r[1] for r in res], dtype=torch.uint8), state_tensors(contracts, A, N),
                            lists))
    return Built(name, A, N, majority, B, addr, stages, launches)


# ------------------------------------------------------------------------------------------------ random cases
class Shape(NamedTuple):
    A: int
    N: int
    majority: int
    B: int
    seed: int


K_RANDOM = 3000
# (the seeds: ones for which every case applies a replacement and meets each status code,
# tests/test_governance_model.py::test_random_cases_are_not_empty)
SHAPES = (Shape(1, 4, 1, 8, 1), Shape(2, 7, 2, 8, 2), Shape(5, 9, 3, 8, 3), Shape(33, 7, 17, 4, 4),
          Shape(64, 7, 33, 3, 5), Shape(64, 7, 1, 4, 6), Shape(64, 300, 2, 3, 7))


def shape_id(s: Shape) -> str:
    return f"A{s.A}-N{s.N}-m{s.majority}"


def random_actions(rng: random.Random, s: Shape, ad: Addresses, K: int) -> List[Action]:
    A, N = s.A, s.N
    out = []
    for _ in range(K):
        b = rng.randrange(s.B)
        u = rng.random()
        if u < 0.80:
            caller = ad.admins[b][rng.randrange(A)]
        elif u < 0.90:
            caller = ad.near_admins[b][rng.randrange(4)]         # an admin's address but for one limb
        else:
            caller = rng.choice(ad.oracles[b] + ad.spares[b])
        if rng.random() < 0.30:
            addr = rng.choice(ad.spares[b]) if rng.random() < 0.75 else rng.choice(ad.oracles[b])
            if rng.random() < 0.15:      # None (the index and the address travel along and must be ignored)
                out.append(Action(b, caller, PROPOSE, 0, N + 5, addr))
            else:
                out.append(Action(b, caller, PROPOSE, 1, rng.randrange(-1, N + 1), addr))
        else:
            v = rng.random()
            which = 0 if v < 0.42 else A - 1 if v < 0.84 else rng.randrange(A) if v < 0.92 else A
            out.append(Action(b, caller, VOTE, which, int(rng.random() < 0.85), 0))
    return out


@functools.lru_cache(maxsize=None)
def random_case(s: Shape, K: int = K_RANDOM, cls=Contract) -> Built:
    rng = random.Random(s.seed)
    ad = make_addresses(rng, s.B, s.A, s.N)
    return build(shape_id(s), s.A, s.N, s.majority, ad, [random_actions(rng, s, ad, K)], cls)


# ------------------------------------------------------------------------------------------------ directed cases
@functools.lru_cache(maxsize=None)
def directed_case(cls=Contract) -> Built:
    """A = 64 with majority 64 (random actions apply nothing there).  One scenario per instance, interleaved in
    one batch; ``directed_marks`` names the actions the model test looks at."""
    A, N, B = 64, 7, 6
    rng = random.Random(64)
    ad = make_addresses(rng, B, A, N)
    adm, orc, sp = ad.admins, ad.oracles, ad.spares
    prop = lambda b, a, idx, addr: Action(b, adm[b][a], PROPOSE, 1, idx, addr)       # noqa: E731
    none = lambda b, a: Action(b, adm[b][a], PROPOSE, 0, 0, 0)                        # noqa: E731
    vote = lambda b, a, w, s=1: Action(b, adm[b][a], VOTE, w, s, 0)                   # noqa: E731
    runs: List[List[Action]] = [[] for _ in range(B)]
    # 0: all 64 admins vote for admin 63's proposition; it applies on the 64th vote (admin 62's) and not before
    runs[0] = [prop(0, 63, 2, sp[0][0])] + [vote(0, a, 63) for a in range(63)]
    # 1: receiver 0, emitter 63 votes last (bit 63 of column 0 decides)
    runs[1] = [prop(1, 0, 6, sp[1][1])] + [vote(1, a, 0) for a in range(1, 64)]
    # 2: emitter 63 votes early and withdraws at 63 votes; admin 1's vote then makes 63, not 64; 63 votes again
    runs[2] = ([prop(2, 0, 0, sp[2][2]), vote(2, 63, 0)] + [vote(2, a, 0) for a in range(2, 63)] +
               [vote(2, 63, 0, 0), vote(2, 1, 0), vote(2, 63, 0)])
    # 3: Some -> None -> the 64th vote reverts (unwrap on None) and its bit is not stored; a new proposition
    #    clears the column
    runs[3] = ([prop(3, 5, 1, sp[3][3]), none(3, 5)] + [vote(3, a, 5) for a in range(64) if a != 5] +
               [prop(3, 5, 1, sp[3][3])])
    # 4: a new address equal to an oracle in three limbs is accepted (once per limb); an oracle's address is not
    runs[4] = ([prop(4, L, L, sp[4][N_SPARES + L]) for L in range(4)] + [prop(4, 9, 3, orc[4][o]) for o in range(N)] +
               [Action(4, ad.near_admins[4][L], VOTE, 0, 1, 0) for L in range(4)])
    # 5: no such instance: -3, B, B + 3 (a real admin's address of instance 5, a real action)
    runs[5] = [Action(i, adm[5][0], PROPOSE, 1, 0, sp[5][0]) for i in (-3, B, B + 3)] + \
              [Action(i, adm[5][1], VOTE, 0, 1, 0) for i in (-3, B, B + 3)]
    actions: List[Action] = []
    for k in range(max(len(r) for r in runs)):         # interleaved: each instance's order is kept
        actions += [r[k] for r in runs if k < len(r)]
    return build("directed-A64-m64", A, N, 64, ad, [actions], cls)


@functools.lru_cache(maxsize=None)
def empty_case() -> Built:
    """K = 0."""
    ad = make_addresses(random.Random(0), 3, 5, 9)
    return build("K0", 5, 9, 3, ad, [[]])


# ------------------------------------------------------------------------------------------------ unique slices
SLICE_B = 640


@functools.lru_cache(maxsize=None)
def slice_case(s: Shape) -> Built:
    """The unordered op (one lane per action, instances unique): SLICE_B instances of the shape at majority 2,
    in shuffled order, two launches -- a proposition everywhere, then the deciding vote."""
    A, N, B = s.A, s.N, SLICE_B
    rng = random.Random(1000 + s.seed)
    ad = make_addresses(rng, B, A, N)
    first, second = [], []
    order1, order2 = list(range(B)), list(range(B))
    rng.shuffle(order1); rng.shuffle(order2)
    who = {}
    for b in order1:
        me = (A - 1, 0, b % A)[b % 3]
        who[b] = me
        u = b % 16
        caller = ad.near_admins[b][b % 4] if u == 13 else ad.admins[b][me]
        addr = (ad.oracles[b][b % N] if u == 11 else ad.spares[b][b % (N_SPARES + 4)])
        idx = -1 if u == 7 else N if u == 9 else b % N
        first.append(Action(b, caller, PROPOSE, 0 if u == 5 else 1, idx, addr))
    for b in order2:
        me, u = who[b], b % 16
        voter = (me + 1 + b % 5) % A
        caller = ad.near_admins[b][(b + 1) % 4] if u == 3 else ad.admins[b][voter]
        which = A if u == 6 else me
        second.append(Action(b, caller, VOTE, which, 0 if u == 10 else 1, 0))
    return build("slice-" + shape_id(s), A, N, 2, ad, [first, second], with_lists=False)


# ------------------------------------------------------------------------------------------------ running a case
def setup(gov, built: Built):
    """``gov``: a svoc.governance.Governance(B, A, N, device, True, majority) made by the test."""
    assert (gov.B, gov.A, gov.N, gov.majority, gov.enable) == (built.B, built.A, built.N, built.majority, True)
    gov.set_addresses(built.addr.admins, built.addr.oracles)
    return gov


def compare(gov, st: torch.Tensor, ap: torch.Tensor, stage: Stage, tag: str) -> None:
    st, ap = st.cpu(), ap.cpu()
    bad = (st != stage.status).nonzero().flatten()
    assert bad.numel() == 0, (tag, "status", bad[:5].tolist(), st[bad[:5]].tolist(), stage.status[bad[:5]].tolist())
    assert torch.equal(ap, stage.applied), (tag, "applied", (ap != stage.applied).nonzero().flatten()[:5].tolist())
    want = stage.state
    for name in ("oracle_addr", "votes", "prop_tag"):
        got = getattr(gov, name).cpu()
        assert torch.equal(got, want[name]), (tag, name, (got != want[name]).nonzero()[:5].tolist())
    some = want["prop_tag"] == 1
    for name in ("prop_idx", "prop_addr"):        # the raw proposition of every admin whose tag is 1
        got = getattr(gov, name).cpu()
        assert torch.equal(got[some], want[name][some]), (tag, name)
    if stage.lists is not None:
        for b, (oracles, props, vm) in enumerate(stage.lists):
            assert gov.oracle_list(b) == oracles, (tag, b, "oracle_list")
            assert gov.propositions(b) == props, (tag, b, "propositions")
            assert gov.vote_matrix(b) == vm, (tag, b, "vote_matrix")


def check_ordered(gov, built: Built) -> None:
    """Every launch through submit_batch (governance_seq: any number of actions per instance, in order)."""
    setup(gov, built)
    for k, stage in enumerate(built.stages):
        st, ap = gov.submit_batch(**stage.actions)
        compare(gov, st, ap, stage, f"{built.name} launch {k} (submit_batch)")


def check_unordered(gov, built: Built) -> None:
    """Every launch through submit_tensors (governance: one lane per action, instances unique)."""
    setup(gov, built)
    for k, stage in enumerate(built.stages):
        inst = stage.actions["inst"]
        assert inst.unique().numel() == inst.numel()
        st, ap = gov.submit_tensors(**{n: t.to(gov.device) for n, t in stage.actions.items()})
        compare(gov, st, ap, stage, f"{built.name} launch {k} (submit_tensors)")
