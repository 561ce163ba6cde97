"""Shared cases of the authenticated-update tests (test_auth_updates.py, test_auth_updates_gpu.py): the planted
address-lookup batches with their Python first-match reference, and the seeded three-phase update stream with
its ``ReferenceContract`` replay."""
import random

import torch

from svoc import reference as ref
from svoc.api import ConsensusService
from svoc.codec import address_to_limbs, addresses_to_limbs
from svoc.config import ConsensusConfig
from svoc.status import ConsensusRevert, Status

LOOKUP_M = [1, 2, 3, 7, 9, 31, 33, 64, 65, 100, 256, 1500, 4096]
LOOKUP_B = 3
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def first_match(table, inst, addr):
    """The contract's linear scan (contract.cairo:505-518) over plain lists."""
    out = []
    for b, a in zip(inst, addr):
        r = -1
        if 0 <= b < len(table):
            for i, row in enumerate(table[b]):
                if row == a:
                    r = i
                    break
        out.append(r)
    return out


def lookup_case(M, K=203, seed=0):
    """(table [3, M, 4], inst [K], addr [K, 4], expected [K]) as tensors.  Instances 0 / 1: random full-range
    limbs (negative ones included) with planted duplicates -- inside one 64-entry chunk (instance 0) and across
    two chunks (instance 1, M > 64) -- and an entry of extreme limbs; instance 2: the zero-initialised table.
    The lookups: every planted entry, the last entry, one-limb-off variants for each of the four limbs, the
    zero address, the instances -1 / B / B + 3, then random known and unknown callers up to K, shuffled."""
    rng = random.Random(seed * 7919 + M)
    B = LOOKUP_B
    limb = lambda: rng.randint(I64_MIN, I64_MAX)  # noqa: E731
    table = [[[limb() for _ in range(4)] for _ in range(M)] for _ in range(2)] + [[[0] * 4 for _ in range(M)]]
    extreme = [I64_MIN, -1, I64_MAX, I64_MIN]
    table[0][M // 2] = list(extreme)
    dups = []
    if M >= 2:
        i, j = (1, 2) if M >= 3 else (0, 1)            # one chunk
        table[0][j] = list(table[0][i])
        dups.append((0, i, j))
    if M > 64:
        i, j = 5, (69 if M > 69 else M - 1)            # two chunks
        table[1][j] = list(table[1][i])
        dups.append((1, i, j))
        if M > 1400:                                   # far apart: many chunks between
            table[1][M - 3] = list(table[1][70])
            dups.append((1, 70, M - 3))
    q = []                                             # (inst, addr)
    for b, i, j in dups:                                # the lowest index wins
        q.append((b, list(table[b][i])))
        q.append((b, list(table[b][j])))
    for b in (0, 1):
        q.append((b, list(table[b][M - 1])))           # the last entry
        q.append((b, list(table[b][0])))
        src = table[b][M - 1]
        for l in range(4):                             # equal on three limbs only
            a = list(src)
            a[l] ^= 1
            q.append((b, a))
            a = list(src)
            a[l] ^= I64_MIN                            # the top bit alone
            q.append((b, a))
    q.append((0, list(extreme)))
    q.append((0, [0, -1, I64_MAX, I64_MIN]))
    q.append((2, [0, 0, 0, 0]))                        # zero address, zero table -> 0
    q.append((0, [0, 0, 0, 0]))
    q.append((2, [0, 0, 1, 0]))
    for b in (-1, B, B + 3):
        q.append((b, list(table[0][0])))               # unknown instance: -1, the table is not read
    q = q[:K]
    while len(q) < K:
        b = rng.randrange(B)
        r = rng.random()
        if r < 0.6:
            q.append((b, list(table[b][rng.randrange(M)])))
        elif r < 0.8:
            q.append((rng.choice([-1, B, B + 3, -(1 << 40), 1 << 40]), list(table[0][rng.randrange(M)])))
        else:
            q.append((b, [limb() for _ in range(4)]))
    rng.shuffle(q)
    inst = [b for b, _ in q]
    addr = [a for _, a in q]
    want = first_match(table, inst, addr)
    t = lambda x, shape: torch.tensor(x, dtype=torch.int64).reshape(shape)  # noqa: E731
    return t(table, (B, M, 4)), t(inst, (K,)), t(addr, (K, 4)), t(want, (K,))


# ---- the three-phase authenticated stream (exact: 7 oracles x 2 dimensions, B = 4) ---------------------------

N, D, F, B = 7, 2, 2, 4
ADMINS = [0x416B61736869, 0x4F7A75, 0x48696775636869]
UNKNOWN = (1 << 251) + 12345


def oracle_book(n=N, batch=B, seed=0):
    """Per-instance oracle addresses: 252-bit values, every limb in use, distinct across instances."""
    rng = random.Random(1000 + seed)
    return [[rng.getrandbits(252) | (1 << 251) for _ in range(n)] for _ in range(batch)]


def new_oracle(b):
    return (1 << 250) + 0xABC0 + b


class Stream:
    """phase1: every oracle submits (re-submissions in between; the last submission activates the consensus);
    gov: a proposition + the second vote replace oracle 4 of instances 1 and 3; phase3: the replaced oracle's old
    address, its new one, an unknown caller with an out-of-interval prediction, an unknown instance, a prediction
    that reverts its round (instance 2: every oracle at one value in column 0), plain updates around them;
    phase4: three updates per instance laid out b * 3 + k with unknown callers inside the layout.
    Items are (instance, caller address, wsad prediction)."""

    def __init__(self, seed=5):
        rng = random.Random(seed)
        val = lambda: rng.randint(0, 1_000_000)  # noqa: E731
        self.book = oracle_book()
        book = self.book
        seqs = []
        for b in range(B):
            first = list(range(N - 1))
            rng.shuffle(first)
            seq = first[:4] + [first[0]] + first[4:] + [first[2]] + [N - 1]
            rows = []
            for o in seq:
                v = [val(), val()]
                if b == 2:      # column 0: oracles 0..4 at one value, 5 and 6 apart (phase 3 closes the gap)
                    v[0] = {5: 300_000, 6: 700_000}.get(o, 500_000)
                rows.append((b, book[b][o], v))
            seqs.append(rows)
        self.phase1 = self._interleave(rng, seqs)
        self.gov = []
        for b in (1, 3):
            self.gov += [("propose", b, ADMINS[0], (4, new_oracle(b))), ("vote", b, ADMINS[1], 0, True)]
        self.phase3 = [
            (0, book[0][1], [val(), val()]),
            (1, book[1][4], [val(), val()]),                  # replaced: NOT_ORACLE
            (1, new_oracle(1), [val(), val()]),               # its new address: accepted
            (0, UNKNOWN, [1_000_001, val()]),                 # INTERVAL_INPUT comes before NOT_ORACLE
            (B + 3, book[0][0], [val(), val()]),              # unknown instance
            (2, book[2][5], [500_000, val()]),
            (2, book[2][6], [500_000, val()]),                # column 0 constant: the round reverts
            (3, new_oracle(1), [val(), val()]),               # instance 1's new oracle is nobody in instance 3
            (2, book[2][6], [600_000, val()]),
            (3, new_oracle(3), [val(), -5]),                  # a known caller out of the interval
            (3, new_oracle(3), [val(), val()]),
            (-1, book[3][0], [val(), val()]),
        ]
        self.phase4 = []
        for b in range(B):
            callers = [self._book_after(b)[rng.randrange(N)] for _ in range(3)]
            callers[b % 3] = UNKNOWN + b if b != 1 else book[1][4]   # unknown callers inside the layout
            for k, c in enumerate(callers):
                v = [val(), val()]
                if b == 0 and k == 2:
                    v[1] = 2_000_000
                self.phase4.append((b, c, v))

    def _book_after(self, b):
        r = list(self.book[b])
        if b in (1, 3):
            r[4] = new_oracle(b)
        return r

    @staticmethod
    def _interleave(rng, seqs):
        cur = [0] * len(seqs)
        out = []
        while any(c < len(s) for c, s in zip(cur, seqs)):
            b = rng.choice([i for i, s in enumerate(seqs) if cur[i] < len(s)])
            out.append(seqs[b][cur[b]])
            cur[b] += 1
        return out

    def batches(self):
        return [("phase1", self.phase1, None), ("gov", self.gov, None), ("phase3", self.phase3, None),
                ("phase4", self.phase4, 3)]

    def resolve(self, phase_items, replaced):
        """Python lookup: the oracle index of every item's caller (-1: unknown caller or instance)."""
        out = []
        for b, c, _ in phase_items:
            lst = (self._book_after(b) if replaced else self.book[b]) if 0 <= b < B else []
            out.append(lst.index(c) if c in lst else -1)
        return out

    def replay_reference(self):
        """One ReferenceContract per instance -> (contracts, {phase: [Status]})."""
        cs = [ref.ReferenceContract(ADMINS, True, 2, F, True, 0, D, self.book[b]) for b in range(B)]
        st = {}
        for name, items, _ in self.batches():
            if name == "gov":
                for act in items:
                    c = cs[act[1]]
                    if act[0] == "propose":
                        c.update_proposition(act[2], act[3])
                    else:
                        c.vote_for_a_proposition(act[2], act[3], act[4])
                continue
            st[name] = []
            for b, caller, v in items:
                if not 0 <= b < B:
                    # no such contract: the batched paths report the interval error first, then NOT_ORACLE
                    bad = any(not 0 <= x <= 1_000_000 for x in v)
                    st[name].append(Status.INTERVAL_INPUT if bad else Status.NOT_ORACLE)
                    continue
                try:
                    st[name].append(cs[b].update_prediction(caller, v))
                except ConsensusRevert as e:
                    st[name].append(e.status)
        return cs, st


def service(device, mode="exact", storage=None, n=N, d=D, f=F, batch=B, book=None):
    cfg = ConsensusConfig(n_oracles=n, dimension=d, n_failing_oracles=f, constrained=True, n_admins=len(ADMINS),
                          required_majority=2, enable_oracle_replacement=True)
    return ConsensusService(cfg, batch, [ADMINS] * batch, book or oracle_book(n, batch), device=device, mode=mode,
                            storage=storage)


def tensors(items, device, mode):
    inst = torch.tensor([b for b, _, _ in items], dtype=torch.int64, device=device)
    caller = addresses_to_limbs((c for _, c, _ in items), device=device)
    vals = torch.tensor([v for _, _, v in items], dtype=torch.int64)
    if mode == "fast":
        vals = vals.to(torch.float32) / 1_000_000
    return inst, caller, vals.to(device)


def run_exact_stream(svc, stream, strided=True):
    """The stream through update_batch / governance -> {phase: [Status]}."""
    dev = svc.engine.device
    st = {}
    for name, items, k in stream.batches():
        if name == "gov":
            codes, applied = svc.governance(items)
            assert codes == [Status.OK] * len(items) and applied == [False, True, False, True]
            continue
        inst, caller, vals = tensors(items, dev, "exact")
        out = svc.update_batch(inst, caller, vals, updates_per_instance=k if strided else None)
        assert out.dtype == torch.int32 and out.device.type == dev.type
        st[name] = [Status(s) for s in out.cpu().tolist()]
    return st


def check_against_contracts(svc, contracts):
    e = svc.engine
    for b, c in enumerate(contracts):
        assert e.values[b, :, :D].tolist() == c.values, b
        assert e.enabled[b].bool().tolist() == [o.enabled for o in c.oracles], b
        assert int(e.n_active[b]) == c.n_active_oracles, b
        assert e.reliable[b].bool().tolist() == [o.reliable for o in c.oracles], b
        assert bool(e.consensus_active[b]) == c.consensus_active(), b
        assert e.consensus[b].tolist() == c.get_consensus_value(), b
        assert [int(x) for x in e.rel[b]] == [c.rel1, c.rel2], b
        assert e.skew[b].tolist() == c.skewness and e.kurt[b].tolist() == c.kurtosis, b
        assert svc.gov.oracle_list(b) == c.get_oracle_list(), b


STATE = ("values", "enabled", "n_active", "reliable", "consensus_active", "consensus", "rel", "skew", "kurt", "status")


def limbs(addr):
    return torch.tensor(address_to_limbs(addr), dtype=torch.int64)
