"""Cases and plain models for the round bookkeeping (csrc/include/svoc/bookkeeping.hpp, csrc/kernels/
bookkeeping.hip): round_prologue / round_epilogue against torch integer ops, and the commit of the staged c1
(commit_rows / commit_words, reached through exact_round in mode 0) against svoc.reference.consensus_round.

No svoc code except svoc.reference and svoc.status; CPU only.  tests/test_bookkeeping_model.py pins cases and
models to the CPU ops, tests/test_bookkeeping_gpu.py runs the same cases through the HIP kernels.

Model of one prologue + epilogue:
    active = (n_active == N) & (touched != 0 if only_touched else True)
    ok     = active & (status == 0)
    consensus_active[ok] = 1, every other entry unchanged;  touched = 0 everywhere
    acc   += [sum_ok rel2_fx, #ok, #active, #(active & ~ok)]
    rel2_fx: fast (fp32 rel)  floor(clamp(rel[:, 1], 0, 1) as float64 * 2^32 + 0.5)
             exact (int64 rel) max(rel[:, 1], 0)

Known untested edge: a NaN rel[:, 1] under an OK status.  The float -> integer conversion of a NaN is undefined
(host and device may differ), and no round kernel produces it: an OK round has a finite reliability.  NaN does
appear here under reverted and inactive instances, where it must not be read into the sum.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple

import torch

from svoc.reference import round_status
from svoc.status import Status

N_ORACLES = 7
CANARY = 0xA5            # byte canary around sliced views
PAD_LO, PAD_HI = 3, 2    # a view t[3 : 3 + B] of a buffer of B + 5 entries: odd b0
ACC0 = (5, 7, 11, 13)    # acc's contents before the first call
STATUSES = (0, 6, 32, 33, -1)


class BookCase(NamedTuple):
    B: int
    fast: bool           # rel dtype: fp32 (fast) or int64 (exact)
    only_touched: bool
    as_bool: bool        # consensus_active / touched / active as bool tensors (else uint8)
    sliced: bool         # every tensor is a view [PAD_LO : PAD_LO + B] of a larger buffer
    acc: bool            # False: acc = None


# 131072 + 300: the epilogue runs 512 workgroups x 256 lanes, so 300 lanes take a second grid-stride pass
BOOK_BS = (1, 255, 256, 257, 131072 + 300)


def book_matrix() -> List[BookCase]:
    out = []
    for B in BOOK_BS:
        for fast in (True, False):
            for ot in (True, False):
                for as_bool in (False, True):
                    out.append(BookCase(B, fast, ot, as_bool, sliced=(fast ^ ot ^ as_bool), acc=True))
            out.append(BookCase(B, fast, True, as_bool=not fast, sliced=fast, acc=False))
    return out


def book_id(c: BookCase) -> str:
    return (f"B{c.B}-{'fast' if c.fast else 'exact'}-{'touched' if c.only_touched else 'all'}-"
            f"{'bool' if c.as_bool else 'u8'}-{'view' if c.sliced else 'whole'}-{'acc' if c.acc else 'noacc'}")


# ------------------------------------------------------------------------------------------------ the models
def model_active(n_active: torch.Tensor, touched_u8: torch.Tensor, N: int, only_touched: bool) -> torch.Tensor:
    a = n_active == N
    if only_touched:
        a = a & (touched_u8 != 0)
    return a


def model_rel2_fx(rel: torch.Tensor, ok: torch.Tensor) -> torch.Tensor:
    x = rel[ok, 1]
    if rel.dtype == torch.float32:
        return torch.floor(x.clamp(0.0, 1.0).to(torch.float64) * 4294967296.0 + 0.5).to(torch.int64)
    return x.clamp(min=0)


def model_epilogue(active: torch.Tensor, status: torch.Tensor, rel: torch.Tensor, ca_u8: torch.Tensor):
    """-> (consensus_active as uint8, the four counters to add to acc)."""
    ok = active & (status == 0)
    ca = ca_u8.clone()
    ca[ok] = 1
    add = torch.stack([model_rel2_fx(rel, ok).sum(), ok.sum(), active.sum(), (active & ~ok).sum()]).to(torch.int64)
    return ca, add


# ------------------------------------------------------------------------------------------------ the data
@functools.lru_cache(maxsize=None)
def book_data(c: BookCase):
    """Two consecutive rounds of inputs, the initial consensus_active, and what the models expect after each."""
    g = torch.Generator().manual_seed(17 * c.B + 8 * c.fast + 4 * c.only_touched + 2 * c.as_bool + c.acc)
    B, N = c.B, N_ORACLES

    def pick(values, weights, dtype):
        idx = torch.multinomial(torch.tensor(weights, dtype=torch.float64), B, replacement=True, generator=g)
        return torch.tensor(values, dtype=dtype)[idx]

    ca = pick((0, 1), (0.7, 0.3), torch.uint8)
    init_ca = ca.clone()
    acc = torch.tensor(ACC0, dtype=torch.int64)
    rounds = []
    for _ in range(2):
        n_active = pick((N, N - 1, N + 1), (0.8, 0.1, 0.1), torch.int32)
        touched = (pick((0, 1), (0.3, 0.7), torch.uint8) if c.as_bool
                   else pick((0, 1, 2, 255), (0.3, 0.3, 0.2, 0.2), torch.uint8))
        status = pick(STATUSES, (0.6, 0.1, 0.1, 0.1, 0.1), torch.int32)      # (stale 0s under active == 0 too)
        if c.fast:
            # mostly near 1 (each adds about 2^32: one wave's partial sum needs the high half of the 64-bit
            # shuffle), the clamp edges, and the largest float below 1
            rel1 = pick((1.0, 1.0 - 2.0 ** -24, 0.0, -0.25, 1.5, 0.999, 0.9375, 2.0 ** -33, 2.0 ** -34),
                        (0.2, 0.2, 0.05, 0.05, 0.05, 0.2, 0.15, 0.05, 0.05), torch.float32)
            rel = torch.stack([torch.full((B,), 0.123, dtype=torch.float32), rel1], 1).contiguous()
        else:
            rel1 = pick((1_000_000, 999_999, 0, -5, 1, (1 << 40) + 3, 123_456), (0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1),
                        torch.int64)
            rel = torch.stack([torch.full((B,), 777, dtype=torch.int64), rel1], 1).contiguous()
        active = model_active(n_active, touched, N, c.only_touched)
        if c.fast:          # NaN where the round did not commit: never read into the sum
            rel[~(active & (status == 0)), 1] = float("nan")
        ca, add = model_epilogue(active, status, rel, ca)
        acc = acc + add
        rounds.append(dict(n_active=n_active, touched=touched, status=status, rel=rel, want_active=active.to(torch.uint8),
                           want_ca=ca, want_acc=acc))
    return init_ca, rounds


class _Buf:
    """A tensor of B rows, whole or as the view [PAD_LO : PAD_LO + B] of a canary-filled buffer."""

    def __init__(self, data: torch.Tensor, sliced: bool, device: str, as_bool: bool = False):
        B = data.shape[0]
        lo, hi = (PAD_LO, PAD_HI) if sliced else (0, 0)
        raw = torch.empty((B + lo + hi,) + tuple(data.shape[1:]), dtype=data.dtype)
        raw.view(torch.uint8).fill_(CANARY)
        raw[lo:lo + B] = data
        self.raw = raw.to(device)
        self.lo, self.B = lo, B
        self.view = self.raw[lo:lo + B]
        self.arg = self.view.view(torch.bool) if as_bool else self.view

    def set(self, data: torch.Tensor) -> None:
        self.view.copy_(data.to(self.view.device))

    def canary_intact(self) -> bool:
        r = self.raw.cpu()
        edge = torch.cat([r[:self.lo].reshape(-1), r[self.lo + self.B:].reshape(-1)])
        return bool((edge.view(torch.uint8) == CANARY).all())


def check_book(c: BookCase, device: str, ops) -> None:
    """Two consecutive prologue + epilogue calls on ``device``; every output byte against the model."""
    init_ca, rounds = book_data(c)
    B = c.B
    r0 = rounds[0]
    bufs = dict(n_active=_Buf(r0["n_active"], c.sliced, device), touched=_Buf(r0["touched"], c.sliced, device, c.as_bool),
                active=_Buf(torch.full((B,), 1, dtype=torch.uint8), c.sliced, device, c.as_bool),
                status=_Buf(r0["status"], c.sliced, device), rel=_Buf(r0["rel"], c.sliced, device),
                ca=_Buf(init_ca, c.sliced, device, c.as_bool))
    acc = torch.tensor(ACC0, dtype=torch.int64, device=device) if c.acc else None
    for k, r in enumerate(rounds):
        for name in ("n_active", "touched", "status", "rel"):
            bufs[name].set(r[name])
        # active pre-filled with the complement of what is expected: the prologue writes every entry
        bufs["active"].set(1 - r["want_active"])
        ops.round_prologue(bufs["n_active"].arg, bufs["touched"].arg, N_ORACLES, c.only_touched, bufs["active"].arg)
        assert torch.equal(bufs["active"].view.cpu(), r["want_active"]), (book_id(c), k, "active")
        assert torch.equal(bufs["touched"].view.cpu(), r["touched"]), (book_id(c), k, "the prologue wrote touched")
        ops.round_epilogue(bufs["active"].arg, bufs["status"].arg, bufs["rel"].arg, bufs["ca"].arg, bufs["touched"].arg,
                           acc)
        assert torch.equal(bufs["ca"].view.cpu(), r["want_ca"]), (book_id(c), k, "consensus_active")
        assert not bool(bufs["touched"].view.cpu().any()), (book_id(c), k, "touched not cleared")
        assert torch.equal(bufs["active"].view.cpu(), r["want_active"]), (book_id(c), k, "the epilogue wrote active")
        if acc is not None:
            assert acc.cpu().tolist() == r["want_acc"].tolist(), (book_id(c), k, acc.cpu().tolist(),
                                                                   r["want_acc"].tolist())
    for name, b in bufs.items():
        assert b.canary_intact(), (book_id(c), name, "bytes outside the view changed")


# ================================================================================================ commit cases
# exact_round in mode 0 stages c1 and commits 2 * D 32-bit words per instance where the round ran and succeeded.
# Every D routes there (csrc/bindings/torch_ops.cpp, exact_round_hip: the staging and the commit do not depend on
# which round kernel runs), so the issue's D values are used unchanged.
COMMIT_N, COMMIT_F = 5, 1
SENTINEL = -(1 << 62) + 12345
N_GOLDEN = 8
REVERT_AT = 2            # the zero-variance round among the golden ones (inside the first 6: B = 6 cases see it)
INACTIVE_EVERY, INACTIVE_AT = 5, 3   # active[b] = 0 where b % 5 == 3 (coprime with N_GOLDEN: every pairing occurs)


class CommitCase(NamedTuple):
    B: int
    D: int
    odd_view: bool       # c1 is rows [1 : 1 + B] of a [B + 2, D] buffer: with D = 129 its base is 8-byte aligned only
    path: str


COMMIT_CASES = (
    CommitCase(6, 3, False, "commit_words, 6 words"),
    CommitCase(350_000, 3, False, "commit_words grid-stride: B * 6 > 8192 * 256"),
    CommitCase(6, 128, False, "commit_rows, 256 words, 16-byte vectors"),
    CommitCase(6, 129, False, "commit_rows, 258 words, word copies"),
    CommitCase(8_200, 128, False, "commit_rows grid-stride: B > 8192"),
    CommitCase(6, 129, True, "commit_rows, 258 words, destination 8-byte aligned only"),
)


def commit_id(c: CommitCase) -> str:
    return f"B{c.B}-D{c.D}{'-oddview' if c.odd_view else ''}"


class Golden(NamedTuple):
    values: torch.Tensor     # int64 [N_GOLDEN, N, D]
    status: List[int]
    c1: torch.Tensor         # int64 [N_GOLDEN, D] (zeros where the round reverts)


@functools.lru_cache(maxsize=None)
def golden_rounds(D: int) -> Golden:
    g = torch.Generator().manual_seed(4000 + D)
    v = 500_000 + torch.randint(-60_000, 60_001, (N_GOLDEN, COMMIT_N, D), generator=g)
    v[:, 0] = torch.randint(0, 1_000_001, (N_GOLDEN, D), generator=g)        # one oracle anywhere in [0, 1]
    v[REVERT_AT, :, D // 2] = 421_337                                          # a column without variance
    status, c1 = [], torch.zeros(N_GOLDEN, D, dtype=torch.int64)
    for i in range(N_GOLDEN):
        st, res = round_status(v[i].tolist(), COMMIT_F, True)
        while i != REVERT_AT and st != Status.OK:      # (wide rounds: some column's Newton sqrt divides by zero)
            v[i, 1:] = 500_000 + torch.randint(-60_000, 60_001, (COMMIT_N - 1, D), generator=g)
            st, res = round_status(v[i].tolist(), COMMIT_F, True)
        status.append(int(st))
        if res is not None:
            c1[i] = torch.tensor(res.c1, dtype=torch.int64)
    return Golden(v, status, c1)


def check_commit(c: CommitCase, device: str, ops) -> None:
    gold = golden_rounds(c.D)
    B, N, D = c.B, COMMIT_N, c.D
    which = torch.arange(B) % N_GOLDEN
    active = (torch.arange(B) % INACTIVE_EVERY != INACTIVE_AT)
    st_g = torch.tensor(gold.status, dtype=torch.int32)[which]
    commit = active & (st_g == int(Status.OK))
    want = torch.where(commit[:, None], gold.c1[which], torch.full((B, D), SENTINEL, dtype=torch.int64))
    values = gold.values[which].contiguous().to(device)
    f = dict(device=device, dtype=torch.int64)
    lo = 1 if c.odd_view else 0
    c1_raw = torch.full((B + 2 * lo, D), SENTINEL, **f)
    c1 = c1_raw[lo:lo + B]
    cons, skew, kurt = (torch.zeros(B, D, **f) for _ in range(3))
    rel, qr = torch.zeros(B, 2, **f), torch.zeros(B, N, **f)
    reliable = torch.zeros(B, N, dtype=torch.uint8, device=device)
    status = torch.full((B,), -1, dtype=torch.int32, device=device)
    ops.exact_round(values, active.to(torch.uint8).to(device), COMMIT_F, True, 0, c1, cons, skew, kurt, rel, qr,
                    reliable, status, False)
    got_st = status.cpu()
    assert torch.equal(got_st[active], st_g[active]), (commit_id(c), "status")
    got = c1_raw.cpu()
    assert torch.equal(got[lo:lo + B], want), (commit_id(c), (got[lo:lo + B] != want).nonzero()[:5].tolist())
    if lo:
        assert bool((got[0] == SENTINEL).all()) and bool((got[-1] == SENTINEL).all()), (commit_id(c), "border rows")
