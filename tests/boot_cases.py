"""Cases and an independent model for torch.ops.svoc.bootstrap_oracles (csrc/include/svoc/bootstrap.hpp, the
CPU twin in csrc/bindings/generator_ops.cpp and csrc/kernels/oracle_gen.hip).

The model shares no code with the op: splitmix64 over Python ints masked to 64 bits, the three draws
(``uniform``, ``below``) and the two key formulas written out from bootstrap.hpp's comments, a Fisher-Yates slot
permutation, a partial Fisher-Yates for the ``min(subset, C)`` distinct comments, and every float32 step done in
numpy float32 in the kernel's order (the D label scores summed left to right, each ``s / tot``, the accumulation
over the picks, the final ``/ float32(k)``).  fp32 add and divide are correctly rounded on both sides and no step
is a multiply-add, so the comparison is on bit patterns.

CPU only (numpy + torch tensors for the op's arguments); tests/test_bootstrap_model.py pins the model to the CPU
op and tests/test_bootstrap_gpu.py runs the same cases through the HIP kernel.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

M64 = (1 << 64) - 1
SENTINEL = -7.0          # no prediction is negative: a row never written, or written twice, shows


class Case(NamedTuple):
    W: int
    C: int
    N: int
    D: int
    f: int
    subset: int
    seed: int            # as the op takes it (int64)


def wrap_i64(x: int) -> int:
    x &= M64
    return x - (1 << 64) if x >> 63 else x


# (W, C, N, D, f, subset, seed): the deployed shape; the limits N = 256, D = 16, C = 64; one comment, one oracle,
# one label; every oracle failing and subset < C with a seed above 2^63 (passed as its int64 wrap); a negative
# seed with subset = C; subset = C = 64 with an odd N; 300 windows (= workgroups)
CASES = (
    Case(3, 30, 7, 6, 2, 10, 42),
    Case(2, 64, 256, 16, 32, 10, 7),
    Case(2, 1, 1, 1, 0, 10, 1),
    Case(2, 5, 9, 3, 9, 3, wrap_i64((1 << 63) + 5)),
    Case(2, 5, 9, 3, 0, 5, -3),
    Case(2, 64, 255, 16, 1, 64, 9),
    Case(300, 30, 64, 6, 8, 10, 7),
)


def case_id(c: Case) -> str:
    return f"W{c.W}-C{c.C}-N{c.N}-D{c.D}-f{c.f}-s{c.subset}-seed{c.seed}"


# ------------------------------------------------------------------------------------------------ the model
def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class Rng:
    def __init__(self, key: int):
        self.s = splitmix64(key & M64)

    def next(self) -> int:
        self.s = splitmix64(self.s)
        return self.s

    def uniform(self) -> np.float32:
        return np.float32(self.next() >> 40) * np.float32(2.0 ** -24)

    def below(self, n: int) -> int:
        return (self.next() >> 32) % n


def perm_key(seed: int, w: int) -> int:
    return (seed ^ ((w * 0x100000001B3) & M64) ^ 0xABCDEF) & M64


def slot_key(seed: int, w: int, j: int) -> int:
    return (seed ^ ((w << 20) & M64) ^ ((j << 4) & M64) ^ 0x5151) & M64


def model(scores: np.ndarray, label_idx: np.ndarray, c: Case) -> np.ndarray:
    """scores float32 [W, C, 28], label_idx [D] -> float32 [W, N, D] as the op leaves an ``out`` pre-filled with
    SENTINEL."""
    assert scores.dtype == np.float32 and scores.shape == (c.W, c.C, 28)
    seed = c.seed & M64
    # each comment's normalised label vector (it does not depend on the slot that draws it): tot summed over the
    # labels left to right, then one divide per label
    tot = np.zeros((c.W, c.C), np.float32)
    for d in range(c.D):
        tot = tot + scores[:, :, int(label_idx[d])]
    vec = scores[:, :, label_idx.astype(np.int64)] / tot[:, :, None]
    assert vec.dtype == np.float32
    out = np.full((c.W, c.N, c.D), SENTINEL, np.float32)
    k = min(c.subset, c.C)
    for w in range(c.W):
        perm = list(range(c.N))
        r = Rng(perm_key(seed, w))
        for j in range(c.N - 1, 0, -1):
            t = r.below(j + 1)
            perm[j], perm[t] = perm[t], perm[j]
        assert sorted(perm) == list(range(c.N))                       # a permutation: every row written once
        for j in range(c.N):
            r = Rng(slot_key(seed, w, j))
            if j < c.f:
                row = np.array([r.uniform() for _ in range(c.D)], np.float32)
            else:
                pick = list(range(c.C))
                acc = np.zeros(c.D, np.float32)
                drawn = []
                for i in range(k):
                    t = i + r.below(c.C - i)
                    pick[t], pick[i] = pick[i], pick[t]
                    drawn.append(pick[i])
                    acc = acc + vec[w, pick[i]]
                assert len(set(drawn)) == k                           # distinct comments
                row = acc / np.float32(k)
            assert row.dtype == np.float32
            out[w, perm[j]] = row
    assert not (out == np.float32(SENTINEL)).any()
    return out


# ------------------------------------------------------------------------------------------------ the data
class Built(NamedTuple):
    scores: torch.Tensor      # float32 [W, C, 28] in [0.01, 0.99]
    label_idx: torch.Tensor   # int32 [D], a random subset of [0, 28) in random order
    want: torch.Tensor        # float32 [W, N, D]


@functools.lru_cache(maxsize=None)
def make(c: Case) -> Built:
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    scores = (0.01 + 0.98 * torch.rand(c.W, c.C, 28, generator=g)).clamp_(0.01, 0.99)
    label_idx = torch.randperm(28, generator=g)[:c.D].to(torch.int32)
    want = torch.from_numpy(model(scores.numpy(), label_idx.numpy(), c))
    return Built(scores, label_idx, want)


def check(c: Case, device: str, op) -> None:
    """Run the op on ``device`` over a sentinel-filled ``out`` and compare fp32 bit patterns with the model."""
    b = make(c)
    out = torch.full((c.W, c.N, c.D), SENTINEL, dtype=torch.float32, device=device)
    op(b.scores.to(device), b.label_idx.to(device), out, c.f, c.subset, c.seed)
    got = out.cpu().view(torch.int32)
    want = b.want.view(torch.int32)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (case_id(c), bad[:5].tolist(), out.cpu()[tuple(bad[0, :2].tolist())].tolist(),
                              b.want[tuple(bad[0, :2].tolist())].tolist())
