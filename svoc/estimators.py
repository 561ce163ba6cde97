"""Rank weights of the L-estimator round (``torch.ops.svoc.lest_round``, ``ConsensusConfig.essence="rank_weighted"``).

A column with sorted values ``x(0) <= ... <= x(n-1)`` is summarised by ``L_w(x) = sum_k w[k] x(k)``.  The reference
names the bell-shaped choice and never builds it (documentation/README.md:150: "the super smooth median: a weighted
sum based on the order, where the weights reproduce a bell shape"; the commented-out ``super_smooth_median`` of
contract/src/math.cairo:128-129).  :func:`rank_weights` is that choice; the other helpers are the weight rows of the
estimators an L-estimator contains -- the smooth median, the mean, a single order statistic, the trimmed mean.

Every row is computed in fp64 on the host and rounded to fp32 once: the kernels read fp32 weights.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import torch

MAX_RANKS = 256   # ranks per row of the op's [2, 256] weight tensor (route.hpp kLestMaxN)


def _f32(w: torch.Tensor) -> torch.Tensor:
    return w.to(torch.float32)


def rank_weights(n: int, sigma: float) -> torch.Tensor:
    """Bell weights over ``n`` ranks: ``u_k = exp(-(k - (n-1)/2)^2 / (2 (sigma n)^2))``, ``w = u / sum(u)``.
    ``sigma`` is the bell's width as a fraction of the count: small -> the median, large -> the mean."""
    n = int(n)
    if n < 1:
        raise ValueError("rank_weights: n >= 1")
    if not (isinstance(sigma, (int, float)) and math.isfinite(sigma) and sigma > 0):
        raise ValueError("rank_weights: sigma must be finite and > 0")
    k = torch.arange(n, dtype=torch.float64)
    u = torch.exp(-((k - (n - 1) / 2.0) ** 2) / (2.0 * (float(sigma) * n) ** 2))
    return _f32(u / u.sum())


def median_weights(n: int) -> torch.Tensor:
    """The smooth median (math.cairo:113-126): 1/2 at ranks ``n // 2 - 1`` and ``n // 2`` -- for odd ``n`` too, the
    contract's dead odd branch, as everywhere else here."""
    n = int(n)
    if n < 2:
        raise ValueError("median_weights: n >= 2")
    w = torch.zeros(n, dtype=torch.float64)
    w[n // 2 - 1] = 0.5
    w[n // 2] = 0.5
    return _f32(w)


def mean_weights(n: int) -> torch.Tensor:
    """The mean: ``1 / n`` at every rank."""
    n = int(n)
    if n < 1:
        raise ValueError("mean_weights: n >= 1")
    return _f32(torch.full((n,), 1.0 / n, dtype=torch.float64))


def one_hot(n: int, k: int) -> torch.Tensor:
    """The ``k``-th order statistic (0-based): the minimum at 0, the maximum at ``n - 1``."""
    n, k = int(n), int(k)
    if not 0 <= k < n:
        raise ValueError("one_hot: 0 <= k < n")
    w = torch.zeros(n, dtype=torch.float64)
    w[k] = 1.0
    return _f32(w)


def trimmed_mean_weights(n: int, trim: int) -> torch.Tensor:
    """The mean of the ranks ``trim .. n - trim - 1`` (``trim`` values dropped at either end)."""
    n, trim = int(n), int(trim)
    if trim < 0 or 2 * trim >= n:
        raise ValueError("trimmed_mean_weights: 0 <= trim and 2 trim < n")
    w = torch.zeros(n, dtype=torch.float64)
    w[trim:n - trim] = 1.0 / (n - 2 * trim)
    return _f32(w)


def check_weights(w, count: int, name: str) -> torch.Tensor:
    """A caller's weight row as the engine accepts it: ``count`` finite, non-negative numbers that sum to 1 within
    1e-5 (fp64 sum of the fp32 values).  Returns it as a 1-D fp32 CPU tensor."""
    w = torch.as_tensor(w).detach().to("cpu")
    if w.dim() != 1 or w.numel() != count:
        raise ValueError(f"{name}: expected {count} weights, got shape {tuple(w.shape)}")
    w = w.to(torch.float32)
    if not bool(torch.isfinite(w).all()):
        raise ValueError(f"{name}: every weight must be finite")
    if bool((w < 0).any()):
        raise ValueError(f"{name}: every weight must be >= 0")
    total = float(w.double().sum())
    if abs(total - 1.0) > 1e-5:
        raise ValueError(f"{name}: the weights must sum to 1 within 1e-5 (sum = {total!r})")
    return w.contiguous()


def pack(w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """The op's ``[2, 256]`` fp32 weight tensor: row 0 = ``w1``, row 1 = ``w2``, zero past their counts."""
    if w1.numel() > MAX_RANKS or w2.numel() > MAX_RANKS:
        raise ValueError(f"at most {MAX_RANKS} ranks")
    out = torch.zeros(2, MAX_RANKS, dtype=torch.float32)
    out[0, : w1.numel()] = w1.to(torch.float32)
    out[1, : w2.numel()] = w2.to(torch.float32)
    return out


def round_weights(n: int, n_failing: int, sigma: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The two bell rows of a round: ``n`` ranks in pass 1, ``n - n_failing`` in pass 2."""
    return rank_weights(n, sigma), rank_weights(n - n_failing, sigma)


__all__: Sequence[str] = ("rank_weights", "median_weights", "mean_weights", "one_hot", "trimmed_mean_weights",
                          "check_weights", "pack", "round_weights", "MAX_RANKS")
