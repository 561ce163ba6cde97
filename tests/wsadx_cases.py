"""Shared helpers of the wide-column exact kernel's GPU tests (test_wsadx_gpu.py, test_wsadx_groups_gpu.py,
test_wsadx_sharded_gpu.py; csrc/kernels/consensus_wsadx.hip): the env-guarded op caller (also the caller of the
model-pinned tests, exact_cases.py), the input recipes and the contract's arithmetic in Python integers."""
import contextlib
import os

import torch

from helpers import alloc_exact_out, beta_oracles
from svoc import ops as svops

DEV = "cuda"
OUTS = ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status")
MS = 10 ** 12             # max_spread (wsad): 1e6 real units
UNIT = 10 ** 6            # one real unit in wsad
OK, DIV_BY_ZERO, OVERFLOW = 0, 4, 7      # svoc/status.py
PATTERN = {"c1": -101, "consensus": -102, "skew": -103, "kurt": -104, "rel": -105, "qr": -106, "reliable": 7,
           "status": -1}


@contextlib.contextmanager
def _switches(env):
    """The exact ops' environment switches set to `env` alone for the launch, then put back."""
    old = {k: os.environ.get(k) for k in ("SVOC_EXACT_I128", "SVOC_EXACT_WSAD_ONLY", "SVOC_EXACT_WSAD_MIN_D")}
    try:
        for k in old:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(values, f, env=None, ms=MS, mode=0, rel_dim=0, inp=None, prefill=False, active=None, constrained=False,
         legacy=False, verdict=False):
    """One launch of exact_round in `mode`; `prefill`: over outputs filled with PATTERN (an unwanted write shows);
    `inp`: the inputs of the half (mode 2: c1, qr, status) copied over them first.  `verdict`: exact_verdict instead
    (status and rel are its outputs; `vstats` its routing counters)."""
    B, N, D = values.shape
    o = alloc_exact_out(B, N, D, values.device)
    if prefill:
        for k, p in PATTERN.items():
            o[k].fill_(p)
    for k, t in (inp or {}).items():
        o[k].copy_(t.to(values.device))
    stats = torch.zeros(2, dtype=torch.int32, device=values.device) if values.is_cuda else None
    vstats = torch.zeros(3, dtype=torch.int32, device=values.device) if values.is_cuda and verdict else None
    if active is not None:
        active = active.to(values.device)
    with _switches(env):
        if verdict:
            svops.ops().exact_verdict(values, active, f, constrained, ms, o["rel"], o["status"], legacy, stats=stats,
                                      vstats=vstats)
        else:
            svops.ops().exact_round(values, active, f, constrained, ms, o["c1"], o["consensus"], o["skew"], o["kurt"],
                                    o["rel"], o["qr"], o["reliable"], o["status"], legacy, mode, rel_dim, stats=stats)
        if values.is_cuda:
            torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in o.items()}
    out["stats"] = stats.cpu().tolist() if stats is not None else None
    out["vstats"] = vstats.cpu().tolist() if vstats is not None else None
    return out


def _prices(B, N, D, f, seed, centre=60_000.0, spread=20_000.0):
    """Beta(20,20) honest / U(0,1) failing draws mapped onto centre +- spread real units (int64 wsad)."""
    x, _ = beta_oracles(B, N, D, f, seed=seed, dtype=torch.float64)
    return (((x[:, :, :D] - 0.5) * (2.0 * spread) + centre) * 1e6).round().to(torch.int64).contiguous()


def _honest(B, N, D, seed, centre=1000 * UNIT, jitter=20_000):
    """Honest oracles: every value within +-jitter wsad of the centre (int64 wsad)."""
    g = torch.Generator().manual_seed(seed)
    return centre + torch.randint(-jitter, jitter + 1, (B, N, D), generator=g, dtype=torch.int64)


def _tdiv(a, b):
    """I128Div: truncation toward zero (signed_decimal.cairo:52-63), b > 0."""
    return a // b if a >= 0 else -((-a) // b)


def _wsqrt(v):
    """The contract's Newton sqrt (math.cairo:271-292) of a wsad value > 1, in Python integers."""
    g, g2 = v // 2, v // 2 + UNIT
    for _ in range(50):
        if g == g2:
            break
        n = (v * UNIT + g // 2) // g
        g2, g = g, (g + n) // 2
    return g


def _column_z(v, cpu, b, c):
    """(variance, sd, exact z per row -- None off the mask) of column c of instance b, in Python integers from
    the CPU engine's mean and mask."""
    mean = int(cpu["consensus"][b, c])
    rel = [int(r) for r in cpu["reliable"][b]]
    d = [int(x) - mean for x in v[b, :, c]]
    dr = [x for x, r in zip(d, rel) if r]
    var = sum((x * x + 500000) // UNIT for x in dr) // len(dr)
    sd = _wsqrt(var)
    return var, sd, [_tdiv(x * UNIT + sd // 2, sd) if r else None for x, r in zip(d, rel)]
