"""Shared cases of the verdict / preview tests (test_preview.py, test_verdict_gpu.py): the instance recipes of a
round's verdict (accept, each way the moments divide by zero, the reliability interval, a value outside the
column kernel's domain), the op callers and the seeded transactional stream with its reverts."""
import random

import torch

from svoc import ops as svops
from svoc.config import ConsensusConfig
from svoc.status import Status

OK = int(Status.OK)
RECIPES = ("plain", "zero_variance", "variance_one", "rel_interval", "out_of_domain", "plain_b")
# the statuses the golden model gives them (checked with svoc/reference.py at N = 8, D = 4, f = 2); the
# out-of-domain one is asserted from the golden model / the CPU engine where it is used
EXPECTED = {"plain": Status.OK, "zero_variance": Status.DIV_BY_ZERO, "variance_one": Status.DIV_BY_ZERO,
            "rel_interval": Status.RELIABILITY_INTERVAL, "plain_b": Status.OK}


def recipe(name, N, D, f, seed=0):
    """One instance [N, D] int64.  Rows 0 .. f - 1 are outliers in every column but the last (100000 against
    values around 500000), so the rank cut masks exactly them and the reliable rows are f .. N - 1."""
    g = torch.Generator().manual_seed(1000 * seed + RECIPES.index(name))
    x = torch.randint(400_000, 600_001, (N, D), generator=g, dtype=torch.int64)
    if name == "rel_interval":          # ceil(3N/8) rows all 0, the rest all 1e6: rel1 = 1 - 2 sqrt(3/8) < 0
        k = (3 * N + 7) // 8
        x[:k] = 0
        x[k:] = 1_000_000
        return x
    if D > 1:
        x[:f, :D - 1] = 100_000
    if name == "zero_variance":         # the last column (the tail slab) holds one value in every row
        x[:, D - 1] = 500_000
    elif name == "variance_one":        # 500000 +- 1000 alternating over the reliable rows: qdev = 1 each
        x[:, D - 1] = 500_000
        r = torch.arange(N - f)
        x[f:, D - 1] = torch.where(r % 2 == 0, 501_000, 499_000)
    elif name == "out_of_domain":       # past the constrained interval: the column kernel hands the round off
        x[N // 2, D // 2] = 1_000_001
    return x


def batch(N, D, f, seed=0):
    return torch.stack([recipe(n, N, D, f, seed) for n in RECIPES])


def run_round(values, f, constrained=True, max_spread=0, legacy=False):
    """exact_round -> (status [B], rel [B, 2]) (fresh outputs)."""
    B, N, D = values.shape
    dev = values.device
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)  # noqa: E731
    rel = torch.full((B, 2), -7, dtype=torch.int64, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    svops.ops().exact_round(values, None, f, constrained, max_spread, z(B, D), z(B, D), z(B, D), z(B, D), rel,
                            z(B, N), torch.zeros(B, N, dtype=torch.uint8, device=dev), status, legacy)
    return status, rel


def run_verdict(values, f, constrained=True, max_spread=0, legacy=False, counters=False):
    """exact_verdict -> (status [B], rel [B, 2], vstats [3] or None)."""
    B = values.shape[0]
    dev = values.device
    rel = torch.full((B, 2), -7, dtype=torch.int64, device=dev)
    status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    vstats = torch.zeros(3, dtype=torch.int32, device=dev) if counters else None
    svops.ops().exact_verdict(values, None, f, constrained, max_spread, rel, status, legacy, None, vstats)
    return status, rel, vstats


def same_verdict(st_v, rel_v, st_r, rel_r):
    """The verdict's status equals the round's, and its rel where the status is OK (untouched elsewhere)."""
    assert st_v.cpu().tolist() == st_r.cpu().tolist()
    ok = (st_r == OK).cpu()
    assert torch.equal(rel_v.cpu()[ok], rel_r.cpu()[ok])
    assert (rel_v.cpu()[~ok] == -7).all()


# ---- the transactional stream ------------------------------------------------------------------------------

STATE = ("values", "enabled", "n_active", "touched", "status", "rel", "c1", "consensus", "skew", "kurt", "qr",
         "reliable", "consensus_active", "metrics_fx")


def snapshot(e):
    return {k: getattr(e, k).clone() for k in STATE}, e.rounds, (None if e._xstats is None else e._xstats.clone())


def assert_unchanged(e, snap):
    state, rounds, xs = snap
    for k, v in state.items():
        assert torch.equal(getattr(e, k), v), k
    assert e.rounds == rounds
    assert xs is None or torch.equal(e._xstats, xs)


def engine(N, D, f, B, device, storage=None):
    from svoc.engine import ConsensusEngine
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    return ConsensusEngine(cfg, batch=B, device=device, mode="exact", storage=storage)


def stream_update(rng, D, flat):
    """A random constrained prediction: often with a pinned column 0 (zero-variance bait), sometimes out of
    range, otherwise uniform (the recipe of test_exact_stream.py)."""
    r = rng.random()
    if r < 0.08:
        return [1_000_001 if rng.random() < 0.5 else -3] + [rng.randint(0, 1_000_000) for _ in range(D - 1)]
    if r < 0.7:
        return [flat[0]] + [rng.randint(0, 1_000_000) for _ in range(D - 1)]
    return [rng.randint(0, 1_000_000) for _ in range(D)]


def stream(seed, N, D, B, per_inst):
    """Per instance: every oracle once (bootstrap), then random oracles (N = an unknown one)."""
    rng = random.Random(seed)
    flats = [[rng.randint(0, 1_000_000) for _ in range(D)] for _ in range(B)]
    ups = []
    for b in range(B):
        seq = [(o, stream_update(rng, D, flats[b])) for o in range(N)]
        for _ in range(per_inst - N):
            seq.append((rng.randrange(N + 1), stream_update(rng, D, flats[b])))
        ups.append(seq)
    return ups


def strided_batches(ups, cuts):
    """The stream cut into steps [lo, hi) of every instance, laid out b * K + k: (inst, oracle, vals, K)."""
    B = len(ups)
    for lo, hi in cuts:
        K = hi - lo
        inst = torch.tensor([b for b in range(B) for _ in range(K)])
        orc = torch.tensor([ups[b][k][0] for b in range(B) for k in range(lo, hi)])
        vals = torch.tensor([ups[b][k][1] for b in range(B) for k in range(lo, hi)], dtype=torch.int64)
        yield inst, orc, vals, K


def _preview_then_step(e, inst, orc, vals, K):
    snap = snapshot(e)
    p = e.preview_updates(inst, orc, vals, updates_per_instance=K)
    assert_unchanged(e, snap)
    s = e.step(inst, orc, vals, updates_per_instance=K)
    assert p.dtype == torch.int32 and p.tolist() == s.tolist()
    return s.tolist()


def run_preview_stream(device, n, d, f, B=6, seed=12, per_inst=None):
    """The 7 x 3 stream recipe of test_exact_stream.py (any shape): before every step the same batch is
    previewed; both layouts.  Returns the statuses seen."""
    per_inst = per_inst or n + 9
    ups = stream(seed, n, d, B, per_inst)
    cuts = [(0, n)] + [(k, min(k + 3, per_inst)) for k in range(n, per_inst, 3)]
    seen = set()
    for strided in (True, False):
        e = engine(n, d, f, B, device)
        for inst, orc, vals, K in strided_batches(ups, cuts):
            if not strided:   # the general layout: the same updates interleaved wave-major
                perm = torch.arange(B * K).view(B, K).t().reshape(-1)
                inst, orc, vals, K = inst[perm], orc[perm], vals[perm], None
            seen |= set(_preview_then_step(e, inst, orc, vals, K))
    return {Status(s) for s in seen}
