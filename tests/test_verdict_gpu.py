"""Verdict rounds on the GPU: the exact_verdict op (the verdict form of the column kernel and the scratch route)
against exact_round and the CPU engine, the strided exact stream judged by verdict waves against the CPU engine's
one-full-round-per-transaction path, preview_updates on the device, and graph capture of the verdict-wave step."""
import random

import pytest
import torch

import verdict_cases as vc
from svoc.status import Status

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAGGED = vc.RECIPES.index("out_of_domain")


def _check_op(x, f, n_verdict, **kw):
    """exact_verdict on the GPU == exact_round on the GPU == the CPU op (status; rel where OK); the counters."""
    st_c, rel_c, _ = vc.run_verdict(x, f, **kw)
    st_r, rel_r = vc.run_round(x.to(DEV), f, **kw)
    st_v, rel_v, vstats = vc.run_verdict(x.to(DEV), f, counters=True, **kw)
    vc.same_verdict(st_v, rel_v, st_r, rel_r)
    vc.same_verdict(st_v, rel_v, st_c, rel_c)
    assert vstats.tolist() == [n_verdict, x.shape[0] - n_verdict, 0]
    return [Status(s) for s in st_c.tolist()]


# NSEG 1 / 2 / 4, padded rows, a partial tile, several slabs with a tail, both storages, and the shapes whose
# full rounds use the window widths 5 and 17
@pytest.mark.parametrize("N,D,f,dtype", [(8, 64, 2, torch.int32), (8, 300, 2, torch.int64), (64, 70, 8, torch.int64),
                                         (96, 70, 10, torch.int32), (130, 130, 5, torch.int32),
                                         (256, 64, 32, torch.int32)])
def test_verdict_kernel_op(N, D, f, dtype):
    x = vc.batch(N, D, f).to(dtype)
    st = _check_op(x, f, n_verdict=len(vc.RECIPES) - 1)     # the out-of-domain instance is handed off
    for k, name in enumerate(vc.RECIPES):
        if name in vc.EXPECTED:
            assert st[k] == vc.EXPECTED[name], name
    # R < 4: the moments divide by zero wherever the reliabilities pass
    st = _check_op(x, N - 3, n_verdict=len(vc.RECIPES) - 1)
    assert st[0] == Status.DIV_BY_ZERO and st[vc.RECIPES.index("rel_interval")] == Status.RELIABILITY_INTERVAL


def test_verdict_scratch_route(monkeypatch):
    # the wide lane groups, a tiny instance (the i128 kernel), unconstrained rounds: the full round into scratch
    _check_op(vc.batch(300, 16, 20).to(torch.int32), 20, n_verdict=0)
    _check_op(vc.batch(7, 3, 2), 2, n_verdict=0)
    _check_op(vc.batch(16, 64, 2), 2, n_verdict=0, constrained=False, max_spread=1_000_000)
    monkeypatch.setenv("SVOC_EXACT_I128", "1")
    st = _check_op(vc.batch(8, 64, 2).to(torch.int32), 2, n_verdict=0)
    assert st[:4] == [vc.EXPECTED[k] for k in vc.RECIPES[:4]]


# ---- the stream ------------------------------------------------------------------------------------------------

OUT = ("values", "enabled", "n_active", "consensus_active", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable",
       "status", "metrics_fx")


def _same_engines(g, c):
    for k in OUT:
        assert torch.equal(getattr(g, k).cpu(), getattr(c, k)), k
    assert g.rounds == c.rounds


N, D, F, B, K = 8, 64, 2, 6, 5
PIN = 123_456


def _stream_steps(seed=21):
    """Steps of K updates per instance (b * K + k), as (oracle [B][K], rows [B][K][D]):
    two bootstrap steps (5 + 3 oracles: the instances turn active inside the second), random steps with pinned
    column-0 baits, out-of-range values and unknown oracles, then two built ones: oracles 0 .. 4 take mid-range
    rows with column 0 pinned; then oracle 5 (column 0 apart) and the outliers 6, 7 make the reliable set
    0 .. 5, and oracle 5 closes column 0 twice -- a revert in the middle of the step and as its last
    transaction -- while instance 0 gets nothing but rejected updates; a last random step follows."""
    rng = random.Random(seed)
    flats = [[rng.randint(0, 1_000_000) for _ in range(D)] for _ in range(B)]
    mid = lambda c0: [c0] + [rng.randint(400_000, 600_000) for _ in range(D - 1)]  # noqa: E731
    upd = lambda b: vc.stream_update(rng, D, flats[b])  # noqa: E731
    steps = [([[0, 1, 2, 3, 4]] * B, [[upd(b) for _ in range(K)] for b in range(B)]),
             ([[5, 6, 7, 0, rng.randrange(N + 1)] for _ in range(B)], [[upd(b) for _ in range(K)] for b in range(B)])]
    for _ in range(3):
        steps.append(([[rng.randrange(N + 1) for _ in range(K)] for _ in range(B)],
                      [[upd(b) for _ in range(K)] for b in range(B)]))
    steps.append(([[0, 1, 2, 3, 4]] * B, [[mid(PIN) for _ in range(K)] for _ in range(B)]))
    orc, rows = [], []
    for b in range(B):
        if b == 0:   # out of range, unknown oracles: nothing is accepted
            orc.append([1, N, 2, N, 3])
            rows.append([[-3] + mid(PIN)[1:], mid(PIN), [1_000_001] + mid(PIN)[1:], mid(PIN), [2_000_000] * D])
        else:
            orc.append([5, 6, 7, 5, 5])
            rows.append([mid(PIN + 50_000), [PIN] + [100_000] * (D - 1), [PIN] + [900_000] * (D - 1), mid(PIN), mid(PIN)])
    steps.append((orc, rows))
    steps.append(([[rng.randrange(N + 1) for _ in range(K)] for _ in range(B)],
                  [[upd(b) for _ in range(K)] for b in range(B)]))
    return steps


def _tensors(orc, rows):
    k = len(orc[0])
    inst = torch.tensor([b for b in range(len(orc)) for _ in range(k)])
    return inst, torch.tensor(orc).reshape(-1), torch.tensor(rows, dtype=torch.int64).reshape(len(orc) * k, -1), k


def _run_stream(expect_verdict):
    g, c = vc.engine(N, D, F, B, DEV), vc.engine(N, D, F, B, "cpu")
    seen, log = set(), []
    for orc, rows in _stream_steps():
        inst, o, v, k = _tensors(orc, rows)
        sg = g.step(inst, o, v, updates_per_instance=k).cpu().tolist()
        sc = c.step(inst, o, v, updates_per_instance=k).tolist()
        assert sg == sc
        _same_engines(g, c)
        seen |= set(sc)
        log.append(sc)
    assert {int(s) for s in (Status.OK, Status.NOT_ACTIVE, Status.DIV_BY_ZERO, Status.INTERVAL_INPUT,
                             Status.NOT_ORACLE)} <= seen
    built = log[-2]
    assert all(s != vc.OK for s in built[:K])                                       # instance 0 accepted nothing
    dz = int(Status.DIV_BY_ZERO)
    assert built[K:2 * K] == [vc.OK, vc.OK, vc.OK, dz, dz]                          # mid-step and last: reverted
    r = g.verdict_routing()
    assert r["mismatch"] == 0 and (r["verdict"] > 0) == expect_verdict, r
    if not expect_verdict:
        assert r == {"verdict": 0, "fallback": 0, "mismatch": 0}
    return log


def test_stream_verdict_waves_equal_full_rounds(monkeypatch):
    a = _run_stream(expect_verdict=True)
    monkeypatch.setenv("SVOC_VERDICT_WAVES", "0")
    assert _run_stream(expect_verdict=False) == a


def test_stream_final_round_window_kernel():
    """256 oracles, f = 32: the waves are verdicts, the step's one full round is the window kernel (H = 17)."""
    n, d, f, b, k = 256, 64, 32, 2, 3
    g, c = vc.engine(n, d, f, b, DEV), vc.engine(n, d, f, b, "cpu")
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(300_000, 700_001, (b, n, d), generator=gen, dtype=torch.int64)
    for e in (g, c):
        e.values.copy_(x.to(e.vdtype))
        e.enabled.fill_(1)
        e.n_active.fill_(n)
    for step in range(2):
        orc = torch.stack([torch.randperm(n, generator=gen)[:k] for _ in range(b)]).reshape(-1)
        vals = torch.randint(0, 1_000_001, (b * k, d), generator=gen, dtype=torch.int64)
        if step == 1:
            vals[k - 1, 0] = 1_000_001          # instance 0's last update is rejected
        inst = torch.arange(b).repeat_interleave(k)
        sg = g.step(inst, orc, vals, updates_per_instance=k).cpu().tolist()
        assert sg == c.step(inst, orc, vals, updates_per_instance=k).tolist()
        assert sg.count(vc.OK) >= b * k - 1
        _same_engines(g, c)
    r = g.verdict_routing()
    assert r["verdict"] > 0 and r["mismatch"] == 0, r


def _preview_stream(device):
    """Every step of the stream above is previewed, then stepped, in both layouts: the state is untouched by the
    preview and the statuses are the step's -- the built steps' reverts in the middle and at the end of a batch
    included (a reverted update is not visible to the later ones of its batch)."""
    seen = set()
    for strided in (True, False):
        e = vc.engine(N, D, F, B, device)
        log = []
        for orc, rows in _stream_steps():
            inst, o, v, k = _tensors(orc, rows)
            if not strided:   # the general layout: the same updates interleaved wave-major
                perm = torch.arange(B * k).view(B, k).t().reshape(-1)
                inst, o, v, k = inst[perm], o[perm], v[perm], None
            snap = vc.snapshot(e)
            p = e.preview_updates(inst, o, v, updates_per_instance=k)
            vc.assert_unchanged(e, snap)
            s = e.step(inst, o, v, updates_per_instance=k)
            assert p.dtype == torch.int32 and p.tolist() == s.tolist()
            log.append(s.tolist())
        seen |= {x for st in log for x in st}
        inst1 = log[-2][K:2 * K] if strided else [log[-2][kk * B + 1] for kk in range(K)]   # instance 1, built step
        dz = int(Status.DIV_BY_ZERO)
        assert inst1 == [vc.OK, vc.OK, vc.OK, dz, dz]
    return {Status(x) for x in seen}


def test_preview_equals_step_gpu():
    seen = _preview_stream(DEV)
    assert {Status.OK, Status.NOT_ACTIVE, Status.DIV_BY_ZERO, Status.INTERVAL_INPUT, Status.NOT_ORACLE} <= seen, seen


def test_verdict_step_graph_capture():
    n, d, f, b, k = 8, 64, 2, 4, 3
    gen = torch.Generator().manual_seed(9)
    x = torch.randint(300_000, 700_001, (b, n, d), generator=gen, dtype=torch.int64)
    a, e = vc.engine(n, d, f, b, DEV), vc.engine(n, d, f, b, DEV)
    for eng in (a, e):
        eng.values.copy_(x.to(eng.vdtype))
        eng.enabled.fill_(1)
        eng.n_active.fill_(n)
    assert a._verdict_ok()

    def batch(i):
        g2 = torch.Generator().manual_seed(100 + i)
        orc = torch.stack([torch.randperm(n, generator=g2)[:k] for _ in range(b)]).reshape(-1)
        vals = torch.randint(0, 1_000_001, (b * k, d), generator=g2, dtype=torch.int64)
        vals[1, :] = vals[0, :]                 # (a repeated row is still a plain update)
        if i == 2:
            vals[k + 1, 3] = -1                 # rejected inside the replayed step
        return torch.arange(b).repeat_interleave(k).to(DEV), orc.to(DEV), vals.to(a.vdtype).to(DEV)

    inst, orc, vals = batch(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # warm-up outside the capture (allocations)
        a.step(inst, orc, vals, updates_per_instance=k)
    torch.cuda.current_stream().wait_stream(s)
    e.step(inst, orc, vals, updates_per_instance=k)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, no parallel branches
        out = a.step(inst, orc, vals, updates_per_instance=k)
    for i in (1, 2):
        bi, bo, bv = batch(i)
        orc.copy_(bo)
        vals.copy_(bv)
        graph.replay()
        want = e.step(bi, bo, bv, updates_per_instance=k)
        assert torch.equal(out, want)
        for key in OUT:
            if key != "metrics_fx":
                assert torch.equal(getattr(a, key), getattr(e, key)), key
    assert torch.equal(a.metrics_fx, e.metrics_fx)
    torch.cuda.synchronize()
    assert a._vstats[2].item() == 0 and a._vstats[0].item() > 0
