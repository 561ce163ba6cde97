"""Pending commit of the open fused pipeline: the accepted rows of step s reach ``values`` from inside the round
of step s + 1 (consensus_fast_winf.hip, FastParams.pend_rows), the last step's at the join.

Reference: the generic transactional path (update kernel with saved rows + round + restore) on a second
engine fed the same seeded batches; everything is compared bit for bit -- the state, every output and the
per-update statuses of every step.  Also here: the fused path's piece map at U = 256 (one byte per piece).
"""
import pytest
import torch

from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine
from svoc.status import Status

pytestmark = pytest.mark.gpu

B, CHUNKS = 6, 2
# N, D, f, U: lane groups 4, 4 (padded N), 1 and 2 (the half-widths and the rest: test_fused_model_gpu.py)
SHAPES = [(256, 128, 32, 64), (200, 300, 20, 50), (64, 700, 8, 16), (128, 132, 8, 32)]
KEYS = ("values", "status", "enabled", "n_active", "c1", "consensus", "rel", "reliable", "skew", "kurt", "qr")
ZV, OK, IV, NO = (int(Status.ZERO_VARIANCE), int(Status.OK), int(Status.INTERVAL_INPUT), int(Status.NOT_ORACLE))


def _engine(N, D, f):
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    e = ConsensusEngine(cfg, batch=B, device="cuda", mode="fast", storage="fp32")
    e.randomize(seed=N + D)
    e.run_round()
    e.values[1, :, 3] = 0.625    # instance 1: column 3 constant (the batches decide when it stays so)
    e.values[4, :, 5] = 0.25     # instance 4: column 5 constant
    return e


def _batches(N, D, U, steps=4):
    """``steps`` batches [(inst, oracle [B * U], rows [B * U, D])] with the cases of the module docstring:
    instance 1 (range 0): step 0 accepted, 3/4 of its rows break the constant column 3; step 1 updates those
      rows again plus fresh ones, all back at the constant -> zero variance, the round reverts while rows of
      step 0 are pending (some updated in both steps, some only in step 0);
    instance 2: step 1 re-updates an oracle of step 0 with a value outside [0, 1];
    instance 4 (range 1): step 0 keeps column 5 constant -> reverts, nothing pending at step 1;
    instance 5: oracle ids outside [0, N) in steps 0 and 1 (one with an invalid row as well)."""
    g = torch.Generator().manual_seed(1000 * N + D)
    orc = [torch.stack([torch.randperm(N, generator=g)[:U] for _ in range(B)]) for _ in range(steps)]
    vals = [torch.rand(B, U, D, generator=g) for _ in range(steps)]
    h = 3 * U // 4
    both = orc[0][1][:h]
    fresh = torch.tensor([o for o in range(N) if o not in set(orc[0][1].tolist())])[:U - h]
    vals[0][1, h:, 3] = 0.625
    orc[1][1] = torch.cat([both, fresh])
    vals[1][1, :, 3] = 0.625
    o = int(orc[0][2][0])
    orc[1][2] = torch.cat([torch.tensor([o]), orc[1][2][orc[1][2] != o]])[:U]
    vals[1][2, 0, D // 2] = 1.5
    vals[0][4, :, 5] = 0.25
    for s in (0, 1):
        orc[s][5][1] = N + 5
        orc[s][5][3] = -1
    vals[1][5, 3, 0] = 2.0
    # an oracle updated in steps 0 and 1, and one in step 0 only (instance 0, as drawn)
    s0, s1 = set(orc[0][0].tolist()), set(orc[1][0].tolist())
    assert s0 & s1 and s0 - s1
    inst = torch.arange(B).repeat_interleave(U).cuda()
    return [(inst, orc[s].reshape(-1).cuda(), vals[s].reshape(B * U, D).cuda()) for s in range(steps)]


def _snap(e):
    e.pipeline_join()
    return {k: getattr(e, k).clone() for k in KEYS}


_REF = {}


def _reference(shape, seq):
    """The generic path over the batch sequence ``seq`` (indices into the 4 batches; "u" = the odd-U batch):
    per step the update statuses and the whole state."""
    key = (shape, tuple(seq))
    if key not in _REF:
        N, D, f, U = shape
        gen = _engine(N, D, f)
        gen._all_active = False      # force the generic path (update kernel + saved rows + restore)
        gen._fused_ok = lambda *a: False
        bat = _all_batches(shape)
        sts, snaps = [], []
        for i in seq:
            inst, orc, vals = bat[i]
            u = inst.numel() // B
            gen.step_pipelined(inst, orc, vals, u, chunks=CHUNKS, overlap=False)
            sts.append(gen._save_bufs[("pipe",)][2][:B * u].clone())
            snaps.append(_snap(gen))
        torch.cuda.synchronize()
        _REF[key] = (sts, snaps)
    return _REF[key]


_BAT = {}


def _all_batches(shape):
    if shape not in _BAT:
        N, D, f, U = shape
        bat = {i: b for i, b in enumerate(_batches(N, D, U))}
        # a step with another U (U - 1 updates per instance): the flush path
        g = torch.Generator().manual_seed(7)
        u2 = U - 1
        bat["u"] = (torch.arange(B).repeat_interleave(u2).cuda(),
                    torch.stack([torch.randperm(N, generator=g)[:u2] for _ in range(B)]).reshape(-1).cuda(),
                    torch.rand(B * u2, D, generator=g).cuda())
        _BAT[shape] = bat
    return _BAT[shape]


def _grab_status(e):
    """A copy of the step's update statuses, taken on each range's own stream (no join: the pipeline stays open)."""
    st = e._last_st
    out = torch.empty_like(st)
    if not getattr(e, "_pipe_open", False):
        out.copy_(st)
        return out
    U = st.numel() // B
    step = (B + CHUNKS - 1) // CHUNKS
    for k in range(CHUNKS):
        sl = slice(k * step * U, min(B, (k + 1) * step) * U)
        s = e._pipe_streams[1 + k]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            out[sl].copy_(st[sl])
    return out


def _check(e, snap, what):
    got = _snap(e)
    torch.cuda.synchronize()
    for k in KEYS:
        a, b_ = got[k], snap[k]
        if not torch.equal(a, b_):
            bad = (a != b_).reshape(B, -1)
            raise AssertionError(f"{what}: {k} differs in instances {bad.any(1).nonzero().flatten().tolist()}, "
                                 f"first (inst, word) {bad.nonzero()[:6].tolist()}")


def _check_statuses(got, ref):
    torch.cuda.synchronize()
    for s, (a, b_) in enumerate(zip(got, ref)):
        assert torch.equal(a, b_), (s, (a != b_).nonzero().flatten()[:8].tolist())


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_holds_every_case(shape):
    """The seeded batches do what their docstring says (read off the generic path)."""
    N, D, f, U = shape
    sts, snaps = _reference(shape, (0, 1, 2, 3))
    st0, st1 = sts[0].view(B, U).cpu(), sts[1].view(B, U).cpu()
    assert snaps[0]["status"][1].item() == OK and snaps[1]["status"][1].item() == ZV
    assert (st0[1] == OK).all() and (st1[1] == ZV).all()
    assert torch.equal(snaps[1]["values"][1], snaps[0]["values"][1])          # instance 1 ends with the step-0 rows
    assert snaps[0]["status"][2].item() == OK and st0[2, 0].item() == OK      # a pending row ...
    assert st1[2, 0].item() == IV and (st1[2, 1:] == OK).all()                # ... whose next update alone is rejected
    assert snaps[0]["status"][4].item() == ZV and (st0[4] == ZV).all()        # nothing pending at step 1
    assert snaps[1]["status"][4].item() == OK
    assert st0[5, 1].item() == NO and st0[5, 3].item() == NO and st1[5, 1].item() == NO and st1[5, 3].item() == IV
    assert all(int((s["status"] == OK).sum()) >= B - 1 for s in snaps)


@pytest.mark.parametrize("mode", ["open", "join_every_step", "switch_off"])
@pytest.mark.parametrize("shape", SHAPES)
def test_pending_commit_matches_generic_path(shape, mode, monkeypatch):
    """4 open steps with one join at the end; the same joined after every step (each step's state is compared);
    and SVOC_DEFERRED_COMMIT=0 (the commit kernel after every round)."""
    N, D, f, U = shape
    if mode == "switch_off":
        monkeypatch.setenv("SVOC_DEFERRED_COMMIT", "0")
    sts, snaps = _reference(shape, (0, 1, 2, 3))
    bat = _all_batches(shape)
    e = _engine(N, D, f)
    assert e._fused_ok(*bat[0], U)
    got = []
    for s in range(4):
        e.step_pipelined(*bat[s], U, chunks=CHUNKS, overlap=True)
        assert (getattr(e, "_defer", None) is not None) == (mode != "switch_off")
        if s > 0 and mode == "open":
            assert e._defer["slot"] == s % 2
        got.append(_grab_status(e))
        if mode == "join_every_step":
            _check(e, snaps[s], f"step {s}")
            assert e._defer is None
    _check(e, snaps[3], "after the join")
    _check_statuses(got, sts)


@pytest.mark.parametrize("shape", SHAPES)
def test_getter_between_steps_joins(shape):
    """A getter between two open steps joins: the state is exact at that point, and the steps after it too."""
    N, D, f, U = shape
    sts, snaps = _reference(shape, (0, 1, 2, 3))
    bat = _all_batches(shape)
    e = _engine(N, D, f)
    for s in (0, 1):
        e.step_pipelined(*bat[s], U, chunks=CHUNKS, overlap=True)
    cons = e.get_consensus_value()
    assert e._defer is None and not e._pipe_open
    torch.cuda.synchronize()
    assert torch.equal(cons, snaps[1]["consensus"]) and torch.equal(e.values, snaps[1]["values"])
    for s in (2, 3):
        e.step_pipelined(*bat[s], U, chunks=CHUNKS, overlap=True)
    _check(e, snaps[3], "after the join")


@pytest.mark.parametrize("shape", SHAPES)
def test_step_with_another_u_flushes(shape):
    """A step with a different U between open steps: the pending batch is flushed first."""
    N, D, f, U = shape
    seq = (0, 1, "u", 2, 3)
    sts, snaps = _reference(shape, seq)
    bat = _all_batches(shape)
    e = _engine(N, D, f)
    got = []
    for i in seq:
        inst, orc, vals = bat[i]
        e.step_pipelined(inst, orc, vals, inst.numel() // B, chunks=CHUNKS, overlap=True)
        got.append(_grab_status(e))
    _check(e, snaps[-1], "after the join")
    _check_statuses(got, sts)


@pytest.mark.parametrize("shape", SHAPES)
def test_captured_steps_replay(shape):
    """Three open steps and the join captured in one graph (after the same three steps run eagerly as a warm-up)
    and replayed twice == the generic engine run eagerly over those steps: every replay starts with nothing
    pending and ends with the flush."""
    N, D, f, U = shape
    sts, snaps = _reference(shape, (0, 1, 2) * 3)
    bat = _all_batches(shape)
    e = _engine(N, D, f)

    def steps():
        for s in range(3):
            e.step_pipelined(*bat[s], U, chunks=CHUNKS, overlap=True)
        e.pipeline_join()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        steps()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _check(e, snaps[2], "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps()
    assert e._defer is None
    graph.replay()
    torch.cuda.synchronize()
    _check(e, snaps[5], "first replay")
    graph.replay()
    torch.cuda.synchronize()
    _check(e, snaps[8], "second replay")


def test_fused_piece_map_with_256_updates():
    """N = 256 with U = 256 (every oracle publishes) on the fused path: slot 255 + 1 does not fit one byte of the
    kernel's piece map (it carries a ninth bit at this U) -- equal to step() (update kernel, round, restore
    kernel)."""
    N, D, f, U = 256, 128, 32, 256
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    ref = ConsensusEngine(cfg, batch=B, device="cuda", mode="fast", storage="fp32")
    pipe = ConsensusEngine(cfg, batch=B, device="cuda", mode="fast", storage="fp32")
    for e in (ref, pipe):
        e.randomize(seed=3)
        e.run_round()
    g = torch.Generator().manual_seed(0)
    inst = torch.arange(B).repeat_interleave(U).cuda()
    orc = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).reshape(-1).cuda()
    vals = torch.rand(B * U, D, generator=g).cuda()
    vals[3 * U:4 * U] = 0.5          # instance 3: one point -> zero variance, the round reverts
    orc[1 * U + 7] = -1              # instance 1: one row stays the state's, beside slot 255
    ref.step(inst, orc, vals)
    assert pipe._fused_ok(inst, orc, vals, U)
    pipe.step_pipelined(inst, orc, vals, U, chunks=CHUNKS, overlap=False)
    pipe.pipeline_join()
    torch.cuda.synchronize()
    assert (pipe._last_st.view(B, U)[3] == ZV).all() and int((pipe._last_st == OK).sum()) == (B - 1) * U - 1
    assert pipe._last_st[1 * U + 7].item() == NO
    assert pipe.status[3].item() == ZV and int((pipe.status == OK).sum()) == B - 1
    for k in KEYS:
        assert torch.equal(getattr(pipe, k), getattr(ref, k)), k
