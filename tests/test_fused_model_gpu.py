"""The fused fp32 transactional round (consensus_fast_winf.hip: FUSED, DEFER and WIDE forms of every lane-group
width and window half-width) against the sequential fp64 model of fused_cases.py, driven at the op level:
fast_round(upd_* [, pend_*]) and commit_updates on one stream, no engine -- a failure names the kernel, and the
instance, slot or column.

Two of the shapes have D % 4 != 0, where the batch rows (pitch D) are only 4-byte aligned for the 16-byte
LDS-DMA pieces and the last row's tail piece runs past the end of the instance's batch descriptor.  Read from
the kernel and slabdma.hpp before they first ran: every such access is a buffer LOAD through a descriptor whose
num_records is the batch's exact byte size, so it cannot touch memory outside the batch (out-of-range dwords are
dropped by the range check); the piece's LDS destination does not depend on the source address; a buffer
dwordx4 access needs dword alignment only; and no store follows from these shapes (the deferred write-back is
refused by the route unless D % 4 == 0, asserted below).  Whether the range check drops single dwords or the
whole piece is what the last slot's last column (fused_cases: slot U - 1, column D - 1) shows: on the MI355X
the in-range dwords of that piece arrive (an accepted value there reaches qr and the state, an invalid one
is reported), i.e. the check is per dword for LDS-DMA loads as for register loads.
"""
import pytest
import torch

import fast_cases
import fused_cases as fc
from fused_cases import OK, ZERO_VARIANCE
from helpers import alloc_fast_out, fast_work
from svoc import ops as svops
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine

pytestmark = pytest.mark.gpu

OUT = ("c1", "consensus", "rel", "reliable", "skew", "kurt", "qr")
FUSED = [pytest.param(s, id=fc.shape_id(s)) for s in fc.SHAPES]
DEFER = [pytest.param(s, id=fc.shape_id(s)) for s in fc.SHAPES if fc.deferred(s)]
by_id = {fc.shape_id(s): s for s in fc.SHAPES}
_RUNS = {}


def _round_up(x, m):
    return (x + m - 1) // m * m


def _route(s, ld):
    r = svops.fast_route("fp32", s.N, s.D, ld, s.f, True)
    assert r.kernel == svops.KERNEL_WINDOW and (r.lane_groups, r.win_h) == (s.nseg, s.h)
    assert r.fused_max_u == 256 and r.defer_max_u == (127 if s.D % 4 == 0 else 0)
    return r


def _run(s, defer, cancel=None, extra_ld=0, pad=0.0):
    """The case's STEPS batches through the kernel; per step the update statuses, the state after the launch
    (and after the commit kernel, where it runs) and every output.  defer: every launch gets the batch before it
    as its pending batch (the first one a batch whose round reverted: nothing pending) and no commit kernel; the
    last batch is committed at the end (``final``)."""
    key = (s, defer, cancel, extra_ld, pad)
    if key in _RUNS:
        return _RUNS[key]
    c = fc.build(s)
    N, D, f, U, B = s.N, s.D, s.f, s.U, c["B"]
    ld = _round_up(D, 8) + extra_ld
    r = _route(s, ld)
    assert U <= (r.defer_max_u if defer else r.fused_max_u)
    o = svops.ops()
    values = torch.full((B, N, ld), pad, dtype=torch.float32)
    values[:, :, :D] = c["x0"]
    values = values.cuda()
    out = alloc_fast_out(B, N, D, "cuda")
    for k in OUT:
        out[k].fill_(3)                       # a reverted first step must leave these
    work = fast_work(B, D, "cuda")
    pend = None
    if defer:
        pend = (torch.full((B * U, D), 0.75, device="cuda"), (torch.arange(B * U, device="cuda") % U) % N,
                torch.full((B * U,), ZERO_VARIANCE, dtype=torch.int32, device="cuda"))
    steps = []
    for orc, rows in c["batches"]:
        rows_d, orc_d = rows.reshape(B * U, D).cuda(), orc.reshape(-1).cuda()
        st = torch.full((B * U,), -7, dtype=torch.int32, device="cuda")
        kw = dict(zip(("pend_rows", "pend_oracle", "pend_status"), pend)) if defer else {}
        o.fast_round(values, None, D, f, True, 1.0, out["c1"], out["consensus"], out["skew"], out["kurt"], out["rel"],
                     out["qr"], out["reliable"], out["status"], 0, 0, 0, False, work, None,
                     upd_rows=rows_d, upd_oracle=orc_d, upd_status=st, upd_per_inst=U, **kw)
        if defer:
            pend = (rows_d, orc_d, st)
        else:
            o.commit_updates(rows_d, orc_d, st, values, U)
        torch.cuda.synchronize()
        steps.append(dict(upd_status=st.cpu().view(B, U), values=values.cpu(), status=out["status"].cpu(),
                          **{k: out[k].cpu() for k in OUT}))
    if defer:
        o.commit_updates(*pend, values, U)
        torch.cuda.synchronize()
    _RUNS[key] = dict(steps=steps, final=values.cpu(), ld=ld, pad=pad)
    return _RUNS[key]


def _check(s, run, defer, tag):
    """Statuses, state and outputs of every step against the model."""
    c = fc.build(s)
    D = s.D
    init = {k: torch.full_like(run["steps"][0][k], 3) for k in OUT}
    for step, (got, m) in enumerate(zip(run["steps"], c["steps"])):
        t = "%s %s step %d" % (tag, fc.shape_id(s), step)
        fc.same(got["upd_status"], m["upd_status"], t, "upd_status [instance, slot]")
        fc.same(got["status"], m["status"], t, "status [instance]")
        fc.same(got["values"][:, :, :D], c["lag"][step] if defer else m["values"], t,
                ("lagging values" if defer else "values") + " [instance, oracle, column]")
        assert (got["values"][:, :, D:] == run["pad"]).all(), (t, "pad columns written")
        ok = (m["status"] == OK).nonzero().flatten()
        o = {k: got[k][ok] for k in OUT}
        o["status"] = got["status"][ok]
        fast_cases.check_round(o, fc.round_case(c, step, ok), t)
        before = run["steps"][step - 1] if step else init
        for b in (m["status"] != OK).nonzero().flatten().tolist():
            for k in OUT:
                fc.same(got[k][b], before[k][b], t, "reverted instance %d wrote %s" % (b, k))
    fc.same(run["final"][:, :, :D], c["steps"][-1]["values"], tag + " " + fc.shape_id(s),
            "state after the final commit [instance, oracle, column]")
    assert (run["final"][:, :, D:] == run["pad"]).all()


@pytest.mark.parametrize("s", FUSED)
def test_fused_round_and_commit_kernel(s):
    """(a) every case, the commit kernel after every round."""
    _check(s, _run(s, False), False, "fused")


@pytest.mark.parametrize("s", DEFER)
def test_deferred_commit(s):
    """(b) three launches with a pending batch each, then the commit kernel for the last batch: the lagging
    ``values`` after every launch (launch.hpp, FastParams.pend_rows) and the exact state at the end."""
    _check(s, _run(s, True), True, "deferred")


@pytest.mark.parametrize("name", ["256x64x32-U128", "128x130x24-U20", "7x6x2-U3"])
def test_op_refuses_pending_batch(name):
    """U = 128 and D % 4 != 0: no deferred commit (a refused call, not a launch)."""
    s = by_id[name]
    c = fc.build(s)
    N, D, U, B = s.N, s.D, s.U, c["B"]
    assert not fc.deferred(s)
    values = torch.zeros(B, N, _round_up(D, 8), device="cuda")
    out = alloc_fast_out(B, N, D, "cuda")
    rows = torch.rand(B * U, D, device="cuda")
    orc = torch.arange(B * U, device="cuda") % U
    st, st2 = (torch.zeros(B * U, dtype=torch.int32, device="cuda") for _ in range(2))
    with pytest.raises(RuntimeError, match="deferred commit"):
        svops.ops().fast_round(values, None, D, s.f, True, 1.0, out["c1"], out["consensus"], out["skew"], out["kurt"],
                               out["rel"], out["qr"], out["reliable"], out["status"], 0, 0, 0, False,
                               fast_work(B, D, "cuda"), None, upd_rows=rows, upd_oracle=orc, upd_status=st,
                               upd_per_inst=U, pend_rows=rows.clone(), pend_oracle=orc, pend_status=st2)
    torch.cuda.synchronize()
    assert int(out["status"].min()) == -1 and int(st.abs().sum()) == 0      # nothing ran


@pytest.mark.parametrize("name,defer", [("64x260x8-U40", False), ("256x72x32-U256", False),
                                        ("128x132x8-U64", True), ("64x4100x8-U8", True)])
def test_cleanup_reads_batch_and_pending_rows(name, defer, monkeypatch):
    """(c) SVOC_WIN_CANCEL = 0.5 sends every column through the exact recomputation (cleanup_col reading batch
    and pending rows), 1e30 none but those the kernel never trusts: both meet the model, and agree exactly in
    everything but the moments."""
    s = by_id[name]
    runs = {}
    for cancel in ("0.5", "1e30"):
        monkeypatch.setenv("SVOC_WIN_CANCEL", cancel)
        runs[cancel] = _run(s, defer, cancel=cancel)
        _check(s, runs[cancel], defer, "cancel=%s%s" % (cancel, " deferred" if defer else ""))
    for step, (a, b) in enumerate(zip(runs["0.5"]["steps"], runs["1e30"]["steps"])):
        for k in ("reliable", "c1", "consensus", "upd_status", "status", "values"):
            fc.same(a[k], b[k], "%s step %d" % (name, step), "%s between the two settings" % k)


@pytest.mark.parametrize("defer", [False, True])
def test_state_pitch_beyond_the_row(defer):
    """(d) ld = round_up(D, 8) + 8 with the state's pad columns at 2.0: no INTERVAL_INPUT from them, the pad
    intact (_check), and every output as with the tight pitch."""
    s = by_id["128x132x8-U64"]
    wide, tight = _run(s, defer, extra_ld=8, pad=2.0), _run(s, defer)
    assert wide["ld"] == tight["ld"] + 8
    _check(s, wide, defer, "ld+8")
    for step, (a, b) in enumerate(zip(wide["steps"], tight["steps"])):
        for k in OUT + ("upd_status", "status"):
            fc.same(a[k], b[k], "step %d" % step, "%s between the two pitches" % k)
        fc.same(a["values"][:, :, :s.D], b["values"][:, :, :s.D], "step %d" % step, "values between the two pitches")


def test_engine_open_pipeline_two_lane_groups():
    """(e) the engine over the NSEG = 2 case: three open steps (fused, commit deferred), one join."""
    s = by_id["128x132x8-U64"]
    c = fc.build(s)
    N, D, f, U, B = s.N, s.D, s.f, s.U, c["B"]
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    e = ConsensusEngine(cfg, batch=B, device="cuda", mode="fast", storage="fp32")
    e.randomize(seed=1)
    e.values[:, :, :D] = c["x0"].cuda()
    e.run_round(only_touched=False)
    assert (e._route().lane_groups, e._route().win_h) == (2, 5)
    inst = torch.arange(B, device="cuda").repeat_interleave(U)
    for orc, rows in c["batches"]:
        bat = (inst, orc.reshape(-1).cuda(), rows.reshape(B * U, D).cuda())
        assert e._fused_ok(*bat, U)
        e.step_pipelined(*bat, U, chunks=2, overlap=True)
        assert e._defer is not None
    e.pipeline_join()
    torch.cuda.synchronize()
    assert e._defer is None
    m = c["steps"][-1]
    st = e._last_st.cpu().view(B, U)
    fc.same(st, m["upd_status"], "engine", "upd_status [instance, slot]")
    fc.same(e.status.cpu(), m["status"], "engine", "status [instance]")
    fc.same(e.values[:, :, :D].cpu(), m["values"], "engine", "values [instance, oracle, column]")
    ok = (m["status"] == OK).nonzero().flatten()
    assert ok.numel() == B
    o = {k: getattr(e, k).cpu()[ok] for k in OUT + ("status",)}
    fast_cases.check_round(o, fc.round_case(c, fc.STEPS - 1, ok), "engine %s" % fc.shape_id(s))
