"""The narrow stored window of the fp32 window kernel (consensus_fast_winf.hip) at every shape that reaches it: fp32,
constrained whole rounds with a hint, 129 <= N <= 256 and a window half-width of 17 -- not only N = 256, f = 32
(tests/test_winf_narrow_gpu.py), whose pass 2 takes the sentinel-free branch.  Everywhere else the removed keys are
padded with sentinels and sorted by the 64-key network, the trust predicate reads sentinels or real keys depending on
f, a window below N = 256 is stored by the tail-slab body alone and the cleanup's counting median ranks padded rows.

References: the same op without a hint (the wide path, bit for bit), fast_cases.ref64 (fp64, plain Python rank rule)
and the CPU model of the trust predicate in tests/winf_narrow_cases.py, whose removed rows come from ref64.  The
model's soundness and the cases' bite are checked on the CPU in tests/test_winf_narrow_cases.py.
"""
import pytest
import torch

import winf_narrow_cases as wc
from fast_cases import TOL, ref64
from helpers import alloc_fast_out, beta_oracles, fast_work
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("status", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable")
FILL = 7.0      # prefill of every float output: an untouched one is told from a written one


def _out(B, N, D):
    o = alloc_fast_out(B, N, D, DEV)
    for k in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
        o[k].fill_(FILL)
    o["reliable"].fill_(3)
    return o


def _round(xg, N, D, f, hint=None, stats=None, legacy=False, active=None, work=None):
    o = _out(xg.shape[0], N, D)
    svops.ops().fast_round(xg, active, D, f, True, 1.0, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"],
                           o["qr"], o["reliable"], o["status"], 0, 0, 0, legacy, work, stats, win_hint=hint)
    return o


def _stats():
    return torch.zeros(3, dtype=torch.int32, device=DEV)


def _hint(B, v):
    return torch.full((B,), v, dtype=torch.int32, device=DEV)


def _same(a, b, keys=KEYS):
    for k in keys:
        # (bit for bit: the float outputs compared as words, so +0.0 / -0.0 and NaN payloads count)
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def _vs_ref64(o, c, tag):
    """The committed instances against the fp64 reference; a reverted one keeps its prefill."""
    ref, ok = c["ref"], c["ok"]
    o = {k: v.cpu() for k, v in o.items()}
    for b in range(c["B"]):
        if b not in ok:
            assert o["status"][b] != 0, (tag, b)
            for k in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
                assert (o[k][b] == FILL).all(), (tag, b, k)
            continue
        assert o["status"][b] == 0, (tag, b, o["status"])
        assert torch.equal(o["reliable"][b].bool(), ref["reliable"][b]), (tag, b, "reliable")
        # one correctly rounded fp32 add of two fp32 values and an exact halving == the fp64 value rounded to fp32
        assert (o["c1"][b].double() == ref["c1"][b].float().double()).all(), (tag, b, "c1")
        bad = torch.nonzero(o["consensus"][b].double() != ref["consensus"][b].float().double()).flatten().tolist()
        assert not bad, (tag, b, "consensus", bad[:8])
        for key, (rtol, atol) in TOL["fp32"].items():
            err = (o[key][b].double() - ref[key][b]).abs()
            frac = float((err / (atol + rtol * ref[key][b].abs())).max())
            assert frac <= 1.0, (tag, b, key, "error / bound = %.3g" % frac)


def _narrow_against_wide(c, tag, work=False):
    """Wide round, forced-narrow round, then a round from the hints the kernel wrote: outputs, counters, hints."""
    N, D, f, B, ok = c["N"], c["D"], c["f"], c["B"], c["ok"]
    fb = c["fallback"] | c["extra"]      # (extra: none but in the conservative corner, winf_narrow_cases.make_corner)
    xg = c["x"].to(DEV)
    w = fast_work(B, D, DEV) if work else None
    wide = _round(xg, N, D, f, legacy=c["legacy"], work=w)
    hint, stats = _hint(B, 1), _stats()
    nar = _round(xg, N, D, f, hint, stats, legacy=c["legacy"], work=w)
    torch.cuda.synchronize()
    n_b = fb.sum(1).tolist()
    after = [wc.hint_after(n_b[b], D) if b in ok else 1 for b in range(B)]
    print(f"{tag}: model {n_b} committed {ok} stats {stats.tolist()} hint {hint.tolist()}")
    _same(nar, wide)
    _vs_ref64(nar, c, tag)
    assert stats.tolist()[1:] == [len(ok), int(fb[ok].sum())], (tag, stats.tolist())
    assert hint.tolist() == after, (tag, hint.tolist(), after)
    again = _round(xg, N, D, f, hint, stats, legacy=c["legacy"], work=w)
    torch.cuda.synchronize()
    _same(again, wide)
    still = [b for b in ok if after[b]]
    assert stats.tolist()[1:] == [len(ok) + len(still), int(fb[ok].sum()) + int(fb[still].sum())], (tag, stats.tolist())
    assert hint.tolist() == after, (tag, hint.tolist())
    return stats.tolist()


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", wc.matrix(), ids=wc.case_id)
def test_narrow_round_at_every_shape(case):
    _narrow_against_wide(wc.make(case), wc.case_id(case))


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("D", wc.D_EDGES)
@pytest.mark.parametrize("N,f", wc.D_EDGE_SHAPES)
def test_d_edges(N, f, D):
    """D below 64 (cap zero), 127 (cap one), 4096 (the last D that runs narrow: the planted columns hit the first and
    last words of the kernel's bit mask, and the cap's worth of them against one more decides the hint) and 4104
    (the narrow instantiation launches and stays wide)."""
    c = wc.make_d_edge(N, f, D)
    tag = f"d_edge-{N}x{D}x{f}"
    if D <= wc.MAX_D:
        _narrow_against_wide(c, tag, work=True)
        return
    xg = c["x"].to(DEV)
    w = fast_work(c["B"], D, DEV)
    wide = _round(xg, N, D, f, work=w)
    hint, stats = _hint(c["B"], 1), _stats()
    nar = _round(xg, N, D, f, hint, stats, work=w)
    torch.cuda.synchronize()
    print(f"{tag}: stats {stats.tolist()} hint {hint.tolist()}")
    assert stats.tolist()[1:] == [0, 0]
    assert hint.tolist() == [0] * c["B"]
    _same(nar, wide)
    _vs_ref64(nar, c, tag)


# ------------------------------------------------------------------------------------------------ 3
def test_inactive_instance_is_left_alone():
    """active[1] = 0 with its hint set: outputs stay prefilled, the hint is untouched, the round is not counted."""
    c = wc.make(("split", 256, 24, 64))
    N, D, f, B, fb = c["N"], c["D"], c["f"], c["B"], c["fallback"]
    xg = c["x"].to(DEV)
    active = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    wide = _round(xg, N, D, f, active=active)
    hint, stats = _hint(B, 1), _stats()
    hint[1] = 5
    nar = _round(xg, N, D, f, hint, stats, active=active)
    torch.cuda.synchronize()
    _same(nar, wide)
    assert nar["status"].tolist() == [0, -1, 0]
    for k in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
        assert (nar[k][1] == FILL).all(), k
    assert (nar["reliable"][1] == 3).all()
    assert stats.tolist()[1:] == [2, int(fb[[0, 2]].sum())]
    assert hint.tolist() == [wc.hint_after(int(fb[0].sum()), D), 5, wc.hint_after(int(fb[2].sum()), D)]
    _vs_ref64(nar, dict(c, ok=[0, 2]), "inactive")


def test_legacy_round_at_a_sentinel_shape():
    c = wc.make_legacy(256, 24, 64)
    _narrow_against_wide(c, "legacy-split-256x64x24")


def test_conservative_corner():
    """A lowest stored key of -0.0 behind a -inf sentinel (both the key 0): the kernel's strict compare sends the
    column to the exact median although the model trusts it.  Sound, and pinned here: one column per instance, and
    the outputs -- a consensus of -0.0 in that column -- are the wide round's and the reference's."""
    c = wc.make_corner()
    assert not c["fallback"].any() and c["extra"].sum(1).tolist() == [1] * c["B"]
    st = _narrow_against_wide(c, "corner-%dx%dx%d" % (wc.CORNER[0], wc.CORNER[2], wc.CORNER[1]))
    assert st[1:] == [2 * c["B"], 2 * c["B"]]


# ------------------------------------------------------------------------------------------------ 4
def _engine_stream(N, f, D, U, overlap, value, steps=4):
    """A 4-instance engine through pipelined steps whose failing rows are U(0,1), except at step 3 (all `value`);
    the state is read back after every step.  Returns the snapshots and the counters."""
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    B = 4
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    e = ConsensusEngine(cfg, batch=B, device=DEV, mode="fast", storage="fp32")
    e.randomize(seed=5)
    fm = e.failing_mask.cpu()
    snaps = []
    for s in range(1, steps + 1):
        fresh, _ = beta_oracles(B, N, D, f, seed=100 + s, dtype=torch.float32)
        inst, orc, rows = [], [], []
        for b in range(B):
            fr, hr = torch.nonzero(fm[b]).flatten(), torch.nonzero(~fm[b]).flatten()
            o = torch.cat([fr, hr])[:U] if U < N else torch.arange(N)
            v = fresh[b, o, :D].clone()
            v[fm[b][o]] = value if s == 3 else torch.rand(int(fm[b][o].sum()), D,
                                                          generator=torch.Generator().manual_seed(7 * s + b))
            inst.append(torch.full((len(o),), b))
            orc.append(o)
            rows.append(v)
        e.step_pipelined(torch.cat(inst).to(DEV), torch.cat(orc).to(DEV), torch.cat(rows).to(DEV), U, chunks=2,
                         overlap=overlap)
        e.pipeline_join()
        torch.cuda.synchronize()
        snap = {k: getattr(e, k).clone() for k in KEYS}
        snap["values"] = e.values.clone()
        snap["upd_status"] = e._last_st.clone()
        snaps.append(snap)
    return snaps, e.net_stats()


@pytest.mark.parametrize("N,f,U,overlap", [(200, 24, 64, True), (200, 24, 64, False), (256, 21, 64, True),
                                           (256, 21, 64, False), (256, 24, 256, False)])
def test_engine_streams_at_sentinel_shapes(N, f, U, overlap, monkeypatch):
    """The fused, deferred-commit and U = 256 instantiations under the engine, at shapes that take the sentinel
    branch: a stream whose failing rows turn one-sided at step 3 (on the side that can fail at this shape), against
    the same engine with SVOC_WIN_NARROW=0 after every step, and the narrow counters -- read through net_stats(),
    also below N = 256 -- against the model run over the states the wide engine went through."""
    B, D = 4, 64
    lo_can, hi_can = wc.sides(N, f)
    value = 0.0 if hi_can else 1.0
    assert hi_can or lo_can
    nar, ns = _engine_stream(N, f, D, U, overlap, value)
    monkeypatch.setenv("SVOC_WIN_NARROW", "0")
    wide, ws = _engine_stream(N, f, D, U, overlap, value)
    assert ws["narrow_rounds"] == 0 and ws["narrow_fallback_cols"] == 0
    maps = []
    for w in wide:
        assert (w["status"] == 0).all()
        x = w["values"][:, :, :D].cpu()
        ref = ref64(x, f, True, 1.0)
        assert torch.equal(w["reliable"].cpu().bool(), ref["reliable"])
        maps.append(wc.untrusted(x, ~ref["reliable"], D))
    rounds, cols = wc.stream_counters(maps, D)
    print(f"{N}x{D}x{f} U {U} overlap {overlap}: model fallback columns {[m.sum(1).tolist() for m in maps]} "
          f"-> rounds {rounds} cols {cols}; narrow {ns} wide {ws}")
    assert maps[2].all()                   # step 3 falls back everywhere ...
    assert rounds == 2 * B                 # ... so steps 2 and 3 are narrow, steps 1 and 4 wide
    assert (ns["narrow_rounds"], ns["narrow_fallback_cols"]) == (rounds, cols)
    assert len(nar) == len(wide) == 4
    for a, w in zip(nar, wide):
        _same(a, w, KEYS + ("values", "upd_status"))
