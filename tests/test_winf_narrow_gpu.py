"""Narrow stored window of the fp32 window kernel (consensus_fast_winf.hip, N = 256, whole constrained rounds;
FastParams.win_hint): an instance whose hint is set stores and reads only HS keys on either side of the column
median, and a column whose pass-2 pair may lie outside that range gets the exact median in the cleanup.

References: the same op without ``win_hint`` (the wide path: every output, status, reliable flag, qr and rel
bit for bit) and svoc/ops/torch_ref.py (as tests/test_f32_gpu.py compares).  The columns that must fall back
are computed on the CPU by a numpy model of the trust predicate (`_untrusted`): with k = 17 - HS, a column is
trusted when at least k removed keys lie strictly below the lowest stored key (full sorted position 128 - HS)
and at least k strictly above the highest (position 127 + HS).
"""
import numpy as np
import pytest
import torch

from helpers import alloc_fast_out, beta_oracles, fast_work
from svoc import ops as svops
from svoc.ops import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, F, H = 256, 32, 17
KEYS = ("status", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable")


def _hs():
    return svops.fast_win_narrow_hs()


def _round(xg, D, hint=None, stats=None, mode=0, out=None, work=None):
    o = out if out is not None else alloc_fast_out(xg.shape[0], N, D, DEV)
    svops.ops().fast_round(xg, None, D, F, True, 1.0, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"],
                           o["qr"], o["reliable"], o["status"], 0, mode, 0, False, work, stats, win_hint=hint)
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


def _vs_torch_ref(o, x, D):
    ref = torch_ref.fast_round(x[:, :, :D].to(DEV), F, True)
    assert (o["status"] == 0).all(), o["status"]
    assert torch.equal(o["c1"], ref["c1"].float())
    assert torch.equal(o["reliable"].bool(), ref["reliable"])
    assert torch.equal(o["consensus"], ref["consensus"])
    torch.testing.assert_close(o["qr"], ref["qr"].float(), rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(o["rel"], ref["rel"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(o["skew"], ref["skew"], rtol=1e-3, atol=5e-4)
    torch.testing.assert_close(o["kurt"], ref["kurt"], rtol=1e-3, atol=5e-4)


def _untrusted(x, reliable, D, only=None):
    """[B, D] bool: the columns a narrow round must recompute (numpy model of the kernel's trust predicate, on
    the kernel's keys: the value's word with the sign bit flipped, so -0.0 sorts just below +0.0).  `only`: the
    instances whose round committed (a reverted round writes no reliable flags; its row stays False)."""
    hs = _hs()
    k = H - hs
    keys = np.ascontiguousarray(x[:, :, :D].numpy()).view(np.uint32) ^ np.uint32(0x80000000)
    full = np.sort(keys, axis=1)
    w_lo, w_hi = full[:, N // 2 - hs, :], full[:, N // 2 - 1 + hs, :]
    rel = reliable.cpu().numpy().astype(bool)
    out = np.zeros((x.shape[0], D), dtype=bool)
    for b in (range(x.shape[0]) if only is None else only):
        rem = np.sort(keys[b][~rel[b]], axis=0)     # [F, D]
        assert rem.shape[0] == F
        out[b] = ~((rem[k - 1] < w_lo[b]) & (rem[F - k] > w_hi[b]))
    return out


def _sym(B, D, seed):
    x, is_fail = beta_oracles(B, N, D, F, seed=seed, dtype=torch.float32)
    return x, is_fail


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("B,D,seed", [(3, 64, 1), (4, 128, 2), (5, 100, 3)])
def test_symmetric_second_round_is_narrow(B, D, seed):
    """Beta(20,20) honest rows, U(0,1) failing rows: the first round (hint zero: wide) sets the hint, the second
    is narrow, needs no fallback column (the model says so for this seed) and returns what the wide path does."""
    x, _ = _sym(B, D, seed)
    xg = x.to(DEV)
    wide = _round(xg, D)
    expect = int(_untrusted(x, wide["reliable"], D).sum())
    print(f"D {D}: model fallback columns {expect}")
    assert expect == 0
    hint, stats, work = _hint(B, 0), _stats(), fast_work(B, D, DEV)
    first = _round(xg, D, hint, stats, work=work)
    assert stats.tolist()[1:] == [0, 0] and hint.tolist() == [1] * B
    second = _round(xg, D, hint, stats, work=work)
    torch.cuda.synchronize()
    print(f"D {D}: stats {stats.tolist()} hint {hint.tolist()}")
    assert stats.tolist()[1:] == [B, expect]
    assert hint.tolist() == [1] * B
    _same(first, wide)
    _same(second, wide)
    _vs_torch_ref(second, x, D)


# ------------------------------------------------------------------------------------------------ 2
def _one_sided(B, D, seed, value):
    x, is_fail = _sym(B, D, seed)
    x[:, :, :D] = torch.where(is_fail[:, :, None], torch.tensor(value), x[:, :, :D])
    return x


@pytest.mark.parametrize("value", [0.0, 1.0])
@pytest.mark.parametrize("B,D", [(3, 64), (6, 128), (4, 100)])
def test_one_sided_rows_fall_back_everywhere(B, D, value):
    """All 32 failing rows at one end: the pass-2 pair sits 16 ranks from the middle, outside every narrow window.
    With the hint forced to narrow every column falls back, the outputs are the wide path's, the hint reads wide
    afterwards and the next round counts as wide."""
    x = _one_sided(B, D, 11, value)
    xg = x.to(DEV)
    wide = _round(xg, D)
    assert _untrusted(x, wide["reliable"], D).all()
    hint, stats = _hint(B, 1), _stats()
    nar = _round(xg, D, hint, stats)
    torch.cuda.synchronize()
    print(f"D {D} value {value}: stats {stats.tolist()} hint {hint.tolist()}")
    assert stats.tolist()[1:] == [B, B * D]
    assert hint.tolist() == [0] * B
    _same(nar, wide)
    _vs_torch_ref(nar, x, D)
    again = _round(xg, D, hint, stats)
    torch.cuda.synchronize()
    assert stats.tolist()[1:] == [B, B * D] and hint.tolist() == [0] * B
    _same(again, wide)


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("B,D", [(3, 64), (4, 128), (5, 100)])
def test_mixed_columns_only_the_expected_fall_back(B, D):
    """Columns with k of the 32 failing values below every honest row and 32 - k above: the pair shifts by
    |k - 16| ranks, inside the stored range up to HS - 1 (k = 17 - HS and 15 + HS are the last trusted ones) and
    outside from HS on.  Symmetric U(0,1) columns in between.  Only the model's columns are counted."""
    hs = _hs()
    x, is_fail = _sym(B, D, 21)
    ks = [0, 16 - hs - 1, 16 - hs, 16 - hs + 1, 16 - hs + 2, 8, 16, 24, 16 + hs - 2, 16 + hs - 1, 16 + hs, 16 + hs + 1, 32]
    cols = {}
    for b in range(B):
        rows = torch.nonzero(is_fail[b]).flatten()
        for i, k in enumerate(ks):
            c = (3 + 4 * i + b) % D          # (other columns per instance; the rest stay symmetric)
            x[b, rows[:k], c] = 0.0
            x[b, rows[k:], c] = 1.0
            cols[(b, c)] = k
    xg = x.to(DEV)
    wide = _round(xg, D)
    bad = _untrusted(x, wide["reliable"], D)
    for (b, c), k in cols.items():
        assert bad[b, c] == (not (H - hs <= k <= F - (H - hs))), (b, c, k)
    hint, stats = _hint(B, 1), _stats()
    nar = _round(xg, D, hint, stats)
    torch.cuda.synchronize()
    print(f"D {D}: model {bad.sum(1).tolist()} stats {stats.tolist()} hint {hint.tolist()}")
    assert stats.tolist()[1:] == [B, int(bad.sum())]
    assert hint.tolist() == [int(n <= D // 64) for n in bad.sum(1)]
    _same(nar, wide)
    _vs_torch_ref(nar, x, D)


# ------------------------------------------------------------------------------------------------ 4
def test_ties_signed_zeros_and_zero_variance():
    """Values on a 1/16 grid (runs of equal keys straddle the stored ends), a column whose middle is a run of
    +0.0 and -0.0 (equal values, different keys), failing rows at +-0.0, and in one instance a zero-variance
    column: the narrow round matches the wide one, the reverted instance included."""
    B, D = 4, 128
    x, is_fail = _sym(B, D, 31)
    x[:, :, :D] = torch.round(x[:, :, :D] * 16) / 16
    for b in range(B):
        fr, hr = torch.nonzero(is_fail[b]).flatten(), torch.nonzero(~is_fail[b]).flatten()
        x[b, hr[:130], 5] = 0.0
        x[b, hr[:130:2], 5] = -0.0
        x[b, fr, 9] = 0.0
        x[b, fr[::2], 9] = -0.0
        x[b, fr[:16], 17] = 0.4375       # failing values inside the honest rows' grid
        x[b, fr[16:], 17] = 0.5625
    x[2, :, 40] = 0.375                  # zero variance: the round reverts
    xg = x.to(DEV)
    wide = _round(xg, D)
    st = wide["status"].tolist()
    assert st[2] != 0 and st[0] == st[1] == st[3] == 0, st
    ok = [b for b in range(B) if st[b] == 0]
    bad = _untrusted(x, wide["reliable"], D, ok)
    hint, stats = _hint(B, 1), _stats()
    nar = _round(xg, D, hint, stats)
    torch.cuda.synchronize()
    print(f"model {bad.sum(1).tolist()} stats {stats.tolist()} hint {hint.tolist()} status {st}")
    _same(nar, wide)
    assert bad[ok][:, 9].all()
    assert stats.tolist()[1:] == [len(ok), int(bad[ok].sum())]
    assert hint.tolist()[2] == 1         # (the reverted round leaves its hint alone)


# ------------------------------------------------------------------------------------------------ 5
def test_cancellation_and_window_fallback_together(monkeypatch):
    """SVOC_WIN_CANCEL = 0.5 lists every column for the exact moments; one-sided columns are listed for their
    window as well, the others for the moments alone."""
    monkeypatch.setenv("SVOC_WIN_CANCEL", "0.5")
    B, D = 3, 128
    x, is_fail = _sym(B, D, 41)
    for b in range(B):
        x[b, torch.nonzero(is_fail[b]).flatten(), 7 + b] = 0.0
    xg = x.to(DEV)
    wide = _round(xg, D)
    bad = _untrusted(x, wide["reliable"], D)
    assert all(bad[b, 7 + b] for b in range(B))
    hint, stats = _hint(B, 1), _stats()
    nar = _round(xg, D, hint, stats)
    torch.cuda.synchronize()
    print(f"model {bad.sum(1).tolist()} stats {stats.tolist()}")
    assert stats.tolist()[1:] == [B, int(bad.sum())]
    _same(nar, wide)
    _vs_torch_ref(nar, x, D)
    monkeypatch.setenv("SVOC_WIN_CANCEL", "1e30")     # ... and the window alone
    wide2 = _round(xg, D)
    nar2 = _round(xg, D, _hint(B, 1), stats)
    torch.cuda.synchronize()
    _same(nar2, wide2)


# ------------------------------------------------------------------------------------------------ 6
def _engine_stream(steps, U, overlap, joins):
    """A 4-instance engine through `steps` pipelined steps whose failing rows are U(0,1), except at step 3 (all
    0.0); after the steps in `joins` the state is read back.  Returns the snapshots and the counters."""
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    B, D = 4, 64
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=F, constrained=True)
    e = ConsensusEngine(cfg, batch=B, device=DEV, mode="fast", storage="fp32")
    e.randomize(seed=5)
    fm = e.failing_mask.cpu()
    snaps = []
    for s in range(1, steps + 1):
        fresh, _ = beta_oracles(B, N, D, F, seed=100 + s, dtype=torch.float32)
        inst, orc, rows = [], [], []
        for b in range(B):
            fr, hr = torch.nonzero(fm[b]).flatten(), torch.nonzero(~fm[b]).flatten()
            o = torch.cat([fr, hr])[:U] if U < N else torch.arange(N)
            v = fresh[b, o, :D].clone()
            v[fm[b][o]] = 0.0 if s == 3 else torch.rand(int(fm[b][o].sum()), D, generator=torch.Generator().manual_seed(7 * s + b))
            inst.append(torch.full((len(o),), b))
            orc.append(o)
            rows.append(v)
        e.step_pipelined(torch.cat(inst).to(DEV), torch.cat(orc).to(DEV), torch.cat(rows).to(DEV), U, chunks=2,
                         overlap=overlap)
        if s in joins:
            e.pipeline_join()
            torch.cuda.synchronize()
            snap = {k: getattr(e, k).clone() for k in ("status", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable")}
            snap["values"] = e.values.clone()
            snap["upd_status"] = e._last_st.clone()
            snaps.append(snap)
    return snaps, e.net_stats()


@pytest.mark.parametrize("U,overlap,joins", [(64, True, (1, 2, 3, 4)), (64, True, (2, 4)), (64, False, (1, 2, 3, 4)),
                                             (256, False, (2, 3, 4))])
def test_engine_streams_match_the_wide_engine(U, overlap, joins, monkeypatch):
    """The fused, deferred-commit and U = 256 instantiations under the engine: a stream whose failing rows turn
    one-sided at step 3 and symmetric again, against the same engine with SVOC_WIN_NARROW=0 after every join."""
    B, D = 4, 64
    nar, ns = _engine_stream(4, U, overlap, joins)
    monkeypatch.setenv("SVOC_WIN_NARROW", "0")
    wide, ws = _engine_stream(4, U, overlap, joins)
    print(f"U {U} overlap {overlap} joins {joins}: narrow {ns} wide {ws}")
    assert ws["narrow_rounds"] == 0 and ws["narrow_fallback_cols"] == 0
    # step 1 wide (hint zero), steps 2 and 3 narrow, step 3 falls back everywhere and step 4 is wide again
    assert ns["narrow_rounds"] == 2 * B
    assert B * D <= ns["narrow_fallback_cols"] <= B * D + B * (D // 64)
    assert len(nar) == len(wide) == len(joins)
    for a, w in zip(nar, wide):
        assert (a["status"] == 0).all()
        _same(a, w, KEYS + ("values", "upd_status"))


# ------------------------------------------------------------------------------------------------ 7
def test_split_modes_and_hintless_calls_stay_wide():
    """Modes 1 and 2 (the D-sharded halves) ignore the hint, and a call without it is wide: no narrow round is
    counted, and the hint is not written."""
    B, D = 3, 128
    x, _ = _sym(B, D, 51)
    xg = x[:, :, :D].contiguous().to(DEV)
    stats, hint, work = _stats(), _hint(B, 1), fast_work(B, D, DEV)
    whole = _round(xg, D, None, stats)
    o = alloc_fast_out(B, N, D, DEV)
    _round(xg, D, hint, stats, mode=1, out=o, work=work)
    _round(xg, D, hint, stats, mode=2, out=o, work=work)
    torch.cuda.synchronize()
    assert stats.tolist()[1:] == [0, 0] and hint.tolist() == [1] * B
    assert (o["status"] == 0).all()
    for k in ("c1", "consensus", "reliable"):
        assert torch.equal(o[k], whole[k]), k
