"""Huge finite outliers (2^20 .. 2^126) in at most n_failing rows: data, fp64 reference and the CPU fast engine.

Runs without a GPU.  fast_extreme_cases.make asserts the preconditions of every case (conditions, not
measurements: a shape that misses one gets another seed, never a wider threshold); the CPU twin
(reference_cpu.cpp fast_round_one) then meets check_extreme on every case, whole and as two column shards, the
clamp of the first reliability is swept over max_spread, and a transactional engine step carries such rows.
check_extreme itself is shown to fail on each poisoned output.  test_fast_extreme_gpu.py runs the HIP kernels on
the same cached cases.
"""
import math

import numpy as np
import pytest
import torch

import fast_cases as fc
import fast_extreme_cases as xc
import fast_shard_cases as sc
import track_cases as tc
from helpers import beta_oracles, run_fast
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine
from svoc.status import Status

CASES = xc.matrix()
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("case", CASES, ids=xc.case_id)
def test_preconditions(case):
    c = xc.make(case)          # (asserts them)
    xc.preconditions(c)
    assert len(c["inst"]) == 20 and {t for t, _, _, _ in c["inst"]} == {"T0", "T1", "T2", "T3"}
    q32 = c["ref"]["qr"].float()
    for b, (tier, _, _, _) in enumerate(c["inst"]):
        assert bool(torch.isinf(q32[b]).any()) == (tier in ("T2", "T3")), (b, tier)


@pytest.mark.parametrize("case", CASES, ids=xc.case_id)
def test_cpu_engine_vs_ref64(case):
    c = xc.make(case)
    o = run_fast(c["x"], c["D"], c["f"], False, c["max_spread"])
    xc.check_extreme(o, c, "cpu " + xc.case_id(case))


@pytest.mark.parametrize("case", xc.split_matrix(), ids=xc.case_id)
def test_cpu_engine_split_modes(case):
    xc.shard_round(xc.make_split(case), sc.cpu_launch, "cpu split " + xc.case_id(case))


def test_check_extreme_has_teeth():
    """Each output poisoned in turn: check_extreme must fail."""
    case = (64, 33, 8, "fp32")
    c = xc.make(case)
    good = run_fast(c["x"], c["D"], c["f"], False, c["max_spread"])
    xc.check_extreme(good, c, "teeth")
    b2 = [t for t, _, _, _ in c["inst"]].index("T2")
    row = int(c["outlier"][b2].nonzero()[0])
    assert math.isinf(float(good["qr"][b2, row]))

    def poisoned(key, index, value):
        o = {k: v.clone() for k, v in good.items()}
        o[key][index] = value
        with pytest.raises(AssertionError):
            xc.check_extreme(o, c, "teeth %s" % key)

    for key in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
        poisoned(key, (b2, 1), float("nan"))
    poisoned("reliable", (b2, row), 1)                                   # an outlier trusted
    honest = int(c["expect"][b2].nonzero()[0])
    poisoned("reliable", (b2, honest), 0)
    poisoned("qr", (b2, row), xc.FLT_MAX)                                # finite where inf is expected
    b1 = [t for t, _, _, _ in c["inst"]].index("T1")
    poisoned("qr", (b1, int(c["outlier"][b1].nonzero()[0])), float("inf"))
    poisoned("status", b2, int(Status.RELIABILITY_INTERVAL))
    poisoned("rel", (b2, 0), -2.0 ** -24)                                # below 0, inside the tolerance
    poisoned("rel", (b2, 0), 1e-3)
    poisoned("consensus", (b2, 0), float(good["consensus"][b2, 0]) + 1e-4)
    poisoned("c1", (b2, 0), float(np.nextafter(np.float32(good["c1"][b2, 0]), np.float32(9))))


# ------------------------------------------------------------------------------------------------ the clamp alone
def test_clamp_constants():
    """Every CLAMP_MS value has fl32(ms * fl32(1 / ms)) != 1 -- the reciprocal form of the small kernel's
    reliability then gives 1 - (1 - 2^-24), not 0.  No fp32 value gives a product ABOVE 1 (one binade searched
    exhaustively here; the product of a power-of-two multiple is the same multiple), so the clamped reliability
    cannot fall below 0 through this product: the constants kept are below-1 ones."""
    found, above = xc.clamp_search()
    assert not above and set(xc.CLAMP_MS) <= set(found) and len(xc.CLAMP_MS) >= 3
    for ms in xc.CLAMP_MS:
        m = np.float32(ms)
        assert np.float32(m * np.float32(np.float32(1) / m)) == np.float32(1) - np.float32(2.0 ** -24)
    b = np.arange(0x3F800000, 0x40000000, dtype=np.uint32).view(np.float32)
    prod = (b * (np.float32(1) / b).astype(np.float32)).astype(np.float32)
    assert not (prod > 1).any() and (prod < 1).any()
    # the EXACT product does exceed 1 wherever the reciprocal rounds up: CLAMP_MS_UP holds such values
    for ms in xc.CLAMP_MS:
        assert xc.reciprocal_excess(ms) < 0
    for ms in xc.CLAMP_MS_UP:
        m = np.float32(ms)
        assert np.float32(m * np.float32(np.float32(1) / m)) == 1 and 0 < xc.reciprocal_excess(ms) < 2.0 ** -23


@pytest.mark.parametrize("N,D,f,storage", xc.CLAMP_SHAPES)
def test_cpu_clamp_sweep(N, D, f, storage):
    c = xc.make((N, D, f, storage))
    rows = xc.clamp_rows(c)
    for ms in xc.clamp_spreads(D):
        o = run_fast(c["x"][rows], D, f, False, ms)
        xc.check_clamp(o, c, ms, "cpu clamp")


# ------------------------------------------------------------------------------------------------ through the engine
EN, ED, EF, EB = 16, 24, 3, 8
# per instance: the oracles that send +-2^80 in the second step (sign by position) -- one, f, none
ENGINE_OUTLIERS = [(0,), (15,), (0, 7, 15), (0, 7, 15), (3, 4, 5), (9,), (), ()]
ENGINE_SIGNS = ["+", "-", "+", "alt", "-", "+", "", ""]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("storage", ["bf16", "fp32"])
@pytest.mark.parametrize("track", [False, True], ids=["plain", "track"])
def test_engine_step_with_t2_rows(device, storage, track):
    """A transactional step whose batch carries 2^80 rows for <= f oracles of six of eight instances (the other
    two update one honest row): every update and every round is OK, the rows are stored, nothing is rolled back,
    the outputs meet check_extreme against ref64 of the resulting state, and the track record equals
    track_cases' model on the engine's own qr (a non-finite qmax scores 2^32 for every oracle)."""
    ms = xc.SCALE * math.sqrt(ED)
    cfg = ConsensusConfig(n_oracles=EN, dimension=ED, n_failing_oracles=EF, constrained=False,
                          unconstrained_max_spread=ms, track_oracles=track)
    e = ConsensusEngine(cfg, EB, device=device, mode="fast", storage=storage)
    base, _ = beta_oracles(EB, EN, ED, 0, seed=77, dtype=torch.float64)
    honest = (base[:, :, :ED] * xc.SCALE - xc.SCALE / 2).to(e.vdtype)
    inst = torch.arange(EB).repeat_interleave(EN)
    st = e.step(inst, torch.arange(EN).repeat(EB), honest.reshape(EB * EN, ED))
    e.pipeline_join()
    assert (st.cpu() == 0).all() and (e.status.cpu() == 0).all()
    model = dict(rounds=[0] * EB, flagged=[[0] * EN for _ in range(EB)], streak=[[0] * EN for _ in range(EB)],
                 score=[[0] * EN for _ in range(EB)])

    def model_step(m):
        qr = [[np.float32(v) for v in row] for row in e.qr.cpu().tolist()]
        return tc.model_update(m, e._active.cpu().tolist(), e.status.cpu().tolist(), e.reliable.cpu().tolist(),
                               qr, exact=False)

    if track:
        model = model_step(model)
    fresh, _ = beta_oracles(EB, 1, ED, 0, seed=78, dtype=torch.float64)
    fresh = (fresh[:, 0, :ED] * xc.SCALE - xc.SCALE / 2).to(e.vdtype)
    bi, bo, rows = [], [], []
    want = honest.clone()
    outlier = torch.zeros(EB, EN, dtype=torch.bool)
    for b, (orcs, sign) in enumerate(zip(ENGINE_OUTLIERS, ENGINE_SIGNS)):
        assert len(orcs) <= EF
        for j, o in enumerate(orcs):
            v = -(2.0 ** 80) if sign == "-" or (sign == "alt" and j % 2) else 2.0 ** 80
            bi.append(b); bo.append(o); rows.append(torch.full((ED,), v, dtype=e.vdtype))
            outlier[b, o] = True
        if not orcs:
            bi.append(b); bo.append(5); rows.append(fresh[b])
        for o, r in zip(bo[-max(len(orcs), 1):], rows[-max(len(orcs), 1):]):
            want[b, o] = r
    vals = torch.stack(rows)
    assert torch.isfinite(vals).all()
    st = e.step(torch.tensor(bi), torch.tensor(bo), vals)
    e.pipeline_join()
    assert (st.cpu() == int(Status.OK)).all(), st
    assert (e.status.cpu() == int(Status.OK)).all(), e.status
    assert (e._active.cpu() == 1).all()
    # the rows are stored and nothing else moved: no roll-back
    assert torch.equal(e.values.cpu()[:, :, :ED], want)
    assert (e.enabled.cpu() == 1).all() and (e.n_active.cpu() == EN).all() and e.consensus_active.cpu().all()
    x = e.values.cpu()
    ref = fc.ref64(x[:, :, :ED], EF, False, ms)
    c = dict(x=x, ref=ref, outlier=outlier, expect=xc.constructed_mask(ref["qr"], outlier, EF), max_spread=ms,
             scale=xc.SCALE, N=EN, D=ED, f=EF, storage=storage)
    assert (fc.cut_gap(ref, EF) >= 1e-4).all() and torch.equal(ref["reliable"], c["expect"])
    assert (ref["rel"][:6, 0] == 0).all() and (ref["rel"][6:, 0] > 0.5).all()
    o = {k: getattr(e, k).cpu() for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status")}
    assert torch.isinf(o["qr"][outlier]).all()
    xc.check_extreme(o, c, "engine %s %s" % (device, storage))
    if track:
        model = model_step(model)
        rec = e.track_record()
        for k, w in tc.record_tensors(model).items():
            assert torch.equal(rec[k].cpu(), w), k
        assert model["rounds"] == [2] * EB
        # qmax = +inf in the six instances: their second round scores 2^32 for every oracle
        alone = tc.record_tensors(model_step(dict(rounds=[0] * EB, flagged=[[0] * EN for _ in range(EB)],
                                                  streak=[[0] * EN for _ in range(EB)],
                                                  score=[[0] * EN for _ in range(EB)])))["score"]
        assert (alone[:6] == tc.FAST_ONE).all()
