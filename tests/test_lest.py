"""The rank-weighted (L-estimator) round on the CPU: the op's CPU twin against the fp64 model of lest_cases, the
engine path (rounds, transactional steps, routing of the default config), the configuration and weight validation,
and the checkpoint round trip."""
import math

import pytest
import torch

import lest_cases as lc
from svoc import estimators as est
from svoc import ops as svops
from svoc import state as svstate
from svoc.api import ConsensusService
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine
from svoc.status import Status

DEV = "cpu"


# ------------------------------------------------------------------------------------------------ weights
def test_rank_weights_formula():
    for n, sigma in ((7, 0.125), (64, 0.03), (256, 1.0), (2, 0.125)):
        w = est.rank_weights(n, sigma)
        assert w.dtype == torch.float32 and w.shape == (n,)
        u = [math.exp(-((k - (n - 1) / 2.0) ** 2) / (2.0 * (sigma * n) ** 2)) for k in range(n)]
        want = torch.tensor([v / sum(u) for v in u], dtype=torch.float64).float()
        assert torch.equal(w, want)
        assert torch.equal(w, w.flip(0)) and abs(float(w.double().sum()) - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        est.rank_weights(8, 0.0)
    with pytest.raises(ValueError):
        est.rank_weights(8, float("nan"))


def test_anchor_weights():
    assert est.median_weights(7).tolist() == [0, 0, 0.5, 0.5, 0, 0, 0]      # the contract's dead odd branch
    assert est.median_weights(8).tolist() == [0, 0, 0, 0.5, 0.5, 0, 0, 0]
    assert est.mean_weights(4).tolist() == [0.25] * 4
    assert est.one_hot(5, 3).tolist() == [0, 0, 0, 1, 0]
    assert est.trimmed_mean_weights(6, 1).tolist() == [0, 0.25, 0.25, 0.25, 0.25, 0]
    p = est.pack(est.one_hot(3, 0), est.mean_weights(2))
    assert p.shape == (2, 256) and p[0, :3].tolist() == [1, 0, 0] and p[1, :3].tolist() == [0.5, 0.5, 0]


# ------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
@pytest.mark.parametrize("variant", [v[0] for v in lc.VARIANTS])
@pytest.mark.parametrize("family", lc.MODEL_FAMILIES, ids=lc.family_id)
def test_op_vs_model(shape, variant, family):
    c = lc.case(shape, variant, family)
    lc.check_round(lc.run_case(svops.ops(), c, DEV), c)


def _model_outputs(c):
    """The fp64 model's own outputs in the op's dtypes, reverted / inactive instances poisoned."""
    o = lc.poisoned(lc.B, c["N"], c["D"], DEV)
    st = lc.expected_status(c)
    o["status"].copy_(st)
    for b in range(lc.B):
        if int(st[b]) == lc.ST_OK:
            for k in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
                o[k][b] = c["ref"][k][b].float()
            o["reliable"][b] = c["ref"]["reliable"][b].to(torch.uint8)
    return o


@pytest.mark.parametrize("variant", ["cons", "unc"])
def test_check_round_rejects_bad_outputs(variant):
    """The shared assertions themselves: the model's outputs pass; NaN, inf or an offset in any toleranced output
    of a committed instance, a flipped mask bit, or a write into a reverted instance fail."""
    c = lc.case((64, 33, 8), variant, ("bell", 0.125))
    lc.check_round(_model_outputs(c), c)
    for key in ("c1", "consensus", "skew", "kurt", "rel", "qr"):
        for bad in (float("nan"), float("inf"), None):
            o = _model_outputs(c)
            if bad is None:
                o[key][0, 0] += 1.0
            else:
                o[key][0, 0] = bad
            with pytest.raises(AssertionError):
                lc.check_round(o, c)
        o = _model_outputs(c)
        o[key][0] = float("nan")            # a whole NaN row
        with pytest.raises(AssertionError):
            lc.check_round(o, c)
    o = _model_outputs(c)
    o["reliable"][0, 0] ^= 1
    with pytest.raises(AssertionError):
        lc.check_round(o, c)
    for b in (lc.INACTIVE, lc.CONSTANT):
        o = _model_outputs(c)
        o["consensus"][b, 0] = 0.5
        with pytest.raises(AssertionError):
            lc.check_round(o, c)


def test_check_round_bound_rejects_nan_by_itself():
    """The bound comparison alone (without the finiteness assertion) fails on NaN: `err <= bound` is False."""
    c = lc.case((7, 6, 2), "cons", ("mean",))
    o = _model_outputs(c)
    o["skew"][0, 0] = float("nan")
    real = torch.isfinite
    try:
        torch.isfinite = lambda t: torch.ones_like(t, dtype=torch.bool)
        with pytest.raises(AssertionError, match="skew"):
            lc.check_round(o, c)
    finally:
        torch.isfinite = real


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_one_hot(shape):
    n = lc.check_one_hot(svops.ops(), shape, DEV)
    assert n > 0 or shape[0] - shape[2] < 4


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_median_weights_equal_fast_round(shape):
    n = lc.check_median_vs_fast(svops.ops(), shape, DEV)
    assert n > 0 or shape[0] - shape[2] < 4


def test_zero_weight_contributes_exactly_zero():
    """A huge value under a zero weight leaves the estimate exact: c1 is the order statistic next to it."""
    N, D, f = 8, 3, 0
    x = lc.data(N, D, f, 1.0, 0.0)[:1].clone()
    x[0, 3, :D] = 3e38                       # the top rank of every column
    xs = torch.sort(x[0, :, :D], dim=0).values
    w = est.pack(est.one_hot(N, N - 2), est.mean_weights(N))
    o = lc.run_lest(svops.ops(), x, None, D, f, False, 1e30, w)
    assert int(o["status"][0]) == lc.ST_OK
    assert lc.same_bits(o["c1"][0], xs[N - 2])


def test_op_rejects_bad_arguments():
    ops = svops.ops()
    c = lc.case((7, 6, 2), "cons", ("median",))
    o = lc.poisoned(lc.B, 7, 6, DEV)
    args = lambda x, w: (x, None, 6, 2, True, 1.0, w, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"],
                         o["reliable"], o["status"])
    with pytest.raises(RuntimeError):
        ops.lest_round(*args(c["x"].bfloat16(), c["weights"]))           # fp32 storage only
    with pytest.raises(RuntimeError):
        ops.lest_round(*args(c["x"], c["weights"][:, :128].contiguous()))  # weights [2, 256]
    with pytest.raises(RuntimeError):
        ops.lest_round(*args(c["x"], c["weights"].double()))


def test_lest_route():
    r = svops.lest_route("fp32", 64, 33, 40, 8, True)
    assert (r.supported, r.lane_groups, r.max_n, r.needs_work) == (1, 1, 256, 1)
    assert svops.lest_route("fp32", 65, 33, 40, 8, False).lane_groups == 2
    assert svops.lest_route("fp32", 256, 72, 72, 32, True).lane_groups == 4
    assert svops.lest_route("fp32", 2, 3, 8, 0, True).supported == 1
    for bad in (dict(storage="bf16"), dict(N=257), dict(N=1, n_failing=0), dict(n_failing=63), dict(n_failing=-1),
                dict(legacy=True), dict(mode=1), dict(mode=2), dict(N=256, D=8, ld=1 << 22)):
        kw = dict(storage="fp32", N=64, D=33, ld=40, n_failing=8, constrained=True, legacy=False, mode=0)
        kw.update(bad)
        assert svops.lest_route(**kw).supported == 0, bad
    # fast_route is untouched by the new route
    assert svops.fast_route("fp32", 64, 33, 40, 8, True).kernel == svops.KERNEL_WINDOW


# ------------------------------------------------------------------------------------------------ engine
def _cfg(N=64, D=33, f=8, **kw):
    return ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True, **kw)


def _fill(e, x, D):
    """Every oracle of every instance commits its row of x ([B, N, ld])."""
    B, N = x.shape[:2]
    inst = torch.arange(B).repeat_interleave(N)
    oracle = torch.arange(N).repeat(B)
    return e.apply_updates(inst, oracle, x[:, :, :D].reshape(B * N, D))


def engine_rounds_equal_op(device):
    """apply_updates + run_round twice on (64, 33, 8): the engine's outputs equal the op called directly."""
    N, D, f = 64, 33, 8
    c = lc.case((N, D, f), "cons", ("bell", 0.125))
    x = c["x"]
    e = ConsensusEngine(_cfg(N, D, f, essence="rank_weighted"), lc.B, device=device, storage="fp32")
    assert torch.equal(e._lest.cpu(), c["weights"])
    st = _fill(e, x, D)
    assert (st.cpu() == 0).all()
    e.run_round()
    x2 = x.clone()
    x2[:, 5, :D] = x[:, 6, :D]
    x2[:, 9, :D] = 0.5 * (x[:, 9, :D] + x[:, 10, :D])
    for xk in (x, x2):
        if xk is x2:
            inst = torch.arange(lc.B).repeat_interleave(2)
            oracle = torch.tensor([5, 9]).repeat(lc.B)
            e.apply_updates(inst, oracle, xk[:, [5, 9], :D].reshape(-1, D))
            e.run_round()
        o = lc.run_lest(svops.ops(), xk.to(device), None, D, f, True, 1.0, c["weights"])
        for b in range(lc.B):
            if b == lc.CONSTANT:
                assert int(e.status[b]) == int(Status.ZERO_VARIANCE) == int(o["status"][b])
                continue
            assert int(e.status[b]) == 0
            for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable"):
                assert torch.equal(getattr(e, k)[b].cpu(), o[k][b]), (k, b)
    return e


def test_engine_rounds_equal_op():
    engine_rounds_equal_op(DEV)


def transactional_step_reverts_one_instance(device):
    """A transactional step whose batch makes one instance revert: that instance's rows, enabled flags and n_active
    go back to their pre-batch state and its updates report the round's code (the sequential model of
    tests/txn_cases.py: a reverted transaction leaves no trace); the other instances commit about the new centre."""
    N, D, f = 64, 33, 8
    c = lc.case((N, D, f), "cons", ("bell", 0.125))
    x = c["x"].clone()
    x[lc.CONSTANT, :, 0] = x[0, :, 0]                      # every instance commits at first
    e = ConsensusEngine(_cfg(N, D, f, essence="rank_weighted"), lc.B, device=device, storage="fp32")
    assert e.transactional
    _fill(e, x, D)
    e.run_round()
    assert (e.status.cpu() == 0).all()
    before = {k: getattr(e, k).clone() for k in ("values", "enabled", "n_active", "consensus", "c1", "qr", "reliable")}
    # the batch: every instance updates oracles 3 and 7; instance 1 is handed a whole constant column 0 (all N
    # oracles), so its round reverts with ZERO_VARIANCE
    bad = 1
    others = torch.tensor([b for b in range(lc.B) if b != bad])
    inst = torch.cat([others.repeat_interleave(2), torch.full((N,), bad)])
    oracle = torch.cat([torch.tensor([3, 7]).repeat(lc.B - 1), torch.arange(N)])
    rows = torch.cat([0.5 * (x[others][:, [3, 7], :D] + x[others][:, [4, 8], :D]).reshape(-1, D),
                      x[bad, :, :D].clone()])
    rows[2 * (lc.B - 1):, 0] = 0.25
    st = e.step(inst, oracle, rows).cpu()
    is_bad = inst == bad
    assert (st[is_bad] == int(Status.ZERO_VARIANCE)).all() and (st[~is_bad] == 0).all()
    assert int(e.status[bad]) == int(Status.ZERO_VARIANCE)
    for k, v in before.items():
        assert torch.equal(getattr(e, k)[bad], v[bad]), ("reverted instance", k)
    want = x.clone()
    want[:, [3, 7], :D] = 0.5 * (x[:, [3, 7], :D] + x[:, [4, 8], :D])
    o = lc.run_lest(svops.ops(), want.to(device), None, D, f, True, 1.0, c["weights"])
    for b in range(lc.B):
        if b == bad:
            continue
        assert torch.equal(e.values[b].cpu(), want[b])
        assert int(e.status[b]) == 0 and int(e.n_active[b]) == N
        for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable"):
            assert torch.equal(getattr(e, k)[b].cpu(), o[k][b]), (k, b)


def test_transactional_step_reverts_one_instance():
    transactional_step_reverts_one_instance(DEV)


def default_config_never_calls_lest(device, monkeypatch):
    """The default essence keeps its route and its op: lest_round is never reached."""
    N, D, f = 64, 33, 8
    calls = []

    class Spy:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name == "lest_round":
                calls.append(name)
            return getattr(self._real, name)

    e = ConsensusEngine(_cfg(N, D, f), lc.B, device=device, storage="fp32")
    assert e.cfg.essence == "smooth_median" and e._lest is None
    assert e._route() == svops.fast_route("fp32", N, D, e.ld, f, True, False, 0, 0, svops.WORK_CALLER)
    monkeypatch.setattr(e, "_ops", Spy(e._ops))
    x = lc.case((N, D, f), "cons", ("median",))["x"]
    _fill(e, x, D)
    e.run_round()
    assert not calls and int(e.status[0]) == 0
    o = lc.run_lest(svops.ops(), x.to(device), None, D, f, True, 1.0, lc.case((N, D, f), "cons", ("median",))["weights"])
    assert lc.same_bits(e.consensus[0].cpu(), o["consensus"][0])
    # ... and a rank-weighted engine does reach it
    e2 = ConsensusEngine(_cfg(N, D, f, essence="rank_weighted"), lc.B, device=device, storage="fp32")
    monkeypatch.setattr(e2, "_ops", Spy(e2._ops))
    _fill(e2, x, D)
    e2.run_round()
    assert calls == ["lest_round"]
    assert not e2._fused_ok(None, None, None, 1) and not e2._kernel_rollback_ok(1)


def test_default_config_never_calls_lest(monkeypatch):
    default_config_never_calls_lest(DEV, monkeypatch)


def test_config_validation():
    assert ConsensusConfig().essence == "smooth_median" and ConsensusConfig().rank_sigma == 0.125
    ConsensusConfig(essence="rank_weighted", rank_sigma=0.5).validate()
    for kw in (dict(essence="bell"), dict(rank_sigma=0.0), dict(rank_sigma=-1.0), dict(rank_sigma=float("nan")),
               dict(rank_sigma=float("inf"))):
        with pytest.raises(ValueError):
            ConsensusConfig(**kw).validate()
    # old-style dicts (no essence / rank_sigma keys) load as the smooth median; unknown keys are ignored
    old = {k: v for k, v in ConsensusConfig().to_dict().items() if k not in ("essence", "rank_sigma")}
    old["some_future_key"] = 1
    assert ConsensusConfig.from_dict(old).essence == "smooth_median"


def test_engine_refuses_what_the_round_does_not_cover():
    rw = dict(essence="rank_weighted")
    mk = lambda cfg, **kw: ConsensusEngine(cfg, 2, device=DEV, **kw)
    with pytest.raises(ValueError):
        mk(_cfg(**rw), mode="exact")
    with pytest.raises(ValueError):
        mk(_cfg(**rw), storage="bf16")
    with pytest.raises(ValueError):
        mk(_cfg(**rw))                                        # the default storage is bf16
    with pytest.raises(ValueError):
        mk(_cfg(variant="nd_legacy", **rw), storage="fp32")
    with pytest.raises(ValueError):
        mk(_cfg(N=300, D=8, f=8, **rw), storage="fp32")
    with pytest.raises(ValueError):
        mk(_cfg(N=8, D=8, f=7, **rw), storage="fp32")         # n_failing > N - 2
    with pytest.raises(ValueError):
        mk(_cfg(), storage="fp32", rank_weights=(est.mean_weights(64), est.mean_weights(56)))   # needs the essence
    N, R = 64, 56
    good = (est.mean_weights(N), est.trimmed_mean_weights(R, 4))
    e = mk(_cfg(**rw), storage="fp32", rank_weights=good)
    w1, w2 = e.rank_weight_rows()
    assert torch.equal(w1, good[0]) and torch.equal(w2, good[1]) and float(e._lest[1, R:].abs().sum()) == 0.0
    neg = est.mean_weights(N).clone()
    neg[0], neg[1] = -neg[0], 3 * neg[1]
    off = est.mean_weights(N) * (1 + 1e-3)
    nan = est.mean_weights(N).clone()
    nan[5] = float("nan")
    for w1 in (neg, est.mean_weights(N - 1), est.mean_weights(N + 1), off, nan):
        with pytest.raises(ValueError):
            mk(_cfg(**rw), storage="fp32", rank_weights=(w1, good[1]))
    for w2 in (est.mean_weights(N), off[:R], nan[:R]):
        with pytest.raises(ValueError):
            mk(_cfg(**rw), storage="fp32", rank_weights=(good[0], w2))
    with pytest.raises(ValueError):
        mk(_cfg(**rw), storage="fp32", rank_weights=good[0])


def test_engine_asks_its_own_route():
    """The limits and the workspace need of a rank-weighted engine come from lest_route, small shapes included."""
    e = ConsensusEngine(_cfg(N=7, D=6, f=2, essence="rank_weighted"), 2, device=DEV, storage="fp32")
    assert e._lest_route == svops.lest_route("fp32", 7, 6, e.ld, 2, True) and e._lest_route.needs_work == 1
    assert e.work() is None                                   # CPU: no workspace at all
    assert ConsensusEngine(_cfg(), 2, device=DEV, storage="fp32")._lest_route is None


def test_run_round_sharded_not_implemented():
    from svoc.parallel.dshard import run_round_sharded
    e = ConsensusEngine(_cfg(essence="rank_weighted"), 2, device=DEV, storage="fp32")
    with pytest.raises(NotImplementedError):
        run_round_sharded(e, 66)


# ------------------------------------------------------------------------------------------------ checkpoints
def _service(cfg, x, D, device, **kw):
    N = cfg.n_oracles
    svc = ConsensusService(cfg, lc.B, list(range(1, cfg.n_admins + 1)), list(range(100, 100 + N)), device=device,
                           mode="fast", storage="fp32", **kw)
    _fill(svc.engine, x, D)
    svc.engine.run_round()
    return svc


def checkpoint_round_trip(device, tmp_path, explicit):
    N, D, f = 64, 33, 8
    x = lc.case((N, D, f), "cons", ("bell", 0.125))["x"]
    kw = dict(rank_weights=(est.trimmed_mean_weights(N, 8), est.trimmed_mean_weights(N - f, 6))) if explicit else {}
    svc = _service(_cfg(N, D, f, essence="rank_weighted", rank_sigma=0.2), x, D, device, **kw)
    path = str(tmp_path / ("lest_%d.svoc" % explicit))
    svstate.save(svc, path)
    back = svstate.load(path, device=device)
    e, e2 = svc.engine, back.engine
    assert back.cfg.essence == "rank_weighted" and back.cfg.rank_sigma == 0.2
    assert e2._lest is not None and lc.same_bits(e2._lest.cpu(), e._lest.cpu())
    assert e2._lest_explicit == explicit
    if explicit:
        assert torch.equal(e2._lest[0, :N].cpu(), kw["rank_weights"][0])
    for eng in (e, e2):                       # the same next step on both
        inst = torch.arange(lc.B)
        eng.step(inst, torch.full((lc.B,), 11), x[:, 12, :D].clone())
    for k in ("values", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status"):
        assert torch.equal(getattr(e, k).cpu(), getattr(e2, k).cpu()), k
    assert int(e2.status[0]) == 0


@pytest.mark.parametrize("explicit", [False, True], ids=["bell", "explicit"])
def test_checkpoint_round_trip(tmp_path, explicit):
    checkpoint_round_trip(DEV, tmp_path, explicit)


def test_old_checkpoint_loads_as_smooth_median(tmp_path, monkeypatch):
    """A checkpoint whose config has no essence / rank_sigma keys (written before they existed)."""
    import json
    N, D, f = 7, 6, 2
    x = lc.case((N, D, f), "cons", ("median",))["x"]
    svc = _service(_cfg(N, D, f), x, D, DEV)
    path = str(tmp_path / "old.svoc")
    full = ConsensusConfig.to_dict
    monkeypatch.setattr(ConsensusConfig, "to_dict",
                        lambda self: {k: v for k, v in full(self).items() if k not in ("essence", "rank_sigma")})
    svstate.save(svc, path)
    monkeypatch.undo()
    meta_s, names, _ = svops.ops().load_state(path)
    assert "essence" not in json.loads(meta_s)["config"] and "rank_weights" not in names
    back = svstate.load(path, device=DEV)
    assert back.cfg.essence == "smooth_median" and back.engine._lest is None
    assert torch.equal(back.engine.consensus, svc.engine.consensus)
