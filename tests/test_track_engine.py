"""The per-oracle track record and the failing-only replacement rule through the engine, the service, governance,
checkpoints, D-sharding and the CLI -- on the CPU and (marked gpu) on the device, the same cases.

Exact mode is compared with the golden model (svoc.reference.ReferenceContract(track_oracles=True)) after every
step; fast mode with the sequential model of tests/track_cases.py fed with the engine's own active / status /
reliable / qr.  Every comparison is torch.equal on whole tensors.
"""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import track_cases as tc
from svoc import ops as svops
from svoc import state
from svoc.api import ConsensusService, OracleConsensus
from svoc.codec import address_to_limbs, addresses_to_limbs
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine
from svoc.governance import Governance
from svoc.reference import ReferenceContract
from svoc.status import ConsensusRevert, Status

pytestmark = pytest.mark.skipif(not svops.available(), reason="svoc/_C.so not built")

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
N, D, B = 7, 6, 3
ADMINS = [11, 12, 13]
ORACLES = [100 + i for i in range(N)]
TRACK = ("rounds", "flagged", "streak", "score", "since")


# ------------------------------------------------------------------------------------------ the scripted stream

@functools.lru_cache(maxsize=None)
def stream(b):
    """Instance b's ~45 update_prediction transactions (oracle, row): activation, two oracles that drift out and
    come back (streaks rise and reset), a second all-zero row (rel < 0: RELIABILITY_INTERVAL) and a column that
    becomes constant (zero variance: DIV_BY_ZERO in exact arithmetic), then a last drift."""
    rng = np.random.default_rng(77 + b)
    base = [[int(x) for x in rng.integers(930_000, 970_000, D)] for _ in range(N)]
    jit = lambda o: [int(min(1_000_000, max(0, v + int(rng.integers(-8000, 8000))))) for v in base[o]]  # noqa: E731
    drift = lambda o, far: [int(v - far + int(rng.integers(-3000, 3000))) for v in base[o]]             # noqa: E731
    d1, d2 = (2 + b) % N, (5 + b) % N
    tx = [(o, jit(o)) for o in range(N)]
    tx += [(d1, drift(d1, 300_000 + 20_000 * r)) for r in range(4)]
    tx += [(d2, drift(d2, 250_000)) for r in range(3)]
    tx += [(o, jit(o)) for o in range(N) if o not in (d1, d2)]
    tx.append((d1, jit(d1)))
    honest = [o for o in range(N) if o not in (d1, d2)]
    tx += [(honest[(r + b) % len(honest)], jit(honest[(r + b) % len(honest)])) for r in range(3)]
    tx.append((d2, jit(d2)))
    tx += [(honest[0], [0] * D), (honest[1], [0] * D), (honest[0], jit(honest[0]))]
    for o in range(N):
        row = jit(o)
        row[0] = 500_000
        tx.append((o, row))
    tx += [(o, jit(o)) for o in range(N)]
    tx += [(d1, drift(d1, 200_000)) for r in range(4)]
    return tuple((o, tuple(r)) for o, r in tx)


STEPS = len(stream(0))


def golden_contract(**kw):
    return ReferenceContract(ADMINS, True, 2, 2, True, 0, D, ORACLES, **kw)


def golden_update(c, caller, row):
    try:
        return int(c.update_prediction(caller, list(row)))
    except ConsensusRevert as e:
        return int(e.status)


@functools.lru_cache(maxsize=None)
def golden_run():
    """The golden model over the whole stream: per step and instance the status, and snapshots of the contracts."""
    import copy
    cs = [golden_contract(track_oracles=True) for _ in range(B)]
    statuses, snaps = [], []
    for t in range(STEPS):
        statuses.append([golden_update(cs[b], ORACLES[stream(b)[t][0]], stream(b)[t][1]) for b in range(B)])
        snaps.append(copy.deepcopy(cs))
    return statuses, snaps


def make_service(device, batch=B, **kw):
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=2, n_admins=3, required_majority=2, **kw)
    return ConsensusService(cfg, batch, ADMINS, ORACLES, device=device, mode="exact")


def assert_same(svc, contracts, where=""):
    """The service's track record, outputs and oracle table against the golden contracts, whole tensors."""
    e = svc.engine
    rec = {k: v.cpu() for k, v in svc.track_record().items()}
    t32 = lambda x: torch.tensor(x, dtype=torch.int32)   # noqa: E731
    assert torch.equal(rec["rounds"], t32([c.track_rounds for c in contracts])), (where, "rounds")
    assert torch.equal(rec["flagged"], t32([c.track_flagged for c in contracts])), (where, "flagged")
    assert torch.equal(rec["streak"], t32([c.track_streak for c in contracts])), (where, "streak")
    assert torch.equal(rec["since"], t32([c.track_since for c in contracts])), (where, "since")
    assert torch.equal(rec["score"], torch.tensor([c.track_score for c in contracts], dtype=torch.int64)), (where, "score")
    t64 = lambda x: torch.tensor(x, dtype=torch.int64)   # noqa: E731
    assert torch.equal(e.consensus.cpu(), t64([c.consensus_value for c in contracts])), (where, "consensus")
    assert torch.equal(e.rel.cpu(), t64([[c.rel1, c.rel2] for c in contracts])), (where, "rel")
    assert torch.equal(e.skew.cpu(), t64([c.skewness for c in contracts])), (where, "skew")
    assert torch.equal(e.kurt.cpu(), t64([c.kurtosis for c in contracts])), (where, "kurt")
    assert e.reliable.cpu().tolist() == [[int(o.reliable) for o in c.oracles] for c in contracts], (where, "reliable")
    assert e.consensus_active.cpu().tolist() == [c.consensus_active() for c in contracts], (where, "active")
    assert [svc.gov.oracle_list(b) for b in range(len(contracts))] == [c.get_oracle_list() for c in contracts], where
    # streak >= 1 exactly where the seat is not reliable, once a round has committed
    for b, c in enumerate(contracts):
        if c.track_rounds and all(s == 0 for s in c.track_since):
            assert (rec["streak"][b] >= 1).tolist() == [not o.reliable for o in c.oracles], (where, b)


def step_batch(t, device, callers=None):
    """Step t of every instance as update_batch arguments."""
    inst = torch.arange(B, dtype=torch.int64, device=device)
    caller = addresses_to_limbs([(callers or {}).get((b, stream(b)[t][0]), ORACLES[stream(b)[t][0]]) for b in range(B)],
                                device=device)
    vals = torch.tensor([stream(b)[t][1] for b in range(B)], dtype=torch.int64, device=device)
    return inst, caller, vals


# ------------------------------------------------------------------------------------------ exact mode, golden model

def test_golden_stream_is_not_idle():
    statuses, snaps = golden_run()
    for b in range(B):
        col = [s[b] for s in statuses]
        assert col.count(int(Status.OK)) >= 30
        assert int(Status.RELIABILITY_INTERVAL) in col and int(Status.DIV_BY_ZERO) in col
        assert snaps[-1][b].track_rounds == col.count(int(Status.OK))
        streaks = [s[b].track_streak for s in snaps]
        d1 = (2 + b) % N
        assert max(s[d1] for s in streaks) >= 4 and any(s[d1] == 0 for s in streaks[12:])   # rose and reset


@pytest.mark.parametrize("device", DEVICES)
def test_exact_stream_matches_golden_after_every_step(device):
    statuses, snaps = golden_run()
    svc = make_service(device, track_oracles=True)
    for t in range(STEPS):
        st = svc.update_batch(*step_batch(t, device))
        assert st.cpu().tolist() == statuses[t], t
        assert_same(svc, snaps[t], where=t)
    if device == "cuda":
        assert svc.engine.verdict_routing()["verdict"] == 0
    assert svc.engine.state_bytes_per_instance() == (ConsensusEngine.bytes_per_instance(N, D, "exact", "int32")
                                                     + 4 + N * 20)


@pytest.mark.parametrize("device", DEVICES)
def test_exact_stream_strided_layout_matches_golden(device):
    """The same stream as ``updates_per_instance=K`` batches (three calls of K = STEPS / 3 waves each)."""
    statuses, snaps = golden_run()
    svc = make_service(device, track_oracles=True)
    K = STEPS // 3
    assert K * 3 == STEPS
    for c in range(3):
        ts = range(c * K, (c + 1) * K)
        inst = torch.arange(B, dtype=torch.int64, device=device).repeat_interleave(K)
        caller = addresses_to_limbs([ORACLES[stream(b)[t][0]] for b in range(B) for t in ts], device=device)
        vals = torch.tensor([stream(b)[t][1] for b in range(B) for t in ts], dtype=torch.int64, device=device)
        st = svc.update_batch(inst, caller, vals, updates_per_instance=K)
        assert st.cpu().view(B, K).tolist() == [[statuses[t][b] for t in ts] for b in range(B)], c
        assert_same(svc, snaps[(c + 1) * K - 1], where=c)
    assert svc.engine.verdict_routing()["verdict"] == 0


@pytest.mark.gpu
def test_tracking_engine_runs_no_verdict_waves():
    """8 x 64 is a shape the verdict waves take: a tracking engine must not (it needs every wave's mask), and its
    strided stream gives the record of the CPU engine."""
    n, d, K = 8, 64, 3
    cfg = ConsensusConfig(n_oracles=n, dimension=d, n_failing_oracles=2, track_oracles=True)
    plain = ConsensusEngine(ConsensusConfig(n_oracles=n, dimension=d, n_failing_oracles=2), 2, device="cuda", mode="exact")
    assert plain._verdict_ok()
    g = torch.Generator().manual_seed(5)
    recs = {}
    for device in ("cpu", "cuda"):
        e = ConsensusEngine(cfg, 2, device=device, mode="exact")
        assert not e._verdict_ok()
        g.manual_seed(5)
        for s in range(3):
            oracle = torch.stack([torch.randperm(n, generator=g)[:K] for _ in range(2)]).reshape(-1)
            if s == 0:   # activation: every oracle once, then the strided steps
                e.step(torch.arange(2).repeat_interleave(n), torch.arange(n).repeat(2),
                       torch.randint(400_000, 600_000, (2 * n, d), generator=g))
            vals = torch.randint(400_000, 600_000, (2 * K, d), generator=g)
            e.step(torch.arange(2).repeat_interleave(K), oracle, vals, updates_per_instance=K)
        assert e.verdict_routing()["verdict"] == 0
        recs[device] = {k: v.cpu() for k, v in e.track_record().items()}
    assert recs["cpu"]["rounds"].tolist() == [10, 10]
    for k in TRACK:
        assert torch.equal(recs["cpu"][k], recs["cuda"][k]), k


@pytest.mark.parametrize("device", DEVICES)
def test_preview_leaves_the_record_untouched(device):
    _, snaps = golden_run()
    svc = make_service(device, track_oracles=True)
    for t in range(20):
        svc.update_batch(*step_batch(t, device))
    before = {k: v.clone() for k, v in svc.track_record().items()}
    for t in (20, 21, 30):   # an accepted update, and the reverting kinds
        svc.preview_batch(*step_batch(t, device))
    K = 5
    inst = torch.arange(B, dtype=torch.int64, device=device).repeat_interleave(K)
    caller = addresses_to_limbs([ORACLES[stream(b)[t][0]] for b in range(B) for t in range(20, 20 + K)], device=device)
    vals = torch.tensor([stream(b)[t][1] for b in range(B) for t in range(20, 20 + K)], dtype=torch.int64, device=device)
    svc.preview_batch(inst, caller, vals, updates_per_instance=K)
    for k, v in svc.track_record().items():
        assert torch.equal(v, before[k]), k
    assert_same(svc, snaps[19])


# ------------------------------------------------------------------------------------------ fast mode, sequential model

FAST_SHAPES = [(7, 6, 2), (64, 128, 8), (256, 64, 32)]     # the small kernel, the window kernels


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("storage", ["bf16", "fp32"])
@pytest.mark.parametrize("n,d,f", FAST_SHAPES)
def test_fast_record_matches_model_on_engine_outputs(device, storage, n, d, f):
    """step_pipelined (chunks = 2; fp32 storage: the fused transactional path once every instance is active), 8
    instances, 6 steps, instance 3 reverting in step 3: after every step the record equals the sequential model
    fed with the engine's own active / status / reliable / qr."""
    Bf = 8
    cfg = ConsensusConfig(n_oracles=n, dimension=d, n_failing_oracles=f, track_oracles=True)
    e = ConsensusEngine(cfg, Bf, device=device, mode="fast", storage=storage)
    g = torch.Generator().manual_seed(n * 1000 + d)
    inst = torch.arange(Bf).repeat_interleave(n)
    oracle = torch.arange(n).repeat(Bf)
    model = dict(rounds=[0] * Bf, flagged=[[0] * n for _ in range(Bf)], streak=[[0] * n for _ in range(Bf)],
                 score=[[0] * n for _ in range(Bf)])
    for s in range(6):
        vals = 0.5 + 0.1 * torch.randn(Bf, n, d, generator=g).clamp(-3, 3)
        vals[:, :f] = torch.rand(Bf, f, d, generator=g)         # the failing oracles
        if s == 2:
            vals[3, :, 0] = 0.5                                  # a constant column: the round reverts
        vals = vals.to(e.vdtype).reshape(Bf * n, d)
        e.step_pipelined(inst, oracle, vals, updates_per_instance=n, chunks=2)
        e.pipeline_join()
        act, st = e._active.cpu().tolist(), e.status.cpu().tolist()
        assert all(act), s
        assert [x != int(Status.OK) for x in st] == [s == 2 and b == 3 for b in range(Bf)], (s, st)
        qr = [[np.float32(x) for x in row] for row in e.qr.cpu().tolist()]
        model = tc.model_update(model, act, st, e.reliable.cpu().tolist(), qr, exact=False)
        rec = e.track_record()
        for k, w in tc.record_tensors(model).items():
            assert torch.equal(rec[k].cpu(), w), (s, k)
        assert int(rec["since"].abs().sum()) == 0
    assert model["rounds"] == [6, 6, 6, 5, 6, 6, 6, 6]
    assert max(max(r) for r in model["streak"]) >= 2 and any(0 in r for r in model["streak"])
    if device == "cuda" and storage == "fp32":
        assert e._fused_ok(inst.to(device), oracle.to(device), vals.to(device), n)   # the later steps ran fused


# ------------------------------------------------------------------------------------------ governance

NEW1, NEW2 = 7001, 7002


def pack_actions(actions, device):
    """Action tuples -> the tensors of Governance.submit_batch (the tensor API)."""
    K = len(actions)
    inst, kind, a0, a1 = [0] * K, [0] * K, [0] * K, [0] * K
    caller, addr = [[0] * 4 for _ in range(K)], [[0] * 4 for _ in range(K)]
    for k, act in enumerate(actions):
        inst[k], caller[k] = act[1], address_to_limbs(act[2])
        if act[0] == "propose":
            if act[3] is not None:
                a0[k], a1[k], addr[k] = 1, act[3][0], address_to_limbs(act[3][1])
        else:
            kind[k], a0[k], a1[k] = 1, act[3], int(act[4])
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=device)   # noqa: E731
    return dict(inst=t(inst, torch.int64), caller=t(caller, torch.int64), kind=t(kind, torch.int32),
                arg0=t(a0, torch.int32), arg1=t(a1, torch.int64), addr=t(addr, torch.int64))


class GovRun:
    """A service and its golden contracts driven in lockstep."""

    def __init__(self, device, k, api):
        self.device, self.api = device, api
        self.svc = make_service(device, batch=2, track_oracles=True, replace_only_failing=k)
        self.gold = [golden_contract(track_oracles=True, replace_only_failing=k) for _ in range(2)]
        self.rng = np.random.default_rng(k)

    def update(self, seat, far, caller=None):
        """One update_prediction of `seat` in both instances (instance 0's caller may be a replaced address)."""
        rows = [[int(940_000 - far + self.rng.integers(-40_000, 40_000)) for _ in range(D)] for _ in range(2)]
        callers = [caller if caller is not None else ORACLES[seat], ORACLES[seat]]
        st = self.svc.update_batch(torch.arange(2, device=self.device), addresses_to_limbs(callers, device=self.device),
                                   torch.tensor(rows, dtype=torch.int64, device=self.device)).cpu().tolist()
        want = [golden_update(self.gold[b], callers[b], rows[b]) for b in range(2)]
        assert st == want
        self.check("update")
        return st

    def act(self, actions):
        """Governance actions in one launch (list or tensor API) and one by one on the golden contracts."""
        if self.api == "list":
            st, ap = self.svc.governance(actions)
            st, ap = [int(s) for s in st], [bool(a) for a in ap]
        else:
            st, ap = self.svc.governance(pack_actions(actions, self.device))
            st, ap = st.cpu().tolist(), [bool(a) for a in ap.cpu().tolist()]
        want_st, want_ap = [], []
        for a in actions:
            c = self.gold[a[1]]
            try:
                if a[0] == "propose":
                    c.update_proposition(a[2], a[3])
                    want_ap.append(False)
                else:
                    want_ap.append(bool(c.vote_for_a_proposition(a[2], a[3], a[4])))
                want_st.append(int(Status.OK))
            except ConsensusRevert as e:
                want_st.append(int(e.status))
                want_ap.append(False)
        assert (st, ap) == (want_st, want_ap), actions
        self.check(actions)
        return st, ap

    def check(self, where):
        assert_same(self.svc, self.gold, where)
        for b, c in enumerate(self.gold):
            assert self.svc.gov.propositions(b) == c.propositions, where
            assert self.svc.gov.vote_matrix(b) == c.vote_matrix, where


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("api", ["list", "tensor"])
def test_failing_only_replacement_against_golden(device, k, api):
    r = GovRun(device, k, api)
    for o in range(N):
        r.update(o, 0)
    t = r.gold[0].track_streak.index(0)             # a seat that is reliable now: streak 0
    for _ in range(k - 1):
        r.update(t, 300_000)                        # ... driven out k - 1 rounds: still below k
    assert r.gold[0].track_streak[t] == k - 1
    # a majority on a seat below k: one ordered launch holds the proposal and two votes of instance 0
    st, ap = r.act([("propose", 0, ADMINS[0], (t, NEW1)), ("vote", 0, ADMINS[1], 0, True),
                    ("vote", 0, ADMINS[2], 0, True)])
    assert st == [0, 0, 0] and ap == [False, False, False]
    assert [row[0] for row in r.svc.gov.vote_matrix(0)] == [True, True, True]      # the vote bits are stored
    assert r.svc.gov.oracle_list(0)[t] == ORACLES[t] and r.svc.gov.propositions(0)[0] == (t, NEW1)
    # a None proposition at majority still reverts
    st, _ = r.act([("vote", 0, ADMINS[0], 2, True)])
    assert st == [0]
    st, _ = r.act([("vote", 0, ADMINS[1], 2, True)])
    assert st == [int(Status.UNWRAP_NONE)]
    # the seat fails its k-th round in a row: the identical vote now applies
    r.update(t, 300_000)
    assert r.gold[0].track_streak[t] == k
    reliable_before = r.svc.engine.reliable.clone()
    st, ap = r.act([("vote", 0, ADMINS[1], 0, True)])
    assert st == [0] and ap == [True]
    rec = {key: v.cpu() for key, v in r.svc.track_record().items()}
    assert [int(rec[key][0, t]) for key in ("flagged", "streak", "score")] == [0, 0, 0]
    assert int(rec["since"][0, t]) == int(rec["rounds"][0]) > 0
    assert torch.equal(r.svc.engine.reliable, reliable_before) and int(reliable_before[0, t]) == 0
    assert r.svc.gov.oracle_list(0)[t] == NEW1 and r.svc.gov.oracle_list(1)[t] == ORACLES[t]
    assert int(rec["since"][1].abs().sum()) == 0 and int(rec["streak"][1, t]) == k   # instance 1: no governance
    # the fresh seat is refused until it fails k rounds itself
    st, ap = r.act([("propose", 0, ADMINS[0], (t, NEW2)), ("vote", 0, ADMINS[1], 0, True)])
    assert st == [0, 0] and ap == [False, False]
    for i in range(k):
        assert r.update(t, 300_000, caller=NEW1)[0] == int(Status.OK)
        if i < k - 1:
            st, ap = r.act([("vote", 0, ADMINS[2], 0, True)])
            assert st == [0] and ap == [False]
    st, ap = r.act([("vote", 0, ADMINS[1], 0, True)])
    assert st == [0] and ap == [True]
    assert r.svc.gov.oracle_list(0)[t] == NEW2
    h = r.svc.handle(0)
    seated, flagged, streak, mean = h.get_oracle_track_record()[t]
    assert (seated, flagged, streak, mean) == (0, 0, 0, 0)
    assert t not in h.get_failing_oracles(1)
    assert torch.equal(r.svc.failing_oracles(1).cpu(), r.svc.track_record()["streak"].cpu() >= 1)


def test_replace_only_failing_needs_tracking():
    with pytest.raises(ValueError):
        ConsensusConfig(replace_only_failing=2).validate()
    with pytest.raises(ValueError):
        make_service("cpu", replace_only_failing=1)
    with pytest.raises(ValueError):
        golden_contract(replace_only_failing=1)
    with pytest.raises(ValueError):
        Governance(1, 3, N, "cpu", min_streak=1)
    with pytest.raises(ValueError):
        OracleConsensus(ADMINS, True, 2, 2, True, 0, D, ORACLES, replace_only_failing=1)
    ConsensusConfig(track_oracles=True, replace_only_failing=2).validate()
    with pytest.raises(RuntimeError):
        make_service("cpu").track_record()
    old = ConsensusConfig().to_dict()
    del old["track_oracles"], old["replace_only_failing"]       # a checkpoint from before the fields existed
    assert ConsensusConfig.from_dict(old) == ConsensusConfig()


def test_facade_record_and_failing_list():
    c = OracleConsensus(ADMINS, True, 2, 2, True, 0, D, ORACLES, track_oracles=True)
    gold = golden_contract(track_oracles=True)
    for o, row in stream(0)[:11]:
        c.update_prediction(ORACLES[o], list(row))
        golden_update(gold, ORACLES[o], row)
    rec = c.get_oracle_track_record()
    assert rec == [(gold.track_rounds, gold.track_flagged[i], gold.track_streak[i],
                    gold.track_score[i] // gold.track_rounds) for i in range(N)]
    assert c.get_failing_oracles(1) == [i for i in range(N) if gold.track_streak[i] >= 1]
    assert 2 in c.get_failing_oracles(4) == [i for i in range(N) if gold.track_streak[i] >= 4]
    c.engine.reset_track([0])
    assert c.get_oracle_track_record() == [(0, 0, 0, 0)] * N


# ------------------------------------------------------------------------------------------ checkpoints

@pytest.mark.parametrize("device", DEVICES)
def test_checkpoint_resume_is_identical(device, tmp_path):
    statuses, snaps = golden_run()
    a = make_service(device, track_oracles=True)
    half = 24
    for t in range(half):
        a.update_batch(*step_batch(t, device))
    # a replacement before the checkpoint, so `since` is not all zero in it
    seat = int(a.track_record()["streak"][0].argmax())
    st, ap = a.governance([("propose", 0, ADMINS[0], (seat, NEW1)), ("vote", 0, ADMINS[1], 0, True)])
    assert ap == [False, True]
    path = str(tmp_path / "track.svoc")
    state.save(a, path)
    b = state.load(path, device=device)
    assert b.cfg.track_oracles and int(b.track_record()["since"][0, seat]) == int(a.track_record()["rounds"][0]) > 0
    callers = {(0, seat): NEW1}
    for t in range(half, STEPS):
        sa = a.update_batch(*step_batch(t, device, callers))
        sb = b.update_batch(*step_batch(t, device, callers))
        assert torch.equal(sa, sb) and sa.cpu().tolist() == statuses[t], t
        for k in TRACK:
            assert torch.equal(a.track_record()[k], b.track_record()[k]), (t, k)
        for k in ("consensus", "rel", "skew", "kurt", "qr", "reliable", "values", "status"):
            assert torch.equal(getattr(a.engine, k), getattr(b.engine, k)), (t, k)
    assert int(a.track_record()["rounds"][0]) == snaps[-1][0].track_rounds
    # a checkpoint written without tracking carries no track sections and loads as before
    plain = make_service(device)
    plain.update_batch(*step_batch(0, device))
    state.save(plain, path)
    assert not state.load(path, device=device).engine.tracking


# ------------------------------------------------------------------------------------------ D-sharding

def _shard_rounds(mode):
    n, d, f, Bs = 16, 11, 3, 4
    g = torch.Generator().manual_seed(41)
    xs = []
    for s in range(4):
        x = 0.5 + 0.08 * torch.randn(Bs, n, d, generator=g).clamp(-3, 3)
        x[:, (s % 2):f + (s % 2)] = torch.rand(Bs, f, d, generator=g)
        if s == 2:
            x[1, :, 1] = 0.5                       # instance 1 reverts in round 3
        xs.append((x * 1e6).to(torch.int64) if mode == "exact" else x.float())
    cfgd = dict(n_oracles=n, dimension=d, n_failing_oracles=f, track_oracles=True)
    return xs, cfgd


def _run_rounds(e, xs, lo, hi, run):
    for x in xs:
        e.values[:, :, : hi - lo] = x[:, :, lo:hi].to(e.values.device, e.values.dtype)
        e.enabled.fill_(1); e.n_active.fill_(e.N); e.touched.fill_(1)
        run(e)
    return {k: v.cpu() for k, v in e.track_record().items()}


def _unsharded_record(mode, device="cpu"):
    xs, cfgd = _shard_rounds(mode)
    e = ConsensusEngine(ConsensusConfig(**cfgd), xs[0].shape[0], device=device, mode=mode,
                        storage=None if mode == "exact" else "fp32")
    rec = _run_rounds(e, xs, 0, cfgd["dimension"], lambda eng: eng.run_round())
    assert rec["rounds"].tolist() == [4, 3, 4, 4] and int(rec["streak"].max()) >= 2
    return rec


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_dshard_world1_record_equals_unsharded(device, mode):
    from svoc.parallel.dshard import run_round_sharded
    xs, cfgd = _shard_rounds(mode)
    e = ConsensusEngine(ConsensusConfig(**cfgd), xs[0].shape[0], device=device, mode=mode,
                        storage=None if mode == "exact" else "fp32")
    rec = _run_rounds(e, xs, 0, cfgd["dimension"], lambda eng: run_round_sharded(eng, cfgd["dimension"], world=1))
    want = _unsharded_record(mode, device)
    for k in TRACK:
        assert torch.equal(rec[k], want[k]), k


def _track_shard_worker(rank, world, port, outdir):
    from test_dist import _init
    import torch.distributed as dist
    from svoc.parallel.dshard import run_round_sharded, shard_bounds
    _init(rank, world, port)
    xs, cfgd = _shard_rounds("exact")
    lo, hi = shard_bounds(cfgd["dimension"], rank, world)
    e = ConsensusEngine(ConsensusConfig(**{**cfgd, "dimension": hi - lo}), xs[0].shape[0], device="cpu", mode="exact")
    rec = _run_rounds(e, xs, lo, hi, lambda eng: run_round_sharded(eng, cfgd["dimension"], world=world))
    torch.save(rec, os.path.join(outdir, f"track{rank}.pt"))
    dist.destroy_process_group()


def test_dshard_gloo_world2_record_equals_unsharded():
    import torch.multiprocessing as mp
    from test_dist import _free_port
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_track_shard_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        recs = [torch.load(os.path.join(d, f"track{i}.pt"), weights_only=True) for i in range(2)]
    want = _unsharded_record("exact")
    for rec in recs:
        for k in TRACK:
            assert torch.equal(rec[k], want[k]), k


# ------------------------------------------------------------------------------------------ CLI

def test_cli_failing_oracles_lists_the_drifted_oracle(tmp_path):
    from svoc.cli import HELP, Client
    assert "failing_oracles [k]" in HELP
    cl = Client(db_path=str(tmp_path / "db.sqlite"), track=True)
    try:
        g = torch.Generator().manual_seed(3)
        assert "no oracle" in cl.query("failing_oracles")
        for r in range(3):
            p = 0.6 + 0.02 * torch.rand(7, 6, generator=g)
            p[4] = 0.1 + 0.02 * r                   # oracle 4 far out in every round
            cl.predictions = p
            assert "REVERT" not in cl.query("commit")
        out = cl.query("failing_oracles 15")     # flagged in every committed round: oracle 4 alone
        assert out.startswith("oracle 4 (") and "for 15 round(s) in a row" in out and "\n" not in out
        assert "oracle 4 (" in cl.query("failing_oracles")
        menu = cl.query("replacement_menu")
        assert menu.count("\n") == 2 and "failing" not in menu      # unchanged
        assert "no oracle" in cl.query("failing_oracles 16")
    finally:
        cl.close()
    plain = Client(db_path=str(tmp_path / "db2.sqlite"))
    try:
        assert plain.query("failing_oracles").startswith("error: no track record")
    finally:
        plain.close()
