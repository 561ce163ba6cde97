"""Exact-mode transactional streaming (ConsensusEngine.step -> _exact_transactions) against the golden
contract replayed one instance at a time: every update is its own transaction (store + full round; a
failing round reverts the whole transaction, contract.cairo:588-603), with injected reverts --
zero-variance columns (DIV_BY_ZERO), out-of-range values (INTERVAL_INPUT), unknown oracles
(NOT_ORACLE).  Both wave groupings: the general device-side one (interleaved batches, uneven counts)
and the strided ``updates_per_instance`` layout.  _exact_transactions only builds the waves; one routine
(ConsensusEngine._waves: update op with saved rows, a round or a verdict, restore op) runs them for both
groupings, for steps and previews, on both devices -- so the two groupings are also compared with each
other on everything a step leaves behind, and the degenerate batches go through it too."""
import random

import pytest
import torch

from svoc import ops as svops
from svoc import reference as ref
from svoc.config import ConsensusConfig
from svoc.status import ConsensusRevert, Status

pytestmark = pytest.mark.skipif(not svops.available(), reason="svoc/_C.so not built")

N, D, F = 7, 3, 2
ADMINS = [1000, 1001, 1002]
ORACLES = [2000 + i for i in range(N)]


def _update(rng, flat):
    """A random constrained prediction: often with a pinned column 0 (zero-variance bait), sometimes out
    of range, otherwise uniform."""
    r = rng.random()
    if r < 0.08:
        return [1_000_001 if rng.random() < 0.5 else -3] + [rng.randint(0, 1_000_000) for _ in range(D - 1)]
    if r < 0.7:   # column 0 pinned to the instance's value: enough of them zero that column's variance
        return [flat[0]] + [rng.randint(0, 1_000_000) for _ in range(D - 1)]
    return [rng.randint(0, 1_000_000) for _ in range(D)]


def _stream(seed, B, per_inst):
    rng = random.Random(seed)
    flats = [[rng.randint(0, 1_000_000) for _ in range(D)] for _ in range(B)]
    ups = []
    for b in range(B):
        seq = [(o, _update(rng, flats[b])) for o in range(N)]       # bootstrap: every oracle once
        for _ in range(per_inst - N):
            o = rng.randrange(N + 1)                                 # N = an unknown oracle
            seq.append((o, _update(rng, flats[b])))
        ups.append(seq)
    return ups


def _replay_reference(ups):
    out = []
    contracts = []
    for seq in ups:
        c = ref.ReferenceContract(ADMINS, True, 2, F, True, 0, D, ORACLES)
        st = []
        for o, v in seq:
            try:
                st.append(c.update_prediction(ORACLES[o] if o < N else 99, v))
            except ConsensusRevert as e:
                st.append(e.status)
        out.append(st)
        contracts.append(c)
    return out, contracts


def _engine(B, device):
    from svoc.engine import ConsensusEngine
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=F, constrained=True)
    return ConsensusEngine(cfg, batch=B, device=device, mode="exact")


def _check(e, contracts, st_eng, st_ref):
    assert st_eng == st_ref
    for b, c in enumerate(contracts):
        assert e.values[b, :, :D].tolist() == c.values, b
        assert int(e.n_active[b]) == c.n_active_oracles, b
        assert bool(e.consensus_active[b]) == c.consensus_active(), b
        if c.consensus_active():
            assert e.consensus[b].tolist() == c.get_consensus_value(), b
            assert [int(x) for x in e.rel[b]] == [c.rel1, c.rel2], b
            assert e.skew[b].tolist() == c.skewness and e.kurt[b].tolist() == c.kurtosis, b


def _run_general(device, seed=3, B=5, per_inst=14, n_batches=3):
    ups = _stream(seed, B, per_inst)
    st_ref, contracts = _replay_reference(ups)
    # interleave the instances' updates at random (order kept per instance), cut into batches
    rng = random.Random(seed + 1)
    cursor = [0] * B
    order = []
    while len(order) < B * per_inst:
        b = rng.choice([i for i in range(B) if cursor[i] < per_inst])
        order.append((b, cursor[b]))
        cursor[b] += 1
    e = _engine(B, device)
    st_eng = [[None] * per_inst for _ in range(B)]
    cuts = sorted(rng.sample(range(1, len(order)), n_batches - 1))
    for lo, hi in zip([0] + cuts, cuts + [len(order)]):
        part = order[lo:hi]
        inst = torch.tensor([b for b, _ in part])
        orc = torch.tensor([ups[b][k][0] for b, k in part])
        vals = torch.tensor([ups[b][k][1] for b, k in part], dtype=torch.int64)
        st = e.step(inst, orc, vals).cpu().tolist()
        for (b, k), s in zip(part, st):
            st_eng[b][k] = Status(s)
    _check(e, contracts, st_eng, st_ref)
    return st_ref


def _run_strided(device, seed=12, B=6, per_inst=7 + 9):
    ups = _stream(seed, B, per_inst)
    st_ref, contracts = _replay_reference(ups)
    e = _engine(B, device)
    st_eng = [[] for _ in range(B)]
    # bootstrap batch (7 per instance), then K = 3 per instance per batch, laid out b * K + k
    for lo, hi in [(0, N)] + [(k, k + 3) for k in range(N, per_inst, 3)]:
        K = hi - lo
        inst = torch.tensor([b for b in range(B) for _ in range(K)])
        orc = torch.tensor([ups[b][k][0] for b in range(B) for k in range(lo, hi)])
        vals = torch.tensor([ups[b][k][1] for b in range(B) for k in range(lo, hi)], dtype=torch.int64)
        st = e.step(inst, orc, vals, updates_per_instance=K).cpu().tolist()
        for b in range(B):
            st_eng[b] += [Status(s) for s in st[b * K:(b + 1) * K]]
    _check(e, contracts, st_eng, st_ref)
    return st_ref


def _covers_reverts(*st_lists):
    seen = {s for st in st_lists for seq in st for s in seq}
    assert {Status.OK, Status.NOT_ACTIVE, Status.DIV_BY_ZERO, Status.INTERVAL_INPUT, Status.NOT_ORACLE} <= seen, seen


def test_exact_stream_general_waves_cpu():
    _covers_reverts(_run_general("cpu"), _run_general("cpu", seed=8, B=4, per_inst=20, n_batches=2))


def test_exact_stream_strided_waves_cpu():
    _covers_reverts(_run_strided("cpu"))


def test_strided_layout_must_divide():
    e = _engine(2, "cpu")
    with pytest.raises(ValueError):
        e.step(torch.tensor([0, 1, 1]), torch.tensor([0, 0, 1]), torch.zeros(3, D, dtype=torch.int64),
               updates_per_instance=2)


@pytest.mark.gpu
def test_exact_stream_gpu():
    _covers_reverts(_run_general("cuda"), _run_strided("cuda"))


DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
# everything a step leaves behind (the golden-contract checks above do not look at metrics_fx, rounds or qr)
STATE = ("values", "enabled", "n_active", "consensus_active", "c1", "consensus", "skew", "kurt", "rel", "qr",
         "reliable", "status", "metrics_fx")


def _snapshot(e):
    return {k: getattr(e, k).clone() for k in STATE + ("touched",)}


def _assert_same(a, b, tag, keys=STATE):
    for k in keys:
        assert torch.equal(a[k], b[k]), (tag, k)


def _batch_of(ups, part):
    """The (instance b, its k-th update) pairs ``part`` as a batch, in that order."""
    return (torch.tensor([b for b, _ in part], dtype=torch.int64),
            torch.tensor([ups[b][k][0] for b, k in part], dtype=torch.int64),
            torch.tensor([ups[b][k][1] for b, k in part], dtype=torch.int64).reshape(-1, D))


@pytest.mark.parametrize("device", DEVICES)
def test_groupings_are_one_computation(device):
    """The same stream through the strided layout and, permuted wave-major, through the general grouping:
    the same waves, so the same statuses and the same state, counters included, after every step; and
    preview_updates, in both forms on both engines, says what the step then returns and changes nothing."""
    B, per_inst = 5, 14
    ups = _stream(21, B, per_inst)
    strided, general = _engine(B, device), _engine(B, device)
    for lo, hi in [(0, N), (N, N + 3), (N + 3, per_inst)]:
        K = hi - lo
        # (rounds counts waves: the general grouping drops unknown ids before it counts an instance's
        # updates, so it issues K waves only if some instance has none in this step)
        assert any(all(ups[b][k][0] < N for k in range(lo, hi)) for b in range(B))
        by_inst = [(b, k) for b in range(B) for k in range(lo, hi)]       # b * K + k
        by_wave = [(b, k) for k in range(lo, hi) for b in range(B)]
        unpermute = torch.tensor([(k - lo) * B + b for b, k in by_inst], device=device)
        forms = [(_batch_of(ups, by_inst), K, None), (_batch_of(ups, by_wave), None, unpermute)]
        previews = []
        for e in (strided, general):
            before = _snapshot(e)
            for batch, k_arg, perm in forms:
                st = e.preview_updates(*batch, updates_per_instance=k_arg)
                previews.append(st if perm is None else st[perm])
                _assert_same(_snapshot(e), before, ("preview", lo, k_arg), STATE + ("touched",))
                assert e.rounds == lo
        st_s = strided.step(*forms[0][0], updates_per_instance=K)
        st_g = general.step(*forms[1][0])[unpermute]
        assert torch.equal(st_s, st_g), lo
        for p in previews:
            assert torch.equal(p, st_s), lo
        _assert_same(_snapshot(strided), _snapshot(general), ("step", lo))
        assert strided.rounds == general.rounds == hi
    seen = {Status(s) for s in st_s.tolist()}
    assert {Status.OK, Status.DIV_BY_ZERO} <= seen, seen      # (the last step both accepts and reverts)


@pytest.mark.parametrize("device", DEVICES)
def test_empty_and_single_update_batches(device):
    """No update at all, and one update per step (a wave of one entry), in both layouts, against the golden
    replay."""
    B, per_inst = 2, N + 4
    ups = _stream(39, B, per_inst)
    st_ref, contracts = _replay_reference(ups)
    _covers_reverts(st_ref)
    e = _engine(B, device)
    none = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, D, dtype=torch.int64))
    for k_arg in (None, 1):
        assert e.step(*none, updates_per_instance=k_arg).numel() == 0
        assert e.preview_updates(*none, updates_per_instance=k_arg).numel() == 0
    assert e.rounds == 0 and int(e.n_active.sum()) == 0
    st_eng = [[] for _ in range(B)]
    for k in range(per_inst):
        for b in range(B):
            # (updates_per_instance=1 with instance 0 is the strided layout; with instance 1 it is not a
            # b * K + k batch and takes the general grouping, as does None)
            st = e.step(*_batch_of(ups, [(b, k)]), updates_per_instance=(1 if k % 2 else None))
            st_eng[b].append(Status(int(st[0])))
    _check(e, contracts, st_eng, st_ref)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("k_arg", [None, 2])
def test_batch_of_unknown_ids_changes_nothing(device, k_arg):
    """Every id of the batch out of range (instance -1 and B, oracle -1 and N): each update gets its status --
    the interval check before the oracle lookup, as in the contract -- and no row, flag or counter moves."""
    B = 3
    ups = _stream(9, B, N)
    e = _engine(B, device)
    e.step(*_batch_of(ups, [(b, k) for b in range(B) for k in range(N)]), updates_per_instance=N)   # bootstrap
    before = _snapshot(e)
    inst = torch.tensor([-1, B, 0, 1])
    orc = torch.tensor([0, 1, -1, N])
    vals = torch.tensor([[5, 6, 7], [1, 2, 3], [1_000_001, 2, 3], [4, 5, 6]], dtype=torch.int64)
    want = [Status.NOT_ORACLE, Status.NOT_ORACLE, Status.INTERVAL_INPUT, Status.NOT_ORACLE]
    assert e.preview_updates(inst, orc, vals, updates_per_instance=k_arg).tolist() == [int(s) for s in want]
    _assert_same(_snapshot(e), before, "preview", STATE + ("touched",))
    assert e.step(inst, orc, vals, updates_per_instance=k_arg).tolist() == [int(s) for s in want]
    _assert_same(_snapshot(e), before, "step")


@pytest.mark.parametrize("device", DEVICES)
def test_one_long_instance_general_waves(device):
    """One instance with more updates than all others: the last waves of the general grouping hold a single
    update.  Against the golden replay."""
    B = 3
    ups = _stream(14, B, N + 6)
    ups = [ups[0]] + [seq[:N + 1] for seq in ups[1:]]
    assert sum(o < N for o, _ in ups[0][N:]) >= 4           # (waves of one update: instance 0's known oracles)
    st_ref, contracts = _replay_reference(ups)
    e = _engine(B, device)
    st_eng = [[None] * len(seq) for seq in ups]
    for lo, hi in [(0, N), (N, N + 6)]:
        part = [(b, k) for k in range(lo, hi) for b in range(B) if k < len(ups[b])]
        st = e.step(*_batch_of(ups, part)).cpu().tolist()
        for (b, k), s in zip(part, st):
            st_eng[b][k] = Status(s)
    _check(e, contracts, st_eng, st_ref)


class _RecordingOps:
    """The engine's op namespace, with every call noted."""

    def __init__(self, ops):
        self.ops, self.calls = ops, []

    def __getattr__(self, name):
        fn = getattr(self.ops, name)

        def call(*args, **kwargs):
            self.calls.append((name, args))
            return fn(*args, **kwargs)
        return call


def test_cpu_strided_steps_take_the_shared_wave_routine():
    """A CPU strided step rolls back through the restore op with inactive_status = NOT_ACTIVE, once per wave,
    as the GPU does: no second implementation of a wave is left in the engine."""
    from svoc.engine import ConsensusEngine
    assert not hasattr(ConsensusEngine, "_exact_transactions_k") and not hasattr(ConsensusEngine, "_preview_k")
    B, K = 4, 3
    ups = _stream(2, B, N + K)
    e = _engine(B, "cpu")
    e.step(*_batch_of(ups, [(b, k) for b in range(B) for k in range(N)]), updates_per_instance=N)
    batch = _batch_of(ups, [(b, k) for b in range(B) for k in range(N, N + K)])
    for run, undo in ((e.preview_updates, K), (e.step, 0)):
        e._ops = rec = _RecordingOps(e._ops)
        run(*batch, updates_per_instance=K)
        e._ops = rec.ops
        restores = [args for name, args in rec.calls if name == "restore_updates"]
        rollbacks = [args for args in restores if len(args) == 11 and args[10] == int(Status.NOT_ACTIVE)]
        assert len(rollbacks) == K and len(restores) == K + undo
        saves = [args for name, args in rec.calls if name == "apply_updates"]
        assert len(saves) == K and all(args[-1] is not None for args in saves)   # (saved_en: the rows are saved)


def test_synthetic_stream_keeps_engine_failing_set():
    """bench.py's update stream draws its U(0,1) rows for the engine's own failing oracles
    (ConsensusEngine.failing_mask): an honest oracle never receives a uniform row, so no instance ends
    up with more than f noisy oracles (which the exact column kernel hands to the i128 kernel)."""
    from svoc.engine import ConsensusEngine
    from svoc.stream import SyntheticUpdateStream
    B, n, d, f, U = 3, 16, 40, 3, 8
    cfg = ConsensusConfig(n_oracles=n, dimension=d, n_failing_oracles=f, constrained=True)
    eng = ConsensusEngine(cfg, batch=B, device="cpu", mode="exact")
    eng.randomize(seed=4)
    m = eng.failing_mask
    assert m.shape == (B, n) and (m.sum(1) == f).all()
    s = SyntheticUpdateStream(B, n, d, U, f, pool=2, device="cpu", seed=1, dtype=torch.int64, failing=m)
    assert torch.equal(s.failing, m)
    for k in range(2):
        inst, orc, vals = s.batch(k)
        # honest rows are Beta(20, 20): none is near 0 or 1 in every column, uniform rows spread out
        spread = (vals.double() / 1e6).std(dim=1)
        fail = m[inst, orc]
        assert (spread[~fail] < 0.15).all() and (spread[fail] > 0.15).all()
    eng.step(*s.batch(0), updates_per_instance=U)
    assert (eng.status == int(Status.OK)).all()
