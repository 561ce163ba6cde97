"""The rank-weighted (L-estimator) round on the GPU: consensus_fast_lest.hip through the op and through
ConsensusEngine, on the cases, model and assertions that test_lest.py pins to the CPU twin (lest_cases).

The shapes reach every instantiation of the kernel (1, 2 and 4 lanes per column, constrained and unconstrained), a
partial slab, more than one slab, and no failing oracle; the route is asserted before the launches.  One-hot
weights pin the rank-to-register mapping of the full sorts (sortnet.hpp sort_oem / sort_group) across the lanes of
a column, and the sentinel handling: a wrong mapping or a multiplied sentinel changes bits."""
import pytest
import torch

import lest_cases as lc
import test_lest as cpu
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"
LANES = {7: 1, 2: 1, 64: 1, 65: 2, 128: 2, 129: 4, 256: 4}


def _assert_route(shape):
    N, D, f = shape
    r = svops.lest_route("fp32", N, D, (D + 7) // 8 * 8, f, True)
    assert (r.supported, r.lane_groups) == (1, LANES[N]), (shape, r)


def test_shapes_cover_every_lane_group():
    assert {LANES[s[0]] for s in lc.SHAPES} == {1, 2, 4}


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
@pytest.mark.parametrize("variant", [v[0] for v in lc.VARIANTS])
def test_kernel_vs_model(shape, variant):
    """Bell (three widths), median and mean weights against the fp64 model, each output within its bound."""
    _assert_route(shape)
    for family in lc.MODEL_FAMILIES:
        c = lc.case(shape, variant, family)
        lc.check_round(lc.run_case(svops.ops(), c, DEV), c)


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_one_hot(shape):
    _assert_route(shape)
    n = lc.check_one_hot(svops.ops(), shape, DEV)
    assert n > 0 or shape[0] - shape[2] < 4


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_median_weights_equal_fast_round(shape):
    n = lc.check_median_vs_fast(svops.ops(), shape, DEV)
    assert n > 0 or shape[0] - shape[2] < 4


def test_caller_workspace_and_none_agree():
    """The caller's workspace (the engine's) and the op's own temporary one give the same bits."""
    c = lc.case((129, 33, 32), "cons", ("bell", 0.125))
    x = c["x"].to(DEV)
    work = torch.empty(svops.fast_work_numel(lc.B, c["D"]), dtype=torch.int32, device=DEV)
    a = lc.run_lest(svops.ops(), x, c["active"], c["D"], c["f"], True, c["max_spread"], c["weights"], work)
    b = lc.run_case(svops.ops(), c, DEV)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_op_refuses_unsupported_shapes():
    ops = svops.ops()
    for N, f in ((300, 8), (8, 7)):
        x = torch.rand(2, N, 8, device=DEV)
        o = lc.poisoned(2, N, 8, DEV)
        w = torch.zeros(2, 256, device=DEV)
        with pytest.raises(RuntimeError):
            ops.lest_round(x, None, 8, f, True, 1.0, w, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"],
                           o["qr"], o["reliable"], o["status"])
    c = lc.case((7, 6, 2), "cons", ("median",))
    o = lc.poisoned(lc.B, 7, 6, DEV)
    with pytest.raises(RuntimeError):   # weights on the wrong device
        ops.lest_round(c["x"].to(DEV), None, 6, 2, True, 1.0, c["weights"], o["c1"], o["consensus"], o["skew"],
                       o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"])


def test_engine_workspace_follows_lest_route():
    """A rank-weighted engine allocates the workspace its own route asks for, at every size (N = 7 included), and
    hands it to the op: no temporary one per round."""
    from svoc.engine import ConsensusEngine
    for N, D, f in ((7, 6, 2), (64, 33, 8)):
        e = ConsensusEngine(cpu._cfg(N, D, f, essence="rank_weighted"), lc.B, device=DEV, storage="fp32")
        assert e._lest_route.needs_work == 1
        w = e.work()
        assert w is not None and w.numel() == svops.fast_work_numel(lc.B, D) and e.work() is w


def test_engine_rounds_equal_op():
    cpu.engine_rounds_equal_op(DEV)


def test_transactional_step_reverts_one_instance():
    cpu.transactional_step_reverts_one_instance(DEV)


def test_pipelined_step_takes_the_generic_path():
    """step_pipelined on a rank-weighted engine: saved rows, then the restore kernel -- the same results as
    apply_updates + run_round."""
    from svoc.engine import ConsensusEngine
    N, D, f = 64, 33, 8
    c = lc.case((N, D, f), "cons", ("bell", 0.125))
    x = c["x"].clone()
    x[lc.CONSTANT, :, 0] = x[0, :, 0]                      # every instance commits at first
    bad = 1
    # the step: every oracle of every instance moves halfway to its neighbour; instance `bad` is handed a constant
    # column 0, so its round reverts with ZERO_VARIANCE
    new = 0.5 * (x[:, :, :D] + x.roll(1, dims=1)[:, :, :D])
    new[bad, :, 0] = 0.25
    inst = torch.arange(lc.B).repeat_interleave(N)
    oracle = torch.arange(N).repeat(lc.B)
    engines = []
    for pipelined in (False, True):
        e = ConsensusEngine(cpu._cfg(N, D, f, essence="rank_weighted"), lc.B, device=DEV, storage="fp32")
        cpu._fill(e, x, D)
        e.run_round()
        assert (e.status == 0).all()
        if pipelined:
            e.step_pipelined(inst, oracle, new.reshape(-1, D), N, chunks=2)
        else:
            e.apply_updates(inst, oracle, new.reshape(-1, D), unique=True)
            e.run_round()
        e.pipeline_join()
        engines.append(e)
    a, b = engines
    for k in ("values", "enabled", "n_active", "c1", "consensus", "skew", "kurt", "rel", "qr", "reliable", "status"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert int(b.status[0]) == 0 and int(b.status[bad]) == 32
    # the reverted instance holds its pre-batch rows, the others the new ones
    assert torch.equal(b.values[bad].cpu(), x[bad]) and torch.equal(b.values[0, :, :D].cpu(), new[0])


def test_default_config_never_calls_lest(monkeypatch):
    cpu.default_config_never_calls_lest(DEV, monkeypatch)


@pytest.mark.parametrize("explicit", [False, True], ids=["bell", "explicit"])
def test_checkpoint_round_trip(tmp_path, explicit):
    cpu.checkpoint_round_trip(DEV, tmp_path, explicit)


def test_round_is_graph_capturable():
    """The op checks shapes, dtypes and devices only: a round replays from a captured graph."""
    c = lc.case((65, 70, 8), "cons", ("bell", 0.125))
    x, w = c["x"].to(DEV), c["weights"].to(DEV)
    D, f = c["D"], c["f"]
    work = torch.empty(svops.fast_work_numel(lc.B, D), dtype=torch.int32, device=DEV)
    o = lc.poisoned(lc.B, c["N"], D, DEV)
    args = (x, None, D, f, True, c["max_spread"], w, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"],
            o["reliable"], o["status"], work)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        svops.ops().lest_round(*args)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    want = {k: v.clone() for k, v in o.items()}
    for v in o.values():
        v.fill_(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        svops.ops().lest_round(*args)
    g.replay()
    torch.cuda.synchronize()
    for k in o:
        if k == "status":
            assert torch.equal(o[k], want[k]), k
        else:
            ok = (want["status"] == 0)
            assert torch.equal(o[k][ok], want[k][ok]), k
