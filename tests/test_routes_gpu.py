"""The fast routes on a real MI355X (csrc/include/svoc/route.hpp): either side of every kernel boundary runs the
kernel the route names and agrees with the CPU op; the transactional pipelined step rolls back on both sides of the
small / window boundary; and an fp32 engine under wave_hint -7 (the two-network kernel: no fused path) takes the
generic path."""
import pytest
import torch

from helpers import beta_oracles, run_fast
from svoc import ops as svops
from svoc.config import ConsensusConfig
from svoc.engine import ConsensusEngine
from svoc.status import Status
from test_ops_gpu import _cmp_fast

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 4
SMALL, WINDOW, TWO = svops.KERNEL_SMALL, svops.KERNEL_WINDOW, svops.KERNEL_TWO_NETWORK

# (N, D, f, kernel): the smallest shapes at which a misrouted kernel is outside its domain
_BF16_ONLY = [(16, 128, 2, SMALL), (17, 128, 2, WINDOW), (16, 136, 2, WINDOW)]
_BOTH = [(64, 64, 8, WINDOW), (65, 64, 8, WINDOW), (128, 64, 8, WINDOW), (129, 64, 8, WINDOW),
         (256, 64, 32, WINDOW), (256, 64, 33, TWO), (256, 64, 8, WINDOW), (257, 64, 8, TWO)]
_GROUPS = {64: 1, 65: 2, 128: 2, 129: 4}


def _cmp_f32_cpu_twin(g, c):
    """test_f32_gpu.test_f32_kernel_vs_cpu_twin's comparison."""
    for k in ("status", "c1", "consensus", "reliable"):
        assert torch.equal(g[k].cpu(), c[k]), k
    for k in ("qr", "rel"):
        torch.testing.assert_close(g[k].cpu(), c[k], rtol=1e-4, atol=1e-5)
    for k in ("skew", "kurt"):
        torch.testing.assert_close(g[k].cpu(), c[k], rtol=1e-3, atol=5e-4)


@pytest.mark.parametrize("storage,N,D,f,kernel",
                         [("bf16",) + s for s in _BF16_ONLY + _BOTH] + [("fp32",) + s for s in _BOTH])
def test_boundary_shapes_default_route(storage, N, D, f, kernel):
    r = svops.fast_route(storage, N, D, (D + 7) // 8 * 8, f, True, work=svops.WORK_NONE)
    assert r.kernel == kernel and r.lane_groups == _GROUPS.get(N, r.lane_groups), r
    x, _ = beta_oracles(B, N, D, f, seed=5 * N + D + f, dtype=torch.float32 if storage == "fp32" else torch.bfloat16)
    g = run_fast(x.to(DEV), D, f, True)
    c = run_fast(x, D, f, True)
    torch.cuda.synchronize()
    assert torch.equal(g["status"].cpu(), c["status"]) and (c["status"] == 0).all(), (g["status"], c["status"])
    if storage == "fp32":
        _cmp_f32_cpu_twin(g, c)
    else:   # the comparison of test_win_gpu / test_ops_gpu, the CPU op as the reference
        _cmp_fast({k: v.cpu() for k, v in g.items()}, dict(c, reliable=c["reliable"].bool()), c["status"] == 0)


def _engines(storage, N, D, f, wave_hint=0):
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=True)
    pipe, twin = (ConsensusEngine(cfg, batch=B, device=DEV, mode="fast", storage=storage) for _ in range(2))
    for e in (pipe, twin):
        e.wave_hint = wave_hint
        e.randomize(seed=N + D)
        e.run_round()
    return pipe, twin


def _batch(pipe, twin, U, revert):
    """U updates for every instance; instance ``revert``'s make column 3 constant: zero variance, its round reverts."""
    N, D = pipe.N, pipe.D
    g = torch.Generator(device=DEV).manual_seed(7)
    inst = torch.arange(B, device=DEV).repeat_interleave(U)
    orc = torch.stack([torch.randperm(N, device=DEV, generator=g)[:U] for _ in range(B)]).reshape(-1)
    vals = torch.rand(B * U, D, device=DEV, generator=g).to(pipe.vdtype)
    for e in (pipe, twin):
        e.values[revert, :, 3] = 0.625
    vals[revert * U:(revert + 1) * U, 3] = 0.625
    return inst, orc, vals


def _same_as_twin(pipe, twin, st_pipe, st_twin, revert, U):
    pipe.pipeline_join()
    torch.cuda.synchronize()
    assert torch.equal(st_pipe, st_twin), (st_pipe.view(B, U), st_twin.view(B, U))
    assert pipe.status[revert].item() == int(Status.ZERO_VARIANCE) and int((pipe.status == 0).sum()) == B - 1
    assert (st_pipe.view(B, U)[revert] == int(Status.ZERO_VARIANCE)).all()
    for k in ("status", "values", "enabled", "n_active", "consensus", "rel", "c1", "reliable", "skew", "kurt", "qr"):
        assert torch.equal(getattr(pipe, k), getattr(twin, k)), k


@pytest.mark.parametrize("N,D,how", [(16, 128, "restore_kernel"), (17, 128, "in_kernel"), (16, 128, "binding_restore")])
def test_rollback_either_side_of_small_window(N, D, how):
    """bf16 pipelined step, U = 2, one reverting instance: at (16, 128) the small-instance kernel runs and the restore
    kernel rolls back after it (queued by the engine -- or by the binding, when the engine hands the saved batch to
    a round whose kernel cannot roll back); at (17, 128) the window kernel rolls back itself.  Bit for bit the
    state and statuses of apply_updates(unique=True); run_round()."""
    U, revert = 2, 1
    pipe, twin = _engines("bf16", N, D, 2)
    assert pipe._route().kernel == (SMALL if N == 16 else WINDOW)
    assert pipe._kernel_rollback_ok(U) == (how == "in_kernel")
    if how == "binding_restore":
        pipe._kernel_rollback_ok = lambda U: True
    inst, orc, vals = _batch(pipe, twin, U, revert)
    st_twin = twin.apply_updates(inst, orc, vals, unique=True)
    twin.run_round()
    pipe.step_pipelined(inst, orc, vals, U, chunks=2)
    _same_as_twin(pipe, twin, pipe._save_bufs[("pipe",)][2][:B * U], st_twin, revert, U)


def test_wave_hint_two_network_fp32_takes_generic_path():
    """fp32 engine under wave_hint -7: the route names the two-network kernel, which has no fused path, so the
    pipelined step saves rows and restores (before the route was asked, the fused batch reached a dispatcher
    that refused it: "launch failed: -3")."""
    U, revert = 2, 2
    pipe, twin = _engines("fp32", 8, 16, 2, wave_hint=-7)
    inst, orc, vals = _batch(pipe, twin, U, revert)
    assert pipe._route().kernel == TWO and not pipe._fused_ok(inst, orc, vals, U)
    assert bool((pipe.n_active == pipe.N).all())
    st_twin = twin.apply_updates(inst, orc, vals, unique=True)
    twin.run_round()
    pipe.step_pipelined(inst, orc, vals, U, chunks=2)
    _same_as_twin(pipe, twin, pipe._save_bufs[("pipe",)][2][:B * U], st_twin, revert, U)
