"""Batched governance kernels (csrc/kernels/governance.hip) vs the in-order CPU implementation and, for the
cases of tests/gov_cases.py, vs the golden contract (one svoc.reference.ReferenceContract per instance)."""
import random

import pytest
import torch

import gov_cases as gc
from svoc.governance import Governance

pytestmark = pytest.mark.gpu


def _run(device, actions, B, A, N):
    g = Governance(B, A, N, device, True, 2)
    admins = [[10_000 * (b + 1) + a for a in range(A)] for b in range(B)]
    oracles = [[20_000 * (b + 1) + o for o in range(N)] for b in range(B)]
    g.set_addresses(admins, oracles)
    st, ap = g.submit(actions)
    return ([t.cpu() for t in (g.oracle_addr, g.votes, g.prop_tag, g.prop_idx, g.prop_addr)],
            st.cpu(), ap.cpu())


def test_governance_gpu_matches_cpu():
    rng = random.Random(0)
    B, A, N = 64, 5, 9
    actions = []
    for _ in range(3000):
        b = rng.randrange(B)
        caller = 10_000 * (b + 1) + rng.randrange(A + 1)       # sometimes not an admin
        if rng.random() < 0.35:
            prop = None if rng.random() < 0.15 else (rng.randrange(-1, N + 1), 20_000 * (b + 1) + rng.randrange(N + 6))
            actions.append(("propose", b, caller, prop))
        else:
            actions.append(("vote", b, caller, rng.randrange(A + 1), rng.random() < 0.85))
    cpu = _run("cpu", actions, B, A, N)
    gpu = _run("cuda", actions, B, A, N)
    for x, y in zip(cpu[0], gpu[0]):
        assert torch.equal(x, y)
    assert torch.equal(cpu[1], gpu[1]) and torch.equal(cpu[2], gpu[2])
    assert int(cpu[2].sum()) > 0          # some replacements happened


def _random_batch(K, B, A, N, seed, device):
    """K mixed actions as tensors (repeated instances, non-admin callers, None propositions, bad indices)."""
    from svoc.codec import address_to_limbs
    g = torch.Generator().manual_seed(seed)
    inst = torch.randint(0, B, (K,), generator=g)
    inst[torch.rand(K, generator=g) < 0.002] = B + 3                                   # out of range
    who = torch.randint(0, A + 1, (K,), generator=g)                                   # A: not an admin
    kind = (torch.rand(K, generator=g) >= 0.35).to(torch.int32)                        # 1 = vote
    arg0 = torch.where(kind == 1, torch.randint(0, A + 1, (K,), generator=g),
                       (torch.rand(K, generator=g) >= 0.15).long()).to(torch.int32)
    arg1 = torch.where(kind == 1, (torch.rand(K, generator=g) < 0.85).long(),
                       torch.randint(-1, N + 1, (K,), generator=g))
    # admin a of instance b: 10_000 (b + 1) + a; oracle o: 20_000 (b + 1) + o (as _run's addresses)
    caller_int = 10_000 * (inst + 1) + who
    new_int = 20_000 * (inst + 1) + torch.randint(0, N + 6, (K,), generator=g)
    limbs = lambda v: torch.tensor([address_to_limbs(int(x)) for x in v.tolist()], dtype=torch.int64)  # noqa: E731
    # (addresses below 2^63: the low limb alone; checked against the codec on a prefix)
    caller = torch.zeros(K, 4, dtype=torch.int64)
    caller[:, 0] = caller_int
    addr = torch.zeros(K, 4, dtype=torch.int64)
    addr[:, 0] = new_int
    assert torch.equal(caller[:64], limbs(caller_int[:64])) and torch.equal(addr[:64], limbs(new_int[:64]))
    return {k: v.to(device) for k, v in dict(inst=inst, caller=caller, kind=kind, arg0=arg0, arg1=arg1, addr=addr).items()}


def _gov(device, B, A, N):
    g = Governance(B, A, N, device, True, 2)
    g.set_addresses([[10_000 * (b + 1) + a for a in range(A)] for b in range(B)],
                    [[20_000 * (b + 1) + o for o in range(N)] for b in range(B)])
    return g


def test_governance_ordered_batch_matches_cpu():
    """submit_batch: action tensors in, any number of actions per instance, the device sorts
    the batch by instance and one launch applies each instance's run in submission order -- statuses, applied
    flags and the whole governance state equal the in-order CPU implementation."""
    B, A, N = 300, 5, 9
    acts = _random_batch(20_000, B, A, N, seed=1, device="cpu")
    out = {}
    for dev in ("cpu", "cuda"):
        g = _gov(dev, B, A, N)
        st, ap = g.submit_batch(**{k: v.to(dev) for k, v in acts.items()})
        out[dev] = [t.cpu() for t in (st, ap, g.oracle_addr, g.votes, g.prop_tag, g.prop_idx, g.prop_addr)]
    for x, y in zip(out["cpu"], out["cuda"]):
        assert torch.equal(x, y)
    assert int(out["cpu"][1].sum()) > 10


def test_governance_service_one_million_mixed_actions():
    """ConsensusService.governance with 1M mixed actions over 1M instances (VERDICT r5 item 7 'done'): tensors
    in, statuses out, no per-action host work; the statuses equal the CPU engine's, well under a second."""
    import time
    from svoc.api import ConsensusService
    from svoc.config import ConsensusConfig
    B, A, N, K = 1 << 20, 3, 7, 1 << 20
    cfg = ConsensusConfig(n_oracles=N, dimension=6, n_failing_oracles=2, n_admins=A, required_majority=2)
    acts = _random_batch(K, B, A, N, seed=2, device="cpu")
    res = {}
    for dev in ("cuda", "cpu"):
        svc = ConsensusService(cfg, B, [0] * A, [0] * N, device=dev, mode="fast")
        b = torch.arange(B, dtype=torch.int64)[:, None]
        svc.gov.admins.zero_()
        svc.gov.admins[:, :, 0] = (10_000 * (b + 1) + torch.arange(A)).to(dev)
        svc.gov.oracle_addr.zero_()
        svc.gov.oracle_addr[:, :, 0] = (20_000 * (b + 1) + torch.arange(N)).to(dev)
        a = {k: v.to(dev) for k, v in acts.items()}
        if dev == "cuda":
            svc.governance(a)                      # warm-up (sort workspace, first launch), on a copy of the state
            svc.gov.votes.zero_(); svc.gov.prop_tag.zero_()
            svc.gov.oracle_addr[:, :, 0] = (20_000 * (b + 1) + torch.arange(N)).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        st, ap = svc.governance(a)
        if dev == "cuda":
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"1M governance actions on the GPU: {dt * 1e3:.1f} ms")
            assert dt < 0.5, dt
        res[dev] = (st.cpu(), ap.cpu(), svc.gov.votes.cpu(), svc.gov.oracle_addr.cpu())
    for x, y in zip(res["cpu"], res["cuda"]):
        assert torch.equal(x, y)


# ---- the golden contract as the reference (tests/gov_cases.py; the CPU ops meet it in test_governance_model.py)
def _gov_for(built):
    return Governance(built.B, built.A, built.N, "cuda", True, built.majority)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_random_case_gpu_matches_golden(shape):
    """submit_batch (device sort + governance_seq): 3000 mixed actions over 3-8 instances with full-width
    addresses one limb apart, 1 to 64 admins; statuses, applied flags and the whole state against one
    ReferenceContract per instance."""
    built = gc.random_case(shape)
    gc.check_ordered(_gov_for(built), built)


def test_directed_majority_64_gpu_matches_golden():
    """A = 64, majority 64: the 64th vote applies (bit 63 of the column last, or first and withdrawn), a majority
    on a None proposition reverts without storing the bit, one-limb-away addresses, instances outside [0, B)."""
    built = gc.directed_case()
    gc.check_ordered(_gov_for(built), built)


def test_empty_batch_gpu():
    built = gc.empty_case()
    gc.check_ordered(_gov_for(built), built)
    gc.check_unordered(_gov_for(built), built)


@pytest.mark.parametrize("shape", gc.SHAPES, ids=gc.shape_id)
def test_unique_slice_gpu_matches_golden(shape):
    """submit_tensors (the unordered governance op, one lane per action): 640 unique instances in shuffled order,
    a proposition everywhere and then the deciding vote, each launch against the golden."""
    built = gc.slice_case(shape)
    gc.check_unordered(_gov_for(built), built)


def test_governance_ops_refuse_a_host_tensor_among_device_tensors():
    """The dispatcher takes the HIP path when any argument is a device tensor; the bindings refuse the call before
    a kernel could read through a host pointer (every tensor position of both ops, the order included)."""
    built = gc.empty_case()
    g = gc.setup(_gov_for(built), built)
    ad = built.addr
    acts = gc.action_tensors([gc.Action(b, ad.admins[b][0], gc.PROPOSE, 1, 0, ad.spares[b][0]) for b in range(built.B)])
    a = {k: v.cuda() for k, v in acts.items()}
    K = built.B
    status = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    applied = torch.zeros(K, dtype=torch.uint8, device="cuda")
    order = torch.arange(K, dtype=torch.int64, device="cuda")
    state = [g.admins, g.oracle_addr, g.votes, g.prop_tag, g.prop_idx, g.prop_addr]
    tensors = state + [a[n] for n in ("inst", "caller", "kind", "arg0", "arg1", "addr")]
    ops = torch.ops.svoc

    def call(seq, t, order, status, applied):
        if seq:
            ops.governance_seq(*t, True, g.majority, order, status, applied)
        else:
            ops.governance(*t, True, g.majority, status, applied)

    for seq in (False, True):
        for k in range(len(tensors)):
            with pytest.raises(RuntimeError):
                call(seq, [(t.cpu() if i == k else t) for i, t in enumerate(tensors)], order, status, applied)
        with pytest.raises(RuntimeError):
            call(seq, tensors, order, status.cpu(), applied)
        with pytest.raises(RuntimeError):
            call(seq, tensors, order, status, applied.cpu())
    with pytest.raises(RuntimeError):
        call(True, tensors, order.cpu(), status, applied)
    torch.cuda.synchronize()
    assert (status == -1).all() and not g.prop_tag.any() and not g.votes.any()
    call(True, tensors, order, status, applied)            # the same call with every tensor on the device runs
    assert (status.cpu() == 0).all() and g.prop_tag[:, 0].cpu().tolist() == [1] * K
