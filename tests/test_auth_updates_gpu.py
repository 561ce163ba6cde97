"""The address-lookup kernel (csrc/kernels/address_lookup.hip) and the authenticated update path on the GPU:
kernel == CPU op on the planted cases, graph replay, the exact mixed stream == the CPU service ==
``ReferenceContract`` (general and strided transaction paths), the lookup inside a full fast step, and the
refusal of host tensors.  All checks are equalities on integers or bit patterns."""
import random

import pytest
import torch

import auth_cases as ac
from svoc import ops as svops
from svoc.codec import addresses_to_limbs
from svoc.status import Status

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("M", ac.LOOKUP_M)
def test_kernel_matches_cpu_op(M):
    """K = 203 leaves the last block and the last wave partial for every lane-group size (203 * L is no multiple
    of 64 for L < 64); with L < 64 a wave then holds lookups of different instances, unknown ones among them.
    K = 1 and K = 67: a single group, and a batch shorter than a block."""
    o = svops.ops()
    for K in (203, 67, 1):
        table, inst, addr, want = ac.lookup_case(M, K=K, seed=K)
        cpu = torch.full_like(inst, 77)
        o.find_address(table, inst, addr, cpu)
        assert torch.equal(cpu, want)
        out = torch.full((K,), 77, dtype=torch.int64, device=DEV)
        o.find_address(table.to(DEV), inst.to(DEV), addr.to(DEV), out)
        assert torch.equal(out.cpu(), cpu), (M, K)
    o.find_address(table.to(DEV), inst[:0].to(DEV), addr[:0].to(DEV), out[:0])     # K = 0: no launch


def test_resolve_oracles_replays_in_a_graph():
    svc = ac.service(DEV)
    book = ac.oracle_book()
    gov = svc.gov
    rng = random.Random(2)
    K = 50
    inst_l = [rng.randrange(-1, ac.B + 1) for _ in range(K)]
    pick = lambda: [book[rng.randrange(ac.B)][rng.randrange(ac.N)] for _ in range(K)]  # noqa: E731
    inst = torch.tensor(inst_l, device=DEV)
    caller = addresses_to_limbs(pick(), device=DEV)
    out = torch.full((K,), 77, dtype=torch.int64, device=DEV)

    def cpu_op():
        want = torch.empty(K, dtype=torch.int64)
        svops.ops().find_address(gov.oracle_addr.cpu(), inst.cpu(), caller.cpu(), want)
        return want

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gov.resolve_oracles(inst, caller, out=out)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # one stream, no parallel branches
        gov.resolve_oracles(inst, caller, out=out)
    out.fill_(77)
    g.replay()
    first = cpu_op()
    assert torch.equal(out.cpu(), first) and int((first >= 0).sum()) > 0 and int((first < 0).sum()) > 0
    # new callers and one replaced table entry, both in place: the replay reads the current memory
    caller.copy_(addresses_to_limbs(pick(), device=DEV))
    caller[0] = ac.limbs(ac.new_oracle(7)).to(DEV)
    inst[0] = 2
    gov.oracle_addr[2, 3] = ac.limbs(ac.new_oracle(7)).to(DEV)
    g.replay()
    second = cpu_op()
    assert torch.equal(out.cpu(), second) and second[0].item() == 3 and not torch.equal(first, second)


def test_exact_stream_matches_cpu_service_and_reference():
    stream = ac.Stream()
    contracts, want = stream.replay_reference()
    cpu, gpu, gpu_general = ac.service("cpu"), ac.service(DEV), ac.service(DEV)
    st_cpu = ac.run_exact_stream(cpu, stream)
    st_gpu = ac.run_exact_stream(gpu, stream)                         # phase 4: strided waves (verdict rounds)
    st_gen = ac.run_exact_stream(gpu_general, stream, strided=False)  # phase 4: the general grouping's waves
    assert st_gpu == want and st_cpu == want and st_gen == want
    assert Status.NOT_ORACLE in want["phase4"] and Status.INTERVAL_INPUT in want["phase4"]
    for svc in (gpu, gpu_general):
        ac.check_against_contracts(svc, contracts)
        for k in ac.STATE:
            if k != "status":
                assert torch.equal(getattr(svc.engine, k).cpu(), getattr(cpu.engine, k)), k
        assert torch.equal(svc.gov.oracle_addr.cpu(), cpu.gov.oracle_addr)


def test_lookup_inside_a_full_fast_step():
    """N = 100 (a multi-chunk lookup), D = 8, B = 3, fp32: update_batch == engine.step with Python-resolved
    indices, statuses and state bit for bit."""
    n, d, batch = 100, 8, 3
    book = ac.oracle_book(n, batch, seed=3)
    auth = ac.service(DEV, "fast", "fp32", n=n, d=d, f=10, batch=batch, book=book)
    plain = ac.service(DEV, "fast", "fp32", n=n, d=d, f=10, batch=batch, book=book)
    rng = random.Random(8)
    g = torch.Generator().manual_seed(8)
    slots = [(b, o) for b in range(batch) for o in range(n)]
    rng.shuffle(slots)
    first = [(b, book[b][o], o) for b, o in slots]                    # the activating batch
    second = [(b, book[b][o], o) for b, o in slots[:40]]
    second += [(0, book[1][5], -1), (1, ac.UNKNOWN, -1), (batch, book[0][0], -1), (2, book[2][99], 99),
               (2, book[2][64], 64), (-3, book[0][1], -1)]
    for items in (first, second):
        inst = torch.tensor([b for b, _, _ in items], device=DEV)
        caller = addresses_to_limbs((c for _, c, _ in items), device=DEV)
        orc = torch.tensor([o for _, _, o in items], device=DEV)
        vals = torch.rand(len(items), d, generator=g).to(DEV)
        if items is second:
            vals[41, 3] = 1.5                                        # an unknown caller out of the interval
        st_a = auth.update_batch(inst, caller, vals)
        st_p = plain.engine.step(inst, orc, vals)
        assert torch.equal(st_a, st_p)
    tail = st_a[40:].tolist()
    assert tail == [int(Status.NOT_ORACLE), int(Status.INTERVAL_INPUT), int(Status.NOT_ORACLE), 0, 0,
                    int(Status.NOT_ORACLE)]
    assert bool(auth.engine.consensus_active.all())
    for k in ac.STATE:
        assert torch.equal(getattr(auth.engine, k), getattr(plain.engine, k)), k


def test_find_address_rejects_host_tensors():
    table, inst, addr, _ = ac.lookup_case(7)
    o = svops.ops()
    dt, di, da = table.to(DEV), inst.to(DEV), addr.to(DEV)
    out = torch.empty_like(di)
    for args in ((dt, inst, da, out), (dt, di, addr, out), (dt, di, da, torch.empty_like(inst)),
                 (table, di, da, out)):
        with pytest.raises(RuntimeError, match="must be on|device"):
            o.find_address(*args)
