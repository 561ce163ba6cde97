"""The status ladder's upper rungs on every fast kernel (csrc/include/svoc/verdict.hpp): f = N reverts with
USIZE_UNDERFLOW (8), f = N - 1 with INDEX_OOB (5), f = N - 2 with TOO_FEW_RELIABLE (33) -- or, under the legacy
contract, which has no moments, commits.  Each shape is the smallest that svoc.ops.fast_route sends to its kernel;
the window kernels take f <= N - 2 only, so their shapes' two high rungs fall to the two-network kernel of the same
storage.  The status is the CPU twin's, and a reverted round leaves every output untouched (test_revert_gpu.py
covers codes 6, 32 and 33 the same way)."""
import pytest
import torch

from helpers import alloc_fast_out, beta_oracles
from svoc import ops as svops
from test_revert_gpu import OUTS, SENT

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, D = 4, 10
KERNEL = {("bf16", svops.KERNEL_SMALL): "small", ("bf16", svops.KERNEL_WINDOW): "win",
          ("bf16", svops.KERNEL_TWO_NETWORK): "reg", ("fp32", svops.KERNEL_WINDOW): "winf",
          ("fp32", svops.KERNEL_TWO_NETWORK): "f32"}

# (storage, N, f, legacy, kernel, status).  N = 36: f = N - 2 > 32 keeps the lowest rung on the two-network kernels
# (their high rungs run at the window shapes).
CASES = [("bf16", 7, 7, False, "small", 8), ("bf16", 7, 6, False, "small", 5),
         ("bf16", 7, 5, False, "small", 33), ("bf16", 7, 5, True, "small", 0),
         ("bf16", 17, 17, False, "reg", 8), ("bf16", 17, 16, False, "reg", 5),
         ("bf16", 17, 15, False, "win", 33), ("bf16", 17, 15, True, "win", 0),
         ("bf16", 36, 34, False, "reg", 33), ("bf16", 36, 34, True, "reg", 0),
         ("fp32", 4, 4, False, "f32", 8), ("fp32", 4, 3, False, "f32", 5),
         ("fp32", 4, 2, False, "winf", 33), ("fp32", 4, 2, True, "winf", 0),
         ("fp32", 36, 34, False, "f32", 33), ("fp32", 36, 34, True, "f32", 0)]


def _run(x, f, legacy):
    o = alloc_fast_out(B, x.shape[1], D, x.device)
    for k, v in SENT.items():
        o[k].fill_(v)
    svops.ops().fast_round(x, None, D, f, True, 1.0, o["c1"], o["consensus"], o["skew"], o["kurt"], o["rel"], o["qr"],
                           o["reliable"], o["status"], 0, 0, 0, legacy, None)
    return o


def test_cases_reach_every_kernel():
    assert {c[4] for c in CASES} == set(KERNEL.values())


@pytest.mark.parametrize("storage,N,f,legacy,kernel,status", CASES)
def test_upper_rungs(storage, N, f, legacy, kernel, status):
    r = svops.fast_route(storage, N, D, (D + 7) // 8 * 8, f, True, legacy, work=svops.WORK_NONE)
    assert KERNEL[(storage, r.kernel)] == kernel, r
    # honest oracles only: the legacy reliability (no division by D) of uniform rows would leave [0, 1]
    x, _ = beta_oracles(B, N, D, 0, seed=N + f, dtype=torch.float32 if storage == "fp32" else torch.bfloat16)
    o = _run(x.to(DEV), f, legacy)
    oc = _run(x, f, legacy)
    torch.cuda.synchronize()
    st = o["status"].cpu()
    assert torch.equal(st, oc["status"]), (st, oc["status"])
    assert st.tolist() == [status] * B
    for k in OUTS:
        for b in range(B):
            untouched = bool((o[k][b].cpu() == SENT[k]).all())
            assert untouched == (status != 0), (k, b)
            assert bool((oc[k][b] == SENT[k]).all()) == untouched, (k, b)   # the CPU twin writes the same set
