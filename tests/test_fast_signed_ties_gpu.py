"""Fast-mode HIP kernels on signed values and on quadratic-risk ties at the rank cut, against ref64.

Every case of fast_cases.matrix() (data and fp64 reference pinned by test_fast_signed_ties.py) runs
through each dispatch: wave_hint 0 (small-instance kernel for N <= 16, D <= 128 bf16; window kernel
for N <= 256, f <= 32; two-network kernel otherwise) and, for N <= 256, wave_hint -7 (two-network
kernel).  Negative bf16 / fp32 sort keys, the sentinel split of the padding rows and the rank rule
(qr ascending, index descending) each meet a reference that shares no code with the kernels:
reliable, c1 and the constrained consensus bit for bit; the unconstrained mean within the forward
bound of an fp32 sum; qr, rel and the moments within the project's fast-mode tolerances.

Unconstrained values so large that a deviation power overflows fp32 (qr = +inf, which ties with the
padding rows of the small kernel's rank count) are test_fast_extreme.py's and test_fast_extreme_gpu.py's.
Non-finite inputs are rejected by the update kernels and are not tested here either.
"""
import pytest
import torch

import fast_cases as fc
from helpers import alloc_fast_out, fast_work, run_fast
from svoc import ops as svops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = fc.matrix()


def _cpu(o):
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_fast_kernels_vs_ref64(case):
    c = fc.make(case)
    xg = c["x"].to(DEV)
    args = (c["D"], c["f"], c["constrained"], c["max_spread"])
    hints = (0, -7) if c["N"] <= 256 else (0,)
    outs = [run_fast(xg, *args, wave_hint=h) for h in hints]
    torch.cuda.synchronize()
    outs = [_cpu(o) for o in outs]
    cpu = run_fast(c["x"], *args)
    for h, o in zip(hints, outs):
        assert torch.equal(o["status"], cpu["status"]), (h, o["status"], cpu["status"])
        fc.check_round(o, c, "hint%d %s" % (h, fc.case_id(case)))
    if len(outs) == 2:      # same order statistics in both kernels
        for k in ("c1", "reliable") + (("consensus",) if c["constrained"] else ()):
            assert torch.equal(outs[0][k], outs[1][k]), k


_SPLIT = [(("tie", False), 256, 72, 32), (("signed", 8.0, -4.0), 128, 64, 16)]


@pytest.mark.parametrize("storage", ["bf16", "fp32"])
@pytest.mark.parametrize("fam,N,D,f", _SPLIT, ids=lambda v: str(v) if isinstance(v, int) else v[0])
def test_split_modes_bitwise(fam, N, D, f, storage):
    """mode 1 + mode 2 through a persistent workspace == the fused round, bit for bit."""
    c = fc.make((fam, N, D, f, storage))
    assert c["expect"] is not None or c["structured"]
    xg = c["x"].to(DEV)
    B = xg.shape[0]
    full = run_fast(xg, D, f, c["constrained"], c["max_spread"])
    o = alloc_fast_out(B, N, D, DEV)
    w = fast_work(B, D, DEV)
    args = (xg, None, D, f, c["constrained"], c["max_spread"], o["c1"], o["consensus"], o["skew"], o["kurt"],
            o["rel"], o["qr"], o["reliable"], o["status"], 0)
    svops.ops().fast_round(*args, 1, D, False, w)
    svops.ops().fast_round(*args, 2, D, False, w)
    torch.cuda.synchronize()
    assert (full["status"] == 0).all()
    for k in full:
        assert torch.equal(o[k], full[k]), k
    fc.check_round(_cpu(o), c, "split %s" % fc.case_id((fam, N, D, f, storage)))
