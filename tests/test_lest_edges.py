"""The rank-weighted round where its centre leaves the honest rows, on the CPU: every case of lest_edge_cases is
built (the builders assert that a case bites: the guard's trigger with its margin, the first-read arithmetic missing
the tolerance, the masks) and the op's CPU twin is held to the fp64 model with the shared checks.  The twin takes
the moments in fp64 about the reliable mean, so it has no guard: what it pins here is the data, the model and the
checks that test_lest_edges_gpu.py applies to consensus_fast_lest.hip."""
import pytest
import torch

import lest_cases as lc
import lest_edge_cases as ec
from svoc import ops as svops

DEV = "cpu"


def test_shapes_cover_every_lane_group():
    assert {ec.LANES[s[0]] for s in ec.SHAPES} == {1, 2, 4}
    for N, D, f in ec.SHAPES:
        r = svops.lest_route("fp32", N, D, (D + 7) // 8 * 8, f, True)
        assert (r.supported, r.lane_groups) == (1, ec.LANES[N])
    assert ec.tie_shapes() == ec.SHAPES          # tie_params can be met at every shape


# ------------------------------------------------------------------------------------------------ family A
@pytest.mark.parametrize("key", ec.a_matrix(), ids=ec.a_id)
def test_displaced_centre(key):
    c = ec.displaced_case(key)
    ec.check_displaced(ec.run_case(svops.ops(), c, DEV), c)


@pytest.mark.parametrize("key", ec.a_matrix(), ids=ec.a_id)
def test_displaced_control(key):
    """The control instance of the same batch: outliers at 0.5 +- M alternating by row, c1 central, no re-read.
    At M = 1024 the honest rows' qr about c1 meets fast_cases.TOL["fp32"] only because c1 is accumulated in fp64
    and rounded once: an fp32 chain over terms ~ w M rounds c1 by ~ 2^-24 w M, ~ 10^-3 of the honest rows' spread,
    and moved these qr by 2.9 .. 6.9 times their tolerance (while c1 itself used 3% of its own bound)."""
    c = ec.displaced_case(key)
    ec.check_control(ec.run_case(svops.ops(), c, DEV), c)


def test_unguarded_arithmetic_is_the_kernels_when_centred():
    """unguarded_fp32 about the reliable mean itself (what the guard's re-read does) meets the tolerance on the
    displaced instances it misses about c1: the emulation fails for the shift, not for a mistake of its own."""
    c = ec.displaced_case(((64, 33, 8), 1024.0, ("mean",), False))
    ref, D = c["ref"], c["D"]
    b = ec.A_KINDS.index("all")
    mask = ref["reliable"][b]
    x = c["x"][b, :, :D]
    sk, ku = ec.unguarded_fp32(x, mask, ref["c1"][b].float())
    assert ec.misses_tol(sk, ref["skew"][b], "skew").any() and ec.misses_tol(ku, ref["kurt"][b], "kurt").any()
    mean = x.double()[mask].mean(0).float()
    sk, ku = ec.unguarded_fp32(x, mask, mean)
    assert not ec.misses_tol(sk, ref["skew"][b], "skew").any() and not ec.misses_tol(ku, ref["kurt"][b], "kurt").any()


def test_displaced_checks_reject_a_first_read_result():
    """check_round fails on the outputs an unguarded pass 2 would commit."""
    c = ec.displaced_case(((64, 33, 8), 16.0, ("mean",), False))
    o = ec.run_case(svops.ops(), c, DEV)
    ec.check_displaced(o, c)
    b = ec.A_KINDS.index("neg")
    sk, ku = ec.unguarded_fp32(c["x"][b, :, :c["D"]], c["ref"]["reliable"][b], c["ref"]["c1"][b].float())
    o["skew"][b], o["kurt"][b] = torch.nan_to_num(sk.float()), torch.nan_to_num(ku.float())
    with pytest.raises(AssertionError, match="skew|kurt"):
        ec.check_displaced(o, c)


# ------------------------------------------------------------------------------------------------ family B
@pytest.mark.parametrize("key", ec.b_matrix(), ids=ec.b_id)
def test_huge_displaced_centre(key):
    c = ec.huge_case(key)
    ec.check_huge(ec.run_case(svops.ops(), c, DEV), c)


def test_huge_checks_reject_nan_and_finite_qr():
    c = ec.huge_case(((7, 6, 2), 80, ("mean",)))
    good = ec.run_case(svops.ops(), c, DEV)
    ec.check_huge(good, c)
    for key, bad in (("skew", float("nan")), ("kurt", float("nan")), ("qr", 1e30), ("rel", 1e-7)):
        o = {k: v.clone() for k, v in good.items()}
        o[key][0, 0] = bad
        with pytest.raises(AssertionError):
            ec.check_huge(o, c)


# ------------------------------------------------------------------------------------------------ family C
@pytest.mark.parametrize("key", ec.c_matrix(), ids=ec.c_id)
def test_extremes_behind_zero_weights(key):
    c = ec.zero_weight_case(key)
    ec.check_zero_weight(ec.run_case(svops.ops(), c, DEV), c)


# ------------------------------------------------------------------------------------------------ family D
@pytest.mark.parametrize("key", ec.d_matrix(), ids=ec.d_id)
def test_rank_cut_ties(key):
    c = ec.tie_case(key)
    ec.check_tie(ec.run_case(svops.ops(), c, DEV), c)


# ------------------------------------------------------------------------------------------------ engine
def engine_round_equals_op(device):
    """A rank-weighted engine with explicit mean weights over a family-A case (unconstrained: the updates of a
    constrained engine must lie in [0, 1]) equals the op, bit for bit."""
    from svoc.config import ConsensusConfig
    from svoc.engine import ConsensusEngine
    import test_lest as tl
    shape = (64, 33, 8)
    N, D, f = shape
    c = ec.displaced_case((shape, 16.0, ("mean",), False))
    cfg = ConsensusConfig(n_oracles=N, dimension=D, n_failing_oracles=f, constrained=False,
                          unconstrained_max_spread=c["max_spread"], essence="rank_weighted")
    e = ConsensusEngine(cfg, lc.B, device=device, storage="fp32", rank_weights=(c["w1"], c["w2"]))
    assert torch.equal(e._lest.cpu(), c["weights"])
    assert (tl._fill(e, c["x"], D).cpu() == 0).all()
    e.run_round()
    o = lc.run_lest(svops.ops(), c["x"].to(device), None, D, f, False, float(cfg.unconstrained_max_spread),
                    c["weights"])
    for b in range(lc.B):
        assert int(e.status[b]) == int(o["status"][b]) == (lc.ST_ZERO_VARIANCE if b == lc.CONSTANT else lc.ST_OK)
        if b != lc.CONSTANT:
            for k in ("c1", "consensus", "skew", "kurt", "rel", "qr", "reliable"):
                assert lc.same_bits(getattr(e, k)[b].cpu().float(), o[k][b].float()), (k, b)
    # ... and the op's outputs are the model's (the inactive instance of the case is active here)
    full = dict(c, active=torch.ones(lc.B, dtype=torch.uint8))
    lc.check_round(o, full)


def test_engine_round_equals_op():
    engine_round_equals_op(DEV)
