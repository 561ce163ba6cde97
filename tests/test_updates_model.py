"""The CPU update / restore / commit ops against the sequential model of update_cases.py.

Runs without a GPU, over the whole case matrix: it pins the model and the CPU twin of updates.hip
(csrc/bindings/ops_extra.cpp) to each other on every machine, by the assertions the GPU tests use,
and checks that the matrix still reaches every branch of the kernels' dispatch.
test_updates_gpu.py then runs the HIP kernels against the same model.
"""
import pytest
import torch

import update_cases as uc
from svoc import ops as svops
from svoc.status import Status

CASES = uc.matrix()


def test_constants_match_the_package():
    assert (uc.OK, uc.NOT_ACTIVE, uc.INTERVAL_INPUT, uc.NOT_ORACLE, uc.RELIABILITY_INTERVAL, uc.ZERO_VARIANCE,
            uc.NON_FINITE) == (Status.OK, Status.NOT_ACTIVE, Status.INTERVAL_INPUT, Status.NOT_ORACLE,
                               Status.RELIABILITY_INTERVAL, Status.ZERO_VARIANCE, Status.NON_FINITE)


@pytest.mark.parametrize("case", CASES, ids=uc.case_id)
def test_case_holds_what_it_is_built_for(case):
    """The builder's promises: every lane of a group has an update whose only bad element it owns, bad
    and valid updates alternate, index edges and duplicates are there, U does not fill its last block."""
    m = uc.make(case)
    st, U, L, C = m["model"]["upd_status"], m["U"], m["L"], m["C"]
    assert U == 1 or U % (256 // L) != 0
    assert not m["model"]["touched"][-1] and m["model"]["touched"][:-1].any()
    if U == 1:
        return
    thinned = case.U and m["n_special"] < min(L, C)
    if not thinned:
        assert m["lanes_hit"] == set(range(min(L, C))), m["lanes_hit"]
    has_bad = bool(uc.edge_values(case.storage, case.constrained)[0])
    codes = set(st.tolist())
    value_code = uc.INTERVAL_INPUT if case.constrained else uc.NON_FINITE
    assert codes == {uc.OK, uc.NOT_ORACLE} | ({value_code} if has_bad else set())
    bad = (st != uc.OK).nonzero().flatten().tolist()
    inst, orc = m["inst"].tolist(), m["oracle"].tolist()
    in_range = [0 <= inst[u] < m["B"] and 0 <= orc[u] < m["N"] for u in range(U)]
    assert all(st[u - 1] == uc.OK and st[u + 1] == uc.OK for u in bad)
    # an update failing both checks reports the value's code
    assert has_bad == any(not in_range[u] and st[u] != uc.NOT_ORACLE for u in bad)
    slots = [(inst[u], orc[u]) for u in range(U) if in_range[u]]
    if case.unique:
        assert len(set(slots)) == len(slots)
    else:
        writers = {}
        for u in range(U):
            if in_range[u]:
                writers.setdefault((inst[u], orc[u]), []).append(u)
        dup = [w for w in writers.values() if len(w) > 1]
        assert {len(w) for w in dup} >= {2, 3}
        win = m["model"]["winner"]
        pre_en, post_en = m["state"]["enabled"], m["model"]["enabled"]
        assert any(st[w[-1]] == uc.OK and len(w) >= 3 for w in dup)                                  # last writer valid
        # a first commit written twice
        assert any(not pre_en[inst[w[0]], orc[w[0]]] and sum(int(st[u] == uc.OK) for u in w) >= 2 for w in dup)
        if has_bad:
            assert any(st[w[-1]] != uc.OK and win[inst[w[0]], orc[w[0]]] in w[:-1] for w in dup)     # previous valid wins
            assert any(win[inst[w[0]], orc[w[0]]] == -1 and not post_en[inst[w[0]], orc[w[0]]] for w in dup)  # untouched


@pytest.mark.parametrize("case", CASES + (uc.restore_grid_case(),), ids=uc.case_id)
def test_cpu_apply_then_restore_vs_model(case):
    m = uc.make(case)
    ops = svops.ops()
    tag = uc.case_id(case)
    r = uc.Run(m, "cpu")
    r.apply(ops)
    uc.check_apply(r, tag, sequential_save=True)
    if not case.save:
        return
    status, active = uc.round_status(m["B"], sparse=case.U > 10000)
    for inactive in (-1, uc.NOT_ACTIVE):
        if inactive != -1:
            r = uc.Run(m, "cpu")
            r.apply(ops)
        r.restore(ops, status, active, inactive)
        want = uc.check_restore(r, status, active, inactive, "%s inactive=%d" % (tag, inactive))
        assert torch.equal(r.touched, m["model"]["touched"])
    # the vectors exercise every rule: kept, reverted with either code, inactive with and without a code
    st0 = m["model"]["upd_status"]
    if m["U"] > 1:
        assert {uc.OK, uc.ZERO_VARIANCE, uc.RELIABILITY_INTERVAL, uc.NOT_ACTIVE} <= set(want["upd_status"].tolist())
        assert not torch.equal(want["values"].view(torch.uint8), m["model"]["values"].view(torch.uint8))
        assert (st0 != uc.OK).sum() == 0 or torch.equal(want["upd_status"][st0 != uc.OK], st0[st0 != uc.OK])


@pytest.mark.parametrize("cc", uc.COMMIT_CASES, ids=lambda cc: "%s-%dx%d-off%d" % (cc[0], cc[1], cc[2], cc[6]))
def test_cpu_commit_vs_model(cc):
    mc = uc.make_commit(cc)
    assert mc["n"] < cc[4] * cc[5] and (mc["st"] != 0).any() and ((mc["oracle"] < 0) | (mc["oracle"] >= cc[3])).any()
    assert not torch.equal(mc["want"].view(torch.uint8), mc["values"].view(torch.uint8))
    uc.run_commit(mc, svops.ops(), "cpu", str(cc))


# every branch of updates.hip the matrix must keep reaching (names: update_cases.kernel_paths)
_LANES = (1, 2, 4, 8, 16, 32, 64)
REQUIRED = (
    {"general/L%d/validate-scalar" % L for L in _LANES} | {"general/L%d/validate-finite" % L for L in _LANES}
    | {"general/L%d/validate-vec" % L for L in _LANES}
    | {"general/L%d/copy16%s" % (L, s) for L in _LANES for s in ("", "-save")}
    | {"general/L1/copy4", "general/L1/copy4-save", "general/L1/copy1", "general/L1/copy1-save",
       "general/L8/copy1", "general/L8/copy4", "general/L8/copy1-save", "general/L8/copy4-save",
       "general/L32/copy4", "general/L32/copy4-save"}
    | {"unique/L%d/RB8/register%s" % (L, s) for L in _LANES for s in ("", "-save")}
    | {"unique/L64/RB16/register", "unique/L64/RB16/register-save"}
    | {"unique/L1/short-row-w%d%s" % (w, s) for w in (3, 4) for s in ("", "-save")}
    | {"unique/L64/RB16/loop/validate-vec", "unique/L64/RB16/loop/validate-scalar",
       "unique/L64/RB16/loop/copy16", "unique/L64/RB16/loop/copy16-save"}
    | {"unique/L1/RB8/loop/validate-scalar", "unique/L1/RB8/loop/validate-none",
       "unique/L1/RB8/loop/copy1", "unique/L1/RB8/loop/copy4", "unique/L1/RB8/loop/copy16",
       "unique/L1/RB8/loop/copy1-save", "unique/L1/RB8/loop/copy4-save", "unique/L1/RB8/loop/copy16-save",
       "unique/L8/RB8/loop/copy1", "unique/L8/RB8/loop/copy4", "unique/L8/RB8/loop/copy1-save",
       "unique/L8/RB8/loop/copy4-save", "unique/L32/RB8/loop/copy4", "unique/L32/RB8/loop/copy4-save",
       "unique/L16/RB8/loop/copy16", "unique/L2/RB8/loop/copy4"}
    | {"restore/copy16", "restore/copy1", "restore/second-iteration"}
    | {"commit/L4/RB8/register", "commit/L4/RB8/bytes", "commit/L16/RB8/register", "commit/L16/RB8/bytes",
       "commit/L64/RB8/register", "commit/L64/RB8/bytes", "commit/L64/RB16/register", "commit/L64/RB16/bytes"})


def test_matrix_reaches_every_branch():
    seen = set()
    for case in CASES + (uc.restore_grid_case(),):
        m = uc.make(case)
        seen |= uc.kernel_paths(m)
        if case.save:
            seen |= uc.restore_paths(m)
    seen |= {uc.commit_path(cc) for cc in uc.COMMIT_CASES}
    assert not REQUIRED - seen, sorted(REQUIRED - seen)
