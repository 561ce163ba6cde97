"""The native CPU exact engine (csrc/engine/reference_cpu.cpp, svoc/wsad.hpp) against the Python golden model on
the cases of exact_cases.py: every route shape of the exact kernels (N up to 4096), unconstrained value ranges up
to and past int64, ties at the rank cut, duplicates, reliable outliers and every revert code, bit for bit on the
status and the eight outputs, over outputs prefilled with a pattern (a revert must leave them untouched).  The
expected values come from svoc.reference alone."""
import pytest
import torch

import exact_cases as xc
from svoc import ops as svops
from wsadx_cases import _run

pytestmark = pytest.mark.skipif(not svops.available(), reason="svoc/_C.so not built")


def _launch(m, **kw):
    return _run(m["values"], m["f"], ms=m["ms"], prefill=True, constrained=m["constrained"], legacy=m["legacy"], **kw)


def test_matrix_reaches_its_routes():
    xc.check_routes()
    codes = {int(s) for c in xc.matrix(("int64",)) for s in xc.make(c)["exp"]["status"]}
    # OK, DIV_BY_ZERO, INDEX_OOB, RELIABILITY_INTERVAL, OVERFLOW, USIZE_UNDERFLOW
    assert codes == {0, 4, 5, 6, 7, 8}, codes


@pytest.mark.parametrize("case", xc.matrix(("int64",)), ids=xc.case_id)
def test_case_is_what_its_builder_intended(case):
    xc.check_case(case)


@pytest.mark.parametrize("case", xc.matrix(), ids=xc.case_id)
def test_exact_round_matches_model(case):
    m = xc.make(case)
    assert not xc.compare(_launch(m), m["exp"])


@pytest.mark.parametrize("case", xc.matrix(), ids=xc.case_id)
def test_exact_verdict_matches_model(case):
    m = xc.make(case)
    out = _launch(m, verdict=True)
    assert not xc.compare(out, m["exp"], keys=("status", "rel"))


@pytest.mark.parametrize("case,cut", xc.SHARDED, ids=lambda p: xc.case_id(p) if isinstance(p, xc.Case) else str(p))
def test_d_sharded_round_matches_model(case, cut):
    assert case in xc.matrix()
    xc.sharded_round(xc.make(case), cut, _launch)
