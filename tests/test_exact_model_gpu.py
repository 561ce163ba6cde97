"""Every route of the exact-round kernels against the Python golden model (the cases of exact_cases.py): the i128
kernel alone (consensus_exact.hip), the dispatcher (column or wide-column kernel, the i128 kernel for what they hand
off), the column kernel alone (consensus_wsad.hip) and the verdict form -- each compared with the model, bit for bit
over outputs prefilled with a pattern, and never with another run.  The routing counters must equal what the case
module derives from the kernels' header contracts and the value ranges, so that a hand-off cannot hide a failure:
an instance the column kernels' domain covers must not reach the i128 kernel."""
import pytest
import torch

import exact_cases as xc
from wsadx_cases import DEV, OUTS, PATTERN, _run

pytestmark = pytest.mark.gpu
I128 = {"SVOC_EXACT_I128": "1"}
DISPATCH = {"SVOC_EXACT_WSAD_MIN_D": "1"}
COLUMN = {"SVOC_EXACT_WSAD_ONLY": "1", "SVOC_EXACT_WSAD_MIN_D": "1"}


def _launch(m, env=None, **kw):
    return _run(m["values"].to(DEV), m["f"], env, ms=m["ms"], prefill=True, constrained=m["constrained"],
                legacy=m["legacy"], **kw)


@pytest.mark.parametrize("case", xc.matrix(("int64",)), ids=xc.case_id)
def test_every_route_matches_model(case):
    m = xc.make(case)
    exp, B = m["exp"], m["values"].shape[0]
    column = [b for b in range(B) if m["column"][b]]
    bad = []      # (route, what): every disagreement of the case, reported together
    # 1. the i128 kernel alone
    out = _launch(m, I128)
    bad += [("i128", x) for x in xc.compare(out, exp)]
    if out["stats"] != [0, 0]:
        bad.append(("i128 stats", out["stats"]))
    # 2. the dispatcher
    out = _launch(m, DISPATCH)
    bad += [("dispatcher", x) for x in xc.compare(out, exp)]
    if out["stats"] != m["stats"]:
        bad.append(("dispatcher stats", out["stats"], "expected", m["stats"]))
    # 3. the column kernel alone: what it hands off stays at the pattern, status included
    out = _launch(m, COLUMN)
    took = [b for b in range(B) if int(out["status"][b]) != PATTERN["status"]]
    bad += [("column", x) for x in xc.compare(out, exp, took)]
    bad += [("column wrote a handed-off instance", k, b) for b in set(range(B)) - set(took) for k in OUTS
            if not (out[k][b] == PATTERN[k]).all()]
    if took != column:
        bad.append(("column kernel took", took, "expected", column))
    # 4. the verdict
    out = _launch(m, DISPATCH, verdict=True)
    bad += [("verdict", x) for x in xc.compare(out, exp, keys=("status", "rel"))]
    bad += [("verdict wrote", k) for k in ("c1", "consensus", "skew", "kurt", "qr", "reliable")
            if not (out[k] == PATTERN[k]).all()]
    verdict_form = m["constrained"] and not m["legacy"] and 4 <= case.N <= 256
    want = [len(column), B - len(column), 0] if verdict_form else [0, B, 0]
    if out["vstats"] != want:
        bad.append(("vstats", out["vstats"], "expected", want))
    assert not bad, bad


@pytest.mark.parametrize("case", xc.matrix(("int32",)), ids=xc.case_id)
def test_int32_storage_matches_model(case):
    m = xc.make(case)
    assert m["values"].dtype == torch.int32
    out = _launch(m, DISPATCH)
    assert not xc.compare(out, m["exp"])
    assert out["stats"] == m["stats"]


@pytest.mark.parametrize("case,cut", xc.SHARDED, ids=lambda p: xc.case_id(p) if isinstance(p, xc.Case) else str(p))
def test_d_sharded_round_matches_model(case, cut):
    xc.sharded_round(xc.make(case), cut, lambda m, **kw: _launch(m, DISPATCH, **kw))
