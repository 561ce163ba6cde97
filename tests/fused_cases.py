"""Sequential fp64 model of the fused fp32 transactional round, and its cases (CPU only).

A fused step (FastParams.upd_rows, csrc/include/svoc/launch.hpp) is one transaction per instance over
the fp32 state [N, D] and a batch (oracle [U], rows [U, D]).  model_step is written from the contract's
order of operations and shares no code with the kernels or with svoc.engine:

  1. a row with any value outside [0, 1] (NaN and +-inf included, -0.0 not) gets INTERVAL_INPUT,
     whatever its oracle;
  2. otherwise an oracle outside [0, N) gets NOT_ORACLE;
  3. otherwise the row is tentatively stored;
  4. the round runs in fp64 on the resulting table (fast_cases.ref64, constrained);
  5. a reliable column constant by value (-0.0 == +0.0) reverts the round with ZERO_VARIANCE: every
     tentatively stored update gets that code, state and outputs stay as before the step;
  6. otherwise the rows are committed and the outputs are the round's.

So an invalid row reverts alone and the round is computed on the state row in its place.  model_deferred
adds what launch.hpp documents for FastParams.pend_rows: the lagging ``values`` after every launch (the
accepted rows of the batch before, except those replaced by an accepted row of this batch) and the exact
state after the final commit.  Row validity and the commit are update_cases' models.

build() makes one case: f planted far oracles per instance (rows alternating 0 / 1 by column, kept far
by every batch), all other rows Beta(20, 20), so the rank cut is wide (cut_gap >= MIN_CUT_GAP, asserted
by test_fused_model.py for every case, step and instance) and ``reliable`` compares exactly.  The
instances of a case play the roles ROLES (see _batch); with B = 2 only INVALID and ZV_SEQUENCE.
Nothing here imports GPU code.
"""
import collections
import functools

import torch

import fast_cases
import update_cases
from helpers import beta_oracles
from update_cases import INTERVAL_INPUT, NOT_ORACLE, OK, ZERO_VARIANCE

STEPS = 3
MIN_CUT_GAP = 2e-3          # 100 x the fp32 qr rtol of fast_cases.TOL
ZCOL, ZVAL = 3, 0.625       # the constant column of the zero-variance roles; its value in ZV_SEQUENCE
OUTSIDE_IDS = lambda N: [-1, N, N + 5, 1 << 40]

Shape = collections.namedtuple("Shape", "N D f U nseg h wide")
# the smallest shapes reaching each instantiation (lane groups NSEG x window half-width H, WIDE: the 9-bit
# piece map at U = 256) and each geometry edge of the DMA piece map
SHAPES = [
    Shape(7, 6, 2, 3, 1, 5, False),          # N < 64, D < two 16-byte pieces, D % 4 != 0
    Shape(63, 40, 6, 10, 1, 5, False),       # padded N, D < one slab
    Shape(64, 260, 8, 40, 1, 5, False),      # full slab + 4-column tail, U > 32
    Shape(64, 64, 20, 16, 1, 17, False),
    Shape(65, 128, 8, 33, 2, 5, False),      # masked form
    Shape(128, 132, 8, 64, 2, 5, False),     # full slab + tail
    Shape(128, 130, 24, 20, 2, 17, False),   # D % 4 != 0: fused but never deferred
    Shape(100, 36, 24, 12, 2, 17, False),    # ... so the deferred (2, 17) form runs here (padded N)
    Shape(129, 68, 8, 16, 4, 5, False),
    Shape(200, 100, 20, 50, 4, 17, False),   # padded N
    Shape(256, 68, 8, 127, 4, 5, False),     # U = kDeferMaxU
    Shape(256, 64, 32, 128, 4, 17, False),   # pruned network (interval extremes from the sorted keys); no deferral
    Shape(256, 72, 32, 256, 4, 17, True),
    Shape(256, 68, 8, 256, 4, 5, True),
    Shape(64, 4100, 8, 8, 1, 5, False),      # D > 4096: pass 2 without LDS staging
]
DEFER_MAX_U = 127


def shape_id(s):
    return "%dx%dx%d-U%d" % (s.N, s.D, s.f, s.U)


def batch_of(s):
    return 2 if s.D > 4096 else 6


def deferred(s):
    """The shapes the deferred commit takes: 16-byte write-back (D % 4 == 0), 7-bit pending slots."""
    return s.D % 4 == 0 and s.U <= DEFER_MAX_U


VALID, INVALID, THREE_INVALID, ZV_AFTER_DROP, ZV_SEQUENCE, NO_ORACLE = range(6)
ROLES = {6: [VALID, INVALID, THREE_INVALID, ZV_AFTER_DROP, ZV_SEQUENCE, NO_ORACLE], 2: [INVALID, ZV_SEQUENCE]}
BAD_KINDS = ["next1", "nan", "inf", "ntiny"]


def bad_value(kind):
    """The invalid element values: 1 + 1 ulp, NaN, +inf, the negative number nearest zero."""
    bits = {"next1": 0x3F800001, "nan": 0x7FC00000, "inf": 0x7F800000, "ntiny": -0x7FFFFFFF}[kind]   # 0x80000001
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32)[0]


# ----------------------------------------------------------------------------------------- the model

def model_step(values, oracle, rows, f):
    """One fused step.  values [B, N, D] fp32: the exact state before it; oracle [B, U] int64; rows
    [B, U, D] fp32.  Returns dict(values: the state after it, table: the tentative table the round ran on,
    ref: ref64 of the table (meaningful where status is OK), status [B], upd_status [B, U])."""
    B, N, D = values.shape
    U = oracle.shape[1]
    flat_rows, flat_orc = rows.reshape(B * U, D), oracle.reshape(-1)
    valid = update_cases._rows_valid(flat_rows, "fp32", True).tolist()
    st = torch.empty(B * U, dtype=torch.int32)
    for u, o in enumerate(flat_orc.tolist()):
        st[u] = INTERVAL_INPUT if not valid[u] else NOT_ORACLE if not 0 <= o < N else OK
    table = update_cases.model_commit(values, flat_rows, flat_orc, st, U)
    ref = fast_cases.ref64(table, f, True, 1.0)
    status = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        assert 0.0 <= float(ref["rel"][b].min()) and float(ref["rel"][b].max()) <= 1.0 and N - f >= 4
        rel = table[b][ref["reliable"][b]].double()
        if bool((rel == rel[0]).all(0).any()):
            status[b] = ZERO_VARIANCE
            sl = st[b * U:(b + 1) * U]
            sl[sl == OK] = ZERO_VARIANCE
    after = update_cases.model_commit(values, flat_rows, flat_orc, st, U)
    return dict(values=after, table=table, ref=ref, status=status, upd_status=st.view(B, U))


def model_sequence(values, batches, f):
    """model_step over ``batches`` [(oracle, rows)], each on the state the one before left."""
    out = []
    for oracle, rows in batches:
        out.append(model_step(values, oracle, rows, f))
        values = out[-1]["values"]
    return out


def model_deferred(values, batches, steps):
    """The lagging ``values`` after every launch of a deferred sequence (launch s gets batch s - 1 as its
    pending batch, the first launch none): the state holds every accepted row of the pending batch except
    those replaced by an accepted row of this batch.  ``steps``: model_sequence's answer."""
    lag, out, pend = values.clone(), [], None
    for (oracle, rows), step in zip(batches, steps):
        B, U = oracle.shape
        if pend is not None:
            p_orc, p_rows, p_st = pend
            for b in range(B):
                again = {o for o, s in zip(oracle[b].tolist(), step["upd_status"][b].tolist()) if s == OK}
                for u, (o, s) in enumerate(zip(p_orc[b].tolist(), p_st[b].tolist())):
                    if s == OK and o not in again:
                        lag[b, o] = p_rows[b, u]
        out.append(lag.clone())
        pend = (oracle, rows, step["upd_status"])
    return out


# ------------------------------------------------------------------------------------- case builder

def _batch(s, ci, role, step, order, far_row, g):
    """Oracles [U] and rows [U, D] of one instance's batch at ``step``.  ``order``: the instance's
    oracles 0 .. N - 2, the far ones last; slot i < U - 1 takes order[(step * h + i) % (N - 1)] (so
    consecutive batches share some oracles and not others), slot U - 1 oracle N - 1.  Roles:
      VALID          every row valid: a -0.0 in slot 0, and slot U - 1 (the end of the instance's batch)
                     with a distinctive value in column D - 1;
      INVALID        the same, and one invalid value in column D - 1: slot U - 2 at step 0, then slot
                     U - 1 (an oracle accepted the step before);
      THREE_INVALID  invalid values in slots 0, U // 2, U - 1 (columns 0, D // 2, D - 1); the first two
                     name oracles of one 64-row segment; a -0.0 elsewhere;
      ZV_AFTER_DROP  step 0: column ZCOL of state and batch constant by value (+0.0 and -0.0 mixed) but for
                     slot 1, which is invalid too: dropped, the round runs on the state row and reverts;
      ZV_SEQUENCE    step 0 breaks the constant column in half of its rows (accepted), step 1 names the
                     same oracles with the constant back: a plain zero-variance revert while rows pend;
      NO_ORACLE      oracle ids -1, N, N + 5, 2^40 rotating over slots and steps, one with a NaN row."""
    N, D, U = s.N, s.D, s.U
    M, h = N - 1, max(1, (U - 1) // 2)
    rot = 0 if (role == ZV_SEQUENCE and step == 1) else step
    orc = [order[(rot * h + i) % M] for i in range(U - 1)] + [N - 1]
    if role == THREE_INVALID and orc[0] // 64 != orc[U // 2] // 64:
        j = next(j for j in range(1, U - 1) if j != U // 2 and orc[j] // 64 == orc[0] // 64)
        orc[j], orc[U // 2] = orc[U // 2], orc[j]
    rows, _ = beta_oracles(1, U, D, 0, seed=int(torch.randint(1 << 30, (1,), generator=g)), dtype=torch.float32)
    rows = rows[0, :, :D].clone()
    for u, o in enumerate(orc):
        if o in far_row:
            rows[u] = far_row[o]
    kind = lambda k: bad_value(BAD_KINDS[(ci + step + k) % 4])
    if role in (VALID, INVALID):
        rows[0, 0] = -0.0
        rows[U - 1, D - 1] = (0.875, 0.8125, 0.90625)[step]
    if role == INVALID:
        rows[U - 2 if step == 0 else U - 1, D - 1] = kind(0)
    if role == THREE_INVALID:
        for k, (u, col) in enumerate(((0, 0), (U // 2, D // 2), (U - 1, D - 1))):
            rows[u, col] = kind(k)
        if U > 3:
            rows[1, 1] = -0.0
    if role == ZV_AFTER_DROP and step == 0:
        rows[:, ZCOL] = 0.0
        rows[::2, ZCOL] = -0.0
        rows[1, ZCOL] = 0.3
        rows[1, D - 1] = kind(0)
    if role == ZV_SEQUENCE and step < 2:
        rows[(max(1, U // 2) if step == 0 else 0):, ZCOL] = ZVAL
    if role == NO_ORACLE:
        slots = [1, 3, 5, 7] if U >= 9 else list(range(min(4, U - 1)))
        for k, u in enumerate(slots):
            orc[u] = OUTSIDE_IDS(N)[(k + len(slots) * step) % 4]
        rows[slots[step % len(slots)], D // 2] = float("nan")
    return torch.tensor(orc, dtype=torch.int64), rows


@functools.lru_cache(maxsize=None)
def build(s):
    """Case ``s``: the initial state x0 [B, N, D] fp32, the far mask [B, N], STEPS batches [(oracle [B, U],
    rows [B, U, D])], the roles, and the model's answers: ``steps`` (model_sequence) and ``lag``
    (model_deferred, where the shape is deferred).  Built once, shared, never modified."""
    N, D, f, U = s.N, s.D, s.f, s.U
    B, ci = batch_of(s), SHAPES.index(s)
    roles = ROLES[B]
    g = torch.Generator().manual_seed(1000 * N + 10 * D + U)
    x0, _ = beta_oracles(B, N, D, 0, seed=N + D + U, dtype=torch.float32)
    x0 = x0[:, :, :D].clone()
    alt = (torch.arange(D) % 2).float()
    far = torch.zeros(B, N, dtype=torch.bool)
    orders, far_rows = [], []
    for b in range(B):
        p = torch.randperm(N - 1, generator=g).tolist()             # oracle N - 1 is never far
        fr, near = p[:f], p[f:]
        far[b, fr] = True
        far_rows.append({o: (alt if j % 2 == 0 else 1.0 - alt) for j, o in enumerate(fr)})
        for o, r in far_rows[b].items():
            x0[b, o] = r
        if roles[b] == ZV_SEQUENCE:
            x0[b, :, ZCOL] = ZVAL
        if roles[b] == ZV_AFTER_DROP:        # constant by value only: +0.0 and -0.0
            x0[b, :, ZCOL] = 0.0
            x0[b, 1::2, ZCOL] = -0.0
            far_rows[b] = {o: torch.cat([r[:ZCOL], torch.tensor([0.0]), r[ZCOL + 1:]]) for o, r in far_rows[b].items()}
        orders.append(near + fr)
    batches = []
    for step in range(STEPS):
        per = [_batch(s, ci, roles[b], step, orders[b], far_rows[b], g) for b in range(B)]
        batches.append((torch.stack([o for o, _ in per]), torch.stack([r for _, r in per])))
    steps = model_sequence(x0, batches, f)
    lag = model_deferred(x0, batches, steps) if deferred(s) else None
    return dict(shape=s, B=B, roles=roles, x0=x0, far=far, batches=batches, steps=steps, lag=lag)


def role_inst(c, role):
    return c["roles"].index(role)


def round_case(c, step, idx):
    """The fast_cases.check_round case of instances ``idx`` (OK ones) at ``step``."""
    s, m = c["shape"], c["steps"][step]
    return dict(ref={k: v[idx] for k, v in m["ref"].items()}, x=m["table"][idx], N=s.N, D=s.D, f=s.f,
                expect=~c["far"][idx], constrained=True, structured=False, storage="fp32", scale=1.0)


def first_diff(a, b):
    """"[instance, position ...]" of the first differing element of two equal-shaped tensors."""
    bad = (a != b).nonzero()
    return "first of %d at %s" % (bad.shape[0], bad[0].tolist()) if bad.numel() else "none"


def same(got, want, tag, what):
    """got == want element for element, or an error naming what differs and where (``what`` says what the
    index means, e.g. "upd_status [instance, slot]"); float tensors are compared on their bits."""
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == torch.float32:
        got, want = bits(got), bits(want)
    if not torch.equal(got, want):
        sel = got != want
        raise AssertionError("%s: %s differs, %s: got %s, expected %s" % (
            tag, what, first_diff(got, want), got[sel][:6].tolist(), want[sel][:6].tolist()))


def bits(t):
    return t.contiguous().view(torch.int32)
