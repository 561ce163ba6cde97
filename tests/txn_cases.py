"""Sequential model of the saved-batch transactional fast round, and its cases (CPU only).

A fast-mode update batch is one transaction per instance: apply_updates(..., saved, saved_en) stores the rows
and saves what they overwrote, the round runs on the instances the batch left fully active, and where it
reverts the rows, ``enabled`` and ``n_active`` go back and every applied update reports the round's code.
model_txn composes models the suite already trusts and shares no code with the kernels or with svoc.engine:

  1. update_cases.model_apply on the instance-grouped batch (U updates per instance);
  2. active[b] = (n_active[b] == N) after the batch;
  3. fast_cases.ref64 on the resulting table, and verdict(): the contract's order of checks
     (svoc/reference.py consensus_round, docs/PARITY.md C12): rel1 outside [0, 1], then rel2 outside [0, 1]
     -> RELIABILITY_INTERVAL; then (not legacy) fewer than 4 reliable oracles -> TOO_FEW_RELIABLE; then (not
     legacy) a reliable column constant by value (-0.0 == +0.0) -> ZERO_VARIANCE;
  4. update_cases.model_restore with inactive_status = -1.

build() makes one case of 8 instances, one role each (roles_of).  f far oracles are planted per instance so that
the rank cut is wide and ``reliable`` compares exactly; conditions() asserts for every instance what the
comparison with a kernel relies on (cut gap, distance of rel1 / rel2 from the interval's ends, variance of the
non-constant reliable columns).  Legacy rounds cannot revert with ZERO_VARIANCE, so their reverting roles
carry a RELIABILITY_INTERVAL fault instead (far rows at full amplitude: the legacy reliability has no / D).
An unconstrained legacy round cannot revert on any valid data (its reliability lies in [0, 1] by
construction and it has no moments): there the model's verdict is OK for every role, constant columns
included, and the case pins that nothing is rolled back.

Run lays a case out on a device, every buffer carved out of canaries (update_cases.Buf); check() holds the
assertions test_txn_model.py (CPU ops) and test_txn_model_gpu.py (HIP kernels) share.  Nothing here imports
GPU code.
"""
import collections
import functools
import math

import torch

import fast_cases
import update_cases
from update_cases import Buf, DT, NOT_SAVED, OK, RELIABILITY_INTERVAL, ZERO_VARIANCE

TOO_FEW_RELIABLE = 33
SCALE, SHIFT = 4.0, -1.5          # unconstrained data: the [0, 1] layout mapped to x * SCALE + SHIFT
SENTINEL, STATUS_PREFILL, UPD_PREFILL = 3, -5, -7
B = 8
SMALL, WINDOW, TWO_NET = 0, 1, 2  # svoc.ops.KERNEL_*

# kernel / nseg / h / rollback: the route the case claims (svoc.ops.fast_route: kernel, lane_groups, win_h,
# rollback), asserted by the GPU test before it runs
Case = collections.namedtuple("Case", "storage N D f constrained legacy hint kernel nseg h rollback dup")


def _c(storage, N, D, f, kernel, nseg, h, rollback, constrained=True, legacy=False, hint=0, dup=False):
    return Case(storage, N, D, f, constrained, legacy, hint, kernel, nseg, h, rollback, dup)


CASES = [
    # bf16, in-kernel roll-back, constrained: lane groups x window half-width, 8 waves, whole-case TOO_FEW_RELIABLE
    _c("bf16", 17, 40, 2, WINDOW, 1, 5, 1),
    _c("bf16", 64, 33, 20, WINDOW, 1, 17, 1),
    _c("bf16", 65, 96, 8, WINDOW, 2, 5, 1),
    _c("bf16", 65, 96, 8, WINDOW, 2, 5, 1, dup=True),
    _c("bf16", 128, 64, 24, WINDOW, 2, 17, 1),
    _c("bf16", 129, 33, 3, WINDOW, 4, 5, 1),
    _c("bf16", 256, 72, 32, WINDOW, 4, 17, 1),
    _c("bf16", 200, 520, 20, WINDOW, 4, 17, 1),
    _c("bf16", 34, 40, 31, WINDOW, 1, 17, 1),
    # ... unconstrained (win_h: what the route states for (N, f); the kernel keeps the H = 5 layout)
    _c("bf16", 63, 7, 1, WINDOW, 1, 5, 1, constrained=False),
    _c("bf16", 100, 24, 10, WINDOW, 2, 17, 1, constrained=False),
    _c("bf16", 255, 40, 31, WINDOW, 4, 17, 1, constrained=False),
    # ... legacy
    _c("bf16", 64, 33, 8, WINDOW, 1, 5, 1, legacy=True),
    _c("bf16", 65, 24, 8, WINDOW, 2, 5, 1, constrained=False, legacy=True),
    # bf16, restore after the round: the small kernel ...
    _c("bf16", 7, 6, 2, SMALL, 0, 5, 0),
    _c("bf16", 16, 128, 3, SMALL, 0, 5, 0),
    _c("bf16", 8, 6, 5, SMALL, 0, 5, 0),                       # whole-case TOO_FEW_RELIABLE (N <= 16: small kernel)
    # ... and the two-network kernel
    _c("bf16", 100, 24, 40, TWO_NET, 2, 0, 0),
    _c("bf16", 100, 24, 40, TWO_NET, 2, 0, 0, dup=True),
    _c("bf16", 300, 24, 30, TWO_NET, 8, 0, 0),
    _c("bf16", 64, 33, 8, TWO_NET, 1, 5, 0, hint=-7),
    _c("bf16", 8, 6, 5, TWO_NET, 1, 5, 0, hint=-7),            # whole-case TOO_FEW_RELIABLE
    # fp32, restore after the round: window kernel (256 x 64 x 32: the pruned network), two-network, unconstrained
    _c("fp32", 64, 33, 8, WINDOW, 1, 5, 0),
    _c("fp32", 129, 33, 3, WINDOW, 4, 5, 0),
    _c("fp32", 256, 64, 32, WINDOW, 4, 17, 0),
    _c("fp32", 300, 16, 30, TWO_NET, 8, 0, 0),
    _c("fp32", 100, 24, 40, TWO_NET, 2, 0, 0),
    _c("fp32", 63, 7, 1, WINDOW, 1, 5, 0, constrained=False),
]


def case_id(c):
    s = "%s-%dx%dx%d-%s" % (c.storage, c.N, c.D, c.f, "con" if c.constrained else "unc")
    return s + ("-legacy" if c.legacy else "") + ("-hint%d" % c.hint if c.hint else "") + ("-dup" if c.dup else "")


def updates_per_instance(N):
    """Between 5 and min(N, 40); at least 6 so that the rejected roles keep a valid update."""
    return min(40, max(6, N // 2))


def ld_of(D):
    return (D + 7) // 8 * 8


def max_spread(c):
    return 1.0 if c.constrained else SCALE * math.sqrt(c.D)


VALID, ZV, REL_AND_ZV, ZV2, ACTIVATE_REVERT, ACTIVATE_OK, INACTIVE, REJECTED_REVERT, REJECTED_OK = range(9)
ROLE_NAMES = ["VALID", "ZV", "REL_AND_ZV", "ZV2", "ACTIVATE_REVERT", "ACTIVATE_OK", "INACTIVE", "REJECTED_REVERT",
              "REJECTED_OK"]
REVERT_ROLES = (ZV, REL_AND_ZV, ZV2, ACTIVATE_REVERT, REJECTED_REVERT)


def roles_of(c):
    """One role per instance.  Unconstrained: a second ZV at another column in place of REL_AND_ZV (no data
    gives an unconstrained reliability fault)."""
    return [VALID, ZV, REL_AND_ZV if c.constrained else ZV2, ACTIVATE_REVERT, ACTIVATE_OK, INACTIVE, REJECTED_REVERT,
            REJECTED_OK]


def const_col(role, D):
    """The constant column (+0.0 and -0.0 mixed) of the zero-variance roles."""
    return {ZV: 3, REL_AND_ZV: 3, ZV2: D - 2, ACTIVATE_REVERT: D - 1, REJECTED_REVERT: 0}.get(role)


def outside_ids(N):
    return [-1, N, N + 5, 1 << 40]


def bad_values(c):
    """Element values apply_updates rejects: out of [0, 1] (constrained) or non-finite (unconstrained)."""
    return [1.5, -0.25, float("nan"), 2.0] if c.constrained else [float("nan"), float("inf"), float("-inf"), float("nan")]


# ----------------------------------------------------------------------------------------- the model

def verdict(table, ref, f, legacy):
    """The round's code for one instance from the contract's order of checks.  table [N, D]: what the round
    ran on; ref: ref64's answer for it (rel [2], reliable [N])."""
    for r in ref["rel"].tolist():                     # rel1, then rel2 (NaN fails both comparisons)
        if not (0.0 <= r <= 1.0):
            return RELIABILITY_INTERVAL
    if legacy:
        return OK
    if table.shape[0] - f < 4:
        return TOO_FEW_RELIABLE
    rows = table[ref["reliable"]].double()
    if bool((rows == rows[0]).all(0).any()):          # by value: -0.0 == +0.0
        return ZERO_VARIANCE
    return OK


def model_txn(state, oracle, rows, c):
    """One saved-batch transaction per instance.  state: update_cases.model_apply's state dict (values
    [B, N, ld]); oracle [B * U] int64, rows [B * U, D], instance-grouped.  Returns dict(post: the state after
    the batch, active [B], table [B, N, D], ref (ref64 of the table), status [B] (STATUS_PREFILL where no round
    ran), final: model_restore's answer)."""
    nB, N, _ = state["values"].shape
    U = oracle.numel() // nB
    inst = torch.arange(nB).repeat_interleave(U)
    post = update_cases.model_apply(state, inst, oracle, rows, c.constrained)
    active = post["n_active"] == N
    table = post["values"][:, :, :c.D].clone()
    ref = fast_cases.ref64(table, c.f, c.constrained, max_spread(c), legacy=c.legacy)
    status = torch.full((nB,), STATUS_PREFILL, dtype=torch.int32)
    for b in range(nB):
        if active[b]:
            status[b] = verdict(table[b], {k: v[b] for k, v in ref.items()}, c.f, c.legacy)
    final = update_cases.model_restore(state, post, inst, oracle, c.D, status, active, -1)
    return dict(post=post, active=active, table=table, ref=ref, status=status, final=final, inst=inst)


# ------------------------------------------------------------------------------------- case builder

def _beta(D, g, a=20.0):
    ga = torch._standard_gamma(torch.full((D,), a), generator=g)
    gb = torch._standard_gamma(torch.full((D,), a), generator=g)
    return (ga / (ga + gb)).double()


class _Layout:
    """The row classes of one instance's N oracles; row(o, g) draws a fresh row of oracle o's class in [0, 1]
    (far and level rows are deterministic, so every batch keeps them where they are).

    standard: f far rows at 0.5 +- amp alternating by column, the others 0.5 + hs * (Beta(20, 20) - 0.5).
    skewed (a constrained reliability fault, rel1 < 0: the median at one end): more than half of the rows low
    (uniform in [0, 0.04]), nh high ones of which the f far at 1.0 and the others at 0.9 -- mean qr / D is about
    0.96 nh / N > 0.2756 while the cut falls between the two high levels (or between low and high where
    nh == f).  Where f > (N - 1) / 2 (R = 3): three tight rows 0.03 +- 0.004 hold the median, N / 2 - 2 rows at
    0.0 below them, the rest at 1.0."""

    def __init__(self, c, skewed, amp, hs, g):
        N, f = c.N, c.f
        self.D, self.amp, self.hs = c.D, amp, hs
        p = torch.randperm(N, generator=g).tolist()
        self.far = torch.zeros(N, dtype=torch.bool)
        self.cls = [None] * N
        if not skewed:
            for j, o in enumerate(p[:f]):
                self.cls[o] = ("far", j % 2)
            for o in p[f:]:
                self.cls[o] = ("honest",)
            self.far[p[:f]] = True
            return
        half = (N - 1) // 2
        if f <= half:
            nh = min(max(math.ceil(0.44 * N), f), half)
            for j, o in enumerate(p[:nh]):
                self.cls[o] = ("level", 1.0 if j < f else 0.9)
            for o in p[nh:]:
                self.cls[o] = ("low",)
            self.far[p[:f]] = True
        else:
            R, m = N - f, N // 2
            assert R == 3, (N, f)
            k0, nh = m - 2, half
            assert k0 + R + nh == N, (N, f)
            for o in p[:nh]:
                self.cls[o] = ("level", 1.0)
            for o in p[nh:nh + k0]:
                self.cls[o] = ("level", 0.0)
            for j, o in enumerate(p[nh + k0:]):
                self.cls[o] = ("tight", j)
            self.far[p[:nh + k0]] = True

    def row(self, o, g):
        k, D = self.cls[o], self.D
        col = torch.arange(D)
        if k[0] == "honest":
            return 0.5 + self.hs * (_beta(D, g) - 0.5)
        if k[0] == "far":
            return 0.5 + self.amp * (1.0 - 2.0 * ((col + k[1]) % 2).double())
        if k[0] == "low":
            return 0.04 * torch.rand(D, generator=g).double()
        if k[0] == "level":
            return torch.full((D,), k[1], dtype=torch.float64)
        return 0.03 + 0.004 * (k[1] - 1) * (1.0 - 2.0 * (col % 2).double())


def _finish(c, x, zc, neg):
    """A [0, 1] row in the case's units and storage type; column zc constant: -0.0 where ``neg`` else +0.0."""
    if not c.constrained:
        x = x * SCALE + SHIFT
    x = x.to(DT[c.storage][0])
    if zc is not None:
        x[zc] = -0.0 if neg else 0.0
    return x


def _pad_pattern(n, storage):
    """Finite, position-dependent values outside [0, 1] for the pad columns: 2.0 + (i mod 64) ulps."""
    dtype, idt, _ = DT[storage]
    base = 0x4000 if storage == "bf16" else 0x40000000
    return (base + torch.arange(n) % 64).to(idt).view(dtype)


@functools.lru_cache(maxsize=None)
def build(c):
    """Case c: the pre-batch state, the batch, the roles and the model's answer (CPU tensors; built once,
    shared, never modified)."""
    N, D, f = c.N, c.D, c.f
    U, ld = updates_per_instance(N), ld_of(D)
    dtype = DT[c.storage][0]
    roles = roles_of(c)
    g = torch.Generator().manual_seed(7919 * N + 31 * D + f + 1000003 * CASES.index(c))
    values = torch.zeros(B, N, ld, dtype=dtype)
    if ld > D:
        values[:, :, D:] = _pad_pattern(B * N * (ld - D), c.storage).view(B, N, ld - D)
    enabled = torch.ones(B, N, dtype=torch.uint8)
    far = torch.zeros(B, N, dtype=torch.bool)
    oracle = torch.empty(B, U, dtype=torch.int64)
    rows = torch.empty(B, U, D, dtype=dtype)
    bad, k_dis = bad_values(c), 2 if N < 17 else 3
    disabled = {}
    for b, role in enumerate(roles):
        rel_fault = c.legacy and c.constrained and role in REVERT_ROLES
        skewed = role == REL_AND_ZV and not c.legacy
        amp, hs = (0.2, 0.25) if c.legacy and c.constrained and not rel_fault else (0.5, 1.0)
        lay = _Layout(c, skewed, amp, hs, g)
        far[b] = lay.far
        zc = const_col(role, D)
        for o in range(N):
            values[b, o, :D] = _finish(c, lay.row(o, g), zc, o % 2 == 1)
        perm = torch.randperm(N, generator=g).tolist()
        must = []
        if role in (ACTIVATE_REVERT, ACTIVATE_OK, INACTIVE):
            dis = perm[:k_dis]
            disabled[b] = dis
            enabled[b, dis] = 0
            for o in dis:                                     # what a reverted activation must bring back
                values[b, o, :D] = _finish(c, torch.full((D,), 0.75, dtype=torch.float64), None, False)
            must = dis if role != INACTIVE else dis[:-1]      # INACTIVE: one slot stays disabled
        orc = [o for o in perm if o not in disabled.get(b, ())][:U - len(must)]
        for i, o in enumerate(must):
            orc.insert(1 + 2 * i, o)
        assert len(orc) == U, (case_id(c), b)
        if c.dup and role == ZV:
            orc[1] = orc[0]                                   # two valid writers of one enabled slot
        if c.dup and role == ACTIVATE_REVERT:
            orc[0] = orc[2] = must[0]                         # three valid writers of one disabled slot
        for u, o in enumerate(orc):
            rows[b, u] = _finish(c, lay.row(o, g), zc, (o + u) % 2 == 0)
        if role in (REJECTED_REVERT, REJECTED_OK):
            for k, u in enumerate((0, 2, 3, U - 1)):
                orc[u] = outside_ids(N)[(k + b) % 4]
            rows[b, 1, D // 2] = bad[b % 4]                   # an invalid row that names an oracle
            rows[b, 3, D - 1] = bad[(b + 1) % 4]              # an invalid row that names none
            if U > 8:
                rows[b, U - 3, 0] = bad[(b + 2) % 4]
        oracle[b] = torch.tensor(orc)
    state = dict(values=values, enabled=enabled, n_active=enabled.sum(1, dtype=torch.int32),
                 touched=torch.zeros(B, dtype=torch.uint8))
    flat_orc, flat_rows = oracle.reshape(-1).clone(), rows.reshape(B * U, D).clone()
    m = model_txn(state, flat_orc, flat_rows, c)
    return dict(case=c, U=U, ld=ld, roles=roles, far=far, state=state, oracle=flat_orc, rows=flat_rows, model=m,
                disabled=disabled)


def cut_gap_min(c):
    return 100 * fast_cases.TOL[c.storage]["qr"][0]


def conditions(m):
    """What the comparison with a kernel relies on, asserted for every instance of built case m; returns the
    model's round codes by role name."""
    c, model, roles = m["case"], m["model"], m["roles"]
    ref, status, active = model["ref"], model["status"], model["active"]
    gap = fast_cases.cut_gap(ref, c.f)
    R = c.N - c.f
    for b, role in enumerate(roles):
        tag = (case_id(c), ROLE_NAMES[role], "instance %d" % b)
        assert bool(active[b]) == (role != INACTIVE), tag
        if not active[b]:
            assert int(model["post"]["n_active"][b]) == c.N - 1, tag
            continue
        st, (rel1, rel2) = int(status[b]), ref["rel"][b].tolist()
        assert float(gap[b]) >= cut_gap_min(c), (tag, "cut gap", float(gap[b]))
        if st == RELIABILITY_INTERVAL:
            assert rel1 <= -0.05, (tag, "rel1", rel1)
        else:
            margin = 0.05 if st == OK else 0.03              # a reverting round's reliabilities: clear of the ends too
            assert margin <= rel1 <= 1 - margin and margin <= rel2 <= 1 - margin, (tag, "rel", rel1, rel2)
        x = model["table"][b][ref["reliable"][b]].double()
        var = x.var(0, unbiased=False)
        const = (x == x[0]).all(0)
        assert float(var[~const].min()) >= 1e-6 * (1.0 if c.constrained else SCALE ** 2), (tag, "variance", float(var[~const].min()))
        zc = const_col(role, c.D)
        assert zc is None or bool(const[zc]), (tag, "constant column")
        if st in (OK, ZERO_VARIANCE):                        # (no earlier check decides: the columns do)
            assert const.sum() == (0 if zc is None else 1), (tag, "constant columns")
        if zc is not None and st == ZERO_VARIANCE:           # +0.0 and -0.0 mixed among the reliable rows
            sign = torch.signbit(model["table"][b][ref["reliable"][b]][:, zc].float())
            assert bool(sign.any()) and not bool(sign.all()), (tag, "zero signs")
        # the role's verdict, from the contract's order
        if c.legacy:
            want = RELIABILITY_INTERVAL if c.constrained and role in REVERT_ROLES else OK
        elif R < 4:
            want = RELIABILITY_INTERVAL if role == REL_AND_ZV else TOO_FEW_RELIABLE
        else:
            want = {REL_AND_ZV: RELIABILITY_INTERVAL}.get(role, ZERO_VARIANCE if role in REVERT_ROLES else OK)
        assert st == want, (tag, "verdict", st, want)
        if st == OK:
            assert torch.equal(ref["reliable"][b], ~m["far"][b]), (tag, "planted far oracles")
    return {ROLE_NAMES[r]: int(status[b]) for b, r in enumerate(roles)}


# ------------------------------------------------------------------------------------ running a case

OUT = ("c1", "consensus", "rel", "reliable", "skew", "kurt", "qr")


class Run:
    """Built case m laid out on a device: state, batch, saved rows / flags and statuses carved out of canary
    buffers; the outputs prefilled with SENTINEL, status with STATUS_PREFILL, upd_status with UPD_PREFILL."""

    def __init__(self, m, device):
        c = self.c = m["case"]
        self.m, self.device = m, device
        dtype, idt, _ = DT[c.storage]
        N, D, U = c.N, c.D, m["U"]
        st = m["state"]
        self.bufs = dict(values=Buf(st["values"].view(idt), device, 0, dtype),
                         upd=Buf(m["rows"].view(idt), device, 0, dtype),
                         saved=Buf(torch.zeros(B * U, D, dtype=idt), device, 0, dtype),
                         saved_en=Buf(torch.full((B * U,), 0x77, dtype=torch.uint8), device),
                         upd_status=Buf(torch.full((B * U,), UPD_PREFILL, dtype=torch.int32), device),
                         oracle=Buf(m["oracle"], device))
        self.bufs["saved"].tensor().view(idt).fill_(self.bufs["saved"].canary)
        for k, b in self.bufs.items():
            setattr(self, k, b.tensor())
        self.enabled, self.n_active, self.touched = (st[k].clone().to(device) for k in ("enabled", "n_active", "touched"))
        self.winner = torch.full((B, N), -1, dtype=torch.int32, device=device)
        self.inst = m["model"]["inst"].to(device)
        f = dict(device=device)
        self.out = dict(
            c1=torch.full((B, D), SENTINEL, dtype=torch.float32, **f), consensus=torch.full((B, D), SENTINEL, dtype=torch.float32, **f),
            skew=torch.full((B, D), SENTINEL, dtype=torch.float32, **f), kurt=torch.full((B, D), SENTINEL, dtype=torch.float32, **f),
            rel=torch.full((B, 2), SENTINEL, dtype=torch.float32, **f), qr=torch.full((B, N), SENTINEL, dtype=torch.float32, **f),
            reliable=torch.full((B, N), SENTINEL, dtype=torch.uint8, **f),
            status=torch.full((B,), STATUS_PREFILL, dtype=torch.int32, **f))

    def apply(self, ops):
        c = self.c
        ops.apply_updates(self.values, self.enabled, self.n_active, self.touched, self.winner, self.inst, self.oracle,
                          self.upd, c.constrained, self.upd_status, not c.dup, self.saved, self.saved_en)

    def active(self):
        return (self.n_active == self.c.N).to(torch.uint8)

    def round(self, ops, active, work=None, rollback=False):
        """fast_round over the batch's instances; rollback: with the saved batch (the GPU op rolls back)."""
        c, o = self.c, self.out
        kw = {}
        if rollback:
            kw = dict(upd_oracle=self.oracle, upd_status=self.upd_status, upd_per_inst=self.m["U"], rst_saved=self.saved,
                      rst_saved_en=self.saved_en, rst_enabled=self.enabled, rst_n_active=self.n_active)
        ops.fast_round(self.values, active, c.D, c.f, c.constrained, max_spread(c), o["c1"], o["consensus"], o["skew"],
                       o["kurt"], o["rel"], o["qr"], o["reliable"], o["status"], c.hint, 0, 0, c.legacy, work, None, **kw)

    def restore(self, ops, active):
        ops.restore_updates(self.values, self.enabled, self.n_active, self.inst, self.oracle, self.upd_status,
                            self.saved, self.saved_en, self.out["status"], active, -1)


def _same(got, want, m, tag, what, index):
    """got == want element for element (floats on their bits), or an error naming the case, the first differing
    element's instance with its role, and what the further indices mean."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.is_floating_point:
        idt = {2: torch.int16, 4: torch.int32}[got.element_size()]
        got, want = got.contiguous().view(idt), want.contiguous().view(idt)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i = bad[0].tolist()
    raise AssertionError("%s %s: %s differs at %d places, first at instance %d (%s) %s %s: got %s, model %s" % (
        tag, case_id(m["case"]), what, bad.shape[0], i[0], ROLE_NAMES[m["roles"][i[0]]], index, i[1:],
        got[tuple(i)].item(), want[tuple(i)].item()))


def check_saved(r, tag):
    """After apply(): what the update op saved (the GPU kernels; with duplicate writers only the last one holds
    the pre-batch row, the others NOT_SAVED).  The sequential CPU op saves update by update: not compared."""
    m, c = r.m, r.c
    post, U = m["model"]["post"], m["U"]
    idt = DT[c.storage][1]
    b, o = m["model"]["inst"], m["oracle"].clamp(0, c.N - 1)
    stored = (post["upd_status"] == OK) & (post["winner"][b, o] == torch.arange(B * U, dtype=torch.int32))
    want_en = torch.where(stored, post["pre_enabled"][b, o], torch.tensor(NOT_SAVED, dtype=torch.uint8))
    canary = torch.full((c.D,), r.bufs["saved"].canary, dtype=idt)
    want_rows = torch.where(stored[:, None], post["pre_values"].view(idt)[b, o, :c.D], canary)
    _same(r.saved_en.view(B, U), want_en.view(B, U), m, tag, "saved_en", "slot")
    _same(r.bufs["saved"].bits().view(B, U, c.D), want_rows.view(B, U, c.D), m, tag, "saved rows", "[slot, column]")


def check(r, tag):
    """Run r after apply, round and roll-back against the model: update statuses, state bits, pad columns,
    enabled / n_active, status, outputs, canaries, and the read-only inputs."""
    m, c = r.m, r.c
    model, U, D = m["model"], m["U"], c.D
    idt = DT[c.storage][1]
    want = model["final"]
    _same(r.upd_status.view(B, U), want["upd_status"].view(B, U), m, tag, "upd_status", "slot")
    got_bits, want_bits = r.bufs["values"].bits(), want["values"].view(idt)
    _same(got_bits[:, :, :D], want_bits[:, :, :D], m, tag, "state", "[oracle, column]")
    _same(got_bits[:, :, D:], m["state"]["values"].view(idt)[:, :, D:], m, tag, "pad columns", "[oracle, pad column]")
    _same(r.enabled, want["enabled"], m, tag, "enabled", "oracle")
    _same(r.n_active.view(B, 1), want["n_active"].view(B, 1), m, tag, "n_active", "")
    _same(r.out["status"].view(B, 1), model["status"].view(B, 1), m, tag, "status", "")
    for k, b in r.bufs.items():
        assert b.margins_intact(), (tag, case_id(c), "canary around " + k)
    _same(r.bufs["upd"].bits(), m["rows"].view(idt), m, tag, "batch rows (read-only)", "")
    _same(r.oracle.view(B, U), m["oracle"].view(B, U), m, tag, "oracle (read-only)", "slot")
    out = {k: v.cpu() for k, v in r.out.items()}
    ok = (model["status"] == OK).nonzero().flatten()
    if ok.numel():
        o = {k: v[ok] for k, v in out.items()}
        case = dict(ref={k: v[ok] for k, v in model["ref"].items()}, x=model["table"][ok], N=c.N, D=D, f=c.f,
                    expect=~m["far"][ok], constrained=c.constrained, structured=False, storage=c.storage,
                    scale=1.0 if c.constrained else SCALE)
        fast_cases.check_round(o, case, "%s %s OK instances %s" % (tag, case_id(c), ok.tolist()))
    for b in (model["status"] != OK).nonzero().flatten().tolist():
        for k in OUT:
            assert bool((out[k][b] == SENTINEL).all()), (
                "%s %s: instance %d (%s) wrote %s" % (tag, case_id(c), b, ROLE_NAMES[m["roles"][b]], k))
