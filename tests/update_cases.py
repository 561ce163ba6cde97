"""Sequential model and case builder for the update / restore / commit storage ops (CPU only).

model_apply / model_restore / model_commit are plain loops written from the contract's rules (check
order: the prediction's interval or finite check before the caller's oracle lookup; a valid update
overwrites columns [0, D) of its slot bit for bit, enables the oracle and raises n_active on the
slot's first commit).  They share no code with csrc/kernels/updates.hip or its CPU twin and work on
integer views of the rows, so every comparison is on raw bits.

matrix() lists the cases; make() builds one (deterministic rows, the model's answer; built once,
shared, never modified); Run lays it out on a device, every buffer carved out of a larger
one filled with a canary; check_apply / check_restore / run_commit hold the assertions that
test_updates_model.py (CPU ops) and test_updates_gpu.py (HIP kernels) share.  kernel_paths() names
the branches of updates.hip a case reaches, from its dispatch rules.  Nothing here imports GPU code.
"""
import collections
import functools

import torch

OK, NOT_ACTIVE, INTERVAL_INPUT, NOT_ORACLE, RELIABILITY_INTERVAL, ZERO_VARIANCE, NON_FINITE = 0, 1, 2, 3, 6, 32, 34
NOT_SAVED = 0xFF
WSAD = 1_000_000

# storage -> (dtype, integer view of the same width, bytes)
DT = {"bf16": (torch.bfloat16, torch.int16, 2), "fp32": (torch.float32, torch.int32, 4),
      "int32": (torch.int32, torch.int32, 4), "int64": (torch.int64, torch.int64, 8)}
CANARY = 0xA5C396E15A3C69D2              # its leading bytes, for the narrower types
MARGIN = 64            # canary elements before and after every carved buffer (a multiple of 16 B)

Case = collections.namedtuple("Case", "storage D ld N B U constrained unique save off_upd off_saved off_values")


def _signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _bits(storage):
    return DT[storage][2] * 8


# bit patterns: (rejected, accepted) per storage and mode
_F = {"bf16": dict(one=0x3F80, next1=0x3F81, nzero=0x8000, zero=0, den=0x0001, nden=0x8001, nan=0x7FC0, nnan=0xFFC0,
                   snan=0x7F81, inf=0x7F80, ninf=0xFF80, big=0x7F7F, nbig=0xFF7F, two=0x4000, none=0xBF80),
      "fp32": dict(one=0x3F800000, next1=0x3F800001, nzero=0x80000000, zero=0, den=1, nden=0x80000001,
                   nan=0x7FC00000, nnan=0xFFC00000, snan=0x7F800001, inf=0x7F800000, ninf=0xFF800000,
                   big=0x7F7FFFFF, nbig=0xFF7FFFFF, two=0x40000000, none=0xBF800000)}


def edge_values(storage, constrained):
    """(rejected, accepted) element values of one storage type, as signed integers of its width."""
    n = _bits(storage)
    if storage in _F:
        f = _F[storage]
        if constrained:
            bad = ["next1", "nden", "nan", "nnan", "inf", "ninf", "two", "none", "snan"]
            good = ["one", "nzero", "den", "zero"]
        else:
            bad = ["nan", "nnan", "inf", "ninf", "snan"]
            good = ["one", "nzero", "den", "nden", "big", "nbig", "next1"]
        return [_signed(f[k], n) for k in bad], [_signed(f[k], n) for k in good]
    lo, hi = -(1 << (n - 1)), (1 << (n - 1)) - 1
    if constrained:
        bad = [-1, WSAD + 1, lo, hi]
        if n == 64:
            bad += [1 << 32, (1 << 32) + 5, -(1 << 32)]     # in range once truncated to 32 bits
        return bad, [0, WSAD, 1, WSAD - 1]
    return [], [lo, hi, -1, 0, WSAD + 1]


def storage_of(t):
    return {v[0]: k for k, v in DT.items()}[t.dtype]


def lanes_of(row_bytes):
    """(16-B chunks per row, lanes per update): the power of two covering the chunks, at most 64."""
    C = (row_bytes + 15) // 16
    L = 1
    while L < C and L < 64:
        L *= 2
    return C, L


# ----------------------------------------------------------------------------------------- the model

def _rows_valid(upd, storage, constrained):
    """Per update: does every element pass the interval (constrained) or finite (unconstrained) check."""
    if storage in _F:
        x = upd.double()                                   # exact for bf16 and fp32
        return ((x >= 0) & (x <= 1)).all(1) if constrained else torch.isfinite(x).all(1)
    if constrained:
        return ((upd >= 0) & (upd <= WSAD)).all(1)
    return torch.ones(upd.shape[0], dtype=torch.bool)


def model_apply(state, inst, oracle, upd, constrained):
    """state: dict(values [B, N, ld], enabled [B, N], n_active [B], touched [B]), not modified.
    Returns dict(values, enabled, n_active, touched, upd_status, winner [B, N] (index of the last valid
    writer, -1 where none), pre_values, pre_enabled (the pre-batch state))."""
    storage = storage_of(upd)
    idt = DT[storage][1]
    values = state["values"].clone()
    vb, ub = values.view(idt), upd.view(idt)
    enabled, n_active, touched = state["enabled"].clone(), state["n_active"].clone(), state["touched"].clone()
    B, N, _ = values.shape
    U, D = upd.shape
    valid = _rows_valid(upd, storage, constrained).tolist()
    status = torch.empty(U, dtype=torch.int32)
    winner = torch.full((B, N), -1, dtype=torch.int32)
    for u, (b, o) in enumerate(zip(inst.tolist(), oracle.tolist())):
        if not valid[u]:
            status[u] = INTERVAL_INPUT if constrained else NON_FINITE
            continue
        if not (0 <= b < B and 0 <= o < N):
            status[u] = NOT_ORACLE
            continue
        status[u] = OK
        vb[b, o, :D] = ub[u]
        if not enabled[b, o]:
            enabled[b, o] = 1
            n_active[b] += 1
        touched[b] = 1
        winner[b, o] = u
    return dict(values=values, enabled=enabled, n_active=n_active, touched=touched, upd_status=status, winner=winner,
                pre_values=state["values"], pre_enabled=state["enabled"])


def model_restore(pre, post, inst, oracle, D, status, active, inactive_status):
    """pre: the pre-batch state; post: model_apply's result.  Returns dict(values, enabled, n_active,
    upd_status) after the round's verdicts status [B] on the instances active [B]."""
    idt = DT[storage_of(pre["values"])][1]
    values, enabled, n_active = post["values"].clone(), post["enabled"].clone(), post["n_active"].clone()
    vb, pb = values.view(idt), pre["values"].view(idt)
    st = post["upd_status"].clone()
    for u, (b, o) in enumerate(zip(inst.tolist(), oracle.tolist())):
        if int(st[u]) != OK:
            continue                                   # did not store: keeps its own code
        if not active[b]:
            if inactive_status >= 0:
                st[u] = inactive_status                # keeps its row
            continue
        if int(status[b]) == OK:
            continue
        vb[b, o, :D] = pb[b, o, :D]
        enabled[b, o] = pre["enabled"][b, o]
        n_active[b] = pre["n_active"][b]
        st[u] = status[b]
    return dict(values=values, enabled=enabled, n_active=n_active, upd_status=st)


def model_commit(values, rows, oracle, upd_status, U):
    """Row u belongs to instance u // U; copied iff its status is OK and its oracle exists."""
    idt = DT[storage_of(values)][1]
    out = values.clone()
    ob, rb = out.view(idt), rows.view(idt)
    N, D = values.shape[1], rows.shape[1]
    for u, (o, s) in enumerate(zip(oracle.tolist(), upd_status.tolist())):
        if s == OK and 0 <= o < N:
            ob[u // U, o, :D] = rb[u]
    return out


# ------------------------------------------------------------------------------------------ buffers

class Buf:
    """A contiguous tensor carved out of a larger flat buffer of canaries, `offset` elements past a
    16-B aligned address: its data pointer is misaligned by offset * element size."""

    def __init__(self, data, device, offset=0, dtype=None):
        self.dtype = dtype or data.dtype
        self.shape, self.n, self.start = tuple(data.shape), data.numel(), MARGIN + offset
        bits = data.element_size() * 8
        self.canary = 0xC3 if data.dtype == torch.uint8 else _signed(CANARY >> (64 - bits), bits)
        flat = torch.full((self.start + self.n + MARGIN,), self.canary, dtype=data.dtype)
        flat[self.start:self.start + self.n] = data.reshape(-1)
        self.flat = flat.to(device)

    def tensor(self):
        return self.flat[self.start:self.start + self.n].view(self.dtype).view(self.shape)

    def bits(self):
        return self.flat[self.start:self.start + self.n].view(self.shape).cpu()

    def margins_intact(self):
        f = self.flat.cpu()
        return bool((f[:self.start] == self.canary).all() and (f[self.start + self.n:] == self.canary).all())


def _pattern(n, storage, salt):
    """Position-dependent bit pattern (a row restored or copied to the wrong place shows), as the
    storage's integer type."""
    bits = _bits(storage)
    i = torch.arange(n, dtype=torch.int64)
    lo = (i * 2654435761 + salt * 1540483477) & 0xFFFFFFFF
    if bits == 64:
        hi = (i * 2246822519 + salt) & 0x7FFFFFFF
        v = hi << 32 | lo
        v = torch.where(i % 2 == 1, -v - 1, v)
    else:
        v = (lo >> 7) & ((1 << bits) - 1)
        v = torch.where(v >= (1 << (bits - 1)), v - (1 << bits), v)
    return v.to(DT[storage][1])


# ------------------------------------------------------------------------------------- case builder

def _lane_targets(D, eb, C, L):
    """(chunk, column) of the lone bad element of one update per lane: chunk c belongs to lane c % L.
    First the row's first element, its last, and chunks of the later register blocks when C > L."""
    epc = 16 // eb
    col_in = lambda c, k: min(D - 1, c * epc + k % epc)
    out = [(0, 0), (C - 1, D - 1)]
    if C > L:
        span = C - 1 - L
        out += [(c, col_in(c, c)) for c in sorted({L + span * i // 7 for i in range(8)})]
    out += [(s, col_in(s, 3 * s + 1)) for s in range(1, min(L, C))]
    seen, uniq = set(), []
    for t in out:
        if t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


_INDEX_EDGES = [(-1, None), ("B", None), (None, -1), (None, "N"), (None, "N+3"), (-1, "N"), ("B", -1)]
# duplicate groups: writers in batch order (V valid, X rejected value), slot enabled before the batch?
_DUP_GROUPS = [("VV", 0), ("VVV", 1), ("VVVV", 0), ("VVX", 0), ("VXX", 1), ("XX", 0), ("XV", 0), ("VX", 1), ("XVXV", 0)]


def _specials(c, rot):
    """The batch's special updates: dict(pokes [(column, value)], idx (inst, oracle) overrides, dup group)."""
    dtype, idt, eb = DT[c.storage]
    C, L = lanes_of(c.D * eb)
    bad, good = edge_values(c.storage, c.constrained)
    lane = []
    for i, (ch, col) in enumerate(_lane_targets(c.D, eb, C, L)):
        pool = bad or good
        lane.append(dict(pokes=[(col, pool[(i + rot) % len(pool)])], lane=ch % L))
    edges = [dict(pokes=[(0, g), (c.D - 1, g), (c.D // 2, g)]) for g in good]
    edges.append(dict(pokes=[(d, good[(d + rot) % len(good)]) for d in range(min(c.D, 64))]))
    index = [dict(idx=e) for e in _INDEX_EDGES]
    if bad:
        index += [dict(idx=e, pokes=[((3 * i + 1) % c.D, bad[(i + rot) % len(bad)])]) for i, e in enumerate(_INDEX_EDGES)]
    dups = []
    if not c.unique:
        groups = [g for g in _DUP_GROUPS if bad or "X" not in g[0]]
        for k in range(4):
            for gi, (w, _) in enumerate(groups):
                if k < len(w):
                    pokes = [((5 * gi + k) % c.D, bad[(gi + k + rot) % len(bad)])] if w[k] == "X" else []
                    dups.append(dict(dup=gi, writers=w, en=groups[gi][1], pokes=pokes))
    return lane, edges, index, dups


def _thin(items, k, rot):
    if len(items) <= k:
        return items
    return [items[(rot + i * len(items) // k) % len(items)] for i in range(k)] if k > 0 else []


@functools.lru_cache(maxsize=None)
def make(c):
    """Build case c: the pre-batch state, the batch and the model's answer (CPU tensors, read-only).
    Every special update sits between two plain valid ones.  A case with a fixed small U (the rows
    above 4096 columns: 63 updates) has room for 31 specials: the first and the last element, a chunk
    of a later register block, and a subset of the other lanes, edges and duplicates that rotates
    with the variant (constrained / unique / save); fp32 2052 x 2056 covers all 64 lanes of a wave."""
    dtype, idt, eb = DT[c.storage]
    C, L = lanes_of(c.D * eb)
    rot = 4 * c.constrained + 2 * c.unique + c.save       # thinned cases: another subset per variant
    lane, edges, index, dups = _specials(c, rot)
    if c.U == 1:
        specials = []
    elif c.U and c.U < 2 * (len(lane) + len(edges) + len(index) + len(dups)) + 1:
        room = (c.U - 1) // 2                              # every special sits between two plain updates
        keep = lane[:3]                                    # first element, last element, a later block
        dsel = [d for d in dups if d["writers"] in ("VV", "VVV", "VVX", "XX")]
        rest = [_thin(edges, 2, rot), _thin(index, 5, rot), dsel]
        n_lane = room - len(keep) - sum(len(r) for r in rest)
        specials = keep + _thin(lane[3:], n_lane, rot) + rest[0] + rest[1] + rest[2]
    else:
        specials = lane + edges + index + dups
    seq = [None]
    for s in specials:
        seq += [s, None]
    U = c.U or max(len(seq), 300 if L == 1 else 151)       # L = 1: 256 updates per workgroup
    assert len(seq) <= U, (c, len(seq))
    seq += [None] * (U - len(seq))
    if not c.U and U % (256 // L) == 0:
        seq.append(None)
        U += 1
    assert U == 1 or U % (256 // L) != 0, (c, U)
    N = c.N
    B = c.B or (U + N - 1) // N + 3
    assert (B - 1) * N >= U, (c, B, U)

    g = torch.Generator().manual_seed(c.D * 131 + c.ld * 7 + rot)
    if c.storage in _F:
        x = torch.rand(U, c.D, generator=g)
        upd = (x if c.constrained else (x - 0.5) * 200.0).to(dtype)
    elif c.constrained:
        upd = torch.randint(0, WSAD + 1, (U, c.D), generator=g).to(dtype)
    else:
        upd = torch.randint(-(1 << 62), 1 << 62, (U, c.D), generator=g).to(dtype)
    ub = upd.view(idt)
    # instance B - 1 is never written; the other slots are handed out in a shuffled order
    slots = torch.randperm((B - 1) * N, generator=g).tolist()
    enabled = (torch.arange(B * N) % 3 == 0).to(torch.uint8).view(B, N)
    inst, oracle, group_slot, lanes_hit = [], [], {}, set()
    sym = {"B": B, "N": N, "N+3": N + 3, -1: -1}
    for u, s in enumerate(seq):
        s = s or {}
        if "dup" in s:
            if s["dup"] not in group_slot:
                group_slot[s["dup"]] = slots.pop()
                b, o = divmod(group_slot[s["dup"]], N)
                enabled[b, o] = s["en"]
            b, o = divmod(group_slot[s["dup"]], N)
        else:
            b, o = divmod(slots.pop(), N)
        ib, io = s.get("idx", (None, None))
        inst.append(b if ib is None else sym[ib])
        oracle.append(o if io is None else sym[io])
        for col, v in s.get("pokes", []):
            ub[u, col] = v
        if "lane" in s:
            lanes_hit.add(s["lane"])
    inst, oracle = torch.tensor(inst, dtype=torch.int64), torch.tensor(oracle, dtype=torch.int64)
    values = _pattern(B * N * c.ld, c.storage, 1 + c.D).view(B, N, c.ld).view(dtype)
    state = dict(values=values, enabled=enabled, n_active=enabled.sum(1, dtype=torch.int32),
                 touched=torch.zeros(B, dtype=torch.uint8))
    model = model_apply(state, inst, oracle, upd, c.constrained)
    return dict(case=c, B=B, N=N, U=U, L=L, C=C, state=state, inst=inst, oracle=oracle, upd=upd, model=model,
                lanes_hit=lanes_hit, n_special=len(specials))


_SHAPES = {
    "bf16": [(1, 8), (6, 8), (6, 6), (5, 5), (8, 8), (8, 10), (8, 12), (16, 16), (24, 24), (40, 40), (72, 72),
             (136, 136), (264, 264), (4104, 4104), (8200, 8200)],
    "fp32": [(1, 8), (3, 8), (4, 8), (6, 8), (100, 104), (2052, 2056), (4100, 4104)],
    "int32": [(4, 4), (6, 6), (7, 7), (36, 36)],
    "int64": [(1, 1), (2, 2), (3, 3), (6, 6), (33, 33)],
}
# misaligned upd / saved: one element, and a 4-B aligned amount that is no multiple of 16 B
_MISALIGNED = [("bf16", 40, 40, (1, 2)), ("fp32", 100, 104, (1, 3))]


def _shape_case(storage, D, ld, constrained, unique, save, **kw):
    N = 5 if D > 4096 else 7 if D <= 8 else 16
    U = 63 if D > 4096 else 0                  # the largest rows: at most 64 updates
    return Case(storage, D, ld, N, 0, kw.pop("U", U), constrained, unique, save, kw.pop("off_upd", 0),
                kw.pop("off_saved", 0), kw.pop("off_values", 0))


@functools.lru_cache(maxsize=None)
def matrix():
    out = []
    variants = [(con, uni, save) for con in (True, False) for uni in (False, True) for save in (False, True)]
    for storage, shapes in _SHAPES.items():
        for D, ld in shapes:
            for con, uni, save in variants:
                if storage == "int32" and not con:
                    continue                   # the exact engine's int32 rows are constrained
                out.append(_shape_case(storage, D, ld, con, uni, save))
    for storage, D, ld, offs in _MISALIGNED:
        for con, uni, save in variants:
            for off in offs:
                out.append(_shape_case(storage, D, ld, con, uni, save, off_upd=off))
                if save:
                    out.append(_shape_case(storage, D, ld, con, uni, save, off_saved=off))
    for con, uni, save in variants:
        out.append(_shape_case("bf16", 6, 8, con, uni, save, U=1))
        out.append(_shape_case("bf16", 6, 6, con, uni, save, off_values=1))     # state only 2-B aligned
    return tuple(out)


def restore_grid_case():
    """16 641 unique updates of 7 x 6 bf16 rows over 2 400 instances: the restore kernel's grid is capped
    at 64 workgroups of 256 threads there, so 257 threads take a second grid-stride iteration."""
    return Case("bf16", 6, 8, 7, 2400, 16641, True, True, True, 0, 0, 0)


def case_id(c):
    s = "%s-%dx%d-%s-%s-%s" % (c.storage, c.D, c.ld, "con" if c.constrained else "unc",
                               "unique" if c.unique else "general", "save" if c.save else "plain")
    if c.U:
        s += "-U%d" % c.U
    for k in ("off_upd", "off_saved", "off_values"):
        if getattr(c, k):
            s += "-%s%d" % (k[4:], getattr(c, k))
    return s


# ------------------------------------------------------------------------------------ running a case

class Run:
    """Case m (make()) laid out on a device; every tensor an op writes is a fresh copy."""

    def __init__(self, m, device):
        c = self.c = m["case"]
        self.m, self.device = m, device
        _, idt, _ = DT[c.storage]
        B, N, U = m["B"], m["N"], m["U"]
        st = m["state"]
        dtype = DT[c.storage][0]
        self.bufs = dict(values=Buf(st["values"].view(idt), device, c.off_values, dtype),
                         upd=Buf(m["upd"].view(idt), device, c.off_upd, dtype),
                         upd_status=Buf(torch.full((U,), -7, dtype=torch.int32), device))
        if c.save:
            sv = torch.zeros(U, c.D, dtype=idt)
            self.bufs["saved"] = Buf(sv, device, c.off_saved, dtype)
            self.bufs["saved"].tensor().view(idt).fill_(self.bufs["saved"].canary)
            self.bufs["saved_en"] = Buf(torch.full((U,), 0x77, dtype=torch.uint8), device)
        self.values, self.upd, self.upd_status = (self.bufs[k].tensor() for k in ("values", "upd", "upd_status"))
        self.saved = self.bufs["saved"].tensor() if c.save else None
        self.saved_en = self.bufs["saved_en"].tensor() if c.save else None
        self.enabled, self.n_active, self.touched = (st[k].clone().to(device) for k in ("enabled", "n_active", "touched"))
        self.winner = torch.full((B, N), -1, dtype=torch.int32, device=device)
        self.inst, self.oracle = m["inst"].to(device), m["oracle"].to(device)

    def apply(self, ops):
        c = self.c
        ops.apply_updates(self.values, self.enabled, self.n_active, self.touched, self.winner, self.inst, self.oracle,
                          self.upd, c.constrained, self.upd_status, c.unique, self.saved, self.saved_en)

    def restore(self, ops, status, active, inactive_status):
        ops.restore_updates(self.values, self.enabled, self.n_active, self.inst, self.oracle, self.upd_status,
                            self.saved, self.saved_en, status.to(self.device), active.to(self.device), inactive_status)


def _eq(a, b, what, tag):
    a, b = a.cpu(), b.cpu()
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError("%s: %s differs at %d places, first %s: got %s, model %s"
                             % (tag, what, len(bad), bad[0].tolist(), a[tuple(bad[0])].item(), b[tuple(bad[0])].item()))


def _check_state(r, want, tag):
    idt = DT[r.c.storage][1]
    _eq(r.upd_status, want["upd_status"], "upd_status", tag)
    _eq(r.bufs["values"].bits().view(torch.uint8), want["values"].view(idt).view(torch.uint8), "values bytes", tag)
    _eq(r.enabled, want["enabled"], "enabled", tag)
    _eq(r.n_active, want["n_active"], "n_active", tag)
    for k, b in r.bufs.items():
        assert b.margins_intact(), (tag, "canary around " + k)
    _eq(r.bufs["upd"].bits(), r.m["upd"].view(idt), "upd (read-only)", tag)
    _eq(r.inst, r.m["inst"], "inst (read-only)", tag)
    _eq(r.oracle, r.m["oracle"], "oracle (read-only)", tag)


def check_apply(r, tag, sequential_save=False):
    """State, statuses, canaries and save buffers of Run r after apply() against the model.
    sequential_save: the op saved update by update (the CPU loop), so on the last-writer path its
    superseded updates hold rows too; their raw saved / saved_en are not compared."""
    m, c = r.m, r.c
    model = m["model"]
    idt = DT[c.storage][1]
    _check_state(r, model, tag)
    _eq(r.touched, model["touched"], "touched", tag)
    assert bool(r.winner.eq(-1).all()), (tag, "winner workspace not reset to -1")
    if not c.save or (sequential_save and not c.unique):
        return
    U, D = m["U"], c.D
    b, o = m["inst"].clamp(0, m["B"] - 1), m["oracle"].clamp(0, m["N"] - 1)
    stored = model["upd_status"] == OK
    if not c.unique:                                   # only each slot's winner holds the pre-batch row
        stored &= model["winner"][b, o] == torch.arange(U, dtype=torch.int32)
    want_en = torch.where(stored, model["pre_enabled"][b, o], torch.tensor(NOT_SAVED, dtype=torch.uint8))
    canary = torch.full((D,), r.bufs["saved"].canary, dtype=idt)
    want_rows = torch.where(stored[:, None], model["pre_values"].view(idt)[b, o, :D], canary)
    _eq(r.saved_en, want_en, "saved_en", tag)
    _eq(r.bufs["saved"].bits(), want_rows, "saved rows", tag)


def round_status(B, sparse=False):
    """Round verdicts per instance mixing OK, ZERO_VARIANCE and RELIABILITY_INTERVAL (sparse: a third
    of the instances reverted), and an active mask with some zeros."""
    i = torch.arange(B)
    status = torch.zeros(B, dtype=torch.int32)
    status[i % 6 == 0 if sparse else i % 3 == 1] = ZERO_VARIANCE
    status[i % 6 == 3 if sparse else i % 3 == 2] = RELIABILITY_INTERVAL
    return status, (i % 4 != 1).to(torch.uint8)


def check_restore(r, status, active, inactive_status, tag):
    """Run r after apply() and restore() against model_restore; touched is not the restore's to change."""
    m = r.m
    want = model_restore(m["state"], m["model"], m["inst"], m["oracle"], r.c.D, status, active, inactive_status)
    _check_state(r, want, tag)
    return want


# commit: (storage, D, ld, N, B, U per instance, element offset of `rows`)
COMMIT_CASES = [
    ("bf16", 6, 8, 7, 40, 5, 0), ("fp32", 16, 16, 7, 30, 6, 0), ("bf16", 24, 24, 9, 30, 7, 0),          # L = 4
    ("int64", 12, 12, 7, 30, 5, 0), ("int32", 36, 36, 12, 20, 9, 0), ("bf16", 128, 136, 9, 20, 7, 0),   # L = 16
    ("fp32", 100, 104, 16, 12, 11, 0), ("bf16", 264, 264, 9, 12, 7, 0),                                 # L = 64, RB = 8
    ("fp32", 2052, 2056, 6, 5, 5, 0), ("bf16", 4104, 4104, 5, 5, 4, 0),                                 # RB = 16
    ("fp32", 4100, 4104, 4, 4, 3, 0), ("bf16", 8200, 8200, 4, 4, 3, 0),                                 # > 16 KiB: bytes
    ("bf16", 40, 40, 9, 20, 7, 1), ("fp32", 100, 104, 16, 12, 11, 3), ("int64", 6, 6, 7, 12, 5, 1)]     # unaligned rows


@functools.lru_cache(maxsize=None)
def make_commit(cc):
    storage, D, ld, N, B, U, off = cc
    dtype, idt, eb = DT[storage]
    n = B * U - (U // 2 + 1)                               # n < B * U: the last instance's rows are short
    g = torch.Generator().manual_seed(D + 3 * N)
    rows = _pattern(n * D, storage, 77 + D).view(n, D).view(dtype)
    oracle = torch.stack([torch.randperm(N, generator=g)[:U] for _ in range(B)]).reshape(-1)[:n].clone()
    st = torch.zeros(n, dtype=torch.int32)
    codes = [ZERO_VARIANCE, RELIABILITY_INTERVAL, NOT_ORACLE, INTERVAL_INPUT, NOT_ACTIVE]
    for k, u in enumerate(range(2, n, 5)):
        st[u] = codes[k % len(codes)]
    for k, u in enumerate(range(1, n, 7)):
        oracle[u] = [-1, N, N + 3][k % 3]                  # out of range, status OK or not
    values = _pattern(B * N * ld, storage, 5 + D).view(B, N, ld).view(dtype)
    want = model_commit(values, rows, oracle, st, U)
    return dict(cc=cc, rows=rows, oracle=oracle, st=st, values=values, want=want, n=n)


def run_commit(mc, ops, device, tag):
    storage, D, ld, N, B, U, off = mc["cc"]
    idt = DT[storage][1]
    rows = Buf(mc["rows"].view(idt), device, off, DT[storage][0])
    values = Buf(mc["values"].view(idt), device, 0, DT[storage][0])
    oracle, st = mc["oracle"].to(device), mc["st"].to(device)
    ops.commit_updates(rows.tensor(), oracle, st, values.tensor(), U)
    _eq(values.bits().view(torch.uint8), mc["want"].view(idt).view(torch.uint8), "values bytes", tag)
    assert values.margins_intact() and rows.margins_intact(), (tag, "canary")
    _eq(rows.bits(), mc["rows"].view(idt), "rows (read-only)", tag)
    _eq(oracle, mc["oracle"], "oracle (read-only)", tag)
    _eq(st, mc["st"], "upd_status (read-only)", tag)


# ---------------------------------------------------------------------------------- dispatch naming

def _granule(*addrs_and_len):
    return 16 if all(a % 16 == 0 for a in addrs_and_len) else 4 if all(a % 4 == 0 for a in addrs_and_len) else 1


def kernel_paths(m):
    """Names of the updates.hip branches case m reaches in apply_updates, by its dispatch rules: lanes
    per update from the row's 16-B chunks, the register / short-row / loop path of the fused unique
    kernel, the validation form and the copy granularity from the addresses' alignment.  Buffers start
    at 16-B aligned addresses plus their element offsets."""
    c = m["case"]
    eb = DT[c.storage][2]
    rb = c.D * eb
    C, L = lanes_of(rb)
    nch = rb // 16
    RB = 16 if L == 64 and nch > 8 * L else 8
    flt, bf16 = c.storage in _F, c.storage == "bf16"
    B, N = m["B"], m["N"]
    stored = (m["model"]["upd_status"] == OK).tolist()
    names = set()
    for u, (b, o) in enumerate(zip(m["inst"].tolist(), m["oracle"].tolist())):
        src = c.off_upd * eb + u * rb
        in_range = 0 <= b < B and 0 <= o < N
        dst = (c.off_values + (b * N + o) * c.ld) * eb if in_range else None
        sv = [c.off_saved * eb + u * rb] if c.save else []
        if not c.unique:
            if c.constrained:
                names.add("general/L%d/validate-%s" % (L, "vec" if bf16 and c.D % 8 == 0 and src % 16 == 0 else "scalar"))
            elif flt:
                names.add("general/L%d/validate-finite" % L)
            if stored[u] and int(m["model"]["winner"][b, o]) == u:
                names.add("general/L%d/copy%d%s" % (L, _granule(src, dst, rb, *sv), "-save" if c.save else ""))
            continue
        if dst is None:
            continue                                        # (the address is computed, never dereferenced)
        vec = rb % 16 == 0 and src % 16 == 0 and dst % 16 == 0
        if flt and vec and nch <= RB * L:
            names.add("unique/L%d/RB%d/register%s" % (L, RB, "-save" if c.save else ""))
        elif L == 1 and bf16 and rb % 4 == 0 and rb <= 16 and c.off_upd * eb % 4 == 0 and c.off_values * eb % 4 == 0 \
                and c.ld % 2 == 0 and (N * c.ld) % 2 == 0:
            names.add("unique/L1/short-row-w%d%s" % (rb // 4, "-save" if c.save else ""))
        else:
            val = "vec" if bf16 and vec else "scalar" if (c.constrained or flt) else "none"
            names.add("unique/L%d/RB%d/loop/validate-%s" % (L, RB, val))
            if stored[u]:
                names.add("unique/L%d/RB%d/loop/copy%d%s" % (L, RB, _granule(src, dst, rb, *sv), "-save" if c.save else ""))
    return names


def restore_paths(m):
    """Branches of upd_restore_kernel for case m (every stored update of a reverted instance)."""
    c = m["case"]
    eb = DT[c.storage][2]
    rb = c.D * eb
    names = set()
    need = (m["U"] + 255) // 256
    blocks = max((need + 1) // 2, min(need, 64))
    if blocks * 256 < m["U"]:
        names.add("restore/second-iteration")
    for u, (b, o) in enumerate(zip(m["inst"].tolist(), m["oracle"].tolist())):
        if int(m["model"]["upd_status"][u]) == OK:
            dst = (c.off_values + (b * m["N"] + o) * c.ld) * eb
            names.add("restore/copy%d" % (16 if _granule(dst, c.off_saved * eb + u * rb, rb) == 16 else 1))
    return names


def commit_path(cc):
    storage, D, ld, N, B, U, off = cc
    eb = DT[storage][2]
    rb = D * eb
    C = (rb + 15) // 16
    L = 4 if C <= 4 else 16 if C <= 16 else 64
    RB = 16 if rb // 16 > 8 * L else 8
    # dst alignment can differ from slot to slot; these cases keep ld * eb a multiple of 16 or never aligned
    aligned = rb % 16 == 0 and off * eb % 16 == 0 and ld * eb % 16 == 0 and rb // 16 <= RB * L
    return "commit/L%d/RB%d/%s" % (L, RB, "register" if aligned else "bytes")
