"""Adversarial cases for the encoder kernels (csrc/kernels/encoder_ops.hip): data, fp64 references, bounds.

Plain PyTorch on the CPU.  Nothing here imports the package, the kernels or the bindings: the references
are written from the operations' definitions (softmax(Q K^T / 8 + mask) V, LayerNorm, mean), in fp64 on
the very bf16 / fp32 values the op receives.  test_encoder_cases.py (CPU ops, no GPU) and
test_encoder_adversarial_gpu.py (HIP kernels) run the same cached cases through the same checkers.

Notation.  u = 2^-8 (bf16 unit roundoff as the bounds use it).  ref64: the fp64 value.  A = P64 |V|: the
attention output with |V| in place of V, the scale every attention error term is relative to.

Attention cases
  one-hot   K rows are +-8 codes of the key index (7 bits, each repeated 9 times, one constant dim), Q rows
            are the code of the key they must pick.  Matching score 64 * 64 / 8 = 512; any other key differs
            in >= 1 bit = 9 dims, so it trails by >= 2 * 9 * 64 / 8 = 144 and exp(-144) is 0 in fp32: P is
            exactly one-hot and the output is the picked V row, bit for bit, in both kernels.
  uniform   Q = 0: every score is 0 whatever K holds, P = 1/n exactly (n a power of two), V small
            integers: every product and sum is exact, the output is sum/n (rounded once for bf16).
  isolation the same call twice, with every value that must not matter replaced: bit-identical rows.
  random    amp * randn, checked against ref64 with the derived bounds attn_ratio() documents.

Every builder is cached: a case is built once per process and must not be modified by its users.
"""
import functools
import math
import zlib

import torch

DH = 64
U = 2.0 ** -8
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SEQ = (32, 64, 96, 128)       # S (padded) or rounded max_len (varlen): one kernel instantiation (NQB) each
EPS = 1e-5
NEG_INF = float("-inf")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------ references
def pack_qkv(q, k, v):
    """q, k, v [B, heads, S, 64] -> the fused projection layout [B, S, 3 * heads * 64]."""
    B, H, S, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * H * DH).contiguous()


def attn_ref(qkv, heads, mask=None, dtype=torch.float64, scale=0.125):
    """softmax(Q K^T * scale + key mask) V over qkv [B, S, 3*heads*64] evaluated in `dtype`.
    Returns (out, A), both [B, S, heads*64]; A uses |V|.  A sequence with no attended key gives NaN."""
    B, S, _ = qkv.shape
    t = qkv.to(dtype).view(B, S, 3, heads, DH).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(~mask.bool()[:, None, None, :], NEG_INF)
    p = torch.softmax(s, -1)
    back = lambda o: o.transpose(1, 2).reshape(B, S, heads * DH)
    return back(p @ t[2]), back(p @ t[2].abs())


def varlen_ref(qkv, lens, heads, dtype=torch.float64, scale=0.125):
    """attn_ref per packed segment: qkv [T, 3*heads*64], segment b = the next lens[b] rows."""
    T = qkv.shape[0]
    out = torch.zeros(T, heads * DH, dtype=dtype)
    A = torch.zeros(T, heads * DH, dtype=dtype)
    lo = 0
    for L in lens:
        if L:
            o, a = attn_ref(qkv[lo:lo + L][None], heads, None, dtype, scale)
            out[lo:lo + L], A[lo:lo + L] = o[0], a[0]
        lo += L
    return out, A


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


# ------------------------------------------------------------------------------------------ attention checks
def attn_ratio(out, ref, A, storage, ref32=None, rows=None):
    """Largest err / bound of an attention output against ref64 (inf if anything is not finite).
    bf16, per element: |out - ref64| <= 2.25 u A.  First order: u A from P rounded to bf16 plus u |ref| from
    the output rounding, |ref| <= A; 12.5 % for the second-order term and the fp32 scores / exponentials.
    fp32, per case: max |out - ref64| <= max(2e-5, 4 e_model), e_model the largest error of the plain
    float32 evaluation `ref32` of the same expression (a different summation order than the MFMA chain)."""
    out = out.double()
    if rows is not None:
        out, ref, A = out[rows], ref[rows], A[rows]
        ref32 = ref32[rows] if ref32 is not None else None
    if out.numel() == 0:
        return 0.0
    if not torch.isfinite(out).all():
        return math.inf
    err = (out - ref).abs()
    if storage == "bf16":
        return (err / (2.25 * U * A)).max().item()
    e_model = (ref32.double() - ref).abs().max().item()
    return err.max().item() / max(2e-5, 4 * e_model)


def old_tolerance_accepts(out, ref32):
    """The check this suite replaces: assert_close(out, fp32 reference, rtol=3e-2, atol=3e-2)."""
    return bool(((out.double() - ref32.double()).abs() <= 3e-2 + 3e-2 * ref32.double().abs()).all())


# ------------------------------------------------------------------------------------------ masks
def hole_mask(g, B, S, keep=0.7):
    """Scattered zeros, never a prefix: key 1 is masked, the last key attended."""
    m = torch.rand(B, S, generator=g) < keep
    m[:, 1], m[:, S - 1] = False, True
    return m.to(torch.uint8)


def prefix_mask(lens, S):
    return (torch.arange(S)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)


# ------------------------------------------------------------------------------------------ one-hot
def codes(S):
    """[S, 64] rows of +-8: the 7-bit row index as +-1, each bit 9 times, plus one constant dim."""
    bits = ((torch.arange(S)[:, None] >> torch.arange(7)) & 1) * 2 - 1
    return 8.0 * torch.cat([bits.repeat(1, 9), torch.ones(S, 1, dtype=bits.dtype)], 1).double()


def _onehot_block(g, att, S, dtype):
    """One (sequence, head): q, k, v [S, 64] and the expected rows [len(att), 64] of the attended queries."""
    k = codes(S)
    q = k.clone()
    pi = att[torch.randperm(len(att), generator=g)]
    q[att] = k[pi]
    v = _randn(g, S, DH).to(dtype)
    return q.to(dtype), k.to(dtype), v, v[pi]


@functools.lru_cache(maxsize=None)
def onehot_padded(S, storage, masked, B=2, heads=3):
    dtype = DTYPES[storage]
    g = _gen("onehot", S, storage, masked)
    mask = hole_mask(g, B, S) if masked else None
    q, k, v = (torch.zeros(B, heads, S, DH, dtype=dtype) for _ in range(3))
    expect = torch.zeros(B, S, heads * DH, dtype=dtype)
    rows = torch.ones(B, S, dtype=torch.bool) if mask is None else mask.bool()
    for b in range(B):
        att = rows[b].nonzero()[:, 0]
        for h in range(heads):
            q[b, h], k[b, h], v[b, h], e = _onehot_block(g, att, S, dtype)
            expect[b, att, h * DH:(h + 1) * DH] = e
    return dict(qkv=pack_qkv(q, k, v), mask=mask, heads=heads, expect=expect, rows=rows, storage=storage)


def exact_lens(S):
    """Segment lengths of the exact varlen cases: S, 1, S - 31, 0 and a short last segment."""
    return (S, 1, S - 31, 0, 5)


@functools.lru_cache(maxsize=None)
def onehot_varlen(S, storage, heads=3):
    dtype = DTYPES[storage]
    g = _gen("onehot_varlen", S, storage)
    lens = exact_lens(S)
    qs, ks, vs, es = [], [], [], []
    for L in lens:
        blocks = [_onehot_block(g, torch.arange(L), L, dtype) for _ in range(heads)]
        for dst, i in ((qs, 0), (ks, 1), (vs, 2), (es, 3)):
            dst.append(torch.stack([blk[i] for blk in blocks], 1).reshape(L, heads * DH))   # [L, heads*64]
    qkv = torch.cat([torch.cat(qs), torch.cat(ks), torch.cat(vs)], 1).contiguous()
    return dict(qkv=qkv, lens=lens, cu=cu_of(lens), max_len=S, heads=heads, expect=torch.cat(es), storage=storage)


# ------------------------------------------------------------------------------------------ uniform
def uniform_counts(S):
    """Attended-key counts of the padded uniform cases: powers of two (1/n is exact), the largest <= S."""
    return (1, 2, 16, 1 << (S.bit_length() - 1))


def _uniform_parts(g, shape, dtype):
    q = torch.zeros(*shape, DH, dtype=dtype)
    k = (50 * _randn(g, *shape, DH)).to(dtype)
    v = torch.randint(-8, 9, (*shape, DH), generator=g).to(dtype)
    return q, k, v


@functools.lru_cache(maxsize=None)
def uniform_padded(S, n, storage, B=2, heads=3):
    dtype = DTYPES[storage]
    g = _gen("uniform", S, n, storage)
    q, k, v = _uniform_parts(g, (B, heads, S), dtype)
    keep = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        keep[b, torch.randperm(S, generator=g)[:n]] = True
    mean = (v.double() * keep[:, None, :, None]).sum(2) / n                     # [B, heads, 64], exact
    expect = mean.reshape(B, 1, heads * DH).expand(B, S, heads * DH).to(dtype).contiguous()
    return dict(qkv=pack_qkv(q, k, v), mask=None if n == S else keep.to(torch.uint8), heads=heads,
                expect=expect, rows=torch.ones(B, S, dtype=torch.bool), storage=storage)


def uniform_lens(S):
    """Power-of-two lengths for the varlen uniform case of kernel instantiation S (max_len = S)."""
    return {32: (32, 1, 2, 4, 8, 16), 64: (64, 1, 32, 2), 96: (64, 8, 64, 4), 128: (128, 64, 16, 128, 1)}[S]


@functools.lru_cache(maxsize=None)
def uniform_varlen(S, storage, heads=3):
    dtype = DTYPES[storage]
    g = _gen("uniform_varlen", S, storage)
    lens = uniform_lens(S)
    T = sum(lens)
    q, k, v = _uniform_parts(g, (T, heads), dtype)
    expect = torch.zeros(T, heads * DH, dtype=dtype)
    lo = 0
    for L in lens:
        expect[lo:lo + L] = (v[lo:lo + L].double().sum(0) / L).reshape(1, heads * DH).to(dtype)
        lo += L
    qkv = torch.cat([t.reshape(T, heads * DH) for t in (q, k, v)], 1).contiguous()
    return dict(qkv=qkv, lens=lens, cu=cu_of(lens), max_len=S, heads=heads, expect=expect, storage=storage)


# ------------------------------------------------------------------------------------------ isolation
@functools.lru_cache(maxsize=None)
def isolation_varlen(S, storage, heads=3):
    """Two packed batches that agree on the target segments only.  Targets: segment 1 (its last key block
    is completed by the next segment's rows) and the short final segment (rows past the buffer: the clamp).
    Finite values only: a non-finite value in a masked row would reach the output as 0 * Inf."""
    dtype = DTYPES[storage]
    g = _gen("isolation_varlen", S, storage)
    lens = (7, S - 20, S, 0, 5)
    cu = cu_of(lens)
    T = sum(lens)
    a = _randn(g, T, 3 * heads * DH).to(dtype)
    b = (1e4 * _randn(g, T, 3 * heads * DH)).to(dtype)
    targets = [slice(int(cu[1]), int(cu[2])), slice(int(cu[4]), int(cu[5]))]
    for t in targets:
        b[t] = a[t]
    return dict(qkv=a, other=b, lens=lens, cu=cu, max_len=S, heads=heads, targets=targets, storage=storage)


@functools.lru_cache(maxsize=None)
def isolation_padded(S, storage, B=3, heads=3):
    """Two padded batches that agree on the attended positions of sequence 1 only (hole mask); the
    attended query rows of sequence 1 must not change.  Finite values only (0 * Inf is out of scope)."""
    dtype = DTYPES[storage]
    g = _gen("isolation_padded", S, storage)
    mask = hole_mask(g, B, S)
    a = _randn(g, B, S, 3 * heads * DH).to(dtype)
    b = (1e4 * _randn(g, B, S, 3 * heads * DH)).to(dtype)
    rows = torch.zeros(B, S, dtype=torch.bool)
    rows[1] = mask[1].bool()
    b[rows] = a[rows]
    return dict(qkv=a, other=b, mask=mask, heads=heads, rows=rows, storage=storage)


# ------------------------------------------------------------------------------------------ random
# (S, B, heads, amp, mask kind, mask dtype): every S at both amplitudes; heads {1, 5, 12}, B {1, 3}, prefix /
# hole / no mask and bool / uint8 / int64 masks each at least once
RANDOM_PADDED = [
    (32, 3, 5, 1, "hole", "uint8"), (32, 1, 12, 6, "prefix", "bool"),
    (64, 1, 1, 1, "prefix", "int64"), (64, 3, 12, 6, "hole", "bool"),
    (96, 3, 1, 1, "none", None), (96, 1, 5, 6, "hole", "int64"),
    (128, 3, 12, 1, "hole", "uint8"), (128, 3, 5, 6, "prefix", "uint8"),
]
# (lens, max_len, heads, amp): lengths 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128 around the block edges,
# an empty segment in the middle and 5 last; one max_len off the multiple of 32; one batch of a single token
RANDOM_VARLEN = [
    ((31, 1, 0, 32, 5), 32, 5, 1), ((31, 1, 0, 32, 5), 32, 1, 6),
    ((33, 1, 0, 5), 33, 12, 1),
    ((33, 64, 0, 63, 5), 64, 1, 1), ((33, 64, 0, 63, 5), 64, 5, 6),
    ((65, 96, 0, 95, 5), 96, 12, 1), ((65, 96, 0, 95, 5), 96, 1, 6),
    ((97, 128, 0, 127, 5), 128, 5, 1), ((97, 128, 0, 127, 5), 128, 12, 6),
    ((1,), 1, 5, 6),
]
MASK_DTYPES = {"bool": torch.bool, "uint8": torch.uint8, "int64": torch.int64}


def _random_qkv(g, rows_shape, heads, amp, dtype):
    x = _randn(g, *rows_shape, 3, heads * DH)
    x[..., :2, :] *= amp
    return x.reshape(*rows_shape, 3 * heads * DH).to(dtype)


@functools.lru_cache(maxsize=None)
def random_padded(spec, storage):
    S, B, heads, amp, kind, mdt = spec
    g = _gen("random", spec, storage)
    qkv = _random_qkv(g, (B, S), heads, amp, DTYPES[storage])
    if kind == "hole":
        mask = hole_mask(g, B, S)
    elif kind == "prefix":
        mask = prefix_mask(torch.randint(1, S + 1, (B,), generator=g).tolist(), S)
    else:
        mask = None
    ref, A = attn_ref(qkv, heads, mask)
    ref32 = attn_ref(qkv, heads, mask, torch.float32)[0]
    return dict(qkv=qkv, mask=None if mask is None else mask.to(MASK_DTYPES[mdt]), heads=heads, ref=ref, A=A,
                ref32=ref32, storage=storage)


@functools.lru_cache(maxsize=None)
def random_varlen(spec, storage):
    lens, max_len, heads, amp = spec
    g = _gen("random_varlen", spec, storage)
    qkv = _random_qkv(g, (sum(lens),), heads, amp, DTYPES[storage])
    ref, A = varlen_ref(qkv, lens, heads)
    ref32 = varlen_ref(qkv, lens, heads, torch.float32)[0]
    return dict(qkv=qkv, lens=lens, cu=cu_of(lens), max_len=max_len, heads=heads, ref=ref, A=A, ref32=ref32,
                storage=storage)


def spec_id(spec):
    return "-".join("x".join(map(str, s)) if isinstance(s, tuple) else str(s) for s in spec)


# ------------------------------------------------------------------------------------------ LayerNorm
LN_H = (256, 512, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 9)          # four rows per workgroup: full groups and every tail
LN_FAMILIES = ("randn", "offset", "constant", "large")


def ulp_bf16(r):
    """Spacing of bf16 at |r| (normal range): 2^(floor(log2 |r|) - 7)."""
    e = torch.frexp(r.double().abs())[1].clamp_min(-125)       # |r| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(r, dtype=torch.float64), e - 8)


def ln_ref64(e, w, b, eps=EPS):
    """fp64 LayerNorm of the rows of e (already fp64) and the fp32-arithmetic allowance
    s = 4 * 2^-24 * max_j |e_ij| * rstd_i * |w_j| + 2e-5: the fp32 error of the row mean amplified by rstd * w
    (it matters for offset and constant rows only), plus the suite's fp32 LayerNorm atol."""
    H = e.shape[-1]
    w, b = w.double(), b.double()
    mean = e.sum(-1, keepdim=True) / H
    d = e - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / H + eps)
    s = 4 * 2.0 ** -24 * e.abs().amax(-1, keepdim=True) * rstd * w.abs() + 2e-5
    return d * rstd * w + b, s


def ln_ratio(out, ref, s, storage):
    """Largest err / bound: fp32 output within s, bf16 output within 0.5 ulp_bf16(ref64) + s."""
    if not torch.isfinite(out).all():
        return math.inf
    bound = s + (0.5 * ulp_bf16(ref) if storage == "bf16" else 0.0)
    return ((out.double() - ref).abs() / bound).max().item()


def ln_inputs(g, family, rows, H, dtype):
    """x, y [rows, H] whose sum follows the row family; w, b [H]."""
    if family == "randn":
        x, y = _randn(g, rows, H), 0.5 * _randn(g, rows, H) + 0.1
    elif family == "offset":                                     # mean 64, std 0.5
        x, y = 64 + 0.45 * _randn(g, rows, H), 0.2 * _randn(g, rows, H)
    elif family == "constant":                                   # variance 0: ref64 is exactly the bias
        x = (3 * _randn(g, rows, 1)).expand(rows, H).clone()     # (y = x: the fp64 row sums stay exact)
        y = x.clone()
    else:                                                        # large
        x, y = 1e4 * _randn(g, rows, H), 1e4 * _randn(g, rows, H)
    w = 1 + 0.1 * _randn(g, H)
    b = 0.1 * _randn(g, H)
    return x.to(dtype), y.to(dtype), w.to(dtype), b.to(dtype)


@functools.lru_cache(maxsize=None)
def ln_case(family, rows, H, storage, broadcast):
    g = _gen("ln", family, rows, H, storage, broadcast)
    x, y, w, b = ln_inputs(g, family, rows, H, DTYPES[storage])
    if broadcast:
        y = y[0].clone()                                         # one [H] row added to every row
    ref, s = ln_ref64(x.double() + y.double(), w, b)
    return dict(x=x, y=y, w=w, b=b, ref=ref, s=s, storage=storage, family=family)


EMBED_T = (1, 5, 130)
EMBED_V, EMBED_P = 50, 131


@functools.lru_cache(maxsize=None)
def embed_case(H, T, storage, ids_dtype="int64"):
    """ids / pos_ids hit the last row of each table, and row 0 once T allows it.  bf16 reference: the two
    adds rounded to bf16 (the kernel's documented contract, the bf16 PyTorch expression), then ln_ref64."""
    dtype = DTYPES[storage]
    g = _gen("embed", H, T, storage)
    tok, pos, typ = (0.5 * _randn(g, n, H) for n in (EMBED_V, EMBED_P, 1))
    tok, pos, typ = tok.to(dtype), pos.to(dtype), typ.to(dtype)
    w, b = (1 + 0.1 * _randn(g, H)).to(dtype), (0.1 * _randn(g, H)).to(dtype)
    ids = torch.randint(0, EMBED_V, (T,), generator=g)
    pid = torch.randint(0, EMBED_P, (T,), generator=g)
    ids[T - 1], pid[T - 1] = EMBED_V - 1, EMBED_P - 1
    if T > 1:
        ids[0], pid[0] = 0, 0
    if storage == "bf16":
        e = ((tok[ids].double() + pos[pid].double()).to(dtype).double() + typ[0].double()).to(dtype).double()
    else:
        e = (tok[ids].double() + pos[pid].double()) + typ[0].double()
    ref, s = ln_ref64(e, w, b)
    idt = {"int64": torch.int64, "int32": torch.int32}[ids_dtype]
    return dict(ids=ids.to(idt), pid=pid.to(idt), tok=tok, pos=pos, typ=typ, w=w, b=b, ref=ref, s=s, storage=storage)


# ------------------------------------------------------------------------------------------ segment mean
# every partial-sum group count G = min(8, 256 / chunks) the launchers can choose (chunks = H/8 bf16, H/4 fp32),
# and one width per dtype that takes the ATen path
SEG_H = {"bf16": (8, 64, 256, 512, 768, 1024, 2048, 12), "fp32": (4, 64, 256, 512, 768, 1024, 6)}
SEG_LENS = (0, 1, 7, 0, 8, 9, 128, 0)      # empty segments first, in the middle and last


def seg_groups(H, storage):
    """The kernel's G for this width, None where the op falls back to ATen."""
    per = 8 if storage == "bf16" else 4
    if H % per or H // per > 256:
        return None
    return min(8, 256 // (H // per))


@functools.lru_cache(maxsize=None)
def seg_case(H, storage):
    """ref64 and the bound L * 2^-24 * mean|x| (fp32 sums of L terms), + 0.5 ulp_bf16 for a bf16 output."""
    g = _gen("seg", H, storage)
    T = sum(SEG_LENS)
    x = _randn(g, T, H).to(DTYPES[storage])
    ref = torch.zeros(len(SEG_LENS), H, dtype=torch.float64)
    bound = torch.zeros(len(SEG_LENS), H, dtype=torch.float64)
    lo = 0
    for i, L in enumerate(SEG_LENS):
        if L:
            seg = x[lo:lo + L].double()
            ref[i] = seg.sum(0) / L
            bound[i] = L * 2.0 ** -24 * seg.abs().sum(0) / L
        lo += L
    if storage == "bf16":
        bound = bound + 0.5 * ulp_bf16(ref)
    empty = torch.tensor([L == 0 for L in SEG_LENS])
    return dict(x=x, cu=cu_of(SEG_LENS), ref=ref, bound=bound, empty=empty, storage=storage)


def seg_ratio(out, c):
    """Largest err / bound over the non-empty segments; empty segments must be exactly 0 (else inf)."""
    if not torch.isfinite(out).all() or (out[c["empty"]] != 0).any():
        return math.inf
    live = ~c["empty"]
    return ((out[live].double() - c["ref"][live]).abs() / c["bound"][live]).max().item()


# ------------------------------------------------------------------------------------------ running a case
# `ops` is the op namespace under test (svoc.ops.ops()), `device` where its inputs go: "cpu" reaches the
# ATen paths, "cuda" the HIP kernels.  The results come back on the CPU.
def run_padded(ops, c, device, qkv=None, mask="case"):
    mask = c["mask"] if isinstance(mask, str) else mask
    qkv = c["qkv"] if qkv is None else qkv
    return ops.attention_qkv(qkv.to(device), None if mask is None else mask.to(device), c["heads"]).cpu()


def run_varlen(ops, c, device, qkv=None):
    qkv = c["qkv"] if qkv is None else qkv
    return ops.attention_varlen(qkv.to(device), c["cu"].to(device), c["max_len"], c["heads"]).cpu()


def run_add_layernorm(ops, c, device, dtype=None):
    """dtype: run the case's values in another dtype (the output is rounded back to the case's)."""
    x, y, w, b = (c[k].to(device, dtype) for k in "xywb")
    return ops.add_layernorm(x, y, w, b, EPS).cpu().to(c["x"].dtype)


def run_embed_layernorm(ops, c, device):
    a = [c[k].to(device) for k in ("ids", "pid", "tok", "pos", "typ", "w", "b")]
    return ops.embed_layernorm(*a, EPS).cpu()


def run_segment_mean(ops, c, device):
    return ops.segment_mean(c["x"].to(device), c["cu"].to(device)).cpu()


# ------------------------------------------------------------------------------------------ sharpness
@functools.lru_cache(maxsize=None)
def flat_case(v_amp=1.0, S=128, B=2, heads=3):
    """bf16, Q and K = 0.1 * randn (a flat softmax: every key weighs about 1/n), V = v_amp * randn, hole
    mask: the input on which one wrong key moves the output least.  test_encoder_cases.py builds wrong
    outputs on it that the replaced rtol = atol = 3e-2 accepts and attn_ratio() rejects."""
    g = _gen("flat", v_amp, S)
    x = _randn(g, B, S, 3, heads * DH)
    x[:, :, :2] *= 0.1
    x[:, :, 2] *= v_amp
    qkv = x.reshape(B, S, 3 * heads * DH).to(torch.bfloat16)
    mask = hole_mask(g, B, S, 0.85)
    ref, A = attn_ref(qkv, heads, mask)
    return dict(qkv=qkv, mask=mask, heads=heads, ref=ref, A=A, ref32=attn_ref(qkv, heads, mask, torch.float32)[0],
                storage="bf16")
