"""The HIP encoder kernels (csrc/kernels/encoder_ops.hip) on the cases of encoder_cases.py.

Exact cases use torch.equal, bounded cases the derived bounds of encoder_cases (attn_ratio, ln_ratio,
seg_ratio): a ratio err / bound above 1 fails.  test_encoder_cases.py runs the same cases through the CPU
ops and shows that the checks reject subtly wrong outputs.  Each test prints its largest ratio.

Largest err / bound observed on an MI355X (all cases of this file):
  attention padded      bf16 0.753   fp32 0.323
  attention varlen      bf16 0.791   fp32 0.484
  add_layernorm         bf16 0.997   fp32 0.540
  embed_layernorm       bf16 0.997   fp32 0.033
  segment_mean          bf16 1.000   fp32 0.383
(The bf16 LayerNorm and mean ratios sit just under 1 by construction: their bound is dominated by the half
ulp of the output rounding, which a correctly rounded output comes arbitrarily close to.)
"""
import pytest
import torch

import encoder_cases as ec
from svoc import ops as svops

pytestmark = pytest.mark.gpu

STORAGES = ("bf16", "fp32")
DEV = "cuda"


def _equal_rows(out, c, what):
    rows = c.get("rows")
    got, want = (out, c["expect"]) if rows is None else (out[rows], c["expect"][rows])
    assert out.dtype == c["expect"].dtype and out.shape == c["expect"].shape
    assert torch.equal(got, want), (what, (got.double() - want.double()).abs().max().item())


# ---------------------------------------------------------------------------------------- attention, exact
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "holes"])
def test_onehot_padded(S, storage, masked):
    """P is exactly one-hot: every attended query row equals the V row its permutation picks, bit for bit
    (K / V staging and swizzle, transposed reads, P as the A operand, the output layout)."""
    c = ec.onehot_padded(S, storage, masked)
    _equal_rows(ec.run_padded(svops.ops(), c, DEV), c, "onehot padded")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_onehot_varlen(S, storage):
    """Packed segments of S, 1, S - 31, 0 and 5 tokens: every row equals its picked V row."""
    c = ec.onehot_varlen(S, storage)
    _equal_rows(ec.run_varlen(svops.ops(), c, DEV), c, "onehot varlen")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_uniform_padded(S, storage):
    """Q = 0, n scattered attended keys (n a power of two), integer V: the output is exactly sum / n.
    A dropped, duplicated or leaked key changes the integer sum.  (S = 96 is no power of two: its largest
    count is 64, and the unmasked S = 96 call is held to the random-case bound instead.)"""
    for n in ec.uniform_counts(S):
        c = ec.uniform_padded(S, n, storage)
        _equal_rows(ec.run_padded(svops.ops(), c, DEV), c, "uniform padded n=%d" % n)
    if S == 96:
        c = ec.uniform_padded(S, 64, storage)
        ref, A = ec.attn_ref(c["qkv"], c["heads"])
        ref32 = ec.attn_ref(c["qkv"], c["heads"], None, torch.float32)[0]
        r = ec.attn_ratio(ec.run_padded(svops.ops(), c, DEV, mask=None), ref, A, storage, ref32)
        assert r <= 1, r


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_uniform_varlen(S, storage):
    """Q = 0 over packed segments of power-of-two lengths 1 .. 128: exactly sum / L."""
    c = ec.uniform_varlen(S, storage)
    _equal_rows(ec.run_varlen(svops.ops(), c, DEV), c, "uniform varlen")


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_isolation_varlen(S, storage):
    """Every row of every other segment replaced by 1e4 * randn: the rows of a segment whose last key block
    is completed by its neighbour's rows, and of the short final segment (rows past the buffer are
    clamped), are bit-identical.  Finite values only: non-finite inputs (0 * Inf) are out of scope."""
    c = ec.isolation_varlen(S, storage)
    a = ec.run_varlen(svops.ops(), c, DEV)
    b = ec.run_varlen(svops.ops(), c, DEV, qkv=c["other"])
    for t in c["targets"]:
        assert torch.isfinite(a[t].float()).all() and torch.equal(a[t], b[t]), t


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_isolation_padded(S, storage):
    """Q / K / V replaced at the masked positions of one sequence and everywhere in the others: its attended
    query rows are bit-identical.  Finite values only: non-finite inputs (0 * Inf) are out of scope."""
    c = ec.isolation_padded(S, storage)
    a = ec.run_padded(svops.ops(), c, DEV)
    b = ec.run_padded(svops.ops(), c, DEV, qkv=c["other"])
    assert torch.isfinite(a[c["rows"]].float()).all() and torch.equal(a[c["rows"]], b[c["rows"]])


# ---------------------------------------------------------------------------------------- attention, bounded
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("spec", ec.RANDOM_PADDED, ids=ec.spec_id)
def test_random_padded(spec, storage):
    """amp * randn (|score| up to about 150 at amp = 6), heads 1 / 5 / 12, prefix and hole masks as bool,
    uint8 and int64, against ref64: bf16 |err| <= 2.25 u A per element, fp32 max |err| <= max(2e-5, 4 e_model).
    Largest err / bound observed: bf16 0.753, fp32 0.323."""
    c = ec.random_padded(spec, storage)
    out = ec.run_padded(svops.ops(), c, DEV)
    assert out.dtype == ec.DTYPES[storage] and out.shape == c["ref"].shape
    r = ec.attn_ratio(out, c["ref"], c["A"], storage, c["ref32"])
    print("attention padded %s %s: err/bound %.3f" % (storage, ec.spec_id(spec), r))
    assert r <= 1, r


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("spec", ec.RANDOM_VARLEN, ids=ec.spec_id)
def test_random_varlen(spec, storage):
    """Segment lengths on both sides of every block edge, an empty segment, a short last one, max_len = 33,
    a batch of one token; same bounds.  Largest err / bound observed: bf16 0.791, fp32 0.484."""
    c = ec.random_varlen(spec, storage)
    out = ec.run_varlen(svops.ops(), c, DEV)
    assert out.dtype == ec.DTYPES[storage] and out.shape == c["ref"].shape
    r = ec.attn_ratio(out, c["ref"], c["A"], storage, c["ref32"])
    print("attention varlen %s %s: err/bound %.3f" % (storage, ec.spec_id(spec), r))
    assert r <= 1, r


@pytest.mark.parametrize("storage", STORAGES)
def test_fully_masked_sequence(storage):
    """A sequence with an all-zero mask row is NaN (-inf - -inf, as ATen's softmax of all -inf), on the GPU
    and in the CPU op; every other sequence is bit-identical to the same call without it."""
    c = ec.random_padded(ec.RANDOM_PADDED[0], storage)
    mask = c["mask"].clone()
    mask[1] = 0
    out = ec.run_padded(svops.ops(), c, DEV, mask=mask)
    cpu = ec.run_padded(svops.ops(), c, "cpu", mask=mask)
    assert torch.isnan(out[1]).all() and torch.isnan(cpu[1]).all()
    keep = [0, 2]
    alone = ec.run_padded(svops.ops(), c, DEV, qkv=c["qkv"][keep], mask=c["mask"][keep])
    assert torch.equal(out[keep], alone) and torch.isfinite(alone.float()).all()


# ---------------------------------------------------------------------------------------- LayerNorm, pooling
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("H", ec.LN_H)
@pytest.mark.parametrize("family", ec.LN_FAMILIES)
def test_add_layernorm(family, H, storage):
    """rows 1 / 3 / 4 / 5 / 9 (four rows per workgroup), y full or one [H] row, against the fp64 LayerNorm:
    fp32 within s, bf16 within 0.5 ulp_bf16(ref64) + s (encoder_cases.ln_ref64)."""
    worst = 0.0
    for rows in ec.LN_ROWS:
        for broadcast in (False, True):
            c = ec.ln_case(family, rows, H, storage, broadcast)
            out = ec.run_add_layernorm(svops.ops(), c, DEV)
            assert out.dtype == ec.DTYPES[storage] and out.shape == c["x"].shape
            worst = max(worst, ec.ln_ratio(out, c["ref"], c["s"], storage))
    print("add_layernorm %s %s H=%d: err/bound %.3f" % (storage, family, H, worst))
    assert worst <= 1, worst


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("H", ec.LN_H)
def test_embed_layernorm(H, storage):
    """T 1 / 5 / 130 with the first and last row of both tables; int32 ids once."""
    worst = 0.0
    for T, idt in [(1, "int64"), (5, "int32"), (130, "int64")]:
        c = ec.embed_case(H, T, storage, idt)
        out = ec.run_embed_layernorm(svops.ops(), c, DEV)
        assert out.dtype == ec.DTYPES[storage] and out.shape == (T, H)
        worst = max(worst, ec.ln_ratio(out, c["ref"], c["s"], storage))
    print("embed_layernorm %s H=%d: err/bound %.3f" % (storage, H, worst))
    assert worst <= 1, worst


@pytest.mark.parametrize("storage,H", [(s, H) for s in STORAGES for H in ec.SEG_H[s]])
def test_segment_mean(storage, H):
    """Every partial-sum group count G the launchers choose and one ATen width, segments of 0 / 1 / 7 / 0 / 8 / 9 /
    128 / 0 rows: within L * 2^-24 * mean|x| (+ 0.5 ulp_bf16), empty segments exactly 0."""
    c = ec.seg_case(H, storage)
    out = ec.run_segment_mean(svops.ops(), c, DEV)
    assert out.dtype == ec.DTYPES[storage] and out.shape == c["ref"].shape
    r = ec.seg_ratio(out, c)
    print("segment_mean %s H=%d G=%s: err/bound %.3f" % (storage, H, ec.seg_groups(H, storage), r))
    assert r <= 1, r


def test_segment_mean_widths_cover_every_group_count():
    for storage in STORAGES:
        assert {ec.seg_groups(H, storage) for H in ec.SEG_H[storage]} == {1, 2, 4, 8, None}
