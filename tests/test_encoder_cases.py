"""The encoder cases of encoder_cases.py without a GPU: the constructions, the CPU ops, the checks' sharpness.

1. The constructions are what they claim: ref64 of the one-hot cases is the picked V row and ref64 of the
   uniform cases is sum / n, exactly; the score gap, the constant rows, the segment widths are asserted as
   preconditions (conditions, not measurements: a seed that misses one gets replaced, never a wider bound).
2. The project's CPU ops (the ATen paths of csrc/bindings/encoder_ops.cpp) pass every exact case and every
   bound: the reference side alone stays inside the bounds, and the CPU fallback is pinned.
3. The checks are sharp: wrong outputs built here, each one accepted by the rtol = atol = 3e-2 the
   attention tests used to have, are rejected.  test_encoder_adversarial_gpu.py runs the same cases and
   checkers on the HIP kernels.
"""
import pytest
import torch
import torch.nn.functional as F

import encoder_cases as ec
from svoc import ops as svops

STORAGES = ("bf16", "fp32")


def _qkv_parts(c):
    B, S, _ = c["qkv"].shape
    return c["qkv"].view(B, S, 3, c["heads"], ec.DH).permute(2, 0, 3, 1, 4)      # [3, B, heads, S, 64]


# ---------------------------------------------------------------------------------------- 1. constructions
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "holes"])
def test_onehot_padded_construction(S, storage, masked):
    c = ec.onehot_padded(S, storage, masked)
    rows, keep = c["rows"], c["rows"][:, None, None, :]
    if masked:                                         # scattered zeros, not a prefix
        m = c["mask"].bool()
        assert (~m).any(1).all() and (m[:, 1:] & ~m[:, :-1]).any(1).all()
    for dtype in (torch.float64, torch.float32):
        q, k, _ = _qkv_parts(c).to(dtype)
        s = (q @ k.transpose(-1, -2) / 8).masked_fill(~keep, ec.NEG_INF)
        top = s.topk(2, -1).values.transpose(1, 2)[rows]                        # attended query rows
        assert (top[..., 0] == 512).all()
        if top.shape[-1] > 1:
            assert (top[..., 0] - top[..., 1] >= 144).all()
        ref = ec.attn_ref(c["qkv"], c["heads"], c["mask"], dtype)[0]
        assert torch.equal(ref[rows], c["expect"].to(dtype)[rows])
    p32 = torch.softmax(s.float(), -1).transpose(1, 2)[rows]
    assert ((p32 > 0).sum(-1) == 1).all() and (p32.max(-1).values == 1).all()   # exactly one-hot in fp32
    assert (c["expect"][rows] != 0).all()              # (a zero would hide a sign or a dropped product)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_onehot_varlen_construction(S, storage):
    c = ec.onehot_varlen(S, storage)
    assert set(c["lens"]) >= {S, 1, S - 31, 0} and 0 < c["lens"][-1] < 32 and c["expect"].shape[0] == sum(c["lens"])
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(ec.varlen_ref(c["qkv"], c["lens"], c["heads"], dtype)[0], c["expect"].to(dtype))


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_uniform_construction(S, storage):
    dtype = ec.DTYPES[storage]
    for n in ec.uniform_counts(S):
        c = ec.uniform_padded(S, n, storage)
        assert n & (n - 1) == 0 and (c["mask"] is None) == (n == S)
        if c["mask"] is not None:
            assert (c["mask"].sum(1) == n).all()
        q, k, v = _qkv_parts(c)
        assert (q == 0).all() and k.float().abs().max() > 50 and (v.float() == v.float().round()).all()
        ref = ec.attn_ref(c["qkv"], c["heads"], c["mask"])[0]
        assert torch.equal(ref.to(dtype), c["expect"])
        if storage == "fp32":
            assert torch.equal(ref, c["expect"].double())
    c = ec.uniform_varlen(S, storage)
    assert all(L & (L - 1) == 0 for L in c["lens"]) and max(c["lens"]) <= S and (S - 1) // 32 == (c["max_len"] - 1) // 32
    assert torch.equal(ec.varlen_ref(c["qkv"], c["lens"], c["heads"])[0].to(dtype), c["expect"])


def test_uniform_varlen_covers_every_power_of_two():
    assert {L for S in ec.SEQ for L in ec.uniform_lens(S)} == {1, 2, 4, 8, 16, 32, 64, 128}


def test_random_matrix_covers_the_issue():
    P, V = ec.RANDOM_PADDED, ec.RANDOM_VARLEN
    assert {(s[0], s[3]) for s in P} == {(S, a) for S in ec.SEQ for a in (1, 6)}
    assert {s[2] for s in P} == {1, 5, 12} and {s[1] for s in P} == {1, 3}
    assert {s[4] for s in P} == {"hole", "prefix", "none"} and {s[5] for s in P} >= {"bool", "uint8", "int64"}
    lens = {L for s in V for L in s[0]}
    assert lens == {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 0, 5}
    assert {(s[1] + 31) // 32 for s in V} == {1, 2, 3, 4} and any(s[1] % 32 for s in V if s[1] > 1)
    assert any(sum(s[0]) == 1 for s in V)
    for s in V:
        if len(s[0]) > 1:
            assert s[0][-1] == 5 and 0 in s[0][1:-1] and max(s[0]) == s[1]
    assert {s[2] for s in V} == {1, 5, 12} and {s[3] for s in V} == {1, 6}


def test_amp6_scores_are_large():
    c = ec.random_padded(ec.RANDOM_PADDED[-1], "bf16")
    q, k, _ = _qkv_parts(c).double()
    assert (q @ k.transpose(-1, -2) / 8).abs().max() > 100


def test_layernorm_reference_and_families():
    for storage in STORAGES:
        c = ec.ln_case("randn", 5, 768, storage, False)
        e = c["x"].double() + c["y"].double()
        torch.testing.assert_close(c["ref"], F.layer_norm(e, (768,), c["w"].double(), c["b"].double(), ec.EPS),
                                   rtol=1e-12, atol=1e-12)
        c = ec.ln_case("offset", 9, 512, storage, False)
        e = c["x"].double() + c["y"].double()
        assert (e.mean(-1) - 64).abs().max() < 0.2 and (e.std(-1) - 0.5).abs().max() < 0.1
        for broadcast in (False, True):
            c = ec.ln_case("constant", 9, 1024, storage, broadcast)
            e = c["x"].double() + c["y"].double()
            assert (e == e[:, :1]).all() and e[:, 0].unique().numel() == 9
            assert torch.equal(c["ref"], c["b"].double().expand(9, 1024))          # exactly the bias
        c = ec.ln_case("large", 4, 256, storage, True)
        assert c["y"].shape == (256,) and c["x"].float().abs().max() > 1e4
    r = torch.tensor([1.0, 1.5, 1.9999, 2.0, -0.75, 3e-3])
    assert torch.equal(ec.ulp_bf16(r), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -16],
                                                    dtype=torch.float64))


def test_embed_and_segment_cases():
    for storage in STORAGES:
        for T in ec.EMBED_T:
            c = ec.embed_case(768, T, storage)
            assert c["ids"][-1] == ec.EMBED_V - 1 and c["pid"][-1] == ec.EMBED_P - 1 and (T == 1 or c["ids"][0] == 0 == c["pid"][0])
        assert ec.embed_case(256, 5, storage, "int32")["ids"].dtype == torch.int32
        assert {ec.seg_groups(H, storage) for H in ec.SEG_H[storage]} == {1, 2, 4, 8, None}
        c = ec.seg_case(64, storage)
        assert c["empty"].tolist() == [L == 0 for L in ec.SEG_LENS] and (c["ref"][c["empty"]] == 0).all()
    assert ec.SEG_LENS[0] == ec.SEG_LENS[-1] == 0 and 0 in ec.SEG_LENS[1:-1] and set(ec.SEG_LENS) == {0, 1, 7, 8, 9, 128}


# ---------------------------------------------------------------------------------------- 2. the CPU ops
def _equal_rows(out, c):
    rows = c.get("rows")
    assert out.dtype == c["expect"].dtype
    assert torch.equal(out, c["expect"]) if rows is None else torch.equal(out[rows], c["expect"][rows])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("S", ec.SEQ)
def test_cpu_ops_exact_cases(S, storage):
    ops = svops.ops()
    for masked in (False, True):
        _equal_rows(ec.run_padded(ops, ec.onehot_padded(S, storage, masked), "cpu"), ec.onehot_padded(S, storage, masked))
    _equal_rows(ec.run_varlen(ops, ec.onehot_varlen(S, storage), "cpu"), ec.onehot_varlen(S, storage))
    for n in ec.uniform_counts(S):
        _equal_rows(ec.run_padded(ops, ec.uniform_padded(S, n, storage), "cpu"), ec.uniform_padded(S, n, storage))
    _equal_rows(ec.run_varlen(ops, ec.uniform_varlen(S, storage), "cpu"), ec.uniform_varlen(S, storage))
    c = ec.isolation_varlen(S, storage)
    a, b = ec.run_varlen(ops, c, "cpu"), ec.run_varlen(ops, c, "cpu", qkv=c["other"])
    assert all(torch.equal(a[t], b[t]) for t in c["targets"]) and not torch.equal(a, b)
    c = ec.isolation_padded(S, storage)
    a, b = ec.run_padded(ops, c, "cpu"), ec.run_padded(ops, c, "cpu", qkv=c["other"])
    assert torch.equal(a[c["rows"]], b[c["rows"]]) and torch.isfinite(b.float()).all() and not torch.equal(a, b)


@pytest.mark.parametrize("storage", STORAGES)
def test_cpu_ops_random_attention(storage):
    ops = svops.ops()
    for spec in ec.RANDOM_PADDED:
        c = ec.random_padded(spec, storage)
        assert ec.attn_ratio(ec.run_padded(ops, c, "cpu"), c["ref"], c["A"], storage, c["ref32"]) <= 1, spec
    for spec in ec.RANDOM_VARLEN:
        c = ec.random_varlen(spec, storage)
        assert ec.attn_ratio(ec.run_varlen(ops, c, "cpu"), c["ref"], c["A"], storage, c["ref32"]) <= 1, spec


@pytest.mark.parametrize("storage", STORAGES)
def test_cpu_ops_layernorm_embed_mean(storage):
    """The bf16 add_layernorm case runs through the CPU op in fp32 and is rounded to bf16 at the end: on bf16
    tensors the ATen path rounds x + y to bf16 before it normalises (PyTorch's bf16 semantics), which the
    kernel's fp32 add and this reference do not."""
    ops = svops.ops()
    for family in ec.LN_FAMILIES:
        for H in ec.LN_H:
            for rows in ec.LN_ROWS:
                for broadcast in (False, True):
                    c = ec.ln_case(family, rows, H, storage, broadcast)
                    out = ec.run_add_layernorm(ops, c, "cpu", torch.float32)
                    assert ec.ln_ratio(out, c["ref"], c["s"], storage) <= 1, (family, H, rows, broadcast)
    for H in ec.LN_H:
        for T, idt in [(1, "int64"), (5, "int32"), (130, "int64")]:
            c = ec.embed_case(H, T, storage, idt)
            assert ec.ln_ratio(ec.run_embed_layernorm(ops, c, "cpu"), c["ref"], c["s"], storage) <= 1, (H, T)
    for H in ec.SEG_H[storage]:
        c = ec.seg_case(H, storage)
        assert ec.seg_ratio(ec.run_segment_mean(ops, c, "cpu"), c) <= 1, H


# ---------------------------------------------------------------------------------------- 3. sharpness
def _rejected_but_formerly_accepted(c, wrong):
    """wrong: a bf16 output for case c.  The replaced tolerance accepts it, the bound does not."""
    assert ec.old_tolerance_accepts(wrong, c["ref32"]), (wrong.double() - c["ref"]).abs().max()
    ratio = ec.attn_ratio(wrong, c["ref"], c["A"], "bf16")
    assert ratio > 1, ratio
    return ratio


def _mutated(c, mask=None, qkv=None, scale=0.125):
    """The correctly rounded bf16 output of a mutated problem."""
    return ec.attn_ref(c["qkv"] if qkv is None else qkv, c["heads"], c["mask"] if mask is None else mask,
                       scale=scale)[0].to(torch.bfloat16)


def test_correct_output_passes_both():
    for c in (ec.flat_case(), ec.flat_case(0.02), ec.random_padded(ec.RANDOM_PADDED[0], "bf16")):
        good = c["ref"].to(torch.bfloat16)
        assert ec.old_tolerance_accepts(good, c["ref32"]) and ec.attn_ratio(good, c["ref"], c["A"], "bf16") <= 0.5


def test_leaked_masked_key_is_rejected():
    """One masked key (the first hole) attended, on the flat-softmax case where it moves the output least
    (about |v| / n): inside 3e-2, several times the bound.  The uniform case rejects it as well: the
    integer sum changes."""
    c = ec.flat_case()
    k = int((c["mask"][0] == 0).nonzero()[0])
    mask = c["mask"].clone()
    mask[0, k] = 1
    assert _rejected_but_formerly_accepted(c, _mutated(c, mask=mask)) > 2
    u = ec.uniform_padded(128, 16, "bf16")
    mask = u["mask"].clone()
    mask[0, int((mask[0] == 0).nonzero()[0])] = 1
    assert not torch.equal(_mutated(u, mask=mask), u["expect"])


def test_dropped_attended_key_is_rejected():
    c = ec.flat_case()
    k = int((c["mask"][0] != 0).nonzero()[0])
    mask = c["mask"].clone()
    mask[0, k] = 0
    assert _rejected_but_formerly_accepted(c, _mutated(c, mask=mask)) > 2
    u = ec.uniform_padded(128, 16, "bf16")
    mask = u["mask"].clone()
    mask[0, int((mask[0] != 0).nonzero()[0])] = 0
    assert not torch.equal(_mutated(u, mask=mask), u["expect"])


def test_swapped_v_row_halves_are_rejected():
    """The two 16-byte halves (8 bf16 each) of one V row of one head swapped: a wrong swizzle term for one
    chunk.  Inside 3e-2 on the flat case, outside the bound; the one-hot case sees it bit for bit."""
    for c, check in ((ec.flat_case(), None), (ec.onehot_padded(128, "bf16", False), "equal")):
        B, S, _ = c["qkv"].shape
        k = 0 if c["mask"] is None else int((c["mask"][0] != 0).nonzero()[0])
        qkv = c["qkv"].clone()
        v = qkv.view(B, S, 3, c["heads"], ec.DH)[0, k, 2, 0]
        v[0:8], v[8:16] = c["qkv"].view(B, S, 3, c["heads"], ec.DH)[0, k, 2, 0, 8:16], \
            c["qkv"].view(B, S, 3, c["heads"], ec.DH)[0, k, 2, 0, 0:8]
        assert not torch.equal(qkv, c["qkv"])
        wrong = _mutated(c, qkv=qkv)
        if check is None:
            assert _rejected_but_formerly_accepted(c, wrong) > 1.5
        else:
            assert not torch.equal(wrong[c["rows"]], c["expect"][c["rows"]])


def test_score_scale_off_by_two_percent_is_rejected():
    """1.02 / 8: invisible on a flat softmax and in the exact cases' margins, inside 3e-2 on randn inputs
    (amp = 1), outside the bound there; at amp = 6 it is far outside."""
    for spec in ec.RANDOM_PADDED:
        if spec[3] == 1:
            c = ec.random_padded(spec, "bf16")
            assert _rejected_but_formerly_accepted(c, _mutated(c, scale=0.125 * 1.02)) > 1.5, spec
    c = ec.random_padded(ec.RANDOM_PADDED[3], "bf16")                            # amp = 6
    assert ec.attn_ratio(_mutated(c, scale=0.125 * 1.02), c["ref"], c["A"], "bf16") > 10


def test_head_written_at_another_offset_is_rejected():
    """Heads 0 and 1 of one sequence exchanged.  On randn V the replaced tolerance does see this; it has no
    scale, though, and accepts any output once the values are small: with V of the size of the embedding
    tables (0.02 * randn) the exchange is inside 3e-2 and hundreds of times the bound.  The one-hot case
    rejects it bit for bit (and ran only with heads = 12 before, where b = bh / 12 was never anything else)."""
    c = ec.flat_case(0.02)
    wrong = c["ref"].to(torch.bfloat16)
    wrong[0, :, 0:64], wrong[0, :, 64:128] = wrong[0, :, 64:128].clone(), wrong[0, :, 0:64].clone()
    assert _rejected_but_formerly_accepted(c, wrong) > 50
    c = ec.onehot_padded(32, "bf16", True)
    wrong = c["expect"].clone()
    wrong[1, :, 0:64], wrong[1, :, 64:128] = c["expect"][1, :, 64:128], c["expect"][1, :, 0:64]
    assert not torch.equal(wrong[c["rows"]], c["expect"][c["rows"]])
