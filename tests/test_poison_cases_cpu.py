"""CPU side of tests/test_gpu_poison.py: the masks of tests/poison_cases.py mark nothing an fp64 reference reads, every case of the GPU
tests keeps every read the contract allows inside its own tensors, and poisoned_empty puts torch back as it found it."""
import pytest
import torch

import attn_cases as ac
import poison_cases as pc
import wavlm_cases as wc

ALL_LAYOUTS = [(n, pc.GEOMETRIES) for n in pc.GEOMETRIES] + [(n, pc.DRIVER_GEOMETRIES) for n in pc.DRIVER_GEOMETRIES]


def _heads(x, H):
    """[n, H 64] -> [H, n, 64] fp64"""
    return x.double().view(x.shape[0], H, 64).transpose(0, 1)


def _reference(lay, qk, vt, gate, table):
    """attn_cases.fwd_ref (plain) and wavlm_cases.biased_attention_ref (gate x table) on the tensors cut to the valid rows and keys"""
    outs = []
    for q, k, v, g in pc.cut_to_valid(lay, qk, vt, gate):
        n = q.shape[0]
        f = ac.fwd_ref(_heads(q, lay.H), _heads(k, lay.H), _heads(v, lay.H), torch.ones(1, n, n, dtype=torch.bool))
        outs += [f["out"], f["lse2"]]
        for h in range(lay.H):
            c = slice(64 * h, 64 * h + 64)
            outs.append(wc.biased_attention_ref(q[:, c].double(), k[:, c].double(), v[:, c].double(), 0.125, g[h].double(), table[h].double(), n))
    return outs


@pytest.mark.parametrize("name,table", ALL_LAYOUTS)
def test_masks_are_disjoint_from_what_the_reference_reads(name, table):
    lay = pc.case_layout(name, table)
    ops = pc.operands(lay, seed=3, tmax=pc.TMAX)
    tab = wc.bias_table(torch.randn(wc.NUM_BUCKETS, lay.H, generator=torch.Generator().manual_seed(4)), pc.TMAX)
    clean = _reference(lay, ops["qk"], ops["vt"], ops["gate"], tab)
    qk = pc.poison_bf16(ops["qk"], lay.qk, pc.NONFINITE_POISON)
    vt = pc.poison_bf16(ops["vt"], lay.vt, pc.NONFINITE_POISON)
    gate = pc.poison_f32(ops["gate"], lay.gate, pc.NONFINITE_POISON)
    # the poison is really there: every masked element is non-finite, and nothing else is
    assert bool((~torch.isfinite(qk.float()) == lay.qk).all()) and bool((~torch.isfinite(vt.float()) == lay.vt).all())
    assert bool((~torch.isfinite(gate) == lay.gate).all())
    dirty = _reference(lay, qk, vt, gate, tab)
    assert all(bool(torch.isfinite(x).all()) for x in clean)
    assert all(pc.bits_equal(a, b) for a, b in zip(clean, dirty))
    # and the masks are the whole complement: what is left unmarked is exactly what the reference was given
    n_valid = sum(lay.lens)
    assert int((~lay.qk).sum()) == n_valid * 2 * lay.D and int((~lay.vt).sum()) == n_valid * lay.D
    assert int((~lay.gate).sum()) == n_valid * lay.H and int(lay.valid_rows.sum()) == n_valid
    assert int(lay.k.sum()) * 2 == int(lay.qk.sum()) and not bool(lay.k[:, : lay.D].any())


def test_finite_poison_is_finite_and_extreme():
    t = pc.poison_bf16(torch.zeros(8, dtype=torch.bfloat16), torch.ones(8, dtype=torch.bool), pc.FINITE_POISON).float()
    assert bool(torch.isfinite(t).all())
    big = float(torch.finfo(torch.bfloat16).max)
    assert t[:4].tolist() == [big, -big, 2.0 ** -133, -(2.0 ** -133)] and t[4:].tolist() == t[:4].tolist()
    f = pc.poison_f32(torch.zeros(4), torch.ones(4, dtype=torch.bool), pc.FINITE_POISON)
    assert f.tolist() == [big, -big, 2.0 ** -133, -(2.0 ** -133)]
    n = pc.poison_bf16(torch.zeros(4, dtype=torch.bfloat16), torch.ones(4, dtype=torch.bool), pc.NONFINITE_POISON).float()
    assert torch.isnan(n[0]) and n[1] == float("inf") and n[2] == -float("inf") and torch.isnan(n[3])


def test_vt_mask_at_pitch_56_includes_the_8_elements_behind_the_last_d_row():
    lay = pc.uniform_layout(56, [50, 50, 50], pc.H_ATT)
    end = lay.D * lay.rows                                       # one past the last d row of the last head of the last image
    assert lay.vt_numel == end + 64 and bool(lay.vt[end: end + 8].all())
    # key tile 0 of that d row: keys 50..55 are pad columns inside the pitch, keys 56..63 the 8 elements behind the row
    row = end - 56
    assert not bool(lay.vt[row: row + 50].any()) and bool(lay.vt[row + 50: row + 64].all())
    assert pc.read_extent(lay)[2] == end + 7
    # ViT-L/14: tile 4 of the last d row reads keys 256..319, 56 of them behind the row
    lay = pc.uniform_layout(264, [257, 257], pc.H_ATT)
    assert pc.read_extent(lay)[2] == lay.D * lay.rows + 55 and pc.read_extent(lay)[1] == lay.rows + 55


@pytest.mark.parametrize("name,table", ALL_LAYOUTS)
def test_every_case_keeps_its_reads_inside_its_tensors(name, table):
    """the condition that makes value poisoning safe: the largest q / k row, V^T element and gate column the contract allows,
    against the allocation (qk [rows + 64, 2 D], vt [D rows + 64], gate [H, rows])"""
    lay = pc.case_layout(name, table)
    q_row, k_row, vt_el, gate_col = pc.read_extent(lay)
    print(f"POISON|{name}|rows {lay.rows}|q row {q_row}|k row {k_row} < {lay.qk_rows}|vt element {vt_el} < {lay.vt_numel}|gate {gate_col}")
    assert q_row < lay.qk_rows and k_row < lay.qk_rows and vt_el < lay.vt_numel and gate_col < lay.rows
    assert pc.within_allocation(lay)
    assert k_row - (lay.rows - 1) <= 56 and vt_el - (lay.D * lay.rows - 1) <= 56          # pitch % 8 == 0: never more than 56 past the end
    assert pc.TMAX >= max(lay.pitch)
    # without the slack the same layout would NOT hold its reads whenever the last utterance's pitch is no multiple of 64
    bare = pc.layout(lay.pitch, lay.lens, lay.H, slack=0, uniform=lay.uniform)
    last_p, last_n = lay.pitch[-1], lay.lens[-1]
    assert pc.within_allocation(bare) == ((last_n + 63) // 64 * 64 <= last_p and (last_p + 31) // 32 * 32 <= last_p)
    # the layer driver's documented workspace holds the same tensors back to back
    total, parts = pc.driver_workspace(lay.rows, lay.D, 2 * lay.D)
    assert parts["qk_slack"] == (lay.rows * 2 * lay.D, 64 * 2 * lay.D) and parts["vt_slack"][1] == 64
    assert parts["qk"][1] + parts["qk_slack"][1] == lay.qk_rows * 2 * lay.D and parts["vt"][1] + parts["vt_slack"][1] == lay.vt_numel
    assert total == lay.rows * (6 * lay.D + 2 * lay.D) + 64 * 2 * lay.D + 64 and all(o % 8 == 0 for o, _ in parts.values())


def test_attention_case_list():
    cases = pc.attention_cases()
    assert len(cases) == len(set(cases)) == 5 * 4 + 4 + 1
    assert ("segment 264/8/136", "bias", False) in cases and ("uniform R=128", "causal32", True) in cases
    assert all(pc.GEOMETRIES[n][0] or i != "causal32" for n, i, _ in cases)


def test_poisoned_empty_fills_floats_only_and_restores():
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pc.poisoned_empty():
        assert torch.empty is not orig[0]
        a = torch.empty(3, 5)
        b = torch.empty_like(torch.zeros(4, dtype=torch.bfloat16))
        c = torch.zeros(2).new_empty((7,), dtype=torch.float64)
        i = torch.empty(6, dtype=torch.int32).fill_(3)
        j = torch.zeros(2, dtype=torch.int64).new_empty(5)
        e = torch.empty(0)
        assert all(bool(torch.isnan(t).all()) for t in (a, b, c)) and (a.shape, b.dtype, c.dtype) == ((3, 5), torch.bfloat16, torch.float64)
        assert i.dtype == torch.int32 and j.dtype == torch.int64 and j.shape == (5,) and e.numel() == 0
        assert bool(torch.isnan(torch.empty(2, 2, requires_grad=True)).all())
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig


def test_poisoned_empty_restores_when_the_body_raises():
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with pc.poisoned_empty():
            assert torch.empty is not orig[0]
            raise KeyError("body")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig
    with pc.poisoned_empty():                                    # and it nests / can be entered again
        with pc.poisoned_empty():
            assert bool(torch.isnan(torch.empty(1)).all())
        assert bool(torch.isnan(torch.empty(1)).all())
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == orig


# ================================================================================================================== backward (tests/test_gpu_poison_bwd.py)
def _bwd_reference(lay, o, causal):
    """attn_cases.bwd_ref per utterance on q / k / v / dout cut to the valid rows and keys"""
    outs = []
    for b, n in enumerate(lay.lens):
        q, k, v, d = (_heads(o[name][b * lay.R: b * lay.R + n], lay.H) for name in ("q", "k", "v", "dout"))
        r = ac.bwd_ref(q, k, v, d, ac.key_mask(n, n, causal)[None].expand(lay.H, -1, -1))
        outs += [r["dq"], r["dk"], r["dv"]]
    return outs


@pytest.mark.parametrize("name", list(pc.BWD_GEOMETRIES))
def test_backward_regions_partition_the_rows(name):
    lay = pc.bwd_case_layout(name)
    for regions, names in ((lay.key, pc.BWD_KEY_REGIONS), (lay.query, pc.BWD_QUERY_REGIONS)):
        assert tuple(regions) == names
        count = sum(m.long() for m in regions.values())
        assert bool((count == 1).all()), "every row lies in exactly one region"
        assert torch.equal(regions["valid"], lay.valid) and int(lay.valid.sum()) == sum(lay.lens)
    size = lambda d: {n: int(m.sum()) for n, m in d.items()}
    if name == "R=128":             # 37: 5 valid + 27 masked keys in one 32-key block, the next one skipped; 1: the single-key utterance
        assert size(lay.key) == {"valid": 166, "tail32": 0 + 31 + 27, "tail128": 0 + 96 + 64, "padded": 0}
        assert size(lay.query) == {"valid": 166, "q_pad": 0 + 127 + 91, "q_blk": 0, "q_far": 0}
    else:                           # 129: one valid key in the second 128-key block; 65: that block wholly padded; q_rows = 200 < 224 < R
        assert size(lay.key) == {"valid": 394, "tail32": 24 + 31 + 31, "tail128": 32 + 96 + 32, "padded": 0 + 0 + 128}
        assert size(lay.query) == {"valid": 394, "q_pad": 0 + 71 + 135, "q_blk": 3 * 24, "q_far": 3 * 32}
        assert all(int(m.sum()) > 0 for m in list(lay.key.values()) + list(lay.query.values())), "this geometry reaches every region"
    # the transposed copies' column masks mark the same rows
    m = lay.key["tail32"]
    assert bool(((pc.head_transpose(pc.row_mask(m, lay.D).to(torch.bfloat16), lay) != 0) == pc.col_mask_T(lay, m)).all())
    assert int(pc.stat_mask(lay, m).sum()) == lay.H * int(m.sum())


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("name", list(pc.BWD_GEOMETRIES))
def test_backward_masks_are_disjoint_from_what_the_reference_reads(name, causal):
    lay = pc.bwd_case_layout(name)
    o = pc.bwd_operands(lay, seed=5)
    clean = _bwd_reference(lay, o, causal)
    excluded = pc.row_mask(~lay.valid, lay.D)
    dirty = {n: pc.poison_bf16(o[n], excluded, pc.NONFINITE_POISON) for n in ("q", "k", "v", "dout")}
    assert all(bool((~torch.isfinite(t.float()) == excluded).all()) for t in dirty.values())
    assert all(bool(torch.isfinite(x).all()) for x in clean) and all(float(x.abs().max()) > 0 for x in clean[2::3])      # (dq = dk = 0 at one key)
    assert all(pc.bits_equal(a, b) for a, b in zip(clean, _bwd_reference(lay, dirty, causal)))
    # the exact complement: what is unmarked is what the reference was given, and the clean operands are exact zeros under the masks
    assert int((~excluded).sum()) == sum(lay.lens) * lay.D
    assert all(bool((o[n][excluded] == 0).all()) for n in ("q", "k", "v", "dout"))
    s = o["scratch"].float()
    assert bool(torch.isfinite(s).all()) and 32 < float(s.std()) < 128, "the ordinary-magnitude scratch is N(0, 64^2)"


def test_every_backward_case_keeps_its_reads_inside_its_tensors():
    for name, (R, lens, q_rows) in pc.BWD_GEOMETRIES.items():
        lay = pc.bwd_case_layout(name)
        ext = pc.bwd_read_extent(lay)
        print(f"POISON|attn_bwd {name}|rows per utterance {R}|largest row read {ext}")
        assert R % 128 == 0 and all(0 <= v < R for v in ext.values())          # whole tiles: no read leaves the utterance's R rows
        assert ext["dq_key"] == (max(lens) + 63) // 64 * 64 - 1 and ext["dkv_query"] == (q_rows + 63) // 64 * 64 - 1
        assert max(lens) <= q_rows, "a row with dout != 0 lies below q_rows"
    valid = pc.reducer_valid()
    assert valid.numel() == 384 and valid.numel() % 128 == 0 and int(valid.sum()) == 128 + 1 + 37        # wgrad: rows % 64, posconv: % 128
    assert (3 * (128 + 2 * 64)) % (128 * 3) == 0                                                         # the posconv slab rows, Z = 3 slices
    short = pc.short_valid()
    assert short.numel() == 96 and int(short.sum()) == 32 + 1 + 17
    assert len(pc.REDUCERS) == len(set(pc.REDUCERS)) == 9


def test_bit_comparison_rejects_one_nan_a_payload_and_the_sign_of_zero():
    """the comparison every poison test ends in: one NaN written into a clean result is rejected (NaN != NaN would also reject a NaN
    that was there before: bit equality does not), so is another NaN payload and -0 for +0"""
    a = torch.randn(16, 8, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    b = a.clone()
    assert pc.bits_equal(a, b)
    b[3, 5] = float("nan")
    assert not pc.bits_equal(a, b) and pc.bits_equal(b, b.clone())
    one = torch.zeros(4, dtype=torch.bool)
    one[0] = True
    n1 = pc.poison_bf16(torch.zeros(4, dtype=torch.bfloat16), one, (0x7FC0,))
    n2 = pc.poison_bf16(torch.zeros(4, dtype=torch.bfloat16), one, (0xFFC1,))
    assert bool(torch.isnan(n1[0])) and bool(torch.isnan(n2[0])) and not pc.bits_equal(n1, n2)
    assert not pc.bits_equal(torch.zeros(2), -torch.zeros(2)) and bool((torch.zeros(2) == -torch.zeros(2)).all())
    f = torch.randn(5, generator=torch.Generator().manual_seed(2))
    g = f.clone()
    g[4] = float("nan")
    assert not pc.bits_equal(f, g) and not pc.bits_equal(f, f.double())
