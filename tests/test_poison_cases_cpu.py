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


# ================================================================================================================== keyword side (tests/test_gpu_poison_kw.py)
import kw_cases as kc          # noqa: E402
import kwpool_cases as kp      # noqa: E402

KW_SHAPES = [(Nk, V) for Nk in pc.KW_NK for V in pc.KW_V]


@pytest.mark.parametrize("Nk,V", KW_SHAPES)
def test_quantiser_masks_are_the_padding_and_nothing_else(Nk, V):
    lay = pc.quantiser_layout(Nk, V)
    assert (lay.Nkp, lay.Vp, lay.Ep) == ({5: 128, 130: 256}[Nk], {200: 256, 8112: 8192}[V], 64)
    assert lay.Nkp > Nk and lay.Vp > V, "every shape has pad rows and pad columns"
    assert int(lay.kw_split.sum()) == (lay.Nkp - Nk) * 6 * lay.Ep and int(lay.kwn_T.sum()) == (lay.Nkp - Nk) * lay.Et
    assert int(lay.table_split.sum()) == (lay.Vp - V) * 6 * lay.Ep and int(lay.norm_T.sum()) == (lay.Vp - V) * lay.Et
    assert int((~lay.cos).sum()) == Nk * V and bool((lay.cos == (lay.cos_rows | lay.cos_cols)).all())
    assert int(lay.s_split.sum()) == (lay.Nkp - Nk) * 3 * lay.Vp and int(lay.w_split.sum()) == 3 * (lay.Vp - V) * lay.Et
    assert not bool(lay.w_split.view(lay.Et, 3, lay.Vp)[:, :, :V].any()) and not bool(lay.cos[:Nk, :V].any())
    # what the fp64 references are given is the unmarked block: poison under the masks does not reach them
    g = torch.Generator().manual_seed(Nk + V)
    cos = torch.zeros(lay.Nkp, lay.Vp)
    cos[:Nk, :V] = torch.rand(Nk, V, generator=g) * 2 - 1
    dirty = pc.poison_f32(cos, lay.cos, pc.NONFINITE_POISON)
    assert bool((~torch.isfinite(dirty) == lay.cos).all())
    a, b = (kc.rowstats_ref(kc.mask_cols(t[:Nk, :V], (0, 2, 3)).double(), 0.1) for t in (cos, dirty))
    assert all(pc.bits_equal(a[k], b[k]) for k in a) and all(bool(torch.isfinite(v.double()).all()) for v in a.values())


def test_cif_masks_and_case():
    c = pc.cif_case()
    T = pc.CIF_T
    assert list(pc.CIF_LENS) == [90, 1, 37, 64] and 1 in pc.CIF_LENS and pc.CIF_S in pc.CIF_LENS and 0 in pc.CIF_TARGETS
    assert c["pad"].sum(1).tolist() == [0, 89, 53, 26] and bool((c["alpha"][c["pad"]] == 0).all()) and bool((c["x"][c["pad"]] == 0).all())
    right, _ = kc.fire_indices(c["csum"], 1.0, T)
    assert right[:, -1].tolist() == c["last"].tolist() == list(pc.CIF_TARGETS), "the keyword count is the slot the last frame lands in"
    assert torch.equal(right.amax(1), c["last"]) and int(c["last"].max()) == T
    total = c["alpha"].double().sum(1)
    assert bool(((total - torch.tensor(pc.CIF_TARGETS).double() - 1e-5).abs() < 1e-6).all())
    for b, n in enumerate(pc.CIF_LENS):                      # csum is constant behind the length: no frame t >= len fires
        assert bool((c["csum"][b, n - 1:] == c["csum"][b, n - 1]).all())
    behind, at = pc.slot_mask(c["last"], T), pc.slot_mask(c["last"], T, at=True)
    assert behind.sum(1).tolist() == [0, 6, 3, 5] and at.sum(1).tolist() == [1, 7, 4, 6]
    # the fp64 formulas read neither x of the frames t >= len (weight 0: finite values only) nor g behind the count
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(c["B"], T + 1, c["C"], generator=gen) * (~behind)[..., None]
    xm = pc.row_mask(c["pad"].reshape(-1), c["C"]).view(c["B"], c["S"], c["C"])
    gm = pc.row_mask(behind.reshape(-1), c["C"]).view(c["B"], T + 1, c["C"])
    clean = kc.fire_formula(c["x"].double(), c["alpha"].double(), c["csum"].double(), g.double(), 1.0, T)
    dirty = kc.fire_formula(pc.poison_f32(c["x"], xm, pc.FINITE_POISON).double(), c["alpha"].double(), c["csum"].double(),
                            pc.poison_f32(g, gm, pc.FINITE_POISON).double(), 1.0, T)
    keep_s, keep_f = ~behind, ~c["pad"]
    assert bool((clean["out"][keep_s] == dirty["out"][keep_s]).all()) and bool((clean["dx"][keep_f] == dirty["dx"][keep_f]).all())
    assert bool((clean["pa"][:, keep_f] == dirty["pa"][:, keep_f]).all()) and bool((clean["pb"][:, keep_f] == dirty["pb"][:, keep_f]).all())
    # ... but slot ``count`` itself is read: the weight left over behind the last fire lands there
    one = torch.zeros_like(gm)
    one[2, int(c["last"][2])] = True
    planted = kc.fire_formula(c["x"].double(), c["alpha"].double(), c["csum"].double(), pc.plant(g, one, 1e6).double(), 1.0, T)
    assert not bool((clean["dx"][keep_f] == planted["dx"][keep_f]).all())


def test_key_and_prompt_masks():
    m = pc.key_mask(pc.KEY_LENS, pc.KEY_N)
    assert m.shape == (3, 72) and m.sum(1).tolist() == [2, 71, 35] and pc.KEY_N % 8 == 0 and pc.KEY_N >= pc.KEY_T
    case = dict(kp.pool_case(pc.KEY_D, 8, 8, pc.KEY_T + 1, 1))
    case["flen"] = torch.tensor(list(pc.KEY_LENS) + [0], dtype=torch.int32)
    out_rows = pc.pool_frames_mask(case["flen"], case["R"], case["row0"])
    assert torch.equal(~out_rows, kp.valid_mask(case)[:, case["C"]:]) and out_rows.sum(1).tolist() == [1, 70, 34, 71]
    assert bool(out_rows[:, 0].all()), "the CLS slot in front of the frames is no frame"
    # the masked softmax in fp64 does not read the scores of masked keys
    rows = 3 * pc.KEY_H * pc.KEY_T
    mrow = m.repeat_interleave(pc.KEY_H * pc.KEY_T, dim=0)
    s = torch.randn(rows, pc.KEY_N, generator=torch.Generator().manual_seed(1)) * ~mrow
    a = kc.softmax_ref(s.double(), m, pc.KEY_H * pc.KEY_T, 0.125)
    b = kc.softmax_ref(pc.poison_f32(s, mrow, pc.NONFINITE_POISON).double(), m, pc.KEY_H * pc.KEY_T, 0.125)
    assert pc.bits_equal(a, b) and bool((a[mrow] == 0).all()) and bool(torch.isfinite(a).all())
    pm = pc.prompt_mask(pc.PROMPT_COUNTS, pc.PROMPT_N)
    assert pm.sum(1).tolist() == [0, 6, 3, 5] and max(pc.PROMPT_COUNTS) + 2 <= pc.PROMPT_NPOS <= pc.PROMPT_SEG


def test_every_keyword_case_keeps_its_reads_inside_its_tensors():
    """the twin of test_every_case_keeps_its_reads_inside_its_tensors for tests/test_gpu_poison_kw.py: the largest element index each
    kernel's contract allows against the numel of the tensor the test hands it"""
    for Nk, V in KW_SHAPES:
        lay = pc.quantiser_layout(Nk, V)
        ext = pc.quantiser_read_extent(lay)
        print(f"POISON|quantiser Nk={Nk} V={V}|{ext}")
        assert all(0 <= last < numel for last, numel in ext.values())
        assert ext["cos"][0] == (Nk - 1) * lay.Vp + V - 1 and max(pc.KW_TOPK) <= min(pc.KW_V)
    c = pc.cif_case()
    ext = pc.cif_read_extent(c)
    print(f"POISON|cif|{ext}")
    assert all(0 <= last < numel for last, numel in ext.values()) and pc.CIF_S <= kc.MAXS and pc.CIF_C % 4 == 0
    ext = pc.key_read_extent(len(pc.KEY_LENS), pc.KEY_H, pc.KEY_N, 8, 8, pc.KEY_T + 1, pc.KEY_D)
    assert all(0 <= last < numel for last, numel in ext.values()) and pc.KEY_D % 64 == 0 and pc.KEY_N % 4 == 0
    B = len(pc.PROMPT_COUNTS)
    ext = pc.prompt_read_extent(B, B + 1, pc.PROMPT_N, pc.PROMPT_W, pc.PROMPT_SEG, pc.PROMPT_NPOS, pc.PROMPT_COUNTS)
    print(f"POISON|prompt|{ext}")
    assert all(0 <= last < numel for last, numel in ext.values()) and pc.PROMPT_W % 8 == 0 and max(pc.PROMPT_COUNTS) <= pc.PROMPT_N


def test_a_planted_check_fails_on_a_vacuous_mask():
    """the planted checks of tests/test_gpu_poison_kw.py end in ``pc.changed(...)`` being non-empty: with a mask that covers nothing,
    pc.plant plants nothing, the rerun carries the clean bits and the verdict is the empty list - the test would fail, as it must; and
    a comparison that compares nothing (no names) can never report a change"""
    m = pc.key_mask(pc.KEY_LENS, pc.KEY_N)
    rpb = pc.KEY_H * pc.KEY_T
    s = torch.randn(3 * rpb, pc.KEY_N, generator=torch.Generator().manual_seed(2))
    run = lambda scores: {"P": kc.softmax_ref(scores, m, rpb, 0.125)}
    clean = run(s)
    empty = torch.zeros_like(s, dtype=torch.bool)
    assert pc.bits_equal(pc.plant(s, empty), s) and pc.changed(run(pc.plant(s, empty)), clean, ["P"]) == []
    live = empty.clone()
    live[2 * rpb + 3, pc.KEY_LENS[2] - 1] = True
    assert pc.changed(run(pc.plant(s, live)), clean, ["P"]) == ["P"]
    masked = empty.clone()
    masked[2 * rpb + 3, pc.KEY_LENS[2]] = True                  # one key behind the length: the mathematics does not read it
    assert pc.changed(run(pc.plant(s, masked)), clean, ["P"]) == []
    assert pc.changed(run(pc.plant(s, live)), clean, []) == []
    # poison under an empty mask is no poison: every mask the GPU tests use marks something
    assert pc.bits_equal(pc.poison_f32(s, empty, pc.NONFINITE_POISON), s)
    for Nk, V in KW_SHAPES:
        lay = pc.quantiser_layout(Nk, V)
        assert all(int(getattr(lay, n).sum()) > 0 for n in ("kw_split", "kwn_T", "table_split", "norm_T", "cos_rows", "cos_cols", "s_split", "w_split"))
    c = pc.cif_case()
    assert int(c["pad"].sum()) > 0 and int(pc.slot_mask(c["last"], pc.CIF_T).sum()) > 0 and int(m.sum()) > 0
    assert int(pc.prompt_mask(pc.PROMPT_COUNTS, pc.PROMPT_N).sum()) > 0
    assert pc.bits_equal(torch.zeros(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8)) and not pc.bits_equal(torch.zeros(3, dtype=torch.uint8), torch.ones(3, dtype=torch.uint8))


def test_the_entropy_bound_of_the_few_row_shape():
    """kw_cases.rowstats_ent_bound: the fp32 evaluation of the kernel's three passes meets it on cosine-like scores at V = 8112, also
    when the row's log-sum-exp is off by one fp32 rounding in either direction (the common shift the bound is written for); it stays
    a bound on rounding - a relative error of 1e-5 in ent, or one dropped column, exceeds it - and it is used at one shape only"""
    Nk, V = kc.ENT_FEW_ROWS
    assert (Nk, V) == (min(pc.KW_NK), max(pc.KW_V))
    x = kc.mask_cols((torch.rand(64, V, generator=torch.Generator().manual_seed(8)) * 2 - 1).float(), (0, 2, 3))
    r64, r32 = kc.rowstats_ref(x.double(), 0.1), kc.rowstats_ref(x, 0.1)
    bound = kc.rowstats_ent_bound(x)
    assert bound.shape == (64,) and bool((bound > 0).all())
    assert bool(((r32["ent"].double() - r64["ent"]).abs() <= bound).all())
    for ulps in (-1.0, 1.0):                                     # l rounded the other way: every p of the row moves together
        l = (r64["lse_1"] * (1 + ulps * 2.0 ** -24)).float()
        p = torch.exp(x - l[:, None])
        ent = -(p * torch.log(p + 1e-9)).sum(-1)
        assert bool(((ent.double() - r64["ent"]).abs() <= bound).all())
    rel = bound / r64["ent"].abs()
    print(f"PARITY|ent bound V={V}|relative|{float(rel.max()):.3e}")
    assert float(rel.max()) < 1e-5, "a relative error of 1e-5 is outside the bound"
    p64 = torch.exp(x.double() - r64["lse_1"][:, None])
    one_column = (p64 * torch.log(p64 + 1e-9)).abs()[:, 5]       # dropping one live column of ~1 / V
    assert bool((one_column > bound).all())
