"""What can be settled without a GPU about tests/text_tower_cases.py: the geometry table of the cases, that an emulation of the
product's arithmetic (fp32 torch on bf16 operands, rounded to bf16 where the product stores, attention through attn_cases.emulate_*)
stays inside every stage bound against the fp64 reference - so the bounds are satisfiable before any kernel runs -, that every planted
error is rejected by the element-wise criterion alone, that the softmax of the cases is not flat, and what the bf16-storage control's
per-sequence error against fp64 is (the GPU module's end-to-end criterion refers to it).  Figures are printed before they are asserted.
Case A in full, case C for its attention stages (causal = 64, two sequences to a 128-row block)."""
import pytest
import torch

import text_tower_cases as tc


@pytest.fixture(scope="module")
def runs():
    """case -> dict(stages, X, dX, out, dx, counts, eot, clip): the emulated forward + backward of the keyword path"""
    clip = tc.make_clip(512)
    tok, pos = clip._prompt_constants(torch.device("cpu"))
    l32 = tc.layers32_of(clip)
    made = {}

    def get(name):
        if name not in made:
            c, inp = tc.CASES[name], tc.case_inputs(name)
            n_pos = tc.n_pos_of(name)
            X, eot = tc.assemble_ref(inp["keywords"], inp["counts"], tok, pos, c["Bp"], c["SEG"], n_pos)
            dX = torch.zeros_like(X)
            dX[eot.long()] = inp["d_rows"].to(torch.bfloat16)
            stages, out, dx = tc.emulate_chain(X, dX, l32, c["heads"], c["SEG"])
            made[name] = dict(stages=stages, X=X, dX=dX, out=out, dx=dx, counts=inp["counts"].tolist(), eot=eot, clip=clip, inp=inp)
        return made[name]
    return get


def test_geometry_table():
    """the table of the issue == the cases' own rule == clip_text_hip._geometry; case B has a 0 and an 8"""
    from speechclip_plus_amd.clip_text_hip import _geometry
    for name, c in tc.CASES.items():
        T = tc.n_pos_of(name)
        assert tc.geometry(c["B"], T)[:3] == (c["SEG"], c["Bp"], c["M"]) and _geometry(c["B"], T) == tc.geometry(c["B"], T), name
    n = tc.counts_of("B")
    assert len(n) == 64 and min(n) == 0 and max(n) == 8 and n == tc.counts_of("B")
    assert [tc.n_pos_of(k) for k in "ABCDE"] == [10, 10, 42, 77, 77]
    assert tc.CASES["C"]["counts"][1] + 1 == 32                       # an EOT at row 32 of its segment
    assert sorted(x + 1 for x in tc.CASES["D"]["counts"][1:]) == [64, 65]


def test_emulation_stays_inside_every_stage_bound(runs):
    rep = tc.Report()
    for st in runs("A")["stages"]:
        tc.check_stage(rep, "A (emulated)", st)
    for st in runs("C")["stages"]:
        if st["kind"].startswith("attn"):
            tc.check_stage(rep, "C (emulated)", st)
    # the zero-gradient promise holds in the emulation: every gradient tensor's dead rows are exactly zero
    for name in "AC":
        r = runs(name)
        c = tc.CASES[name]
        live = tc.live_rows(r["counts"], c["Bp"], c["SEG"])
        for st in r["stages"]:
            if " bwd " in st["name"]:
                tc.check_dead_rows(rep, name, st["name"], st["dqkv"] if st["kind"] == "attn_bwd" else st["got"], live)
    rep.done()


def test_every_planted_error_is_rejected(runs):
    for name in "AC":
        r = runs(name)
        got = tc.planted_suite(r["stages"], f"{name} (emulated)", tc.CASES[name]["SEG"], r["counts"])
        assert len(got) == 7 and all(v > 1.0 for v in got.values()), got


def test_softmax_is_not_flat_and_the_control(runs):
    """fp64 whole tower on case A: over the queries (inside the prompts' n_pos positions) that see at least 8 keys, the median of the
    largest probability is at least 0.3.  And the control's per-sequence rel-L2 against fp64, printed: EOT output row and d keywords."""
    r = runs("A")
    c = tc.CASES["A"]
    lw = tc.layer_weights(r["clip"])
    ref, gref, pmax = tc.tower64(r["X"], r["dX"], lw, c["heads"], c["SEG"], rounded=False)
    ctl, gctl, _ = tc.tower64(r["X"], r["dX"], lw, c["heads"], c["SEG"], rounded=True)
    n_pos = tc.n_pos_of("A")
    meds = []
    for li, p in enumerate(pmax):                                    # [Bp heads, 32]: problem = (sequence, head)
        p = p.view(c["Bp"], c["heads"], c["SEG"])[: c["B"], :, 7: n_pos]        # query t sees t + 1 keys
        meds.append(float(p.median()))
        print(f"NOTFLAT|A layer {li}|median of the largest probability over {p.numel()} queries with >= 8 keys: {meds[-1]:.3f}|factor {tc.QK_FACTOR}")
    allp = torch.cat([p.view(c["Bp"], c["heads"], c["SEG"])[: c["B"], :, 7: n_pos].reshape(-1) for p in pmax])
    print(f"NOTFLAT|A|median over both layers {float(allp.median()):.3f}")
    assert float(allp.median()) >= tc.NOT_FLAT and min(meds) >= tc.NOT_FLAT
    for b, n in enumerate(r["counts"]):
        e = int(r["eot"][b])
        rows = slice(b * c["SEG"] + 1, b * c["SEG"] + 1 + n)
        print(f"CONTROL|A seq {b} count {n}|EOT row rel-L2 control {tc.seq_rel_l2(ctl[e], ref[e]):.3e}, emulation {tc.seq_rel_l2(r['out'][e], ref[e]):.3e}|"
              f"d keywords control {tc.seq_rel_l2(gctl[rows], gref[rows]):.3e}, emulation {tc.seq_rel_l2(r['dx'][rows], gref[rows]):.3e}")
        assert tc.seq_rel_l2(ctl[e], ref[e]) < 1e-2 and tc.seq_rel_l2(gctl[rows], gref[rows]) < 2e-2
    live = tc.live_rows(r["counts"], c["Bp"], c["SEG"])
    assert float(gref[~live].abs().max()) == 0.0 and float(gctl[~live].abs().max()) == 0.0
