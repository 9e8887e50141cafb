"""CPU: the host half of keyword detokenisation (speechclip_plus_amd/keyword_neighbors.py) - the reference's result structure for the
fixed and the dynamic form, the reduced -> original id mapping, ``decode=``, the hit rate and the statistics - on hand-made
(vals, idx) and against tests/golden/kw_neighbors.npz (the reference's own functions, tests/golden/make_golden_kwneighbors.py).
The scores and the selection themselves run on the device only: tests/test_gpu_keyword_neighbors.py."""
import json
import os

import numpy as np
import pytest
import torch

from speechclip_plus_amd import keyword_neighbors as kn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kw_neighbors.npz")


class NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def stub_model(reduced_ids=None, keyword_num=None, bs=3, E=32, tokenizer=None):
    clip = NS(selected_text_emb_ids=reduced_ids)
    if reduced_ids is not None:
        clip.reducedl2Original = {n: int(o) for n, o in enumerate(reduced_ids.tolist())}
    if tokenizer is not None:
        clip.tokenizer = tokenizer
    return NS(config=NS(data=NS(dev_batch_size=bs)), clip=clip, subword_embd_dim=E, keyword_num=keyword_num)


def cpu_neighbors(keywords, table, K, keywords_len, method):
    """what the device path computes, restated in fp64 on the CPU (stands in for keyword_neighbors through ``_neighbors=``)"""
    kw, tb = keywords.double(), table.double()
    if method == "cosine":
        s = torch.nn.functional.normalize(kw, dim=-1, eps=1e-8) @ torch.nn.functional.normalize(tb, dim=-1, eps=1e-8).t()
    else:
        s = kw @ torch.linalg.pinv(tb.t()).t()
    v, i = torch.sort(s, dim=-1, descending=True, stable=True)
    return v[..., :K].float(), i[..., :K]


def test_entries_from_hand_made_vals_idx():
    vals = torch.tensor([[[0.9, 0.5], [0.8, 0.1]], [[0.7, 0.6], [float("-inf"), float("-inf")]]])
    idx = torch.tensor([[[2, 0], [1, 2]], [[0, 1], [-1, -1]]])
    dec = kn.TokenDecoder(stub_model(torch.tensor([40, 50, 60])).clip)
    out = kn.neighbors_to_entries(vals, idx, ["a cat", "a dog"], [2, 1], dec)
    assert [e["gold"] for e in out] == ["a cat", "a dog"]
    assert dict(out[0]["neighbors"]) == {"keyword_0": [[60, pytest.approx(0.9)], [40, 0.5]], "keyword_1": [[50, pytest.approx(0.8)], [60, pytest.approx(0.1)]]}
    assert dict(out[1]["neighbors"]) == {"keyword_0": [[40, pytest.approx(0.7)], [50, pytest.approx(0.6)]]}
    json.dumps(out)                                   # what validation_epoch_end writes


def test_decoder_precedence_and_mapping():
    ids = torch.tensor([7, 11, 13])
    tok = NS(decoder={7: "a</w>", 11: "b</w>", 13: "c</w>", 1: "x"})
    assert kn.TokenDecoder(stub_model(ids).clip).decode(2) == 13                        # no tokenizer: the ORIGINAL id
    assert kn.TokenDecoder(stub_model(ids, tokenizer=tok).clip).decode(1) == "b</w>"    # reduced -> original -> sub-word
    assert kn.TokenDecoder(stub_model(None, tokenizer=tok).clip).decode(1) == "x"       # full vocabulary: no mapping
    assert kn.TokenDecoder(stub_model(ids, tokenizer=tok).clip, decode=lambda o: f"<{o}>").decode(0) == "<7>"
    assert kn.TokenDecoder(None).decode(5) == 5


def test_fixed_form_against_the_reference_fixture():
    fx = np.load(GOLDEN)
    table, ids, K = torch.from_numpy(fx["table"]), torch.from_numpy(fx["reduced_ids"]), int(fx["K"])
    kw = torch.from_numpy(fx["fixed_keywords"])
    gold = fx["fixed_gold_in"].tolist()
    U, N, _ = kw.shape
    for method in ("cosine", "pseudo_inverse"):
        model = stub_model(ids, keyword_num=N, bs=int(fx["dev_batch_size"]))
        out = kn.extract_fixed_keyword_neighbors(model, K, method, table, kw, gold, _neighbors=cpu_neighbors)
        assert len(out) == U                                          # the last batch (one utterance of three) included
        for u, e in enumerate(out):
            assert sorted(e["neighbors"]) == [f"keyword_{i}" for i in range(N)]
            for i in range(N):
                toks = [t for t, _ in e["neighbors"][f"keyword_{i}"]]
                sc = [s for _, s in e["neighbors"][f"keyword_{i}"]]
                assert toks == fx[f"fixed_{method}_tokens"][u, i].tolist()
                np.testing.assert_allclose(sc, fx[f"fixed_{method}_scores"][u, i], atol=1e-6, rtol=0)
        # gold_texts[i + x] here; the reference wrote gold_texts[x] (the fixture records what it wrote)
        assert [e["gold"] for e in out] == gold
        bs = int(fx["dev_batch_size"])
        assert fx[f"fixed_{method}_gold"].tolist() == [gold[u % bs] for u in range(U)]


def test_dynamic_form_against_the_reference_fixture():
    fx = np.load(GOLDEN)
    table, ids, K = torch.from_numpy(fx["table"]), torch.from_numpy(fx["reduced_ids"]), int(fx["K"])
    kws = [[torch.from_numpy(fx[f"dyn_keywords_{b}"])] for b in range(3)]
    counts, gold = fx["dyn_counts"].tolist(), fx["dyn_gold_in"].tolist()
    assert 0 in counts and kws[-1][0].shape[0] < int(fx["dev_batch_size"])      # a keyword-less utterance, a short last batch
    for method in ("cosine", "pseudo_inverse"):
        model = stub_model(ids, bs=int(fx["dev_batch_size"]))
        out = kn.extract_dynamic_keyword_neighbors(model, K, method, [None] * 3, table, kws, gold, counts, _neighbors=cpu_neighbors)
        assert [e["gold"] for e in out] == gold
        assert [len(e["neighbors"]) for e in out] == counts
        for u, e in enumerate(out):
            for i in range(counts[u]):
                assert [t for t, _ in e["neighbors"][f"keyword_{i}"]] == fx[f"dyn_{method}_tokens"][u, i].tolist()
                np.testing.assert_allclose([s for _, s in e["neighbors"][f"keyword_{i}"]], fx[f"dyn_{method}_scores"][u, i], atol=1e-6, rtol=0)


def test_dynamic_form_scores_only_the_counted_slots_and_takes_decode():
    torch.manual_seed(0)
    table = torch.randn(20, 8)
    kws = [[torch.randn(2, 3, 8)], [torch.randn(1, 2, 8)]]
    seen = {}

    def spy(keywords, tab, K, keywords_len, method):
        seen["rows"] = keywords.shape[1]
        return cpu_neighbors(keywords, tab, K, keywords_len, method)

    out = kn.extract_dynamic_keyword_neighbors(stub_model(None, bs=2, E=8), 3, "cosine", [None, None], table, kws, ["a", "b", "c"],
                                               [3, 0, 1], decode=lambda o: f"t{o}", _neighbors=spy)
    assert seen["rows"] == 4                                           # 3 + 0 + 1 slots, not the 8 the tensors hold
    assert [len(e["neighbors"]) for e in out] == [3, 0, 1]
    assert all(isinstance(t, str) and t.startswith("t") for e in out for n in e["neighbors"].values() for t, _ in n)
    ref_v, ref_i = cpu_neighbors(kws[1][0][0, :1], table, 3, None, "cosine")
    assert [t for t, _ in out[2]["neighbors"]["keyword_0"]] == [f"t{i}" for i in ref_i[0].tolist()]
    # every utterance without keywords: still one entry each
    out = kn.extract_dynamic_keyword_neighbors(stub_model(None, bs=2, E=8), 3, "cosine", [None], table, [[torch.randn(2, 1, 8)]], ["a", "b"], [0, 0],
                                               _neighbors=spy)
    assert [dict(e["neighbors"]) for e in out] == [{}, {}]


def test_keyword_hit_rate_worked_by_hand():
    SOT, EOT = 49406, 49407
    # reduced index r -> original id
    r2o = torch.tensor([0, 320, 530, SOT, EOT, 1125, 2368])
    gold = torch.zeros(2, 77, dtype=torch.long)
    gold[0, :4] = torch.tensor([SOT, 320, 1125, EOT])                 # caption 0: tokens 320, 1125
    gold[1, :3] = torch.tensor([SOT, 2368, EOT])                      # caption 1: token 2368
    idx = torch.tensor([
        [[1, 2], [3, 4], [0, 2]],        # utt 0: kw0 has 320 -> hit; kw1 only <sot>, <eot> -> no hit; kw2 the padding id 0 and 530 -> no hit
        [[5, 1], [2, 6], [-1, -1]],      # utt 1: kw0 1125, 320 (caption 0's words) -> no hit; kw1 has 2368 -> hit; kw2 unscored
    ])
    r = kn.keyword_hit_rate(idx, gold, r2o)
    assert r["hits"].tolist() == [[True, False, False], [False, True, False]]
    assert r["valid"].tolist() == [[True, True, True], [True, True, False]]
    assert r["per_slot"].tolist() == [0.5, 0.5, 0.0]
    assert float(r["mean"]) == pytest.approx(2 / 5)
    # without a mapping the ids are original ids already
    r = kn.keyword_hit_rate(torch.tensor([[[320, 9], [SOT, 0]]]), gold[:1])
    assert r["hits"].tolist() == [[True, False]] and float(r["mean"]) == 0.5


def test_keyword_statistics_fixed_and_ragged():
    torch.manual_seed(1)
    kw, table = torch.randn(6, 3, 8) * 2 + 0.5, torch.randn(30, 8)
    s = kn.keyword_statistics(kw, table)
    for i in range(3):                                                # kwClip.py:338-346
        assert float(s["mean"][f"kw_{i}"]) == pytest.approx(float(kw[:, i].mean(0).mean()), abs=1e-6)
        assert float(s["std"][f"kw_{i}"]) == pytest.approx(float(kw[:, i].std(0).mean()), abs=1e-5)
        assert float(s["norm"][f"kw_{i}"]) == pytest.approx(float(kw[:, i].norm(p=2, dim=-1).mean()), abs=1e-5)
    flat = kw.reshape(-1, 8)
    assert float(s["kw_mean_mse"]) == pytest.approx(float((flat.mean(0) - table.mean(0)).norm()), abs=1e-6)
    assert float(s["kw_std_mse"]) == pytest.approx(float((flat.std(0) - table.std(0)).norm()), abs=1e-5)
    lens = torch.tensor([3, 1, 2, 0, 3, 2])
    s = kn.keyword_statistics(kw, table, lens)
    have2 = kw[lens > 2][:, 2]
    assert float(s["mean"]["kw_2"]) == pytest.approx(float(have2.mean(0).mean()), abs=1e-6)
    assert float(s["std"]["kw_2"]) == pytest.approx(float(have2.std(0).mean()), abs=1e-5)
    valid = torch.cat([kw[u, : lens[u]] for u in range(6)])
    assert float(s["norm"]["kw"]) == pytest.approx(float(valid.norm(dim=-1).mean()), abs=1e-5)


def test_default_chunk_fits_half_the_infinity_cache():
    assert kn.SCORE_SCRATCH_BYTES == 128 << 20
    for V, rows in ((8112, 4096), (19787, 1664), (49408, 640)):
        c = kn.default_chunk_rows(V)
        assert c == rows and c % 128 == 0
        assert c * 4 * ((V + 127) // 128 * 128) <= kn.SCORE_SCRATCH_BYTES
    assert kn.default_chunk_rows(10 ** 7) == 128


def test_device_only():
    with pytest.raises(RuntimeError, match="device tensors only"):
        kn.keyword_neighbors(torch.zeros(1, 2, 8), torch.zeros(5, 8), 3)
    with pytest.raises(NotImplementedError):
        kn.keyword_neighbors(torch.zeros(1, 2, 8), torch.zeros(5, 8), 3, retrieve_method="dot")
