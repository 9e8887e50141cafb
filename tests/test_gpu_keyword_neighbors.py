"""GPU: keyword detokenisation - the per-row top-K kernel (csrc/topk.hip), keyword_neighbors against fp64, the reference fixture
through the C ABI and the validation path end to end.

Criteria (docs/parity.md, "Keyword detokenisation"):
  selection   ops.topk_rows == torch.sort(descending=True, stable=True)[:k] on the same fp32 matrix: values bit-equal, indices equal,
              every row, nothing excluded.
  neighbours  against fp64 cosine + top-K on the CPU with tol = 1e-6, the margin
              test_cosine_scores_as_one_bf16_gemm_over_three_way_splits_vs_fp64 uses for the same score path:
              (1) every row, every rank r: the fp64 score of the returned column >= the fp64 r-th best - tol, and the returned value
                  is within tol of that column's fp64 score;
              (2) on rows whose K + 1 best fp64 scores are pairwise more than tol apart the index lists are identical; the share of
                  rows (2) leaves out is capped at 2 %, 2 % and 10 % for the three shapes (fp64 alone leaves out 0.44 %, 0.49 % and
                  4.3 % with seeded 0.01 * randn tables).
  pseudo_inverse  the same two criteria against fp64 pinv on the CPU with tol = 1e-6 x the row's largest |fp64 score|.  Where that
              comes from: the product runs in fp32 (E = 32 fp32 multiply-adds per score) on a pseudo-inverse rounded from fp64 to
              fp32, so a score carries at most about (E + 1) roundings of relative size 2^-24 = 6e-8 on terms no larger than the
              row's largest scores - in quadrature sqrt(33) x 6e-8 = 3.4e-7 of that scale; 1e-6 is three times that.

Measured on the first runs (MI355X): selection 26 of 26 cases exact; cosine - worst shortfall to the fp64 r-th best 0 / 0 / 1.1e-7, worst
|value - fp64 score| 7.5e-9, rows left out by (2) 0.59 % / 0.68 % / 4.79 %; pseudo_inverse - shortfall 0, value error 3.0e-8 against
tol 1.8e-7, 0.20 % left out.  Before the K reported values were re-evaluated with fp64 accumulation a table row's own score came back
1.8e-6 ... 2.8e-6 below 1 (the fp32 accumulation of the score matrix) and missed the 1e-6 line.
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kw_neighbors.npz")
TOL = 1e-6


def _expect(scores, V, k):
    """stable descending sort of the first V columns, padded with -inf / -1 behind the V-th entry"""
    v, i = torch.sort(scores[:, :V], dim=1, descending=True, stable=True)
    rows = scores.shape[0]
    ev = torch.full((rows, k), float("-inf"), device=scores.device)
    ei = torch.full((rows, k), -1, device=scores.device, dtype=torch.int32)
    n = min(k, V)
    ev[:, :n], ei[:, :n] = v[:, :n], i[:, :n].int()
    return ev, ei


def _check(scores, V, k, what):
    from speechclip_plus_amd import ops
    vals, idx = ops.topk_rows(scores, V, k)
    ev, ei = _expect(scores, V, k)
    torch.cuda.synchronize()
    bad_i = (idx != ei).any(1).nonzero().flatten()
    assert bad_i.numel() == 0, (what, "indices", bad_i[:5].tolist(), idx[bad_i[:1]].tolist(), ei[bad_i[:1]].tolist())
    assert torch.equal(vals.view(torch.int32), ev.view(torch.int32)), (what, "value bits")
    return vals, idx


@pytest.mark.parametrize("V", [1, 7, 63, 64, 65, 8112, 19787, 49408])
def test_topk_rows_exact_on_random_scores(V):
    g = torch.Generator(device="cuda").manual_seed(V)
    for rows in (1, 3):
        s = torch.randn(rows, V, device="cuda", generator=g)
        for k in (1, 5, 10, 32):                     # V < k included: the tail is -inf / -1
            _check(s, V, k, f"random rows {rows} V {V} k {k}")


def test_topk_rows_exact_on_many_rows_and_repeats():
    from speechclip_plus_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    s = torch.randn(4097, 8112, device="cuda", generator=g)
    v1, i1 = _check(s, 8112, 10, "4097 rows")
    v2, i2 = ops.topk_rows(s, 8112, 10)
    assert torch.equal(v1.view(torch.int32), v2.view(torch.int32)) and torch.equal(i1, i2)
    _check(s[:, :65], 65, 32, "4097 rows, a view of pitch 8112 with V = 65")


@pytest.mark.parametrize("V", [65, 8112, 49408])
def test_topk_rows_exact_on_ties(V):
    g = torch.Generator(device="cuda").manual_seed(11 + V)
    five = torch.tensor([-1.5, -0.0, 0.0, 0.25, 3.0], device="cuda")        # -0 and +0 are one value: the lower column wins
    s = five[torch.randint(0, 5, (64, V), device="cuda", generator=g)]
    s[7] = 0.25                                                             # a row of all equal values
    s[8] = -0.0
    s[9, : V // 2] = 3.0                                                    # more equal maxima than any lane keeps
    for k in (1, 5, 10, 32):
        _check(s, V, k, f"ties V {V} k {k}")


@pytest.mark.parametrize("V", [7, 64, 8112, 19787])
def test_topk_rows_exact_with_nan_and_inf(V):
    g = torch.Generator(device="cuda").manual_seed(3 + V)
    s = torch.randn(48, V, device="cuda", generator=g)
    u = torch.rand(48, V, device="cuda", generator=g)
    s[u < 0.02] = float("nan")
    s[(u >= 0.02) & (u < 0.04)] = float("inf")
    s[(u >= 0.04) & (u < 0.06)] = float("-inf")
    s[5] = float("nan")
    s[6] = float("-inf")
    s[7] = float("inf")
    s[8, 1:] = float("-inf")
    s[9] = torch.randn(V, device="cuda", generator=g)
    s[9, V - 1] = float("nan")                                              # one NaN in the last column ranks first
    for k in (1, 5, 10, 32):
        _check(s, V, k, f"nan/inf V {V} k {k}")


@pytest.mark.parametrize("V,ld", [(8112, 8192), (8109, 8192), (8112, 8115), (63, 67), (19787, 19840), (1, 4)])
def test_topk_rows_never_returns_padding(V, ld):
    g = torch.Generator(device="cuda").manual_seed(V + ld)
    buf = torch.randn(5, ld, device="cuda", generator=g)
    buf[:, V:] = 1e9                                                        # larger than every valid score
    buf[2, V:] = float("nan")
    for k in (1, 10, 32):
        vals, idx = _check(buf, V, k, f"pitch {ld} V {V} k {k}")
        assert int(idx.max()) < V


@pytest.mark.parametrize("off", [1, 2, 3])
def test_topk_rows_base_not_16_byte_aligned(off):
    g = torch.Generator(device="cuda").manual_seed(off)
    for V, ld in ((8112, 8112), (65, 68), (19787, 19788)):
        flat = torch.randn(3 * ld + off, device="cuda", generator=g)
        s = flat[off:].view(3, ld)
        assert s.data_ptr() % 16 != 0
        for k in (5, 32):
            _check(s, V, k, f"offset {off} V {V} ld {ld} k {k}")


def test_topk_rows_argument_checks():
    from speechclip_plus_amd import ops
    s = torch.randn(2, 16, device="cuda")
    for bad_k in (0, 33):
        with pytest.raises(RuntimeError, match="1 <= k <= 32"):
            ops.topk_rows(s, 16, bad_k)
    v, i = ops.topk_rows(s[:0], 16, 4)                                      # rows == 0: a no-op
    assert v.shape == (0, 4) and i.shape == (0, 4)


# ------------------------------------------------------------------------------------------------ neighbours against fp64
def _table_and_keywords(V, E, rows, seed):
    g = torch.Generator().manual_seed(seed)
    table = 0.01 * torch.randn(V, E, generator=g)
    own = torch.randint(0, V, (rows // 2,), generator=g)
    kw = torch.cat([table[own], 0.01 * torch.randn(rows - rows // 2, E, generator=g)])      # table rows, then free Gaussian embeddings
    return table, kw, own


def _fp64_topk(scores64, K):
    v, i = torch.sort(scores64, dim=1, descending=True, stable=True)
    return v[:, : K + 1], i[:, : K + 1]


def _criteria(vals, idx, s64, K, tol_row, cap, what):
    """vals / idx [rows, K] (host), s64 [rows, V] fp64, tol_row [rows, 1]"""
    best_v, best_i = _fp64_topk(s64, K)
    got64 = s64.gather(1, idx)
    short = (best_v[:, :K] - tol_row) - got64                               # (1) > 0: a returned column scores below the r-th best - tol
    err = (vals.double() - got64).abs() - tol_row
    print(f"{what}: worst shortfall to the fp64 r-th best {float((best_v[:, :K] - got64).max()):.3e}, worst |value - fp64 score| "
          f"{float((vals.double() - got64).abs().max()):.3e} (tol {float(tol_row.max()):.1e})")
    assert float(short.max()) <= 0, (what, float(short.max()))
    assert float(err.max()) <= 0, (what, float(err.max()))
    clear = ((best_v[:, :-1] - best_v[:, 1:]) > tol_row).all(1)            # sorted: neighbours apart = pairwise apart
    share = 1.0 - float(clear.float().mean())
    print(f"{what}: {share:.2%} of the rows have a near-tie among their {K + 1} best fp64 scores (cap {cap:.0%})")
    assert share <= cap, (what, share)
    assert torch.equal(idx[clear], best_i[clear][:, :K]), (what, int((idx[clear] != best_i[clear][:, :K]).any(1).sum()))


@pytest.mark.parametrize("V,E,K,cap", [(8112, 512, 10, 0.02), (19787, 768, 10, 0.02), (49408, 512, 32, 0.10)])
def test_keyword_neighbors_vs_fp64(V, E, K, cap):
    from speechclip_plus_amd.keyword_neighbors import keyword_neighbors
    rows = 2048
    table, kw, own = _table_and_keywords(V, E, rows, seed=0)
    vals, idx = keyword_neighbors(kw.cuda().view(rows // 8, 8, E), table.cuda(), K)
    assert vals.shape == (rows // 8, 8, K) and idx.dtype == torch.int64 and vals.dtype == torch.float32
    vals, idx = vals.view(rows, K).cpu(), idx.view(rows, K).cpu()
    t64, k64 = table.double(), kw.double()
    s64 = (k64 / k64.norm(dim=1, keepdim=True).clamp_min(1e-8)) @ (t64 / t64.norm(dim=1, keepdim=True).clamp_min(1e-8)).t()
    # table rows: rank 1 is the row's own index with score 1
    assert torch.equal(idx[: rows // 2, 0], own)
    assert float((vals[: rows // 2, 0] - 1).abs().max()) <= TOL
    _criteria(vals, idx, s64, K, torch.full((rows, 1), TOL, dtype=torch.float64), cap, f"cosine V {V} E {E} K {K}")


def test_keyword_neighbors_keywords_len_and_chunks():
    from speechclip_plus_amd.keyword_neighbors import keyword_neighbors
    V, E, K, B, N = 8112, 512, 10, 37, 9
    table, kw, _ = _table_and_keywords(V, E, B * N, seed=1)
    kw = kw[torch.randperm(B * N, generator=torch.Generator().manual_seed(2))].view(B, N, E).cuda()
    table = table.cuda()
    dense_v, dense_i = keyword_neighbors(kw, table, K)
    lens = torch.randint(1, N, (B,), generator=torch.Generator().manual_seed(3))
    lens[4], lens[5] = 0, N                                                 # a zero-keyword utterance and one at the maximum
    v, i = keyword_neighbors(kw, table, K, keywords_len=lens.cuda())
    scored = (torch.arange(N).unsqueeze(0) < lens.unsqueeze(1)).cuda()
    assert torch.equal(v[scored].view(torch.int32), dense_v[scored].view(torch.int32)) and torch.equal(i[scored], dense_i[scored])
    assert bool((v[~scored] == float("-inf")).all()) and bool((i[~scored] == -1).all())
    assert int(scored.sum()) < B * N and not bool(scored[4].any()) and bool(scored[5].all())
    # a chunk smaller than the row count that does not divide it: the same bits as one chunk
    for chunk in (128, 256):
        assert (B * N) % chunk != 0 and B * N > chunk
        cv, ci = keyword_neighbors(kw, table, K, chunk_rows=chunk)
        assert torch.equal(cv.view(torch.int32), dense_v.view(torch.int32)) and torch.equal(ci, dense_i)
    cv, ci = keyword_neighbors(kw, table, K, keywords_len=lens.cuda(), chunk_rows=128)
    assert torch.equal(cv.view(torch.int32), v.view(torch.int32)) and torch.equal(ci, i)


def test_keyword_neighbors_pseudo_inverse_vs_fp64():
    from speechclip_plus_amd.keyword_neighbors import keyword_neighbors
    V, E, K, rows = 300, 32, 10, 512
    table, kw, _ = _table_and_keywords(V, E, rows, seed=4)
    cache, table_dev = {}, table.cuda()
    vals, idx = keyword_neighbors(kw.cuda(), table_dev, K, retrieve_method="pseudo_inverse", tables=cache)
    assert vals.shape == (rows, K)
    pinv_first = cache["tables"]._pinv
    keyword_neighbors(kw.cuda(), table_dev, K, retrieve_method="pseudo_inverse", tables=cache)
    assert cache["tables"]._pinv is pinv_first                               # once per table version
    s64 = kw.double() @ torch.linalg.pinv(table.double().t()).t()
    tol_row = TOL * s64.abs().max(dim=1, keepdim=True).values
    _criteria(vals.cpu(), idx.cpu(), s64, K, tol_row, 0.02, "pseudo_inverse V 300 E 32")


def test_reference_fixture_through_the_c_abi():
    from speechclip_plus_amd import keyword_neighbors as kn
    fx = np.load(GOLDEN)
    table, ids, K = torch.from_numpy(fx["table"]).cuda(), torch.from_numpy(fx["reduced_ids"]), int(fx["K"])

    class NS:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    def model(keyword_num):
        clip = NS(selected_text_emb_ids=ids, reducedl2Original={n: int(o) for n, o in enumerate(ids.tolist())})
        return NS(config=NS(data=NS(dev_batch_size=int(fx["dev_batch_size"]))), clip=clip, subword_embd_dim=table.shape[1],
                  keyword_num=keyword_num, device="cuda")

    kw_fixed = torch.from_numpy(fx["fixed_keywords"]).cuda()
    kws = [[torch.from_numpy(fx[f"dyn_keywords_{b}"]).cuda()] for b in range(3)]
    counts = fx["dyn_counts"].tolist()
    for method in ("cosine", "pseudo_inverse"):
        out = kn.extract_fixed_keyword_neighbors(model(kw_fixed.shape[1]), K, method, table, kw_fixed, fx["fixed_gold_in"].tolist())
        assert [e["gold"] for e in out] == fx["fixed_gold_in"].tolist()
        for u, e in enumerate(out):
            for i in range(kw_fixed.shape[1]):
                pairs = e["neighbors"][f"keyword_{i}"]
                assert [t for t, _ in pairs] == fx[f"fixed_{method}_tokens"][u, i].tolist(), (method, u, i)
                assert np.abs(np.array([s for _, s in pairs]) - fx[f"fixed_{method}_scores"][u, i]).max() <= TOL, (method, u, i)
        out = kn.extract_dynamic_keyword_neighbors(model(None), K, method, [None] * 3, table, kws, fx["dyn_gold_in"].tolist(), counts)
        assert [len(e["neighbors"]) for e in out] == counts
        for u, e in enumerate(out):
            for i in range(counts[u]):
                pairs = e["neighbors"][f"keyword_{i}"]
                assert [t for t, _ in pairs] == fx[f"dyn_{method}_tokens"][u, i].tolist(), (method, u, i)
                assert np.abs(np.array([s for _, s in pairs]) - fx[f"dyn_{method}_scores"][u, i]).max() <= TOL, (method, u, i)


# ------------------------------------------------------------------------------------------------ end to end
def _make(kind, **cfg_over):
    from speechclip_plus_amd import (KWClip_GeneralTransformer, cascaded_plus_base_config, hybrid_plus_large_config,
                                     random_hubert_state_dict)
    from speechclip_plus_amd.speech_encoder import ARCHS
    large = kind == "hybrid_large"
    arch = dataclasses.replace(ARCHS["hubert_large_ll60k" if large else "hubert"], layers=2)
    sd = random_hubert_state_dict(arch, seed=41 if large else 42)
    torch.manual_seed(41 if large else 42)
    cfg = hybrid_plus_large_config() if large else cascaded_plus_base_config()
    cfg.audio_encoder.max_audio_len = -1
    for k, v in cfg_over.items():
        cfg[k] = v
    model = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, hubert_arch=arch).eval()
    with torch.no_grad():
        model.cascaded_branch.downsampling.weight_proj[1].bias.add_(-0.5)
        model.audio_encoder.weightedsum_layer.weights.copy_(torch.tensor([0.3, -0.2, 0.5]))
    return model


def _batches(model, E):
    g = torch.Generator().manual_seed(7)
    ids_vocab = model.clip.selected_text_emb_ids
    out = []
    for lens, ids in (([40000, 26000, 33000, 17000], [0, 0, 1, 2]), ([22000, 40000, 30000], [3, 4, 4])):
        B = len(lens)
        wav = torch.zeros(B, max(lens))
        for b, l in enumerate(lens):
            wav[b, :l] = torch.randn(l, generator=g) * 0.5
        text = torch.zeros(B, 77, dtype=torch.long)
        for b in range(B):
            n = 3 + b
            text[b, 0], text[b, 1: 1 + n], text[b, 1 + n] = 49406, ids_vocab[torch.randint(0, len(ids_vocab) - 2, (n,), generator=g)], 49407
        out.append({"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": torch.randn(B, E, generator=g).cuda(),
                    "id": torch.tensor(ids).cuda(), "text": text})
    return out


def _validate(model, batches):
    outs = [model.validation_step_end(model.validation_step(b, i)) for i, b in enumerate(batches)]
    return outs, model.validation_epoch_end(outs)


@pytest.mark.parametrize("kind", ["cascaded_base", "hybrid_large"])
def test_validation_detokenises_keywords_end_to_end(kind, tmp_path):
    from speechclip_plus_amd import Config
    E = 768 if kind == "hybrid_large" else 512
    model = _make(kind, log_setting=Config({"log_detokenize_results": True, "log_detokenize_results_every_n_epoch": 1}))
    model.config.trainer.default_root_dir = str(tmp_path)
    batches = _batches(model, E)
    outs, result = _validate(model, batches)
    assert all("gold_text" in o for o in outs)
    U = sum(b["wav"].shape[0] for b in batches)
    det = model.detokenized
    assert len(det) == U
    K = model.config.model_settings.cascaded_branch.keyword.detokenized_K_neighbors
    r2o = model.clip.reducedl2Original
    u = 0
    for o, b in zip(outs, batches):
        targets = o["vq_results"]["targets"].squeeze(-1).cpu()
        for x, n in enumerate(o["keywords_len"].tolist()):
            e = det[u]
            assert sorted(e["neighbors"], key=lambda s: int(s.split("_")[1])) == [f"keyword_{i}" for i in range(n)]
            ids = b["text"][x].tolist()
            assert e["gold"] == ids[: ids.index(49407) + 1]
            for i in range(n):
                pairs = e["neighbors"][f"keyword_{i}"]
                assert len(pairs) == K
                assert pairs[0][0] == r2o[int(targets[x, i])], (u, i)            # rank 1: the token the quantiser chose
                assert abs(pairs[0][1] - 1.0) <= TOL, (u, i, pairs[0][1])
            u += 1
    path = tmp_path / "retokenizeText" / "keywords_ep0.json"
    assert path.exists()
    on_disk = json.loads(path.read_text())
    assert len(on_disk) == U and on_disk[0]["neighbors"]["keyword_0"][0][0] == det[0]["neighbors"]["keyword_0"][0][0]
    assert "kw_mean_mse" in model.logged and "kw_std_mse" in model.logged and "kw_hit_rate" in model.logged
    assert 0.0 <= float(model.keyword_hits["mean"]) <= 1.0
    # K given by hand, and batches without text: the gold entry is empty, nothing breaks
    assert len(model.detokenize_keywords(outs, K=3)[0]["neighbors"]["keyword_0"]) == 3
    no_text = [{k: v for k, v in b.items() if k != "text"} for b in batches]
    outs_nt, result_nt = _validate(model, no_text)
    assert all(e["gold"] == "" for e in model.detokenized) and len(model.detokenized) == U
    # a config without log_setting: validation exactly as before, and the same retrieval tuple
    del model.config["log_setting"]
    del model.detokenized
    outs_off, result_off = _validate(model, batches)
    assert not hasattr(model, "detokenized") and all("gold_text" not in o for o in outs_off)
    assert result == result_off == result_nt
    # the inference entry: targets as ORIGINAL token ids
    wav = batches[0]["wav"][0, : 40000]
    kws = model.extract_keywords(wav)
    enc = model.encode_speech([wav])
    got = kws["vq_results"]["targets"]
    assert isinstance(got, list) and len(got) > 0 and all(isinstance(t, int) and 0 <= t < 49408 for t in got)
    assert got == [r2o[t] for t in enc["vq_results"]["targets"].flatten().tolist()]
    assert int(kws["dsample_results"]["dsample_feats_length"][0]) >= 1
