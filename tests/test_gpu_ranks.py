"""GPU: retrieval ranks (csrc/rank.hip through retrieval.mutual_ranks / mutual_recall / KWClip_GeneralTransformer.validation_epoch_end)
against int64 and fp64 on the CPU.  The rule, the ids and the degenerate case live in tests/rank_cases.py, the score builders and the
fp64 yardstick in tests/search_cases.py; every expectation is computed there, never from the kernel's own output.  Shapes are the
smallest at which the kernel can go wrong: one row / column tile and several, 1-row and 1-column tails, one slab and several, E below
one 64-wide K-tile."""
import pytest
import torch

import rank_cases as rk
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("ahead_AB", "ahead_BA", "best_AB", "best_BA")


def _ranks(A, B, a_ids, b_ids, slabs=None, cosine=False):
    from speechclip_plus_amd import mutual_ranks
    out = mutual_ranks(A.to(DEV), B.to(DEV), a_ids.to(DEV), b_ids.to(DEV), cosine=cosine, slabs=slabs)
    torch.cuda.synchronize()
    assert set(out) == set(KEYS)
    assert out["ahead_AB"].dtype == out["ahead_BA"].dtype == torch.int64 and out["best_AB"].dtype == out["best_BA"].dtype == torch.float32
    assert out["ahead_AB"].shape == out["best_AB"].shape == (A.shape[0],) and out["ahead_BA"].shape == out["best_BA"].shape == (B.shape[0],)
    return {key: v.cpu() for key, v in out.items()}


def _assert_equals_reference(got, ref):
    for key in ("ahead_AB", "ahead_BA"):
        bad = (got[key] != ref[key]).nonzero().flatten()[:5]
        assert torch.equal(got[key], ref[key]), (key, bad.tolist(), got[key][bad].tolist(), ref[key][bad].tolist())
    for key in ("best_AB", "best_BA"):
        assert torch.equal(got[key].double(), ref[key]), key             # exact integers (or -inf): the fp32 value IS the reference


def _bitwise_equal(x, y):
    return all(torch.equal(x[k], y[k]) for k in ("ahead_AB", "ahead_BA")) and \
        all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in ("best_AB", "best_BA"))


# ---------------------------------------------------------------------------------------------------- 1. exact, integer data
@pytest.mark.parametrize("nA,nB,E", ((1, 1, 64), (5, 3, 20), (129, 257, 64), (300, 130, 128)))
def test_integer_data_is_exact(nA, nB, E):
    q, gal = sc_cases.int_case(nA, nB, E, seed=nA + nB + E)
    a_ids, b_ids = rk.caption_ids(nA, nB, seed=nA)
    ref = rk.both_directions(q.long() @ gal.long().t(), a_ids, b_ids)
    for S in (1, 2, None):
        _assert_equals_reference(_ranks(q.float(), gal.float(), a_ids, b_ids, S), ref)


# ---------------------------------------------------------------------------------------------------- 2. degenerate values
def test_nan_inf_zero_rows_and_an_absent_id():
    A, B, a_ids, b_ids, ref = rk.degenerate_case()
    for S in (1, 2):
        _assert_equals_reference(_ranks(A, B, a_ids, b_ids, S), ref)


# ---------------------------------------------------------------------------------------------------- 3. slab invariance, determinism
@pytest.fixture(scope="module")
def gauss():
    q, gal, s64, bound = sc_cases.gauss_case(300, 1100, 512, 3)      # 3 row tiles, 9 column tiles, the last of each partial
    a_ids, b_ids = rk.caption_ids(300, 1100, seed=3)
    return q, gal, s64, bound, a_ids, b_ids, _ranks(q, gal, a_ids, b_ids, 1)


def test_result_does_not_depend_on_the_slab_count_or_the_run(gauss):
    q, gal, _, _, a_ids, b_ids, base = gauss
    for S in (1, 2, 7, None, None):
        assert _bitwise_equal(_ranks(q, gal, a_ids, b_ids, S), base), S


# ---------------------------------------------------------------------------------------------------- 4. accuracy, no query left out
def _interval(s64, bound, q_ids, c_ids):
    """per query: (lo, hi, best64, b*) of the module docstring of the accuracy test; has = the query has a correct candidate"""
    correct = q_ids.view(-1, 1) == c_ids.view(1, -1)
    has = correct.any(dim=1)
    ninf = torch.full_like(s64, float("-inf"))
    best64 = torch.where(correct, s64, ninf).amax(dim=1, keepdim=True)
    bstar = torch.where(correct, bound, torch.zeros_like(bound)).amax(dim=1, keepdim=True)
    above = s64 - bound > best64 + bstar
    lo = above.sum(dim=1)
    hi = (~correct & (s64 + bound >= best64 - bstar)).sum(dim=1) + (correct & above).sum(dim=1)
    return lo, hi, best64.squeeze(1), bstar.squeeze(1), has


def test_float_ranks_within_the_interval_the_bound_allows(gauss):
    """With f the kernel's score and s the fp64 score, |f - s| <= bound per pair (search_cases.yardstick: (6 Ep + 8) 2^-24 sum |a_i||b_i|,
    derived).  So the kernel's best lies within b* (the largest bound among the query's correct candidates) of the fp64 best, a
    candidate with s - bound > best64 + b* is certainly counted, and a wrong candidate is counted only if s + bound >= best64 - b*:
    lo <= ahead <= hi for EVERY query with a correct candidate, in both directions; one without has ahead = all candidates."""
    q, gal, s64, bound, a_ids, b_ids, got = gauss
    for tag, s, b, qi, ci in (("AB", s64, bound, a_ids, b_ids), ("BA", s64.t(), bound.t(), b_ids, a_ids)):
        lo, hi, best64, bstar, has = _interval(s, b, qi, ci)
        ahead, best = got["ahead_" + tag], got["best_" + tag].double()
        err = (best[has] - best64[has]).abs()
        print(f"{tag}: {int(has.sum())} of {has.numel()} queries have a correct candidate; max |best - best64| / b* = "
              f"{float((err / bstar[has]).max()):.4f}; hi - lo max = {int((hi - lo)[has].max())}; ahead == lo == hi in "
              f"{int(((ahead == lo) & (lo == hi))[has].sum())}")
        assert 0 < int(has.sum()) < has.numel()
        assert bool((err <= bstar[has]).all())
        assert bool(((lo <= ahead) & (ahead <= hi))[has].all())
        assert bool((ahead[~has] == s.shape[1]).all()) and bool(torch.isinf(best[~has]).all())


# ---------------------------------------------------------------------------------------------------- 5. planted margins
@pytest.fixture(scope="module", params=(512, 768))
def planted(request):
    q, gal, planted, s64, _ = sc_cases.planted_case(70, 1500, request.param, 10, 11)
    a_ids, b_ids = rk.planted_ids(planted, 1500)
    return sc_cases.unnormalised(q, 1), sc_cases.unnormalised(gal, 2), a_ids, b_ids, rk.both_directions(s64, a_ids, b_ids)


def test_planted_margins_give_the_fp64_ranks(planted):
    A, B, a_ids, b_ids, ref = planted
    got = _ranks(A, B, a_ids, b_ids, cosine=True)
    assert torch.equal(got["ahead_AB"], ref["ahead_AB"]) and torch.equal(got["ahead_BA"], ref["ahead_BA"])
    assert got["ahead_AB"].tolist() == [i % 10 for i in range(70)]


# ---------------------------------------------------------------------------------------------------- 6. the fused search agrees
def test_first_correct_item_of_the_fused_search_sits_at_position_ahead(gauss):
    """same operands, same arithmetic, same key order; no ties on this data: a mismatch is a finding about one of the two kernels"""
    from speechclip_plus_amd import search
    q, gal, _, _, a_ids, b_ids, got = gauss
    _, idx = search(q.to(DEV), gal.to(DEV), 32, route="fused")
    hit = b_ids[idx.cpu()] == a_ids.view(-1, 1)                      # [nA, 32]
    lead = (hit.cumsum(dim=1) == 0).sum(dim=1)                       # items in front of the first correct one; 32: there is none
    first = torch.where(lead < 32, lead, torch.full_like(lead, -1))
    ahead = got["ahead_AB"]
    short = ahead < 32
    assert 0 < int(short.sum()) < 300
    assert torch.equal(first[short], ahead[short]), (first[short][:10], ahead[short][:10])
    assert bool((first[~short] == -1).all())


# ---------------------------------------------------------------------------------------------------- 7. no matrix
def test_peak_memory_stays_far_below_the_score_matrix():
    from speechclip_plus_amd import mutual_recall
    nA, nB, E = 3000, 40000, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    A, B = torch.randn(nA, E, device=DEV, generator=g), torch.randn(nB, E, device=DEV, generator=g)
    a_ids, b_ids = torch.arange(nA, device=DEV) // 5, torch.arange(nB, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    AB, BA, mean = mutual_recall(A, B, a_ids, b_ids, [1, 10])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the inputs: {peak / 2 ** 20:.1f} MiB; the score matrix would be {nA * nB * 4 / 2 ** 20:.1f} MiB")
    assert peak < nA * nB * 4 // 4
    assert 0.0 <= AB["recall@1"] <= AB["recall@10"] <= 100.0 and set(AB) == set(BA) == set(mean) == {"recall@1", "recall@10"}


# ---------------------------------------------------------------------------------------------------- 8. metrics
def test_mutual_recall_equals_recall_from_reference_ranks(planted):
    from speechclip_plus_amd import mutual_recall, recall_from_ranks
    A, B, a_ids, b_ids, ref = planted
    ks = [1, 5, 10, 50, 2000]                                        # 2000: more than either side's candidates
    got = mutual_recall(A.to(DEV), B.to(DEV), a_ids.to(DEV), b_ids.to(DEV), recall_at=ks, cosine=True, rank_stats=True)
    want_AB = recall_from_ranks(ref["ahead_AB"], 1500, ks)
    want_BA = recall_from_ranks(ref["ahead_BA"], 70, ks)
    want = (want_AB, want_BA, {key: 0.5 * (want_AB[key] + want_BA[key]) for key in want_AB})
    for g, w in zip(got, want):
        assert set(g) == set(w) == {f"recall@{k}" for k in ks} | {"median_rank", "mean_rank"}
        # the ranks are integers: one query counted differently moves a recall by 100 / 1500 at least, a mean rank by 1 / 1500
        assert all(abs(g[key] - w[key]) < 1e-4 for key in w), (g, w)
    assert want_AB["recall@1"] == pytest.approx(10.0) and want_AB["recall@5"] == pytest.approx(50.0) and want_AB["recall@10"] == 100.0
    assert want_AB["median_rank"] == 5.5 and want_AB["mean_rank"] == 5.5
    assert want_BA["recall@2000"] == 100.0 and want_BA["recall@50"] == pytest.approx(100.0 * 70 / 1500)


# ---------------------------------------------------------------------------------------------------- 9. model level
def test_validation_epoch_end_with_fused_ranks_reports_the_same_recalls():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, mutualRetrieval, random_hubert_state_dict
    q, gal, planted_idx, _, _ = sc_cases.planted_case(70, 1500, 512, 10, 11)
    # audio i belongs to image i; its image embedding is the row planted at rank i % 10; audio 69 repeats image 3's id (a second
    # caption, and the image embedding seen last is the one kept)
    ids = torch.arange(70)
    ids[69] = 3
    img = gal[planted_idx[torch.arange(70), torch.arange(70) % 10]]
    outputs, r0 = [], 0
    for n in (7, 30, 1, 32):                                         # 4 uneven batches
        sl = slice(r0, r0 + n)
        outputs.append({"id": ids[sl].to(DEV), "parallel_audio_feat": q[sl].to(DEV), "image_feat": img[sl].to(DEV)})
        r0 += n
    state = random_hubert_state_dict(HubertArch(), seed=7122)
    results = {}
    for fused in (True, False):
        cfg = base_parallel_config()
        cfg.audio_encoder.max_audio_len = -1
        if fused:
            cfg.retrieval.fused_ranks = True
        assert ("fused_ranks" in cfg.retrieval) == fused
        torch.manual_seed(7122)
        model = KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=state).eval()
        results[fused] = model.validation_epoch_end([{"others": o} for o in outputs])
    assert results[True] == results[False], (results[True], results[False])
    # without the key: today's path, bit for bit - the recalls of mutualRetrieval on the stock matmul of the same rows
    img_ids, img_feats = torch.arange(69), img[:69].clone()           # ids in first-seen order ...
    img_feats[3] = img[69]                                           # ... image 3 with the embedding seen last
    score = q.to(DEV) @ img_feats.to(DEV).t()
    assert results[False] == mutualRetrieval(score, score.t(), ids.to(DEV), img_ids.to(DEV), [1, 5, 10])
    assert results[False][1]["recall@1"] == 100.0 and results[False][0]["recall@10"] > 95.0     # audio 3 lost its planted image
