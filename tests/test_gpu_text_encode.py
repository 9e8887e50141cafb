"""GPU: caption tokens through the frozen CLIP text tower - sc_text_assemble bit for bit against torch, ClipModel.encode_text against
transformers' fixture and against the CPU oracle at all three segment classes, batch independence, the unbucketed baseline, the
forward-only tower, and forward_text / reportRetrieval on a model with a reduced vocabulary."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EOT_POSITIONS = [1, 5, 12, 30, 31, 32, 33, 63, 64, 76]
NAN_BITS = 0x7FC0


def rel(a, b):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return float((a - b).norm() / b.norm())


def _bits(x):
    return x.contiguous().view(torch.int16)


def _assemble_case(B, Bp, SEG, n_pos, W, V, L, ids_pitch, table_pitch, seed):
    from speechclip_plus_amd import ops
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V, table_pitch, generator=g).cuda()[:, :W]           # leading dimension table_pitch
    pos = (torch.randn(77, W, generator=g) * 0.3).cuda()
    store = torch.randint(0, V - 2, (B, ids_pitch), generator=g)
    ids = store[:, :L]                                                        # row stride ids_pitch
    ends = torch.randint(1, n_pos, (B,), generator=g)
    for b in range(B):
        ids[b, int(ends[b])] = V - 1
        ids[b, int(ends[b]) + 1:] = 0
    if B >= 2:
        ids[0, :] = 0
        ids[0, 0], ids[0, 1] = V - 2, V - 1                                   # [SOT, EOT] only
        ids[1, :] = 0
        ids[1, :5] = torch.tensor([V - 2, 3, V - 1, 4, V - 1])                # the largest id twice: the first position wins
    ids_d = store.cuda()[:, :L]
    out = torch.full((Bp * SEG, W), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    X, eot_row, bad = ops.text_assemble(ids_d, table, pos, Bp, SEG, n_pos, out=out)
    assert X.data_ptr() == out.data_ptr()
    want = torch.zeros(Bp, SEG, W, device="cuda", dtype=torch.bfloat16)
    want[:B, :n_pos] = (table[ids_d[:, :n_pos]] + pos[:n_pos]).to(torch.bfloat16)
    assert torch.equal(_bits(X.view(Bp, SEG, W)), _bits(want))
    assert not bool((_bits(X) == NAN_BITS).all(dim=1).any())                  # no row left as it was
    assert float(X.view(Bp, SEG, W)[:B, n_pos:].float().abs().sum()) == 0 and float(X.view(Bp, SEG, W)[B:].float().abs().sum()) == 0
    assert eot_row.dtype == torch.int32
    assert eot_row.tolist() == (torch.arange(B) * SEG + ids.argmax(-1)).tolist()
    if B >= 2:
        assert eot_row[:2].tolist() == [1, SEG + 2]
    assert int(bad) == 0


@pytest.mark.parametrize("B,Bp,SEG,n_pos,W,V,L,ids_pitch,table_pitch", [
    (5, 8, 32, 12, 128, 100, 77, 77, 128),        # pad samples, a prefix shorter than the segment
    (3, 4, 64, 33, 520, 100, 40, 50, 520),        # a column count that wraps the 512-column thread loop; strided id rows
    (2, 2, 128, 77, 8, 50, 77, 77, 16),           # fewer columns than one thread stride; a table with a leading dimension
])
def test_text_assemble_bit_exact(B, Bp, SEG, n_pos, W, V, L, ids_pitch, table_pitch):
    _assemble_case(B, Bp, SEG, n_pos, W, V, L, ids_pitch, table_pitch, seed=B * 1000 + W)


def test_text_assemble_counts_and_neutralises_bad_input():
    """an id of V + 3, an id of -1 (zero embedding, nothing read outside the table) and an end-of-text position behind the prefix
    (clamped): three counts, and a counter handed in is added to"""
    from speechclip_plus_amd import ops
    B, Bp, SEG, n_pos, W, V = 3, 4, 32, 6, 128, 100
    g = torch.Generator().manual_seed(5)
    table, pos = torch.randn(V, W, generator=g).cuda(), torch.randn(77, W, generator=g).cuda()
    ids = torch.tensor([[98, 5, V + 3, 7, 6, 0, 0, 0, 0, 0],
                        [98, -1, 4, 99, 0, 0, 0, 0, 0, 0],
                        [98, 1, 2, 3, 4, 5, 6, 7, 99, 0]])
    X, eot_row, bad = ops.text_assemble(ids.cuda(), table, pos, Bp, SEG, n_pos)
    assert int(bad) == 3
    assert eot_row.tolist() == [2, SEG + 3, 2 * SEG + n_pos - 1]
    X = X.view(Bp, SEG, W)
    assert torch.equal(_bits(X[0, 2]), _bits(pos[2].to(torch.bfloat16))) and torch.equal(_bits(X[1, 1]), _bits(pos[1].to(torch.bfloat16)))
    safe = ids.clamp(0, V - 1).cuda()
    want = (table[safe[:, :n_pos]] + pos[:n_pos]).to(torch.bfloat16)
    keep = torch.ones(B, n_pos, dtype=torch.bool)
    keep[0, 2] = keep[1, 1] = False
    assert torch.equal(_bits(X[:B, :n_pos])[keep], _bits(want)[keep])
    assert float(X[:B, n_pos:].float().abs().sum()) == 0 and float(X[B:].float().abs().sum()) == 0
    _, _, bad2 = ops.text_assemble(ids.cuda(), table, pos, Bp, SEG, n_pos, bad=bad)
    assert bad2 is bad and int(bad) == 6


def test_encode_text_vs_hf_fixture(golden):
    """plain token ids against transformers' CLIPTextModelWithProjection (tests/golden/clip_text_w128.npz: ``out_ids``); the captions end
    at 4, 2, 76, 11 and 9: the 32 and the 128 class both run.  Bound: the one this tower holds against this fixture (bf16 storage
    between kernels, fp32 accumulation)."""
    from conftest import weights_from
    from speechclip_plus_amd import clip_text
    from speechclip_plus_amd.clip_text_hip import text_buckets
    fx = golden("clip_text_w128.npz")
    W = {k[len("clip.model."):]: v for k, v in weights_from(fx).items()}
    V = W["token_embedding.weight"].shape[0]
    clip_text.CLIP_TEXT_ARCHS["hf-fixture-w128"] = dict(width=128, heads=int(fx["heads"]), layers=2, embed_dim=W["text_projection"].shape[1])
    try:
        vocab = torch.cat([torch.arange(V - 2), torch.tensor([clip_text.SOT_TOKEN, clip_text.EOT_TOKEN])])
        clip = clip_text.ClipModel("hf-fixture-w128", device="cuda:0", reduce_subword_embbedding=vocab).eval()
    finally:
        del clip_text.CLIP_TEXT_ARCHS["hf-fixture-w128"]
    clip.model.load_state_dict({k: v for k, v in W.items()}, strict=True)
    ids = torch.from_numpy(fx["ids"])
    assert ids.argmax(-1).tolist() == [4, 2, 76, 11, 9]
    assert [(s, n) for s, n, _ in text_buckets(ids.argmax(-1).tolist())] == [(32, 12), (128, 77)]
    ref = torch.from_numpy(fx["out_ids"])
    out = clip.encode_text(ids.cuda())
    assert out.shape == ref.shape and out.dtype == torch.float32 and not out.requires_grad
    assert rel(out, ref) < 2e-2, rel(out, ref)
    assert rel(clip.encode_text(ids.cuda(), bucket=False), ref) < 2e-2
    assert int(clip.text_bad) == 0


@pytest.fixture(scope="module")
def oracle_case():
    """ClipModel ViT-B/32 at 3 layers with perturbed LayerNorms, 10 captions ending at EOT_POSITIONS, and the fp32 CPU reference:
    oracle.clip_text_transformer over all 77 positions -> ln_final -> end-of-text row -> @ text_projection (computed once)."""
    import oracle
    from speechclip_plus_amd.clip_text import EOT_TOKEN, SOT_TOKEN, ClipModel
    torch.manual_seed(2)
    clip = ClipModel("ViT-B/32", device="cuda:0", layers=3).eval()
    core = clip.model
    with torch.no_grad():
        for blk in core.transformer.resblocks:
            for ln in (blk.ln_1, blk.ln_2):
                ln.weight.add_(torch.randn_like(ln.weight) * 0.1)
                ln.bias.add_(torch.randn_like(ln.bias) * 0.1)
        core.ln_final.weight.add_(torch.randn_like(core.ln_final.weight) * 0.1)
        core.ln_final.bias.add_(torch.randn_like(core.ln_final.bias) * 0.1)
    W = {"model." + k: v.detach().cpu().float() for k, v in core.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    B = len(EOT_POSITIONS)
    ids = torch.zeros(B, 77, dtype=torch.long)
    for b, e in enumerate(EOT_POSITIONS):
        ids[b, 0] = SOT_TOKEN
        ids[b, 1:e] = torch.randint(1, 49406, (e - 1,), generator=g)
        ids[b, e] = EOT_TOKEN
    ids[2, 13:40] = torch.randint(1, 49406, (27,), generator=g)           # junk behind the end-of-text token: causal, never seen
    with torch.no_grad():
        x = W["model.token_embedding.weight"][ids] + W["model.positional_embedding"]
        y = oracle.clip_text_transformer(W, "model.", x, heads=8)
        y = F.layer_norm(y, (512,), W["model.ln_final.weight"], W["model.ln_final.bias"])
        ref = y[torch.arange(B), torch.tensor(EOT_POSITIONS)] @ W["model.text_projection"]
    return clip, ids, ref


def test_encode_text_matches_the_oracle_at_all_three_classes(oracle_case):
    clip, ids, ref = oracle_case
    out = clip.encode_text(ids.cuda())
    assert out.shape == (10, 512) and out.dtype == torch.float32
    assert rel(out, ref) < 2e-2, rel(out, ref)
    # ids on the host: positions computed there, the same launches
    assert torch.equal(clip.encode_text(ids), out)
    assert torch.equal(clip.encode_text(ids.cuda().to(torch.int32)), out)
    assert int(clip.text_bad) == 0
    with pytest.raises(ValueError, match="49408"):
        bad = ids.clone()
        bad[3, 2] = 49408
        clip.encode_text(bad.cuda())


def test_encode_text_batch_independence_and_baseline(oracle_case, monkeypatch):
    """a caption's embedding does not depend on its neighbours, its place in the batch, the bucketing or the chunking; different
    attention kernels serve different classes, so the bound is the tower's 2e-2 and not equality"""
    from speechclip_plus_amd import clip_text_hip
    clip, ids, ref = oracle_case
    out = clip.encode_text(ids.cuda())
    perm = torch.tensor([7, 2, 9, 0, 5, 3, 8, 1, 6, 4])
    inv = torch.argsort(perm)
    out_p = clip.encode_text(ids[perm].cuda())[inv.cuda()]
    assert rel(out_p, out) < 2e-2 and rel(out_p, ref) < 2e-2, (rel(out_p, out), rel(out_p, ref))
    flat = clip.encode_text(ids.cuda(), bucket=False)
    assert rel(flat, out) < 2e-2 and rel(flat, ref) < 2e-2, (rel(flat, out), rel(flat, ref))
    one = clip.encode_text(ids[4:5].cuda())                                  # a batch of one, padded to a whole attention block
    assert rel(one, ref[4:5]) < 2e-2
    monkeypatch.setattr(clip_text_hip, "TEXT_CHUNK_ROWS", 128)               # 4 / 2 / 1 captions per tower call
    chunked = clip.encode_text(ids.cuda())
    assert rel(chunked, out) < 2e-2 and rel(chunked, ref) < 2e-2, (rel(chunked, out), rel(chunked, ref))


@pytest.mark.parametrize("causal", [32, 64, 1])
def test_tower_forward_only_keeps_nothing_and_gives_the_same_bits(oracle_case, causal):
    from speechclip_plus_amd.clip_text_hip import tower_forward
    clip = oracle_case[0]
    g = torch.Generator().manual_seed(causal)
    X = (torch.randn(256, 512, generator=g) * 0.5).to(torch.bfloat16).cuda()
    weights = clip._tower_weights(X.device)
    full, saved = tower_forward(X, weights, 8, causal)
    fwd, nothing = tower_forward(X, weights, 8, causal, save=False)
    assert len(saved) == 3 and nothing == []
    assert torch.equal(_bits(fwd), _bits(full)) and bool(torch.isfinite(fwd.float()).all())


def test_forward_text_reduced_vocabulary_and_speech_to_text_retrieval():
    """forward_text maps ORIGINAL ids onto a reduced table (the caller's tensor untouched) and gives encode_text's bits for the reduced
    ids; on a parallel model with text_encoder="clip" its output and encode_speech's feed reportRetrieval"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    from speechclip_plus_amd.clip_text import EOT_TOKEN, SOT_TOKEN
    from speechclip_plus_amd.speech_encoder import ARCHS
    g = torch.Generator().manual_seed(31)
    vocab = torch.cat([torch.tensor([0]), torch.randperm(49405, generator=g)[:500] + 1, torch.tensor([SOT_TOKEN, EOT_TOKEN])])
    arch = dataclasses.replace(ARCHS["hubert"], layers=2)
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    cfg.clip["layers"] = 2
    cfg.clip["reduce_subword_embbedding"] = vocab
    model = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=random_hubert_state_dict(arch, seed=3), hubert_arch=arch,
                                      text_encoder="clip").eval()
    assert model.clip.model.token_embedding.weight.shape == (503, 512)
    ends = [3, 9, 1, 40, 17, 6]
    text = torch.zeros(6, 77, dtype=torch.long)
    reduced = torch.zeros(6, 77, dtype=torch.long)
    for b, e in enumerate(ends):
        pick = torch.randint(1, 501, (e - 1,), generator=g)
        text[b, 0], text[b, 1:e], text[b, e] = SOT_TOKEN, vocab[pick], EOT_TOKEN
        reduced[b, 0], reduced[b, 1:e], reduced[b, e] = 501, pick, 502
    text_d = text.cuda()
    keep = text_d.clone()
    feat = model.forward_text(text_d)
    assert torch.equal(text_d, keep)
    assert feat.shape == (6, 512) and torch.equal(feat, model.clip.encode_text(reduced.cuda()))
    assert torch.equal(model.forward_text(text), feat)                       # host ids
    absent = next(i for i in range(1, 49406) if i not in set(vocab.tolist()))
    with pytest.raises(ValueError, match=f"token id {absent} "):
        wrong = text_d.clone()
        wrong[1, 2] = absent
        model.forward_text(wrong)
    wavs = [torch.randn(n, generator=g) * 0.5 for n in (9000, 12000, 8000, 16000, 10000, 11000)]
    with torch.no_grad():
        audio = model.encode_speech([w.cuda() for w in wavs])["parallel_audio_feat"].float()
    assert audio.shape == (6, 512)
    score = F.normalize(audio, dim=-1) @ F.normalize(feat, dim=-1).t()
    ids = torch.arange(6)
    AT, TA, mean = model.reportRetrieval(score_per_A=score, score_per_B=score.t(), AB_answers=ids, BA_answers=ids,
                                         metadata={"modality_A_title": "audio", "modality_B_title": "text",
                                                   "modality_A_logAbbr": "A", "modality_B_logAbbr": "T"})
    for d in (AT, TA, mean):
        assert set(d) == {"recall@1", "recall@5", "recall@10"} and all(0.0 <= v <= 100.0 for v in d.values())
    assert AT["recall@10"] == TA["recall@10"] == 100.0                       # 6 candidates: everything is inside the top 10
    assert {"val_recall_AT", "val_recall_TA", "val_recall_mean", "val_recall_mean_10"} <= set(model.logged)
