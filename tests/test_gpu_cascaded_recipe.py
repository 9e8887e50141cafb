"""GPU: the original SpeechCLIP cascaded recipe (config/speechCLIP/model_base/spchclp_c.yaml: KW_CascadedBranch, 8 learned keyword
queries) at its OWN dimensions - 1 head of 768, Linear 768 -> 512, eachKw BatchNorm, vocabulary 8 112, 12-layer ViT-B/32 text
tower, HuBERT-base order at 2 layers - against the restatement of tests/kwpool_cases.cascaded_ref: one whole train step (forward
dict, contrastive loss, every trainable gradient), then evaluation on the running statistics, keyword extraction and validation.

The criteria are those of tests/test_gpu_recipes.py::test_plus_recipe_train_step_vs_oracle_at_full_dims: a token differs from the
restatement's only where the restatement's own margin is below NEAR_TIE; agreement >= 0.9; with the discrete choices shared,
unit-norm embeddings cosine >= 0.999, |loss difference| <= 1e-2, gradients rel-L2 <= 6e-2 (the weighted-sum logits 8e-2: nearly
scalars, a small difference of large per-frame terms that carry the bf16 noise of the features).

The seed (42) was chosen on the CPU: the fp32 restatement on fp32 encoder features against the same restatement on the
oracle.bf16_store emulation of the device encoder agrees on 48 of 48 tokens (seeds 43 and 44: 46 of 48, worst flipped margin
8e-4) - the 0.9 is a cap, not a measurement."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import kwpool_cases as kc

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-2
SEED = 42


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-20))


@pytest.fixture(scope="module")
def setup():
    import oracle
    from speechclip_plus_amd import KWClip_GeneralTransformer, cascaded_base_config, random_hubert_state_dict, set_dropout
    from speechclip_plus_amd.speech_encoder import ARCHS
    arch = dataclasses.replace(ARCHS["hubert"], layers=2)
    sd = random_hubert_state_dict(arch, seed=SEED)
    torch.manual_seed(SEED)
    cfg = cascaded_base_config()
    cfg.audio_encoder.max_audio_len = -1
    cfg.log_setting = {"log_detokenize_results": True, "log_detokenize_results_every_n_epoch": 1}
    model = set_dropout(KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, hubert_arch=arch).train(), False)
    with torch.no_grad():
        model.audio_encoder.weightedsum_layer.weights.copy_(torch.tensor([0.3, -0.2, 0.5]))
    o_arch = oracle.HubertArch.base()
    o_arch.layers = 2
    g = torch.Generator().manual_seed(7)
    lens = [40000, 26000, 33000, 17000, 40000, 22000]
    wavs = [torch.randn(l, generator=g) * 0.5 for l in lens]
    wav = torch.zeros(len(lens), max(lens))
    for b, w in enumerate(wavs):
        wav[b, : len(w)] = w
    img = torch.randn(len(lens), 512, generator=g)
    ids = torch.tensor([0, 0, 1, 2, 2, 3])
    batch = {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": img.cuda(), "id": ids.cuda()}
    hs, fl = oracle.speech_encoder_forward(sd, o_arch, wavs)               # the encoder restatement, computed once
    return {"model": model, "oracle": oracle, "wavs": wavs, "batch": batch, "img": img, "ids": ids, "hs": hs, "fl": fl}


def test_cascaded_recipe_train_step_vs_restatement_at_full_dims(setup):
    model, oracle, img, ids, hs, fl = (setup[k] for k in ("model", "oracle", "img", "ids", "hs", "fl"))
    from speechclip_plus_amd import KW_CascadedBranch
    br = model.cascaded_branch
    assert isinstance(br, KW_CascadedBranch) and model.keyword_num == 8
    assert br.self_att.multihead_attn_layer.num_heads == 1 and br.self_att.multihead_attn_layer.embed_dim == 768
    assert model.clip.model.token_embedding.weight.shape == (8112, 512) and len(model.clip.model.transformer.resblocks) == 12
    B, K = len(ids), 8
    model.train()
    W = {k: v.detach().cpu().float().clone() for k, v in br.state_dict().items()}       # before the step: running buffers at init
    model.zero_grad(set_to_none=True)
    losses_, log_metrics, others = model(setup["batch"])
    out = model.compute_loss(losses_)
    out["loss"].backward()
    assert others["keywords"].shape == (B, K, 512) and others["dsample_results"] is None and others["keywords_len"] is None
    tok_hip = others["vq_results"]["targets"].reshape(B, K).cpu()
    for k in W:
        if not k.startswith("clip.") and W[k].is_floating_point() and "running_" not in k:
            W[k].requires_grad_(True)
    ws_w = model.audio_encoder.weightedsum_layer.weights.detach().cpu().clone().requires_grad_(True)
    assert not model.criterion.temperature_trainable                      # (the base yaml: a fixed temperature of 0.07)
    inv_t = float(model.criterion.temperature)
    kw = dict(nhead=1, training=True, nhead_clip=8, sot=model.clip.startOfTxt_reduced, eot=model.clip.endOfTxt_reduced)

    def run(forced):
        aux = {}
        feat = oracle.weighted_sum(ws_w, [h.detach() for h in hs], False)
        return kc.cascaded_ref(W, feat, fl, forced_tokens=forced, aux=aux, **kw), aux

    with torch.no_grad():
        _, aux = run(None)
    differ = tok_hip != aux["tokens"]
    cos = aux["cos"]
    margin = cos.gather(-1, aux["tokens"].unsqueeze(-1)) - cos.gather(-1, tok_hip.unsqueeze(-1))
    worst = float(margin[differ.unsqueeze(-1)].max()) if differ.any() else 0.0
    agreement = 1.0 - float(differ.sum()) / float(differ.numel())
    print(f"cascaded_base: token agreement {agreement:.3f} over {differ.numel()} keywords; worst margin of a flipped one {worst:.2e}")
    assert worst < NEAR_TIE, (margin[differ.unsqueeze(-1)], int(differ.sum()))
    assert agreement >= 0.9, agreement
    # ---- the discrete choices shared: everything continuous
    (casc, kws), aux = run(tok_hip)
    i_n = img / img.norm(dim=-1, keepdim=True)
    c_n = casc / casc.norm(dim=-1, keepdim=True)
    loss_o = oracle.masked_contrastive_loss(c_n, i_n, ids, inv_temperature=inv_t)
    cos_c = F.cosine_similarity(others["cascaded_audio_feat"].detach().float().cpu(), c_n.detach(), dim=-1)
    assert float(cos_c.min()) > 0.999, cos_c
    assert abs(out["c_cl_loss"].item() - loss_o.item()) < 1e-2, (out["c_cl_loss"].item(), loss_o.item())
    assert abs(out["loss"].item() - loss_o.item()) < 1e-2
    assert rel(others["keywords"], kws) < 1e-5                                    # same tokens -> same table rows
    loss_o.backward()
    # A bias in front of the train-mode BatchNorm shifts every utterance of a (slot, channel) alike and the batch mean takes the shift
    # out again: the gradients of linear_proj.bias and of the LayerNorm bias (which reaches the BatchNorm through the linear
    # projection) are ZERO in exact arithmetic.  What either side holds is the rounding residue of a cancelling sum, so the two are
    # not compared with each other; each must be small against the gradient of its module's weight (the same 6e-2).
    zero = {"linear_proj.bias": "linear_proj.weight", "self_att.attentionBlock_Norm.bias": "self_att.attentionBlock_Norm.weight"}
    errs = {}
    for n_, p in br.named_parameters():
        if not p.requires_grad:
            continue
        ref = W[n_].grad
        assert p.grad is not None and ref is not None, n_
        if n_ in zero:
            scale = float(W[zero[n_]].grad.norm())
            assert float(ref.norm()) <= 1e-4 * scale, (n_, float(ref.norm()), scale)          # the premise, on the restatement
            errs[n_] = float(p.grad.float().norm()) / scale
        elif float(ref.norm()) > 1e-7:
            errs[n_] = rel(p.grad, ref)
    errs["weightedsum"] = rel(model.audio_encoder.weightedsum_layer.weights.grad, ws_w.grad)
    for k, v in errs.items():
        print(f"PARITY|cascaded_base|d {k}|{v:.3e}|{8e-2 if k == 'weightedsum' else 6e-2:.1e}", flush=True)
    assert {"cls", "self_att.multihead_attn_layer.in_proj_weight", "linear_proj.weight", "bn_layer.bn_layer.weight"} <= set(errs)
    bad = {k: v for k, v in errs.items() if v > (8e-2 if k == "weightedsum" else 6e-2)}
    assert not bad, (bad, errs)
    # the running statistics after this one step: the restatement's (they are means over the keyword rows, which carry the bf16
    # noise of the features like every gradient above: the same 6e-2)
    bn = br.bn_layer.bn_layer
    assert int(bn.num_batches_tracked) == 1
    assert rel(bn.running_mean, aux["running_mean"]) < 6e-2 and rel(bn.running_var, aux["running_var"]) < 6e-2
    setup["trained"] = True


def test_cascaded_recipe_eval_keywords_and_validation(setup):
    """Eval: the BatchNorm uses the running statistics (the restatement on the same buffers picks the same tokens up to near-ties),
    extract_keywords returns 8 original CLIP ids per utterance, validation runs with audio_feat_src: cascaded and the keywords
    detokenise through the fixed-count route."""
    model, oracle, hs, fl, wavs = (setup[k] for k in ("model", "oracle", "hs", "fl", "wavs"))
    br = model.cascaded_branch
    model.eval()
    bn = br.bn_layer.bn_layer
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    vs = model.validation_step(setup["batch"])
    others = model.validation_step_end(vs)
    assert torch.equal(before[0], bn.running_mean) and torch.equal(before[1], bn.running_var) and before[2] == int(bn.num_batches_tracked)
    W = {k: v.detach().cpu().float().clone() for k, v in br.state_dict().items()}
    aux = {}
    with torch.no_grad():
        feat = oracle.weighted_sum(model.audio_encoder.weightedsum_layer.weights.detach().cpu(), list(hs), False)
        kc.cascaded_ref(W, feat, fl, nhead=1, training=False, nhead_clip=8, sot=model.clip.startOfTxt_reduced,
                        eot=model.clip.endOfTxt_reduced, aux=aux)
    tok = others["vq_results"]["targets"].reshape(len(wavs), 8).cpu()
    differ = tok != aux["tokens"]
    margin = aux["cos"].gather(-1, aux["tokens"].unsqueeze(-1)) - aux["cos"].gather(-1, tok.unsqueeze(-1))
    assert (float(margin[differ.unsqueeze(-1)].max()) if differ.any() else 0.0) < NEAR_TIE
    assert 1.0 - float(differ.sum()) / differ.numel() >= 0.9
    # the discrete choices shared (the device's tokens forced into the restatement): the embeddings, always
    with torch.no_grad():
        casc, _ = kc.cascaded_ref(W, feat, fl, nhead=1, training=False, nhead_clip=8, sot=model.clip.startOfTxt_reduced,
                                  eot=model.clip.endOfTxt_reduced, forced_tokens=tok)
    c_n = casc / casc.norm(dim=-1, keepdim=True)
    cos_c = F.cosine_similarity(others["cascaded_audio_feat"].float().cpu(), c_n, dim=-1)
    assert float(cos_c.min()) > 0.999, cos_c
    # inference entry: 8 tokens per utterance as ORIGINAL CLIP ids
    res = model.extract_keywords(wavs[1].cuda())
    targets = res["vq_results"]["targets"]
    originals = set(model.clip.selected_text_emb_ids.tolist())
    assert len(targets) == 8 and all(t in originals for t in targets) and res["dsample_results"] is None
    # validation: retrieval over the cascaded embeddings, detokenised keywords through the fixed-count route
    assert model.config.retrieval.audio_feat_src == "cascaded"
    recall = model.validation_epoch_end([others])
    assert recall is not None
    entries = model.detokenize_keywords([others])
    assert len(entries) == len(wavs)
    assert all(len(e["neighbors"]) == 8 and all(len(v) == 5 for v in e["neighbors"].values()) for e in entries)
