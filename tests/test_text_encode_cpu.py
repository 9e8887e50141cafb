"""CPU checks of the caption entrance of the CLIP text tower (ClipModel.encode_text / prep_text, KWClip_GeneralTransformer.forward_text /
reportRetrieval, clip_text_hip.text_buckets, sc_text_assemble's wiring): the host logic, the errors raised before any launch and
the state-dict contract.  The arithmetic is checked on the GPU (tests/test_gpu_text_encode.py)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
from speechclip_plus_amd.clip_text import CLIP_VOCAB, EOT_TOKEN, SOT_TOKEN, ClipModel

EOT_POSITIONS = [1, 5, 12, 30, 31, 32, 33, 63, 64, 76]


def test_text_buckets_class_boundaries():
    """a caption with e + 1 <= 32 positions runs at 32, <= 64 at 64, else at 128; positions 31 | 32 and 63 | 64 are the boundaries"""
    from speechclip_plus_amd.clip_text_hip import text_buckets
    assert text_buckets(EOT_POSITIONS) == [(32, 32, [0, 1, 2, 3, 4]), (64, 64, [5, 6, 7]), (128, 77, [8, 9])]
    assert text_buckets(torch.tensor(EOT_POSITIONS)) == text_buckets(EOT_POSITIONS)
    # input order inside a class, whatever the order of the batch
    assert text_buckets([76, 3, 40, 1, 64, 33]) == [(32, 4, [1, 3]), (64, 41, [2, 5]), (128, 77, [0, 4])]


def test_text_buckets_short_captions_only():
    from speechclip_plus_amd.clip_text_hip import text_buckets
    assert text_buckets([4, 2, 11, 9, 2]) == [(32, 12, [0, 1, 2, 3, 4])]
    assert text_buckets([40, 33]) == [(64, 41, [0, 1])]           # a class without captions yields no bucket
    assert text_buckets([0]) == [(32, 1, [0])]


def test_sc_text_assemble_is_exported_declared_and_bound():
    from speechclip_plus_amd import _lib
    assert "sc_text_assemble" in _lib.SIGNATURES and len(_lib.SIGNATURES["sc_text_assemble"]) == 16
    assert hasattr(_lib.lib(), "sc_text_assemble")
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    decl = re.search(r"int sc_text_assemble\(([^;]*)\);", header)
    assert decl is not None and len(decl.group(1).split(",")) == 16          # as many parameters as the ctypes signature
    assert "clip_official.py:213-220" in header
    assert _lib.lib().sc_abi_version() == 7                                  # 7 since the encoder entry points merged; this entry was additive


def test_no_cpu_path():
    from speechclip_plus_amd import ops
    ids = torch.tensor([[SOT_TOKEN, 5, EOT_TOKEN, 0]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.text_assemble(ids, torch.zeros(CLIP_VOCAB, 8), torch.zeros(77, 8), 4, 32, 3)
    clip = ClipModel("ViT-B/32", device="cpu", layers=1)
    with pytest.raises(RuntimeError, match="device tensors only"):
        clip.encode_text(ids)
    with pytest.raises(ValueError, match="49408"):                            # the host check comes first and names the id
        clip.encode_text(torch.tensor([[SOT_TOKEN, CLIP_VOCAB, EOT_TOKEN]]))
    with pytest.raises(ValueError, match="-2"):
        clip.encode_text(torch.tensor([[SOT_TOKEN, -2, EOT_TOKEN]]))
    with pytest.raises(ValueError):
        clip.encode_text(torch.zeros(2, 78, dtype=torch.long))                # longer than the context
    with pytest.raises(TypeError):
        clip.encode_text(torch.zeros(2, 7))                                   # not integer ids
    with pytest.raises(NotImplementedError, match="text_encoder_trainable"):
        ClipModel("ViT-B/32", device="cpu", layers=1, text_encoder_trainable=True).encode_text(ids)


def test_prep_text_needs_a_tokenizer_and_follows_clip_tokenize():
    reduced = torch.tensor([0, 3, 11, SOT_TOKEN, EOT_TOKEN])
    clip = ClipModel("ViT-B/32", device="cpu", layers=1, reduce_subword_embbedding=reduced)
    with pytest.raises(RuntimeError, match="tokenizer"):
        clip.prep_text(["a dog"])

    class Tok:                                   # SimpleTokenizer's interface: encode(str) -> BPE ids
        def encode(self, s):
            return [{"a": 3, "dog": 11, "cat": 5}[w] for w in s.split()]
    clip.tokenizer = Tok()
    out = clip.prep_text(["a dog", "dog"])
    assert out.shape == (2, 77) and out.dtype == torch.int64
    # [SOT, ids, EOT, 0 ...] in original ids, then mapped to the reduced table: 0 -> 0, 3 -> 1, 11 -> 2, SOT -> 3, EOT -> 4
    assert out[0].tolist() == [3, 1, 2, 4] + [0] * 73 and out[1].tolist() == [3, 2, 4] + [0] * 74
    with pytest.raises(ValueError, match="token id 5 "):
        clip.prep_text(["a cat"])
    full = ClipModel("ViT-B/32", device="cpu", layers=1)
    full.tokenizer = Tok()
    out = full.prep_text(["a dog", "dog"])
    assert out[0].tolist() == [SOT_TOKEN, 3, 11, EOT_TOKEN] + [0] * 73 and out[1].tolist() == [SOT_TOKEN, 11, EOT_TOKEN] + [0] * 74
    with pytest.raises(RuntimeError, match="too long"):
        full.prep_text(["dog " * 76])


@pytest.fixture(scope="module")
def models():
    reduced = torch.cat([torch.tensor([0, 320, 7, 1929]), torch.tensor([SOT_TOKEN, EOT_TOKEN])])
    plain = KWClip_GeneralTransformer(base_parallel_config(), device="cpu")
    cfg = base_parallel_config()
    cfg.clip["layers"] = 1
    cfg.clip["reduce_subword_embbedding"] = reduced
    with_text = KWClip_GeneralTransformer(cfg, device="cpu", text_encoder="clip")
    return plain, with_text, reduced


def test_forward_text_maps_original_ids_without_touching_the_callers_tensor(models):
    _, m, reduced = models
    text = torch.tensor([[SOT_TOKEN, 320, 1929, EOT_TOKEN, 0, 0], [SOT_TOKEN, 7, EOT_TOKEN, 0, 0, 0]])
    keep = text.clone()
    mapped = m.clip.to_reduced_ids(text)
    assert mapped.tolist() == [[4, 1, 3, 5, 0, 0], [4, 2, 5, 0, 0, 0]] and torch.equal(text, keep)
    assert mapped.argmax(-1).tolist() == [3, 2]                  # the end-of-text token has the largest id of the reduced table too
    # forward_text: the mapping passes, the tower then refuses the CPU - and the caller's ids are still the original ones
    with pytest.raises(RuntimeError, match="device tensors only"):
        m.forward_text(text)
    assert torch.equal(text, keep)
    with pytest.raises(ValueError, match="token id 9 "):
        m.forward_text(torch.tensor([[SOT_TOKEN, 9, EOT_TOKEN]]))
    with pytest.raises(ValueError, match=str(CLIP_VOCAB + 5)):   # outside the CLIP vocabulary: refused, never an index into the lookup
        m.forward_text(torch.tensor([[SOT_TOKEN, CLIP_VOCAB + 5, EOT_TOKEN]]))
    with pytest.raises(ValueError):
        m.forward_text(torch.zeros(2, 3, 4, dtype=torch.long))
    with pytest.raises(TypeError):
        m.forward_text({"text": text})
    with pytest.raises(RuntimeError, match="tokenizer"):
        m.forward_text(["a dog"])
    # full vocabulary: ids pass through unmapped
    full = ClipModel("ViT-B/32", device="cpu", layers=1)
    assert full.to_reduced_ids(text) is text


def test_text_encoder_argument_and_state_dict_contract(models):
    plain, m, _ = models
    with pytest.raises(RuntimeError, match='text_encoder="clip"'):
        plain.forward_text(torch.tensor([[SOT_TOKEN, EOT_TOKEN]]))
    with pytest.raises(ValueError, match="'clip'"):
        KWClip_GeneralTransformer(base_parallel_config(), device="cpu", text_encoder="bert")
    assert plain.clip is None and not any(k.startswith("clip.") for k in plain.state_dict())
    keys = [k for k in m.state_dict() if k.startswith("clip.")]
    assert keys and all(k.startswith("clip.model.") for k in keys)
    assert "clip.model.token_embedding.weight" in keys and m.state_dict()["clip.model.token_embedding.weight"].shape == (6, 512)
    assert set(m.state_dict()) - set(keys) == set(plain.state_dict())
    # the text tower is frozen and never trainable
    names = lambda mod: sorted(n for n, p in mod.named_parameters() if any(p is q for q in mod.getTrainableParams()))
    assert names(m) == names(plain) and not any(n.startswith("clip.") for n in names(m))
    assert all(not p.requires_grad for p in m.clip.parameters())
    # a text tower alone is no keyword branch
    with pytest.raises(RuntimeError, match="needs a keyword branch"):
        m._token_table()
    m.config["log_setting"] = {"log_detokenize_results": True}
    try:
        assert m._detokenize_enabled() is False
    finally:
        del m.config["log_setting"]


def test_text_tower_loads_from_a_reference_checkpoint_by_name():
    cfg = base_parallel_config()
    cfg.clip["layers"] = 1
    src = ClipModel("ViT-B/32", device="cpu", layers=1, seed=99)
    ck = {"clip.model." + k: v.clone() for k, v in src.model.state_dict().items()}
    ck["clip.model.logit_scale"] = torch.tensor(4.6)
    m = KWClip_GeneralTransformer.from_reference_checkpoint(cfg, ck, device="cpu", text_encoder="clip")
    for k, v in ck.items():
        if k != "clip.model.logit_scale":
            assert torch.equal(m.state_dict()[k], v), k
    assert set(ck) - {"clip.model.logit_scale"} <= set(m._reference_load_report["loaded"])


def test_report_retrieval_returns_and_logs_what_mutual_retrieval_gives(models):
    from speechclip_plus_amd.retrieval import mutualRetrieval
    _, m, _ = models
    fx = dict(np.load(os.path.join(GOLDEN, "retrieval.npz")))
    score = torch.from_numpy(fx["score"])
    a_ids, b_ids = torch.from_numpy(fx["a_ids"]), torch.from_numpy(fx["b_ids"])
    want = mutualRetrieval(score_per_A=score, score_per_B=score.t(), AB_answers=a_ids, BA_answers=b_ids, recall_at=m.recall_at,
                           modality_A_title="audio", modality_B_title="text")
    assert [want[0][f"recall@{k}"] for k in (1, 5, 10)] == pytest.approx(fx["AB"].tolist())      # the reference's own numbers
    meta = {"modality_A_title": "audio", "modality_B_title": "text", "modality_A_logAbbr": "A", "modality_B_logAbbr": "T"}
    m.logged = {}
    got = m.reportRetrieval(score_per_A=score, score_per_B=score.t(), AB_answers=a_ids, BA_answers=b_ids, metadata=meta)
    assert got == want
    assert set(m.logged) == {"val_recall_AT", "val_recall_TA", "val_recall_mean", "val_recall_mean_10"}
    assert (m.logged["val_recall_AT"], m.logged["val_recall_TA"], m.logged["val_recall_mean"]) == want
    assert m.logged["val_recall_mean_10"] == want[2]["recall@10"]
    m.logged = {}
    m.reportRetrieval(score_per_A=score, score_per_B=score.t(), AB_answers=a_ids, BA_answers=b_ids)           # default: audio / image
    assert {"val_recall_AI", "val_recall_IA"} <= set(m.logged)
    for missing in meta:
        with pytest.raises(AssertionError):
            m.reportRetrieval(score_per_A=score, score_per_B=score.t(), AB_answers=a_ids, BA_answers=b_ids,
                              metadata={k: v for k, v in meta.items() if k != missing})
