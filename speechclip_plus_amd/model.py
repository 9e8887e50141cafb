"""KWClip_GeneralTransformer: host-side mirror of avssl/model/kwClip.py for the contrastive hot path.

Kept API: ``forward(batch) -> (losses, log_metrics, others)`` with the reference's keys
(kwClip.py:898-963), ``compute_loss(dict)`` (:999-1040), ``encode_speech(wav)`` (:1042-1091),
``feature_extractor_s3prl(wav)`` (:965-997), ``processWavs`` (:600-615), ``getTrainableParams``,
``training_step`` / ``training_step_end`` semantics (:145-193) so it drops into the existing
PyTorch-Lightning loop (it is a plain ``nn.Module``; pytorch_lightning is not installed here).

``batch["image"]`` may already hold the CLIP image embeddings (B, E).  For pixel input (the reference's ``load_image: true``
recipes) pass ``image_encoder="clip"``: the frozen CLIP image tower of ``config.clip.name`` on the library's kernels
(clip_image.ClipImageEncoder, weights from a reference checkpoint's ``clip.model.visual.*`` keys through
``from_reference_checkpoint``), or any frozen callable of your own.
"""
import logging
from typing import Callable, List, Optional, Tuple, Union

import torch
from torch import nn

from . import losses
from .clip_image import ClipImageEncoder
from .clip_text import ClipModel
from .head_tail import unit_rows
from .kw_branches import KW_CascadedBranch, KW_CascadedBranchPlus, KW_HybridBranchPlus, KW_ParallelBranch
from .speech_encoder import FairseqSpeechEncoder_Hubert, S3prlSpeechEncoderPlus

logger = logging.getLogger(__name__)


from .config import Config, load_config, synthetic_reduced_vocab  # noqa: E402,F401


def _cif_args(d: int) -> dict:
    return {"quantity_loss_weight": 0.25, "using_gt_len": False, "cif_output_dim": d, "encoder_embed_dim": d,
            "produce_weight_type": "conv", "cif_threshold": 1.0, "conv_cif_layer_num": 1, "conv_cif_width": 3,
            "conv_cif_dropout": 0.1, "apply_scaling": True, "scaling_step": 5000, "apply_tail_handling": True,
            "tail_handling_firing_threshold": 0.5, "add_cif_ctxt_layers": False}


def cascaded_plus_base_config(**overrides) -> Config:
    """config/speechCLIP+/model_base/spchclip_c+.yaml (BASELINE configs[2]) restricted to the keys the path reads
    (tests/test_host_cpu.py::test_builtin_configs_equal_the_reference_yamls holds every one of them against the yaml)."""
    cfg = base_parallel_config()
    cfg.audio_encoder.name = "hubert_base"
    ms = cfg.model_settings
    ms.cascaded_objective_weight, ms.parallel_objective_weight = 1.0, 0.0
    ms.cascaded_branch = Config({
        "type": "CascadedBranch_dynamic",
        "vq": {"activation": "gelu", "type": "SimpleVectorQuantizer",
               "args": {"temp": "fixed=0.1", "time_first": True, "use_gumbel": False, "hard": True}},
        "downsampling": {"type": "cif", "cif": _cif_args(768)},
        "keyword": {"detokenized_K_neighbors": 5, "retrieve_method": "cosine",
                    "batchnorms": {"type": "eachKw", "std_scale": 1.0, "learnable": True, "parallel": True}},
        "transformer_args": {"type": "MultiheadAttentionAndNorm", "n_layers": 1, "d_model": 768, "nhead": 1,
                             "dim_feedforward": 3072, "dropout": 0.1, "activation": "gelu", "layer_norm_eps": 1.0e-5,
                             "batch_first": True, "norm_first": False}})
    cfg.cl_loss.args.temperature_trainable = True
    cfg.retrieval.audio_feat_src = "cascaded"
    cfg.clip = Config({"name": "ViT-B/32", "embed_dim": 512, "reduce_subword_embbedding": synthetic_reduced_vocab(8112)})
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def cascaded_base_config(**overrides) -> Config:
    """config/speechCLIP/model_base/spchclp_c.yaml (the original SpeechCLIP cascaded model, 8 learned keyword queries) restricted to
    the keys the path reads (tests/test_cascaded_cpu.py holds every one of them against the yaml, tests/golden/recipes_cascaded.json)."""
    cfg = base_parallel_config()
    ms = cfg.model_settings
    ms.cascaded_objective_weight, ms.parallel_objective_weight = 1.0, 0.0
    ms.cascaded_branch = Config({
        "type": "KW_CascadedBranch", "transformer_type": "MultiheadAttentionAndNorm",
        "transformer_args": {"n_layers": 1, "d_model": 768, "nhead": 1, "dim_feedforward": 3072, "dropout": 0.1,
                             "activation": "gelu", "layer_norm_eps": 1.0e-5, "batch_first": True, "norm_first": False},
        "keyword": {"number": 8, "detokenized_K_neighbors": 5, "retrieve_method": "cosine",
                    "batchnorms": {"type": "eachKw", "std_scale": 1.0, "learnable": True, "parallel": True}},
        "vq": {"bn_before_vq": True, "activation": "gelu", "type": "SimpleVectorQuantizer",
               "args": {"temp": "fixed=0.1", "time_first": True, "use_gumbel": False, "hard": True}}})
    cfg.retrieval.audio_feat_src = "cascaded"
    cfg.clip = Config({"name": "ViT-B/32", "embed_dim": 512, "image_encoder_trainable": False, "text_encoder_trainable": False,
                       "reduce_subword_embbedding": synthetic_reduced_vocab(8112)})
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def cascaded_large_config(**overrides) -> Config:
    """config/speechCLIP/model_large/flickr/spchclp_c.yaml: HuBERT-large ll60k with normalised hidden states, a 1024-wide block of one
    head, CLIP ViT-L/14 (token width 768), trainable temperature.  (The coco yaml differs in the reduced vocabulary: 19787 sub-words.)"""
    cfg = cascaded_base_config()
    ms = cfg.model_settings
    for ta in (ms.parallel_branch.transformer_args, ms.cascaded_branch.transformer_args):
        ta.d_model, ta.dim_feedforward = 1024, 4096
    cfg.audio_encoder.name = "hubert_large_ll60k"
    cfg.audio_encoder.normalize_hiddenstates = True
    cfg.cl_loss.args.temperature_trainable = True
    cfg.clip.name, cfg.clip.embed_dim = "ViT-L/14", 768
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def hybrid_plus_large_config(**overrides) -> Config:
    """config/speechCLIP+/model_large/coco/spchclip_h+.yaml (BASELINE configs[4]) restricted to the keys the path reads.  Unlike the
    PARALLEL large recipe this yaml has no ``normalize_hiddenstates`` key: the reference default applies (False,
    speech_encoder_plus.py:350) - round 4 inherited True from large_parallel_config; and the recipe accumulates
    two micro-batches per optimiser step (``trainer.accumulate_grad_batches: 2``, :138)."""
    cfg = large_parallel_config()
    cfg.audio_encoder.normalize_hiddenstates = False
    cfg.trainer.accumulate_grad_batches = 2
    ms = cfg.model_settings
    ms.cascaded_objective_weight, ms.parallel_objective_weight = 1.0, 1.0
    ms.cascaded_branch = Config({
        "type": "HybridBranch_dynamic",
        "vq": {"activation": "gelu", "type": "SimpleVectorQuantizer",
               "args": {"temp": "fixed=0.1", "time_first": True, "use_gumbel": False, "hard": True}},
        "downsampling": {"type": "cif", "cif": _cif_args(1024)},
        "keyword": {"detokenized_K_neighbors": 5, "retrieve_method": "cosine",
                    "batchnorms": {"type": "eachKw", "std_scale": 1.0, "learnable": True, "parallel": True},
                    "kw_projection": {"dropout": 0.1, "dimensions": [1024, 1024, 768]}},
        "transformer_args": {"type": "MultiheadAttentionAndNorm", "n_layers": 1, "d_model": 1024, "nhead": 8,
                             "dim_feedforward": 4096, "dropout": 0.1, "activation": "gelu", "layer_norm_eps": 1.0e-5,
                             "batch_first": True, "norm_first": False}})
    cfg.cl_loss.args.temperature_trainable = True
    cfg.clip = Config({"name": "ViT-L/14", "embed_dim": 768, "reduce_subword_embbedding": synthetic_reduced_vocab(19787)})
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def large_parallel_config(**overrides) -> Config:
    """config/speechCLIP/model_large/flickr/spchclp_p.yaml restricted to the keys the hot path reads
    (HuBERT-large ll60k, normalised hidden states, 1024-wide head, CLIP ViT-L/14 joint width 768)."""
    cfg = base_parallel_config()
    cfg.model_settings.parallel_branch.transformer_args.d_model = 1024
    cfg.model_settings.parallel_branch.transformer_args.dim_feedforward = 4096
    cfg.clip = Config({"name": "ViT-L/14", "embed_dim": 768})
    cfg.audio_encoder.name = "hubert_large_ll60k"
    cfg.audio_encoder.normalize_hiddenstates = True
    cfg.cl_loss.args.temperature_trainable = True
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def base_parallel_config(**overrides) -> Config:
    """config/speechCLIP/model_base/spchclp_p.yaml restricted to the keys the hot path reads."""
    cfg = Config({
        "model_settings": {
            "cascaded_objective_weight": 0.0,
            "parallel_objective_weight": 1.0,
            "parallel_branch": {
                "transformer_type": "TransformerEncoder",
                "transformer_args": {"n_layers": 1, "d_model": 768, "nhead": 8, "dim_feedforward": 3072, "dropout": 0.1,
                                     "activation": "gelu", "layer_norm_eps": 1.0e-5, "batch_first": True,
                                     "norm_first": False},
                "need_projection": True,
            },
        },
        "cl_loss": {"type": "MaskedContrastiveLoss",
                    "args": {"temperature": 0.07, "temperature_trainable": False, "margin": 0.0, "dcl": False,
                             "a2b": True, "b2a": True}},
        "retrieval": {"audio_feat_src": "parallel", "recall_at": [1, 5, 10]},
        "clip": {"name": "ViT-B/32", "embed_dim": 512},
        "audio_encoder": {"type": "FairseqHubert", "name": "hubert", "pretrained": True, "trainable": False,
                          "feat_select_idx": "weighted_sum", "layer_drop": 0.0, "max_audio_len": 102400,
                          "normalize_hiddenstates": False,
                          "optim": {"name": "Adam", "args": {"lr": 1.0e-4, "weight_decay": 1.0e-6}},
                          "scheduler": {"name": "linear_warmup_decay", "warmup": 5000, "max_step": 50000,
                                        "final_lr": 1.0e-8}},
        "trainer": {"gradient_clip_val": 4, "accumulate_grad_batches": 1},
    })
    for k, v in overrides.items():
        cfg[k] = v
    return cfg


def set_dropout(model: nn.Module, enabled: bool) -> nn.Module:
    """Switch every train-mode dropout site of ``model`` off (or back on): the frozen HuBERT's (speech_encoder.HubertArch), the
    parallel head's four sites (head_tail.ParallelHeadFn), nn.MultiheadAttention's and every nn.Dropout.  The reference has no
    such switch (its train step always runs them); the deterministic form is what the parity tests compare with the oracle.
    The original probabilities are remembered on the modules, so ``set_dropout(model, True)`` restores them."""
    from .transformer_models import TransformerEncoder
    for m in model.modules():
        if isinstance(m, FairseqSpeechEncoder_Hubert):
            m.hubert_dropout = bool(enabled)
        elif isinstance(m, nn.Dropout):
            if not hasattr(m, "_sc_p"):
                m._sc_p = m.p
            m.p = m._sc_p if enabled else 0.0
        elif isinstance(m, (nn.MultiheadAttention, TransformerEncoder)):
            if not hasattr(m, "_sc_p"):
                m._sc_p = m.dropout
            m.dropout = m._sc_p if enabled else 0.0
    return model


class KWClip_GeneralTransformer(nn.Module):
    def __init__(self, config, image_encoder: Optional[Union[Callable, str]] = None, device: str = "cuda", hubert_state_dict=None,
                 hubert_arch=None, text_encoder: Optional[str] = None):
        super().__init__()
        if isinstance(config, str):                   # path of a reference yaml recipe (config/**/*.yaml parse unchanged)
            config = load_config(config)
        self.config = config if isinstance(config, Config) else load_config(config)
        config = self.config
        self._device = torch.device(device)
        if isinstance(image_encoder, str):
            if image_encoder != "clip":
                raise ValueError(f"image_encoder={image_encoder!r}: 'clip' (the frozen CLIP image tower), a callable or None")
            # frozen submodule (state-dict keys image_encoder.*); getTrainableParams lists modules by name and never includes it
            image_encoder = ClipImageEncoder(config.clip.get("name", "ViT-B/32"),
                                             image_encoder_trainable=bool(config.clip.get("image_encoder_trainable", False)))
        if text_encoder is not None and text_encoder != "clip":
            raise ValueError(f"text_encoder={text_encoder!r}: 'clip' (the frozen CLIP text tower) or None")
        self.audio_encoder_type = config.audio_encoder.type
        # kwClip.py:59-65: "FairseqHubert" -> FairseqSpeechEncoder_Hubert, "s3prl_plus" -> S3prlSpeechEncoderPlus (the WavLM upstreams the
        # recipes name as alternatives).  A WavLM ``name`` under FairseqHubert builds the same encoder.
        if self.audio_encoder_type not in ("FairseqHubert", "s3prl_plus"):
            raise NotImplementedError(f"audio_encoder.type = {self.audio_encoder_type}: FairseqHubert and s3prl_plus are built "
                                      "(every shipped config uses one of them)")
        enc_args = {k: v for k, v in config.audio_encoder.items() if k not in ("type", "optim", "scheduler", "device")}
        enc_cls = S3prlSpeechEncoderPlus if self.audio_encoder_type == "s3prl_plus" else FairseqSpeechEncoder_Hubert
        self.audio_encoder = enc_cls(device=device, state_dict=hubert_state_dict, arch=hubert_arch, **enc_args)
        self.audio_embd_dim = self.audio_encoder.out_dim
        self.image_encoder = image_encoder
        # CLIP joint embedding width (512 ViT-B/32, 768 ViT-L/14): width of image_feat and of the branch projection
        self.subword_embd_dim = int(config.clip.get("embed_dim", 512))
        self.recall_at = config.retrieval.recall_at
        self.criterion = getattr(losses, config.cl_loss.type)(**config.cl_loss.args)
        self.keyword_num = None
        self.cascaded_branch = None
        self.parallel_branch = None
        ms = config.model_settings
        self.clip = None
        if ms.cascaded_objective_weight > 0:
            # kwClip.py:684-745.  The CLIP text tower is frozen; without a checkpoint offline it is seeded random
            # (load real weights with self.clip.load_state_dict).
            clip_args = {k: v for k, v in config.clip.items() if k not in ("embed_dim", "device")}
            self.clip = ClipModel(device=device, **clip_args)
            text_dim = self.clip.model.token_embedding.weight.size(-1)
            cBranchType = ms.cascaded_branch.type.replace("KW_", "").replace("dynamic", "plus")
            if cBranchType == "CascadedBranch_plus":
                self.cascaded_branch = KW_CascadedBranchPlus(config=config, audio_dim=self.audio_embd_dim,
                                                             text_dim=text_dim, clip=self.clip)
            elif cBranchType == "HybridBranch_plus":
                assert ms.parallel_objective_weight > 0, ms.parallel_objective_weight
                self.cascaded_branch = KW_HybridBranchPlus(config=config, audio_dim=self.audio_embd_dim,
                                                           text_dim=text_dim, out_dim=self.subword_embd_dim,
                                                           clip=self.clip)
            elif cBranchType == "CascadedBranch":
                # kwClip.py:722-740: the original SpeechCLIP cascaded branch, a fixed number of keywords
                self.cascaded_branch = KW_CascadedBranch(config=config, audio_dim=self.audio_embd_dim, text_dim=text_dim,
                                                         clip=self.clip)
                self.keyword_num = self.cascaded_branch.keyword_num
            elif cBranchType == "HybridBranch":
                raise NotImplementedError("KW_HybridBranch (config/speechCLIP+/**/spchclip_h.yaml): the fixed-keyword hybrid branch - "
                                          "its parallel_proj and two losses over the shared block - is not built; the pooling "
                                          "kernel already takes its 9 queries (csrc/kwpool.hip)")
            else:
                raise NotImplementedError(f"cascaded_branch.type = {ms.cascaded_branch.type}: KW_CascadedBranch, "
                                          "KW_CascadedBranch_plus / _dynamic and KW_HybridBranch_plus / _dynamic are built")
            ds = ms.cascaded_branch.get("downsampling", None)
            if ds is not None and ds.type == "cif":
                self.quantity_loss_weight = ds.cif.get("quantity_loss_weight", 1.0)
                self.quantity_loss_criteria = nn.L1Loss()
        if self.clip is None and text_encoder == "clip":
            # a recipe without a keyword branch holds no text tower: built on request for forward_text (caption embeddings, zero-shot
            # retrieval).  Same module and state-dict keys (clip.model.*) as the keyword recipes', frozen, never in getTrainableParams.
            self.clip = ClipModel(device=device, **{k: v for k, v in config.clip.items() if k not in ("embed_dim", "device")})
        if ms.parallel_objective_weight > 0 and self.cascaded_branch is None:
            logger.info("Create Parallel Branch")
            self.parallel_branch = KW_ParallelBranch(config=config, audio_dim=self.audio_embd_dim,
                                                     text_dim=self.subword_embd_dim)
        # frames behind feat_len the encoder still has to compute (speech_encoder.segment_pitches): the CIF weight conv of the plus
        # branches looks conv_cif_width // 2 frames past the last valid one (avssl/module/cif.py:44-52); the CLS head reads none
        if self.cascaded_branch is None or isinstance(self.cascaded_branch, KW_CascadedBranch):
            self.audio_encoder.tail_rows = 0          # (the fixed-keyword branch pools the valid frames, like the CLS head)
        else:
            ds = ms.cascaded_branch.get("downsampling", None)
            width = ds.cif.get("conv_cif_width", 5) if (ds is not None and ds.type == "cif") else 5
            self.audio_encoder.tail_rows = max(1, int(width) // 2)
            self.audio_encoder.branch_inplace = True      # the branch's attention block reads the encoder's output rows in place
        self.img_enc_proj_net = None
        self.p_branch_proj_net = None
        self.c_branch_proj_net = None
        self.global_step = 0
        self.to(self._device)

    @property
    def device(self):
        return self._device

    # ---------------------------------------------------------------------------------------------
    def prefetch_after_step(self) -> None:
        """Called by the trainer on its side stream right after the optimiser step: computes what the next forward needs from the
        parameters alone (head_tail.cls_query, cached per parameter version), off the critical path."""
        pb = self.parallel_branch
        if pb is not None and getattr(pb, "self_att", None) is not None and hasattr(pb.self_att, "cls_forward"):
            from .head_tail import cls_query
            with torch.no_grad():
                cls_query(pb.self_att, pb.cls)
        cb = self.cascaded_branch
        if isinstance(cb, KW_CascadedBranch) and cb.cls.is_cuda:
            from .kw_query import kw_query
            with torch.no_grad():
                kw_query(cb.self_att, cb.cls)

    def getTrainableParams(self) -> list:
        """kwClip.py:620-644 + :812-837."""
        _params = []
        _params += self.audio_encoder.trainable_params()
        _params += list(self.criterion.parameters())
        if self.cascaded_branch is not None:
            _params += [p for p in self.cascaded_branch.parameters() if p.requires_grad]
        if self.parallel_branch is not None:
            _params += list(self.parallel_branch.parameters())
        return _params

    def set_eval_weights(self, mode: str, hubert_state_dict: Optional[dict] = None):
        """'bf16' (default) or 'split': what the frozen HuBERT GEMMs multiply in eval mode (``model.eval()``) - bf16(W), or W_hi + W_lo
        without the common embedding shift of the weight rounding (config key ``audio_encoder.eval_weights``;
        FairseqSpeechEncoder_Hubert.set_eval_weights).  Train mode is the same either way.  ``hubert_state_dict``: the fp32 HuBERT
        weights, needed when the model was not built with ``audio_encoder.eval_weights: split``."""
        self.audio_encoder.set_eval_weights(mode, state_dict=hubert_state_dict)
        return self

    def forward_audio(self, wav, wav_len=[], return_hidden_states: bool = False):
        return self.audio_encoder(wav, wav_len, return_hidden_states=return_hidden_states)

    def forward_image(self, images: Union[list, torch.Tensor]) -> torch.Tensor:
        if isinstance(images, torch.Tensor) and images.dim() == 2:
            return images.to(self._device)                     # pre-computed (frozen) CLIP image embeddings
        if self.image_encoder is None:
            raise RuntimeError("pixel input needs an image encoder: construct with image_encoder=\"clip\" (the frozen CLIP image "
                               "tower) or a callable, or pass CLIP embeddings (B, E) in batch['image'] instead")
        if isinstance(images, torch.Tensor) and (images.dim() != 4 or images.shape[1] != 3):
            raise ValueError(f"Incorrect image tensor shape {images.shape}")
        with torch.no_grad():
            return self.image_encoder(images)                  # pixels [B, 3, 224, 224], or raw images (kwClip.py:484-507: a list)

    def prep_image(self, images: list) -> torch.Tensor:
        """ClipModel.prep_image (clip_official.py:153-166): raw images -> normalised fp32 [B, 3, 224, 224] on the device
        (ClipImageEncoder.prep_image)"""
        if not hasattr(self.image_encoder, "prep_image"):
            raise RuntimeError("prep_image needs the frozen CLIP image tower: construct with image_encoder=\"clip\"")
        return self.image_encoder.prep_image(images)

    def forward_text(self, sents: Union[list, torch.Tensor]) -> torch.Tensor:
        """kwClip.py:509-527: sentences (through ``clip.prep_text``: needs a tokenizer) or a 2-D tensor of ORIGINAL CLIP token ids ->
        caption embeddings [B, embed_dim] fp32 (un-normalised, as the reference returns them).  With a reduced vocabulary the ids are
        mapped through one lookup tensor into a new tensor; the reference rewrites the caller's tensor element by element."""
        if self.clip is None:
            raise RuntimeError("forward_text needs the CLIP text tower: a keyword recipe holds one, any other builds it with "
                               "text_encoder=\"clip\"")
        if isinstance(sents, list):
            return self.clip.encode_text(self.clip.prep_text(sents))
        if not isinstance(sents, torch.Tensor):
            raise TypeError(f"Unknown text type {type(sents)}")
        if sents.dim() != 2:
            raise ValueError(f"Incorrect text tensor shape {sents.shape}")
        if self.clip.selected_text_emb_ids is None:
            return self.clip.encode_text(sents)
        return self.clip.encode_text(self.clip.to_reduced_ids(sents), _original=sents)

    def reportRetrieval(self, score_per_A: torch.Tensor, score_per_B: torch.Tensor, AB_answers: torch.Tensor, BA_answers: torch.Tensor,
                        metadata: dict = {"modality_A_title": "audio", "modality_B_title": "image", "modality_A_logAbbr": "A",
                                          "modality_B_logAbbr": "I"}):
        """kwClip.py:529-598: recall@k in both directions (retrieval.mutualRetrieval, on the device) under the modality names of
        ``metadata``, logged as ``val_recall_{AB}`` / ``val_recall_{BA}`` / ``val_recall_mean`` / ``val_recall_mean_10`` through
        log_dict; also returns the three dictionaries (the reference only logs them)."""
        from .retrieval import mutualRetrieval
        assert "modality_A_title" in metadata
        assert "modality_B_title" in metadata
        assert "modality_A_logAbbr" in metadata
        assert "modality_B_logAbbr" in metadata
        recall_AB, recall_BA, recall_mean = mutualRetrieval(score_per_A=score_per_A, score_per_B=score_per_B, AB_answers=AB_answers,
                                                            BA_answers=BA_answers, recall_at=self.recall_at,
                                                            modality_A_title=metadata["modality_A_title"],
                                                            modality_B_title=metadata["modality_B_title"])
        ab = "{}{}".format(metadata["modality_A_logAbbr"], metadata["modality_B_logAbbr"])
        ba = "{}{}".format(metadata["modality_B_logAbbr"], metadata["modality_A_logAbbr"])
        logged = {f"val_recall_{ab}": recall_AB, f"val_recall_{ba}": recall_BA, "val_recall_mean": recall_mean}
        if "recall@10" in recall_mean:                  # the reference's checkpoint monitor (it requires 10 in recall_at)
            logged["val_recall_mean_10"] = recall_mean["recall@10"]
        self.log_dict(logged, sync_dist=True)
        return recall_AB, recall_BA, recall_mean

    def processWavs(self, wav, sample_rate=None):
        """``sample_rate`` None: ``wav`` is 16 kHz mono fp32 and goes on as it is.  Otherwise (one int, or one per item) ``wav`` is raw
        PCM - a list of int16 / fp32 arrays or tensors, 1-D or [frames, channels], or paths of 16-bit WAV files - and is down-mixed and
        resampled to 16 kHz on the device first (audio_prep.prep_audio): a padded fp32 batch and its lengths."""
        if sample_rate is not None:
            from .audio_prep import prep_audio
            if not isinstance(wav, (list, tuple)):
                wav = [wav]                                    # one utterance
            return prep_audio(list(wav), sample_rate, self._device)
        wav_len = [len(x) for x in wav]
        return wav, wav_len

    # ---------------------------------------------------------------------------------------------
    def forward(self, batch: dict) -> tuple:
        """kwClip.py:839-963."""
        if batch.get("wav_sr") is not None:                    # raw PCM (data.collate_general): packed samples + host frame counts, channels, rates
            from .audio_prep import RawAudioBatch, prep_audio
            wav, wav_len = prep_audio(RawAudioBatch(batch["wav"], batch["wav_frames"], batch["wav_ch"], batch["wav_sr"]), None, self._device)
        else:
            wav, wav_len = batch["wav"], batch["wav_len"]
        image, id = batch["image"], batch["id"]
        audio_feat, audio_feat_len = self.forward_audio(wav, wav_len, return_hidden_states=False)
        if batch.get("image_hw") is not None:                  # ragged raw images (data.collate_general): packed bytes + host sizes
            image = (image, batch["image_hw"])
        image_feat = self.forward_image(image)
        image_feat = unit_rows(image_feat.float())
        if self.cascaded_branch is not None:                                       # kwClip.py:859-880
            otherInputs = {"global_step": self.global_step}
            if getattr(self.cascaded_branch, "using_gt_len", False):
                assert "text" in batch, f"Text captions are required, {batch.keys()}"
                target_len = torch.LongTensor([(t.squeeze().tolist().index(49407) - 1) for t in batch["text"]]).to(self._device)
            else:
                target_len = getattr(audio_feat_len, "_sc_target20", None)     # uploaded with the batch's other integers (speech_encoder)
                if target_len is None:
                    target_len = (audio_feat_len / 20).round().long()
                    lens_host = getattr(audio_feat_len, "_sc_host", None)
                    if lens_host is not None:          # host twin of the targets: the CIF output is sized without a device read
                        from .kw_branches import target_len_host
                        target_len._sc_host = target_len_host(lens_host)
            otherInputs["target_len"] = target_len
            output = self.cascaded_branch(audio_feat=audio_feat, audio_feat_len=audio_feat_len, otherInputs=otherInputs)
        if self.parallel_branch is not None:
            output = self.parallel_branch(audio_feat=audio_feat, audio_feat_len=audio_feat_len)
        parallel_audio_feat = output["parallel_audio_feat"]
        cascaded_audio_feat = output["cascaded_audio_feat"]
        vq_results, keywords, dsample_results = output["vq_results"], output["keywords"], output["dsample_results"]
        keywords_len = dsample_results["dsample_feats_length"] if dsample_results is not None else None
        id = id.to(self._device)
        losses_ = {"id": id, "image_feat": image_feat}
        if cascaded_audio_feat is not None:
            cascaded_audio_feat = unit_rows(cascaded_audio_feat.float())
            losses_["cascaded_audio_feat"] = cascaded_audio_feat
        if parallel_audio_feat is not None:
            parallel_audio_feat = unit_rows(parallel_audio_feat.float())
            losses_["parallel_audio_feat"] = parallel_audio_feat
        if self.cascaded_branch is not None and getattr(self.cascaded_branch, "downsampling_type", None) == "cif":
            assert "target_len" in dsample_results and "quantity_out" in dsample_results, f"{dsample_results.keys()}"
            losses_["cif_quantity_out"] = dsample_results["quantity_out"]
            losses_["cif_target_len"] = dsample_results["target_len"]
        log_metrics = {"cl_temp": self.criterion.temperature_for_logging}   # kwClip.py: .item() per step; here no host sync
        if hasattr(self.criterion, "bias_for_logging"):                      # SigmoidContrastiveLoss: its second scalar
            log_metrics["cl_bias"] = self.criterion.bias_for_logging
        if vq_results is not None:
            log_metrics["softmax_temp"] = vq_results["temp"]
        if self.cascaded_branch is not None:
            if dsample_results is not None and "dsample_len_diff" in dsample_results:
                log_metrics["dsample_len_diff"] = dsample_results["dsample_len_diff"]
            log_metrics.update({k: vq_results[k] for k in ["temp", "code_perplexity", "prob_perplexity", "ent_per_t"]})
        return (losses_, log_metrics,
                {"id": id, "image_feat": image_feat, "parallel_audio_feat": parallel_audio_feat,
                 "cascaded_audio_feat": cascaded_audio_feat, "vq_results": vq_results, "keywords": keywords,
                 "dsample_results": dsample_results, "keywords_len": keywords_len})

    def set_negative_bank(self, embeddings: torch.Tensor, ids: torch.Tensor, k: int):
        """Mined negatives for the contrastive loss: ``embeddings`` [N, E] are image embeddings of the training set (the image tower is
        frozen, so they are constants: computed once, never stale, no gradient), ``ids`` [N] int64 their ids in the batch's id space.
        The rows are normalised (``unit_rows``), kept, and indexed (``GalleryIndex(rows, ids=ids)``).  From then on ``compute_loss`` in
        TRAIN mode mines, per branch term, ``hard_negatives(feat.detach(), index, id, None, k)`` and hands the criterion the bank, its
        ids and the lists; eval mode and ``clear_negative_bank()`` give the plain loss.  ``search``'s own limits (1 <= k <= 1024, at most
        262 144 rows at k > 32) raise as they do there.  ``compute_loss`` runs on the gathered batch on every rank, so data parallelism
        needs no new collective."""
        from .retrieval import WIDE_MAX_K, GalleryIndex
        k = int(k)
        if not 1 <= k <= WIDE_MAX_K:
            raise ValueError(f"set_negative_bank: 1 <= k <= {WIDE_MAX_K} (k {k})")
        if not isinstance(embeddings, torch.Tensor) or embeddings.dim() != 2:
            raise ValueError("set_negative_bank: embeddings must be a [N, E] tensor")
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.shape != (embeddings.shape[0],):
            raise ValueError(f"set_negative_bank: ids must be torch.int64 of shape ({embeddings.shape[0]},)")
        if getattr(self, "_neg_queue", None) is not None:
            raise ValueError("set_negative_bank: a negative queue is set - extra negatives come from a bank or a queue, not both "
                             "(clear_negative_queue() first)")
        rows = unit_rows(embeddings.detach().float()).detach()
        ids = ids.detach().to(rows.device).contiguous()
        self._neg_bank = (rows, ids, GalleryIndex(rows, ids=ids), k)

    def clear_negative_bank(self):
        self._neg_bank = None

    def _loss_terms(self):
        """the branch terms of ``compute_loss``, in its order"""
        return [t for t in ("cascaded", "parallel") if self.config.model_settings.get(f"{t}_objective_weight", 0.0) > 0.0]

    def set_negative_queue(self, size: int):
        """A cross-batch negative queue for the contrastive loss: rings of the last ``size`` speech and image embeddings the model
        produced, used by ``compute_loss`` in TRAIN mode as plain negatives in both directions (``MaskedContrastiveLoss.forward``'s
        ``queue_A`` / ``queue_B`` / ``queue_ids``); they get no gradient.  One [size, E] speech ring per branch term, one image ring and
        one id ring, on the model's device, as plain attributes - no buffers: the state-dict keys stay the reference's.  ``head`` (the
        next row to write) and ``n_valid`` (rows filled, at most ``size``) are host integers.

        A train-mode ``compute_loss`` first writes the rows the PREVIOUS train-mode call stashed (at most two slice copies on wrap-around;
        of a batch longer than the ring its last ``size`` rows), then hands the criterion ``ring[:n_valid]``, then stashes its own detached
        features and ids: tensors saved for a backward are never modified before it runs, and the first call, whose queue is empty, is
        the plain loss to the bit.  Eval mode and ``clear_negative_queue()`` neither read nor write.  ``compute_loss`` runs on the
        gathered batch on every rank, so every rank enqueues the same rows: data parallelism needs no new collective."""
        size = int(size)
        if size < 1:
            raise ValueError(f"set_negative_queue: size >= 1 (size {size})")
        if getattr(self, "_neg_bank", None) is not None:
            raise ValueError("set_negative_queue: a negative bank is set - extra negatives come from a bank or a queue, not both "
                             "(clear_negative_bank() first)")
        dev, E = self._device, int(self.subword_embd_dim)
        self._neg_queue = {
            "size": size, "head": 0, "n_valid": 0, "pending": None,
            "speech": {t: torch.zeros(size, E, device=dev, dtype=torch.float32) for t in self._loss_terms()},
            "image": torch.zeros(size, E, device=dev, dtype=torch.float32),
            "ids": torch.zeros(size, device=dev, dtype=torch.int64),
        }

    def clear_negative_queue(self):
        self._neg_queue = None

    @staticmethod
    def _ring_write(ring: torch.Tensor, rows: torch.Tensor, head: int):
        """``rows`` (at most the ring's length) into ``ring`` from row ``head`` on: one slice copy, two where the batch straddles the end"""
        size, n = ring.shape[0], rows.shape[0]
        first = min(n, size - head)
        ring[head: head + first].copy_(rows[:first])
        if first < n:
            ring[: n - first].copy_(rows[first:])

    def _queue_advance(self, q: dict):
        """write what the previous train-mode call stashed"""
        pending, q["pending"] = q["pending"], None
        if pending is None:
            return
        speech, image, ids = pending
        size, n = q["size"], ids.shape[0]
        keep = min(n, size)                         # a batch longer than the ring leaves its last ``size`` rows
        for t, ring in q["speech"].items():
            self._ring_write(ring, speech[t][n - keep:], q["head"])
        self._ring_write(q["image"], image[n - keep:], q["head"])
        self._ring_write(q["ids"], ids[n - keep:], q["head"])
        q["head"] = (q["head"] + keep) % size
        q["n_valid"] = min(size, q["n_valid"] + keep)

    def compute_loss(self, inputDict: dict):
        """kwClip.py:999-1040.  With a negative bank set (``set_negative_bank``) and the model in train mode, every branch term takes
        the bank rows mined for its anchors beside the batch; with a negative queue set (``set_negative_queue``), the queued rows."""
        assert isinstance(inputDict, dict)
        required_keys = {"id", "image_feat"}
        assert required_keys.issubset(set(inputDict.keys())), f"required: {required_keys}, input: {inputDict.keys()}"
        losses_ = {}
        terms = []                                  # (weight, loss term): summed below without 0 + / 1.0 * launches
        image_feat = inputDict["image_feat"].float()
        id = inputDict["id"]
        queue = getattr(self, "_neg_queue", None) if self.training else None
        if queue is not None:
            if image_feat.shape[1] != queue["image"].shape[1]:
                raise ValueError(f"compute_loss: the negative queue holds rows of width {queue['image'].shape[1]}, the features have "
                                 f"{image_feat.shape[1]}")
            self._queue_advance(queue)
        for branchType in ["cascaded", "parallel"]:
            loss_weight = self.config.model_settings.get(f"{branchType}_objective_weight", 0.0)
            if loss_weight > 0.0:
                feats_key = f"{branchType}_audio_feat"
                assert feats_key in inputDict, f"{inputDict.keys()}"
                mined = {}                          # train mode with a bank set: the bank, its ids and this term's mined lists
                neg_bank = getattr(self, "_neg_bank", None) if self.training else None
                if queue is not None:               # ... with a queue set: this term's speech ring, the image ring and the id ring
                    nv = queue["n_valid"]
                    mined = {"queue_A": queue["speech"][branchType][:nv], "queue_B": queue["image"][:nv], "queue_ids": queue["ids"][:nv]}
                    if id is None:
                        del mined["queue_ids"]
                elif neg_bank is not None:
                    from .retrieval import hard_negatives
                    rows, bank_ids, index, k = neg_bank
                    lists = hard_negatives(inputDict[feats_key].float().detach(), index, id, None, k)[1]
                    mined = {"bank": rows, "bank_ids": bank_ids, "neg_idx": lists}
                losses_[f"{branchType[0]}_cl_loss"] = self.criterion(feat_A=inputDict[feats_key].float(),
                                                                     feat_B=image_feat, index=id, **mined)
                terms.append((float(loss_weight), losses_[f"{branchType[0]}_cl_loss"]))
        if queue is not None:                       # enqueued at the start of the next train-mode call, not here: see set_negative_queue
            queue["pending"] = ({t: inputDict[f"{t}_audio_feat"].detach().float() for t in queue["speech"]}, image_feat.detach(),
                                id.detach().to(torch.int64))
        if "cif_quantity_out" in inputDict and "cif_target_len" in inputDict and hasattr(self, "quantity_loss_criteria"):
            losses_["quantity_loss"] = self.quantity_loss_criteria(inputDict["cif_quantity_out"], inputDict["cif_target_len"])
            terms.append((float(self.quantity_loss_weight), losses_["quantity_loss"]))
        total = 0
        for w, t in terms:
            t = t if w == 1.0 else w * t
            total = t if isinstance(total, int) else total + t
        losses_["loss"] = total
        return losses_

    def transfer_batch_to_device(self, batch: dict, device=None, dataloader_idx: int = 0) -> dict:
        """The LightningModule hook of the same name (what hands kwClip.py:145-147 its device batch): see
        data.transfer_batch_to_device - host twin of ``wav_len``, the waveform copied on its own stream with a completion event."""
        from .data import transfer_batch_to_device
        return transfer_batch_to_device(batch, self._device if device is None else device)

    def training_step(self, batch: dict) -> dict:
        losses_, log_metrics = self.forward(batch)[:2]
        return {"loss_feats": losses_, "log_metrics": log_metrics}

    def training_step_end(self, outputs: dict) -> dict:
        """kwClip.py:149-193: the loss is computed on the gathered batch."""
        if "loss" in outputs:
            return {"loss": torch.mean(outputs["loss"])}
        losses_ = self.compute_loss(outputs["loss_feats"])
        return {"loss": losses_["loss"], **{f"train_{k}": v for k, v in losses_.items()}}

    # --------------------------------------------------------------------------------------------- Lightning-shaped hooks
    def configure_optimizers(self):
        """kwClip.py:646-674: ``([optimizer], [{"scheduler": ..., "interval": "step"}])`` over getTrainableParams().  The optimiser
        is the flat fused clip + Adam (optim.FlatAdamOptimizer, a torch.optim.Optimizer), the schedule a LambdaLR."""
        from .optim import FlatAdamOptimizer, get_scheduler
        oc = self.config.audio_encoder.optim
        if oc.name != "Adam":
            raise NotImplementedError(f"optimizer {oc.name}: the shipped recipes use Adam")
        opt = FlatAdamOptimizer(self.getTrainableParams(), **{k: v for k, v in dict(oc.args).items()})
        sched = self.config.audio_encoder.get("scheduler", None)
        if sched is None:
            return [opt], []
        return [opt], [{"scheduler": get_scheduler(opt, **dict(sched)), "interval": "step"}]

    def log_dict(self, metrics: dict, **kwargs) -> None:
        """Stand-in for LightningModule.log_dict (pytorch_lightning is not installed here): keeps the last values."""
        self.logged = getattr(self, "logged", {})
        self.logged.update(metrics)

    # --------------------------------------------------------------------------------------------- validation (f4)
    def validation_step(self, batch: dict, batch_idx: int = 0) -> dict:
        """kwClip.py:195-246: ``{"loss_feats", "log_metrics", "others"}`` (the reference's keys)."""
        with torch.no_grad():
            losses_, log_metrics, others = self.forward(batch)
        if self._detokenize_enabled() and "text" in batch:
            others["gold_text"] = batch["text"]                 # kwClip.py:237: the captions the keywords are written next to
        return {"loss_feats": losses_, "log_metrics": log_metrics, "others": others}

    def validation_step_end(self, outputs: dict) -> dict:
        """kwClip.py:248-285: loss on the gathered features, logged as ``val_*``; returns ``others``.  The reference moves every
        tensor of ``others`` to the CPU here (a synchronisation per validation step); they stay on the device - the epoch-end
        retrieval runs there."""
        assert isinstance(outputs, dict)
        with torch.no_grad():
            losses_ = self.compute_loss(outputs["loss_feats"])
        result = {f"val_{k}": v for k, v in losses_.items()}
        result.update({f"val_{k}": (v.float().mean() if isinstance(v, torch.Tensor) else v) for k, v in outputs["log_metrics"].items()})
        self.log_dict(result, on_step=True, on_epoch=True, prog_bar=True, logger=True, sync_dist=True)
        return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in outputs["others"].items()}

    def validation_epoch_end(self, outputs: list, group=None) -> dict:
        """kwClip.py:447-482: one image embedding per id (the last seen, as the reference's dict does), audio x image scores
        and recall@k in both directions - everything stays on the device (retrieval.mutualRetrieval).  ``outputs``: the
        ``others`` dicts returned by validation_step_end (or validation_step's full dicts).

        ``group``: a torch.distributed process group whose ranks each hold the outputs of their own validation batches; the call is
        then COLLECTIVE, needs ``retrieval.fused_ranks: true`` and returns, on every rank, the recall of the WHOLE validation set -
        what the single-process call returns on the ranks' outputs concatenated in rank order (``_sharded_recall``)."""
        if group is not None and not self.config.retrieval.get("fused_ranks", False):
            raise ValueError("validation_epoch_end(group=...) runs on the sharded ranks: set retrieval.fused_ranks: true")
        outputs = [o["others"] if "others" in o else o for o in outputs]
        src = self.config.retrieval.get("audio_feat_src", "parallel")
        key = "cascaded_audio_feat" if src == "cascaded" else "parallel_audio_feat"
        ids = torch.cat([o["id"] for o in outputs], dim=0)
        audio = torch.cat([o["audio_feat"] if "audio_feat" in o else o[key] for o in outputs], dim=0).float()
        imgs = torch.cat([o["image_feat"] for o in outputs], dim=0).float()
        if group is not None:
            result = self._sharded_recall(ids, audio, imgs, group)
        else:
            result = self._recall_on_one_device(ids, audio, imgs)
        if self._detokenize_enabled() and outputs and outputs[0].get("keywords", None) is not None:
            every = int(self.config.log_setting.get("log_detokenize_results_every_n_epoch", 1) or 1)
            if int(getattr(self, "current_epoch", 0)) % every == 0:
                self._log_detokenized(outputs)
        return result

    def _sharded_recall(self, ids: torch.Tensor, audio: torch.Tensor, imgs: torch.Tensor, group) -> tuple:
        """``validation_epoch_end`` over the ranks of ``group``: this rank's ids [n], audio and image embeddings [n, E] -> the three
        recall dictionaries of the whole set.  The global sample order is the ranks' samples in rank order.  The ids are all-gathered
        (int64, small), every rank computes the same "last occurrence of every id" and keeps, as its shard of the gallery, the image
        rows of its own range that are one; the embeddings stay where they were encoded (retrieval.mutual_recall_sharded).  Recall
        does not depend on the order of the gallery's rows, so the result equals the single-process one key for key."""
        import torch.distributed as dist
        from .retrieval import ShardedGalleryIndex, _exchange_counts, _gather_rows, mutual_recall_sharded
        ids = ids.long().contiguous()
        n = ids.shape[0]
        counts = [c[0] for c in _exchange_counts([n], ids.device, group)]
        own0 = sum(counts[: dist.get_rank(group)])
        every = _gather_rows(ids, counts, group) if sum(counts) else ids
        uniq, inv = torch.unique(every, return_inverse=True)
        pos = torch.arange(every.shape[0], device=ids.device)
        last = torch.zeros(uniq.shape[0], dtype=torch.long, device=ids.device).scatter_reduce(0, inv, pos, "amax", include_self=False)
        rows = torch.sort(last[(last >= own0) & (last < own0 + n)]).values - own0        # this rank's rows that are a global last occurrence
        index = ShardedGalleryIndex(imgs[rows].contiguous(), ids=ids[rows].contiguous(), group=group)
        return mutual_recall_sharded(audio, index, ids, self.recall_at)

    def _recall_on_one_device(self, ids: torch.Tensor, audio: torch.Tensor, imgs: torch.Tensor) -> tuple:
        """``validation_epoch_end`` without a group: all ids [n], audio and image embeddings [n, E] on this device"""
        from .retrieval import mutualRetrieval
        # last occurrence of every id, ids kept in first-seen order (python dict semantics of the reference)
        uniq, inv = torch.unique(ids, return_inverse=True)
        n = ids.shape[0]
        pos = torch.arange(n, device=ids.device)
        last = torch.zeros(uniq.shape[0], dtype=torch.long, device=ids.device).scatter_reduce(0, inv, pos, "amax", include_self=False)
        first = torch.full((uniq.shape[0],), n, dtype=torch.long, device=ids.device).scatter_reduce(0, inv, pos, "amin", include_self=False)
        order = torch.argsort(first)
        img_ids, img_feats = uniq[order], imgs[last[order]]
        if self.config.retrieval.get("fused_ranks", False):
            # opt-in: both directions' ranks out of the score GEMM's epilogue (csrc/rank.hip), no [nA, nB] matrix
            from .retrieval import mutual_recall
            result = mutual_recall(audio, img_feats, ids, img_ids, self.recall_at)
        else:
            score_per_audio = audio @ img_feats.t()
            result = mutualRetrieval(score_per_A=score_per_audio, score_per_B=score_per_audio.t(), AB_answers=ids, BA_answers=img_ids,
                                     recall_at=self.recall_at)
        return result

    # --------------------------------------------------------------------------------------------- keyword detokenisation
    def _detokenize_enabled(self) -> bool:
        """``log_setting.log_detokenize_results`` (kwClip.py:87-89).  The reference defaults to True; here a config without the key -
        or without ``log_setting`` - keeps validation exactly as it was."""
        ls = self.config.get("log_setting", None)
        if self.cascaded_branch is None:               # a text tower alone (text_encoder="clip") has no keywords to detokenise
            return False
        return bool(ls.get("log_detokenize_results", False)) if ls is not None else False

    def _token_table(self) -> torch.Tensor:
        if self.clip is None or self.cascaded_branch is None:
            raise RuntimeError("keyword detokenisation needs a keyword branch (cascaded+ / hybrid+ recipe): this model has no CLIP text side")
        return self.clip.model.token_embedding.weight

    def _reduced_to_original(self) -> Optional[torch.Tensor]:
        """[V] original CLIP token id of every reduced index, on the device (None: full vocabulary)."""
        ids = self.clip.selected_text_emb_ids
        if ids is None:
            return None
        cached = getattr(self, "_r2o_dev", None)
        if cached is None or cached.device != self._device or cached.shape[0] != ids.shape[0]:
            cached = self._r2o_dev = ids.to(self._device)
        return cached

    @staticmethod
    def _padded_keywords(outputs: list):
        """The validation outputs' keyword tensors [b, n_b, E] as one [U, N, E] tensor (N = the largest n_b) and counts [U]."""
        n_max = max(o["keywords"].shape[1] for o in outputs)
        kws, lens = [], []
        for o in outputs:
            kw = o["keywords"]
            b, n, _ = kw.shape
            kws.append(kw if n == n_max else torch.nn.functional.pad(kw, (0, 0, 0, n_max - n)))
            kl = o.get("keywords_len", None)
            lens.append(torch.full((b,), n, device=kw.device, dtype=torch.long) if kl is None else kl.to(kw.device).long().clamp(max=n))
        return torch.cat(kws, dim=0), torch.cat(lens, dim=0)

    def _gold_texts(self, outputs: list) -> list:
        """One gold entry per utterance: the decoded caption when the CLIP wrapper has a tokenizer, else the caption's token ids up to
        <|endoftext|>; "" for batches that carried no ``text``."""
        tok = getattr(self.clip, "tokenizer", None)
        gold = []
        for o in outputs:
            texts = o.get("gold_text", None)
            if texts is None:
                gold += [""] * int(o["keywords"].shape[0])
                continue
            for sent in texts:
                ids = torch.as_tensor(sent).reshape(-1).tolist()
                if tok is not None:
                    gold.append(tok.decode(ids))
                else:
                    gold.append(ids[: ids.index(49407) + 1] if 49407 in ids else [i for i in ids if i != 0])
        return gold

    def detokenize_keywords(self, outputs: list, K: Optional[int] = None, decode: Optional[Callable] = None) -> list:
        """kwClip.py:380-437: ``outputs`` as validation_epoch_end takes them -> the reference's JSON structure, one ``{"gold",
        "neighbors": {"keyword_i": [[token, score] x K]}}`` per utterance with as many keywords as its ``keywords_len``.  ``K``
        defaults to ``cascaded_branch.keyword.detokenized_K_neighbors`` (10), the scores to its ``retrieve_method`` (cosine)."""
        from .keyword_neighbors import extract_dynamic_keyword_neighbors, extract_fixed_keyword_neighbors
        outputs = [o["others"] if "others" in o else o for o in outputs]
        kwcfg = self.config.model_settings.cascaded_branch.keyword
        retrieve_method = kwcfg.get("retrieve_method", "cosine")
        if retrieve_method not in ["cosine", "pseudo_inverse"]:
            raise NotImplementedError(retrieve_method)
        K = int(kwcfg.get("detokenized_K_neighbors", 10)) if K is None else int(K)
        table = self._token_table()
        gold_texts = self._gold_texts(outputs)
        if self.keyword_num is not None:
            kw = torch.cat([o["keywords"].reshape(-1, self.keyword_num, self.subword_embd_dim) for o in outputs], dim=0)
            return extract_fixed_keyword_neighbors(model=self, K=K, retrieve_method=retrieve_method, tokenEmbeddings=table,
                                                   keywordEmbeddings=kw, gold_texts=gold_texts, decode=decode)
        lengths = []
        for o in outputs:
            kl = o.get("keywords_len", None)
            lengths += [int(o["keywords"].shape[1])] * int(o["keywords"].shape[0]) if kl is None else kl.tolist()
        return self._extract_dynamic(outputs, K, retrieve_method, table, gold_texts, lengths, decode)

    def _extract_dynamic(self, outputs, K, retrieve_method, table, gold_texts, lengths, decode):
        """extract_dynamic_keyword_neighbors cuts ``gold_texts`` / ``kwEmbedLengths`` by ``config.data.dev_batch_size``; the batches
        handed in here carry their own sizes, so each goes in as one batch of its own size (one call, one device-to-host copy)."""
        from .keyword_neighbors import extract_dynamic_keyword_neighbors
        sizes = [int(o["keywords"].shape[0]) for o in outputs]
        bs = max(sizes)
        # pad every batch's slice of the flat lists to ``bs`` entries: the function indexes them by i * bs
        gold_p, len_p, at = [], [], 0
        for n in sizes:
            gold_p += gold_texts[at: at + n] + [None] * (bs - n)
            len_p += lengths[at: at + n] + [0] * (bs - n)
            at += n

        class _M:                                           # the three attributes the function reads
            pass
        m = _M()
        m.config = Config({"data": {"dev_batch_size": bs}})
        m.subword_embd_dim, m.clip, m.device = self.subword_embd_dim, self.clip, self._device
        m.cascaded_branch = self.cascaded_branch             # its quantiser's VocabTables cache is reused
        return extract_dynamic_keyword_neighbors(model=m, K=K, retrieve_method=retrieve_method, outputs=outputs, tokenEmbeddings=table,
                                                 keywordEmbeddings_list=[[o["keywords"]] for o in outputs], gold_texts=gold_p,
                                                 kwEmbedLengths=len_p, decode=decode)

    def keyword_statistics(self, outputs: list) -> dict:
        """kwClip.py:325-353: mean / std / norm per keyword slot, kw_mean_mse, kw_std_mse over the epoch's keywords, computed on the
        device (keyword_neighbors.keyword_statistics) and logged through log_dict."""
        from .keyword_neighbors import keyword_statistics
        outputs = [o["others"] if "others" in o else o for o in outputs]
        kw, lens = self._padded_keywords(outputs)
        stats = keyword_statistics(kw, self._token_table(), lens)
        flat = {f"kw_{s}/{k}": v for s in ("mean", "std", "norm") for k, v in stats[s].items()}
        flat.update({"kw_mean_mse": stats["kw_mean_mse"], "kw_std_mse": stats["kw_std_mse"]})
        self.log_dict(flat, sync_dist=True)
        return stats

    def keyword_hit_rate(self, idx: torch.Tensor, gold_text: torch.Tensor) -> dict:
        """Share of keywords with one of their K neighbours in the caption (keyword_neighbors.keyword_hit_rate); ``idx`` holds
        indices into this model's token table."""
        from .keyword_neighbors import keyword_hit_rate
        return keyword_hit_rate(idx, gold_text, self._reduced_to_original())

    def _log_detokenized(self, outputs: list) -> None:
        import json
        import os
        self.detokenized = self.detokenize_keywords(outputs)
        self.keyword_stats = self.keyword_statistics(outputs)
        if all(o.get("gold_text", None) is not None for o in outputs):
            from .keyword_neighbors import keyword_neighbors
            kwcfg = self.config.model_settings.cascaded_branch.keyword
            kw, lens = self._padded_keywords(outputs)
            _, idx = keyword_neighbors(kw, self._token_table(), int(kwcfg.get("detokenized_K_neighbors", 10)), keywords_len=lens,
                                       retrieve_method=kwcfg.get("retrieve_method", "cosine"),
                                       tables=self.cascaded_branch.vector_quantizer._tables)
            gold = torch.cat([torch.stack([torch.as_tensor(t).reshape(-1) for t in o["gold_text"]]) for o in outputs], dim=0)
            self.keyword_hits = self.keyword_hit_rate(idx, gold)
            self.log_dict({"kw_hit_rate": self.keyword_hits["mean"]}, sync_dist=True)
        root = self.config.get("trainer", {}).get("default_root_dir", None)
        if root:
            text_dir = os.path.join(root, "retokenizeText")
            os.makedirs(text_dir, exist_ok=True)
            with open(os.path.join(text_dir, f"keywords_ep{int(getattr(self, 'current_epoch', 0))}.json"), "w") as f:
                json.dump(self.detokenized, f, indent=4)

    # --------------------------------------------------------------------------------------------- checkpoints (f4)
    @staticmethod
    def split_reference_state_dict(sd: dict):
        """A PyTorch-Lightning checkpoint of the reference (``ckpt["state_dict"]``) -> (hubert_state_dict in fairseq naming,
        rest).  Reference keys: ``audio_encoder.encoder.<fairseq HubertModel key>``, ``audio_encoder.weightedsum_layer.weights``,
        ``parallel_branch.* / cascaded_branch.*`` (same module names here), ``criterion.temperature``, ``clip.model.*`` (the text
        side is kept, ``clip.model.visual.*`` is dropped: image embeddings are inputs)."""
        hubert, rest = {}, {}
        for k, v in sd.items():
            if k.startswith("audio_encoder.encoder."):
                hubert[k[len("audio_encoder.encoder."):]] = v
            elif k.startswith("clip.model.visual.") or k in ("clip.model.logit_scale",):
                continue
            else:
                rest[k] = v
        return hubert, rest

    @classmethod
    def from_reference_checkpoint(cls, config, state_dict: dict, **kw):
        """Build the model on the reference's weights: the HuBERT part is converted by the encoder's loader (fairseq key names,
        weight-normed pos_conv accepted), everything else loads by name (non-strict for keys this build does not hold).  With
        ``image_encoder="clip"`` the ``clip.model.visual.*`` keys load into the image tower as well (strict)."""
        hubert, rest = cls.split_reference_state_dict(state_dict)
        model = cls(config, hubert_state_dict=hubert if hubert else None, **kw)
        own = model.state_dict()
        loadable = {k: v for k, v in rest.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
        visual = {}
        if kw.get("image_encoder") == "clip":
            pre = "clip.model.visual."
            visual = {k: v for k, v in state_dict.items() if k.startswith(pre)}
            if visual:
                model.image_encoder.load_reference_state_dict({k[len(pre):]: v for k, v in visual.items()})
        missing = [k for k in own if k not in loadable and not k.startswith("audio_encoder.train_layers.")
                   and not (visual and k.startswith("image_encoder."))]
        model.load_state_dict(loadable, strict=False)
        model._reference_load_report = {"loaded": sorted(list(loadable) + list(visual)), "not_in_checkpoint": missing,
                                        "ignored": sorted(k for k in rest if k not in loadable)}
        return model

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, config=None, **kw):
        """example.py:9-10 ``KWClip_GeneralTransformer.load_from_checkpoint(path)``: a PyTorch-Lightning checkpoint file holds
        ``state_dict`` and (via save_hyperparameters, avssl/base/base_model.py:14) the config under ``hyper_parameters``."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        if config is None:
            hp = ckpt.get("hyper_parameters", {})
            config = hp.get("config", hp)
        return cls.from_reference_checkpoint(config, ckpt["state_dict"], **kw)

    # ---------------------------------------------------------------------------------------------
    def encode_speech(self, wav, sample_rate=None) -> dict:
        """kwClip.py:1042-1091 (un-normalised branch output).  ``sample_rate``: ``wav`` is raw PCM at that rate (processWavs)."""
        wav, wav_len = self.processWavs(wav, sample_rate)
        audio_feat, audio_feat_len = self.forward_audio(wav, wav_len)
        if self.cascaded_branch is not None:
            output = self.cascaded_branch(audio_feat=audio_feat, audio_feat_len=audio_feat_len)
        if self.parallel_branch is not None:
            output = self.parallel_branch(audio_feat=audio_feat, audio_feat_len=audio_feat_len)
        return {"cascaded_audio_feat": output["cascaded_audio_feat"], "parallel_audio_feat": output["parallel_audio_feat"],
                "vq_results": output["vq_results"], "keywords": output["keywords"]}

    def retrieve(self, queries, gallery, k: Optional[int] = None, src: Optional[str] = None, query_ids: Optional[torch.Tensor] = None,
                 gallery_ids: Optional[torch.Tensor] = None):
        """Which gallery items a query retrieves: (vals [nQ, k] fp32, idx [nQ, k] int64), best first (retrieval.search; the
        ranking avssl/module/retrieval.py:45-46 computes from the scores of kwClip.py:447-482 and drops).  ``queries``: a [nQ, E]
        tensor of speech embeddings, or a list of waveforms - those go through ``encode_speech``, and ``src`` ("cascaded" /
        "parallel"; None: ``config.retrieval.audio_feat_src``) picks the branch output.  ``gallery``: image or caption embeddings
        [N, E] (what ``forward_image`` / ``forward_text`` return) or a retrieval.GalleryIndex / CompactGalleryIndex built with
        ``cosine=True``.  Query
        and gallery rows are brought to unit length as ``forward`` does, so the scores are cosines.  ``k``: None = max(recall_at); 1 <= k <= 1024 on a tensor or a
        GalleryIndex (k > 32 runs retrieval.search's wide selection), k <= 32 on a CompactGalleryIndex.
        ``query_ids`` [nQ] / ``gallery_ids`` [N] (int64 device tensors): a gallery row whose id equals the query's is left out of that
        query's list (retrieval.search's filter - a spoken caption must not retrieve itself or its siblings).  A tensor gallery takes
        ``gallery_ids``; a GalleryIndex or CompactGalleryIndex brings its own ``ids`` and its ``live`` mask (the compact one goes
        through retrieval.search_compact's filtered call and its exact fallback).  Without ids the call is the unfiltered one.
        A retrieval.ShardedGalleryIndex (built with ``cosine=True``; one device or one shard per rank of a process group, where the call
        is collective): retrieval.search_sharded - the same lists, global rows as ``idx``, the index's own ids and removed rows."""
        from .retrieval import CompactGalleryIndex, GalleryIndex, ShardedGalleryIndex, search
        sharded = isinstance(gallery, ShardedGalleryIndex)            # a gallery in shards: retrieval.search_sharded, the same lists
        if sharded:
            if gallery_ids is not None:
                raise ValueError("retrieve: a ShardedGalleryIndex brings its own ids (build it with ids=); gallery_ids must be None")
            g_cuda = gallery.device.type == "cuda"
        elif isinstance(gallery, CompactGalleryIndex):
            g_cuda = gallery.coarse.is_cuda
        else:
            g_cuda = gallery.split.is_cuda if isinstance(gallery, GalleryIndex) else (isinstance(gallery, torch.Tensor) and gallery.is_cuda)
        if not g_cuda or (isinstance(queries, torch.Tensor) and not queries.is_cuda):
            raise RuntimeError("retrieve runs on the HIP kernels: device tensors only")
        if isinstance(queries, (list, tuple)):
            src = src if src is not None else self.config.retrieval.get("audio_feat_src", "parallel")
            if src not in ("cascaded", "parallel"):
                raise ValueError(f"retrieve: src = {src!r} (\"cascaded\" or \"parallel\")")
            key = "cascaded_audio_feat" if src == "cascaded" else "parallel_audio_feat"
            with torch.no_grad():
                feat = self.encode_speech(list(queries))[key]
            if feat is None:
                raise RuntimeError(f"retrieve: this recipe has no {key} (src = {src!r})")
            queries = feat
        if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
            raise ValueError("retrieve: queries must be a [nQ, E] tensor of embeddings or a list of waveforms")
        k = int(max(self.recall_at)) if k is None else int(k)
        queries = unit_rows(queries.detach().float())
        if sharded:
            from .retrieval import search_sharded
            return search_sharded(queries, gallery, k, query_ids=query_ids)
        if not isinstance(gallery, (GalleryIndex, CompactGalleryIndex)):
            gallery = unit_rows(gallery.detach().float())
        if query_ids is None and gallery_ids is None:
            return search(queries, gallery, k)
        if isinstance(gallery, CompactGalleryIndex):                  # the filtered compact call is search_compact's (it certifies)
            from .retrieval import search_compact
            return search_compact(queries, gallery, k, query_ids=query_ids, gallery_ids=gallery_ids)[:2]
        return search(queries, gallery, k, query_ids=query_ids, gallery_ids=gallery_ids)

    def extract_keywords(self, wav, sample_rate=None) -> dict:
        """kwClip.py:1093-1103, the inference entry of the keyword recipes: ``wav`` one 1-D waveform (or a list of them) ->
        ``{"vq_results", "dsample_results"}`` with ``vq_results["targets"]`` flattened to a list of ORIGINAL CLIP token ids
        (``clip.reducedl2Original`` when the vocabulary is reduced; slots past an utterance's ``dsample_feats_length`` included, as
        in the reference).  ``sample_rate``: ``wav`` is raw PCM at that rate (processWavs)."""
        if self.cascaded_branch is None:
            raise RuntimeError("extract_keywords needs a keyword branch (cascaded+ / hybrid+ recipe)")
        if isinstance(wav, torch.Tensor) and wav.dim() == 1:
            wav = [wav]
        wav, wav_len = self.processWavs(wav, sample_rate)
        with torch.no_grad():
            audio_feat, audio_feat_len = self.forward_audio(wav, wav_len)
            output = self.cascaded_branch(audio_feat=audio_feat, audio_feat_len=audio_feat_len, otherInputs={})
        vq_results, dsample_results = output["vq_results"], output["dsample_results"]
        targets = vq_results["targets"].flatten().tolist()
        if self.clip.selected_text_emb_ids is not None:
            targets = [self.clip.reducedl2Original[t] for t in targets]
        vq_results["targets"] = targets
        return {"vq_results": vq_results, "dsample_results": dsample_results}

    def feature_extractor_s3prl(self, wav, sample_rate=None) -> Tuple[torch.Tensor, Tuple]:
        """kwClip.py:965-997: the HuBERT states (fresh tensors: the encoder clones what it hands out) followed by the branch
        layer's hidden states (full-sequence layer on the library's kernels).  ``sample_rate``: ``wav`` is raw PCM at that rate."""
        wav, wav_len = self.processWavs(wav, sample_rate)
        audio_feat, audio_len, hidden_states = self.forward_audio(wav, wav_len, return_hidden_states=True)
        assert isinstance(hidden_states, tuple)
        with torch.no_grad():
            if self.cascaded_branch is not None:
                hidden_states = hidden_states + tuple(self.cascaded_branch.extract_hidden_states(audio_feat, audio_len)[1:])
            if self.parallel_branch is not None:
                hidden_states = hidden_states + tuple(self.parallel_branch.extract_hidden_states(audio_feat, audio_len)[1:])
        return hidden_states[-1], hidden_states
