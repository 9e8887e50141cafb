"""Host side of the original SpeechCLIP cascaded recipe (config/speechCLIP/**/spchclp_c.yaml: KW_CascadedBranch, 8 learned keyword
queries, the fixed-count keyword BatchNorm): construction, state-dict layout, trainable parameters, the built-in configs against
the reference yamls (tests/golden/recipes_cascaded.json) and the BatchNorm restatement of tests/kwpool_cases.py against the
reference module's recorded results (tests/golden/kw_bn_fixed.npz).  No device is needed."""
import json
import os

import numpy as np
import pytest
import torch

import kwpool_cases as kc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _flat(c, pre=""):
    out = {}
    for k, v in c.items():
        if hasattr(v, "items"):
            out.update(_flat(v, pre + k + "."))
        else:
            out[pre + k] = v
    return out


def _recipes():
    with open(os.path.join(ROOT, "tests", "golden", "recipes_cascaded.json")) as f:
        return json.load(f)


def _nested(rec):
    nested = {}
    for k, v in rec.items():
        *path, leaf = k.split(".")
        node = nested
        for p in path:
            node = node.setdefault(p, {})
        node[leaf] = v["path"] if isinstance(v, dict) else v
    return nested


BUILTINS = (("cascaded_base_config", "speechCLIP/model_base/spchclp_c.yaml"),
            ("cascaded_large_config", "speechCLIP/model_large/flickr/spchclp_c.yaml"))


@pytest.mark.parametrize("name,rel", BUILTINS)
def test_builtin_cascaded_configs_equal_the_reference_yamls(name, rel):
    """Every key the built-in holds equals what load_config gives the reference's yaml; trainer.accumulate_grad_batches is in the yaml."""
    import speechclip_plus_amd as sc
    builtin, fy = getattr(sc, name)(), _recipes()[rel]
    flat = _flat(builtin)
    assert flat["model_settings.cascaded_branch.keyword.number"] == 8
    for k, v in flat.items():
        if isinstance(v, torch.Tensor):                                    # the reduced vocabulary: same size as the yaml's table
            assert v.numel() == fy[k]["rows"], (rel, k, v.numel(), fy[k])
        else:
            assert k in fy and v == fy[k], (rel, k, v, fy.get(k, "not in the yaml"))
    assert set(fy) == set(flat), set(fy) ^ set(flat)
    coco = _recipes()["speechCLIP/model_large/coco/spchclp_c.yaml"]
    assert coco["clip.reduce_subword_embbedding"]["rows"] == 19787


def _expected_branch_state(D, E, K):
    return {"cls": (1, K, D),
            "self_att.multihead_attn_layer.in_proj_weight": (3 * D, D), "self_att.multihead_attn_layer.in_proj_bias": (3 * D,),
            "self_att.multihead_attn_layer.out_proj.weight": (D, D), "self_att.multihead_attn_layer.out_proj.bias": (D,),
            "self_att.attentionBlock_Norm.weight": (D,), "self_att.attentionBlock_Norm.bias": (D,),
            "linear_proj.weight": (E, D), "linear_proj.bias": (E,),
            "bn_layer.bn_layer.weight": (E * K,), "bn_layer.bn_layer.bias": (E * K,), "bn_layer.bn_layer.running_mean": (E * K,),
            "bn_layer.bn_layer.running_var": (E * K,), "bn_layer.bn_layer.num_batches_tracked": (),
            "vector_quantizer.curr_temp": (1,)}                             # (a buffer of the quantiser, as in the plus branches)


def _check_model(m, D, E):
    from speechclip_plus_amd import KW_CascadedBranch
    br = m.cascaded_branch
    assert isinstance(br, KW_CascadedBranch) and m.parallel_branch is None
    assert m.keyword_num == 8 and br.keyword_num == 8 and m.audio_encoder.tail_rows == 0
    sd = {k: tuple(v.shape) for k, v in br.state_dict().items() if not k.startswith("clip.")}
    assert sd == _expected_branch_state(D, E, 8), set(sd.items()) ^ set(_expected_branch_state(D, E, 8).items())
    assert any(k.startswith("clip.") for k in br.state_dict())
    # BatchNorm initialised from the token table, in the reference's d * K + k layout
    emb = m.clip.model.token_embedding.weight
    bn = br.bn_layer.bn_layer
    assert torch.equal(bn.weight.detach().view(8, E), torch.std(emb, dim=0).expand(8, E))
    assert torch.equal(bn.bias.detach().view(8, E), torch.mean(emb, dim=0).expand(8, E))
    trainable = {id(p) for p in m.getTrainableParams()}
    for n, p in br.named_parameters():
        assert (id(p) in trainable) == (not n.startswith("clip.")), n
    assert not any(id(p) in trainable for p in m.clip.parameters())
    assert not any(id(p) in trainable for n, p in m.audio_encoder.named_parameters() if "weightedsum" not in n)
    assert id(m.audio_encoder.weightedsum_layer.weights) in trainable


@pytest.mark.parametrize("name,D,E", (("cascaded_base_config", 768, 512), ("cascaded_large_config", 1024, 768)))
def test_model_builds_from_the_builtin_configs(name, D, E):
    import speechclip_plus_amd as sc
    _check_model(sc.KWClip_GeneralTransformer(getattr(sc, name)(), device="cpu"), D, E)


def test_model_builds_from_the_yaml_values():
    """the flattened values of the base yaml (the fixture), through load_config as a yaml file's would go"""
    import speechclip_plus_amd as sc
    cfg = sc.load_config(_nested(_recipes()["speechCLIP/model_base/spchclp_c.yaml"]), allow_synthetic_vocab=True)
    assert cfg.model_settings.cascaded_branch.type == "KW_CascadedBranch"
    _check_model(sc.KWClip_GeneralTransformer(cfg, device="cpu"), 768, 512)


def test_hybrid_branch_still_raises_with_its_own_message():
    import speechclip_plus_amd as sc
    cfg = sc.cascaded_base_config()
    cfg.model_settings.cascaded_branch.type = "KW_HybridBranch"
    cfg.model_settings.parallel_objective_weight = 1.0
    with pytest.raises(NotImplementedError, match="KW_HybridBranch"):
        sc.KWClip_GeneralTransformer(cfg, device="cpu")


def test_kw_batchnorm_constructor():
    from speechclip_plus_amd.vector_quantizers import Kw_BatchNorm
    z = np.load(os.path.join(ROOT, "tests", "golden", "kw_bn_fixed.npz"))
    t = lambda k: torch.from_numpy(z[k])
    for kind, parallel in (("eachKw", True), ("same", False)):
        m = Kw_BatchNorm(kw_num=8, kw_dim=16, batchnorm_type=kind, init_bias=t("init_bias"), init_scale=t("init_scale"),
                         std_scale=float(z["std_scale"]), learnable=False, parallel=parallel)
        assert set(m.state_dict()) == {f"bn_layer.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
        reps = 8 if kind == "eachKw" else 1                    # kw_bn.py:76-95 (the generator asserts the reference module does this)
        assert torch.equal(m.bn_layer.weight.detach(), (t("init_scale") * float(z["std_scale"])).repeat(reps))
        assert torch.equal(m.bn_layer.bias.detach(), t("init_bias").repeat(reps))
        assert not m.bn_layer.weight.requires_grad and not m.bn_layer.bias.requires_grad
        with pytest.raises(RuntimeError, match="device tensors only"):
            m(torch.zeros(2, 8, 16))
    with pytest.raises(NotImplementedError, match="no shipped recipe"):
        Kw_BatchNorm(kw_num=8, kw_dim=16, batchnorm_type="eachKw", init_bias=t("init_bias"), init_scale=t("init_scale"), parallel=False)


# the fixture stores the reference's fp64 results rounded to fp32: 2^-24 relative, and the same again for a restatement in double
BN_FIXTURE_TOL = 2.0 ** -22


@pytest.mark.parametrize("kind", ("eachKw", "same"))
def test_bn_restatement_equals_the_reference_module(kind):
    """kwpool_cases.bn_ref in double against the reference's Kw_BatchNorm (kw_bn_fixed.npz): step-1 output and gradients, the running
    buffers after two steps, the eval output - the yardstick the GPU test holds the module against."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "kw_bn_fixed.npz"))
    t = lambda k: torch.from_numpy(z[k]).double()
    n = t(f"{kind}.weight").numel()
    assert n == (8 * 16 if kind == "eachKw" else 16)
    rm, rv = torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    x, w, b = (t(k).requires_grad_(True) for k in ("x1", f"{kind}.weight", f"{kind}.bias"))
    y = kc.bn_ref(x, w, b, rm, rv, True, kind=kind)
    y.backward(t("dy"))
    kc.bn_ref(t("x2"), w, b, rm, rv, True, kind=kind)
    ye = kc.bn_ref(t("x2"), w, b, rm, rv, False, kind=kind)
    assert int(z[f"{kind}.num_batches_tracked"]) == 2
    for got, k in ((y, "y1"), (x.grad, "dx1"), (w.grad, "dweight"), (b.grad, "dbias"), (rm, "running_mean"), (rv, "running_var"),
                   (ye, "y_eval")):
        ref = t(f"{kind}.{k}")
        err = float((got.detach() - ref).abs().max() / ref.abs().max())
        assert err <= BN_FIXTURE_TOL, (kind, k, err)
