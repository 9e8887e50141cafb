"""Shared by tests/test_split_weights_cpu.py, tests/test_gpu_split_weights.py and tests/golden/make_split_weights_fixture.py: the small
frozen encoders of tests/test_gpu_frozen_fwd.py (two layers at the shipped widths, random weights) on three utterances of unequal
length, the oracle's emulations of the two eval-weight modes, and the distance d(x) the split-weight checks are stated in."""
import dataclasses
import os
import sys

import torch

LENS = [48123, 20777, 40601]            # samples: T = 150, valid frames 150 / 65 / 127
CASES = ("base_small", "large_small")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_weights_small.npz")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
SITES = ("conv", "ln", "proj", "residual", "qkv", "p", "ctx", "ffn_act")


def small_case(case):
    """-> (encoder name, speech_encoder.HubertArch, fp32 state dict, padded waveforms [3, L]); the seeds are the committed ones"""
    from speechclip_plus_amd import random_hubert_state_dict
    from speechclip_plus_amd import speech_encoder as se
    name = "hubert_large_ll60k" if case == "large_small" else "hubert"
    a = dataclasses.replace(se.ARCHS[name], layers=2)
    sd = random_hubert_state_dict(a, seed=97 + len(case))
    g = torch.Generator().manual_seed(5 + len(case))
    wav = torch.zeros(len(LENS), max(LENS))
    for b, l in enumerate(LENS):
        wav[b, :l] = torch.randn(l, generator=g) * 0.5
    return name, a, sd, wav


def oracle_arch(a):
    import oracle
    return oracle.HubertArch(**{f.name: getattr(a, f.name) for f in dataclasses.fields(oracle.HubertArch) if hasattr(a, f.name)})


def split_emulation_weights(sd):
    """the weights as the split eval mode multiplies them (tools/recall_eval.split_emulation_weights: the one definition)"""
    import recall_eval
    return recall_eval.split_emulation_weights(sd)


def oracle_states(case, mode):
    """hidden states [B, T, D] fp32 of ``mode``: 'fp32' (the oracle), 'bf16' (all storage sites + bf16 weights = the shipped path's
    emulation), 'split' (all storage sites + split weights); and feat_len"""
    import oracle
    _, a, sd, wav = small_case(case)
    W = {"fp32": lambda: sd, "bf16": lambda: oracle.bf16_weights(sd), "split": lambda: split_emulation_weights(sd)}[mode]()
    store = None if mode == "fp32" else oracle.SitedStore(set(SITES))
    with torch.no_grad():
        hs, fl = oracle.speech_encoder_forward(W, oracle_arch(a), [wav[b, :l] for b, l in enumerate(LENS)], store=store)
    return [h.float() for h in hs], [int(v) for v in fl.tolist()]


def dist(hs, ref, feat_len):
    """d(x): rms distance of x's weighted-sum features (uniform weights, as oracle.weighted_sum(zeros, .)) from the reference's, over the
    valid frames of every utterance"""
    f = sum(h.double() for h in hs) / len(hs)
    r = sum(h.double() for h in ref) / len(ref)
    d = torch.cat([(f[b, :n] - r[b, :n]).reshape(-1) for b, n in enumerate(feat_len)])
    return d.pow(2).mean().sqrt().item()


def rehearse(case):
    """-> (d(emulation, all sites + w_split), d(emulation, all sites + bf16 weights)) against the fp32 oracle"""
    ref, fl = oracle_states(case, "fp32")
    return dist(oracle_states(case, "split")[0], ref, fl), dist(oracle_states(case, "bf16")[0], ref, fl)
