"""Writes tests/golden/wavlm_small.npz: a tiny random-weight ``transformers.WavLMModel`` (one post-LN, one stable-LayerNorm variant)
run on a padded batch - the independent implementation tests/wavlm_cases.py and the HIP path are held against.  Data only in the
.npz; run with the repository root on sys.path:  python tests/golden/make_golden_wavlm.py

Per variant (prefix post_ / stable_; wav [3, L] and lens are shared): W_<transformers key> weights (weight-norm of pos_conv kept as
its two parameters), valid (frames HF admits), hidden [3, sum(valid), D] (every hidden state, valid frames of the padded batch, utterance after
utterance), gates [2, H, sum(valid)] (each layer's gate_output), bias_row / bias_col [H, 1000] = layer 0's position_bias[h, 0, :] and [h, :, 0] at T = 1000 (the full [H, T, T] matrix is
asserted Toeplitz first, so the two hold all of it)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from oracle.lengths import conv_out_lengths, fairseq_valid_frames      # noqa: E402

T_MAX = 1000
L = 27200                 # 84 frames; chunk of the fairseq mask rule = 27200 // 84 = 323 samples


def agreeing_lengths(T):
    """two shorter lengths on which fairseq's chunk rule and HF's conv-formula rule admit the same frames: one above the 64-key tile
    of the attention kernel (65 frames), one short (30; below 27 frames the two rules cannot agree at this chunk)"""
    out = []
    for want in (65, 30):
        for l in range(400, L):
            if conv_out_lengths(l)[-1] == want and fairseq_valid_frames([l], L, T)[0] == want:
                out.append(l)
                break
    assert len(out) == 2, out
    return out


def main():
    from transformers import WavLMConfig, WavLMModel
    from transformers.models.wavlm import modeling_wavlm
    arrs = {}
    T = conv_out_lengths(L)[-1]
    assert T == 84, T                       # crosses the 64-key tile and the exact / logarithmic bucket boundary at 80
    lens = [L] + agreeing_lengths(T)
    for variant, stable in (("post", False), ("stable", True)):
        torch.manual_seed(11 if not stable else 12)
        cfg = WavLMConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, conv_dim=(32,) * 7,
                          conv_bias=stable, feat_extract_norm="layer" if stable else "group", do_stable_layer_norm=stable,
                          num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=2, num_buckets=320, max_bucket_distance=800,
                          hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0,
                          apply_spec_augment=False)
        hf = WavLMModel(cfg).eval()
        with torch.no_grad():
            for n, p in hf.named_parameters():
                if "norm" in n or n.endswith("bias") or "gru_rel_pos_const" in n:
                    p.add_(0.1 * torch.randn_like(p))
            # size: random fp32 does not compress.  Every parameter is put on a grid of 1 / 32 (a handful of levels at the initial
            # scales) and pos_conv repeats its first 4 input channels across each group (a 1M-element tensor otherwise), BEFORE the model runs - the model that produced the states is exactly the
            # stored one, and deflate packs the few distinct values.
            for n, p in hf.named_parameters():
                if n.endswith("original1") or n.endswith("weight_v"):
                    p.copy_((torch.sign(p[:, :4, :]) * (p[:, :4, :].abs() > 0.01) / 32.0).repeat(1, p.shape[1] // 4, 1))
                if "rel_attn_embed" not in n:
                    p.copy_(torch.round(p * 32.0) / 32.0)
        gates = []
        orig = modeling_wavlm.WavLMAttention.torch_multi_head_self_attention

        def spy(self, hidden_states, attention_mask, gated_position_bias, output_attentions):
            # gated_position_bias [B H, T, T] = gate_output x position_bias: recover gate_output from a column where the bias is not 0
            pb = self._pb
            j = int(pb[0, 0].abs().argmax())
            Bh, Tn, _ = gated_position_bias.shape
            g = gated_position_bias[:, :, j] / pb.repeat(Bh // pb.shape[0], 1, 1)[:, :, j]
            gates.append(g.view(-1, self.num_heads, Tn).clone())
            return orig(self, hidden_states, attention_mask, gated_position_bias, output_attentions)

        wav = torch.randn(3, L, generator=torch.Generator().manual_seed(5)).half().float()    # one batch for both variants, stored as float16
        am = (torch.arange(L).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)).long()
        wav = wav * am
        with torch.no_grad():
            pb = hf.encoder.layers[0].attention.compute_bias(T, T)           # [H, T, T]
            for layer in hf.encoder.layers:
                layer.attention._pb = pb
            modeling_wavlm.WavLMAttention.torch_multi_head_self_attention = spy
            try:
                out = hf(wav, attention_mask=am, output_hidden_states=True)
            finally:
                modeling_wavlm.WavLMAttention.torch_multi_head_self_attention = orig
            valid = hf._get_feature_vector_attention_mask(out.last_hidden_state.shape[1], am).sum(1)
            big = hf.encoder.layers[0].attention.compute_bias(T_MAX, T_MAX)  # [H, 1000, 1000]
        assert valid.tolist() == fairseq_valid_frames(lens, L, T), (valid, lens)
        # Toeplitz: the bias depends on j - i only, so row 0 and column 0 hold the whole matrix
        i = torch.arange(T_MAX)
        d = i[None, :] - i[:, None]
        rebuilt = torch.where(d >= 0, big[:, 0, :][:, d.clamp(min=0)], big[:, :, 0][:, (-d).clamp(min=0)])
        assert torch.equal(rebuilt, big)
        assert len(gates) == 2
        sd = hf.state_dict()
        vk = [k for k in sd if k.endswith("original1") or k.endswith("weight_v")][0]
        # pos_conv's direction tensor [128, 64, 128] is its first 4 input channels x 16, values in {-1, 0, 1} / 32: stored as that
        # [128, 4, 128] int8 block (key posv_<name>), tests/wavlm_cases.py load_fixture rebuilds the tensor
        base = torch.round(sd[vk][:, :4, :] * 32.0).to(torch.int8)
        assert torch.equal((base.float() / 32.0).repeat(1, 16, 1), sd[vk])
        arrs[f"{variant}_posv_{vk}"] = base.numpy()
        arrs.update({f"{variant}_W_{k}": v.numpy() for k, v in sd.items() if "masked_spec_embed" not in k and k != vk})
        # hidden states: the valid frames only, utterance after utterance [NL + 1, sum(valid), D], the low 8 mantissa bits cleared
        # (2^-16 relative, far inside the tolerance they are compared at) so that a quarter of the bytes compresses away
        hs = torch.stack(out.hidden_states)
        hs = torch.cat([hs[:, b, :v] for b, v in enumerate(valid.tolist())], dim=1).contiguous()
        hs = (hs.view(torch.int32) & ~0xff).view(torch.float32)
        g = torch.stack(gates)                             # [NL, B, H, T]: valid frames likewise -> [NL, H, sum(valid)]
        g = torch.cat([g[:, b, :, :v] for b, v in enumerate(valid.tolist())], dim=2).contiguous()
        arrs.update({"wav": wav.half().numpy(), "lens": np.array(lens), f"{variant}_valid": valid.numpy(),
                     f"{variant}_hidden": hs.numpy(), f"{variant}_gates": g.numpy(),
                     f"{variant}_bias_row": big[:, 0, :].numpy(), f"{variant}_bias_col": big[:, :, 0].numpy()})
    path = os.path.join(HERE, "wavlm_small.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, len(arrs), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
