"""Raw-audio input on the GPU (speechclip_plus_amd/audio_prep.py, csrc/audio_prep.hip): PCM of any rate down-mixed and resampled to
16 kHz on the device.
  parity          every output sample against the closed form in float64 (audio_prep.resample_reference), within
                  (taps + 4) 2^-24 sum_j |h_j x_j| - fp32 accumulation plus one rounding per coefficient, no free constant
  batching        an utterance's bits do not depend on the batch, the rates beside it or the call; 16 kHz is the input's own bits
  confinement     NaN patterns between and behind the sources and a NaN-filled output: no NaN comes out, the padding is exact zeros
  long            310 s at 44 100 Hz: the last outputs, where (m P) leaves 32 bits
  end to end      encode_speech / forward on raw PCM == the same calls on the pre-resampled samples, bit for bit"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 22050, 44100, 48000, 96000)
DEV = "cuda:0"


def _noise(n, ch, dtype, seed):
    """full-scale uniform noise [n, ch] (or [n] for one channel): every tap matters, unlike with a sine"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        x = torch.randint(-32768, 32768, (n, ch), generator=g).to(torch.int16)
    else:
        x = torch.rand(n, ch, generator=g) * 2 - 1
    return x[:, 0].contiguous() if ch == 1 else x


def _frames_for(n_out_min, sr):
    """the fewest source frames that give at least n_out_min outputs"""
    from speechclip_plus_amd.audio_prep import out_len, resample_geometry
    P, Q, _ = resample_geometry(sr)
    n = max(n_out_min * P // Q - 2, 1)
    while out_len(n, sr) < n_out_min:
        n += 1
    return n


def _check_against_fp64(got, x, sr, start=0, stop=None):
    from speechclip_plus_amd.audio_prep import resample_geometry, resample_reference
    taps = resample_geometry(sr)[2]
    want, mag = resample_reference(x, sr, torch.float64, start=start, stop=stop, return_abs=True)
    tol = (taps + 4) * 2.0 ** -24 * mag
    err = (got.double().cpu() - want).abs()
    worst = int(torch.argmax(err - tol))
    assert got.shape == want.shape and bool((err <= tol).all()), \
        f"sr {sr}: output {start + worst}: |{got[worst].item()} - {want[worst].item()}| = {err[worst].item():.3e} > {tol[worst].item():.3e}"
    return float((err / tol.clamp(min=1e-30)).max())


# ---------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("dtype", (torch.int16, torch.float32), ids=("int16", "fp32"))
@pytest.mark.parametrize("sr", RATES)
def test_parity_with_the_closed_form_in_fp64(sr, dtype, ch):
    from speechclip_plus_amd.audio_prep import out_len, prep_audio, tile_outputs
    tile = tile_outputs(sr)
    frames = [1, 5, _frames_for(tile, sr), _frames_for(tile + 1, sr), int(0.3 * sr) + 7, int(0.31 * sr)]
    assert out_len(frames[2], sr) == tile and tile < out_len(frames[3], sr) <= tile + 2
    xs = [_noise(n, ch, dtype, seed=1000 + i) for i, n in enumerate(frames)]
    wav, wav_len = prep_audio(xs, sr, DEV)
    n_out = [out_len(n, sr) for n in frames]
    assert wav.is_cuda and wav.dtype == torch.float32 and tuple(wav.shape) == (6, max(n_out))
    assert wav_len.is_cuda and wav_len.dtype == torch.int64 and wav_len._sc_host == n_out and wav_len.tolist() == n_out
    ratio = 0.0
    for b, x in enumerate(xs):
        ratio = max(ratio, _check_against_fp64(wav[b, : n_out[b]], x, sr))
        assert not wav[b, n_out[b]:].any()
    print(f"sr {sr} {dtype} ch {ch}: worst error / tolerance {ratio:.3f}")


# ---------------------------------------------------------------------------------------------------- 2. / 3. batching
@pytest.fixture(scope="module")
def mixed():
    """three rates, both sample formats, mono and stereo in ONE call (shared, left unchanged)"""
    from speechclip_plus_amd.audio_prep import prep_audio
    xs = [_noise(3001, 1, torch.float32, 1), _noise(9000, 2, torch.int16, 2), _noise(7000, 1, torch.int16, 3), _noise(2500, 2, torch.float32, 4),
          _noise(4100, 1, torch.float32, 5)]
    rates = [16000, 44100, 48000, 16000, 44100]
    wav, wav_len = prep_audio(xs, rates, DEV)
    return xs, rates, wav, wav_len


def test_mixed_rates_equal_each_utterance_alone(mixed):
    from speechclip_plus_amd.audio_prep import out_len, prep_audio
    xs, rates, wav, wav_len = mixed
    assert wav_len._sc_host == [out_len(int(x.shape[0]), r) for x, r in zip(xs, rates)] and wav.shape[1] == max(wav_len._sc_host)
    for b, (x, r) in enumerate(zip(xs, rates)):
        alone, alone_len = prep_audio([x], r, DEV)
        n = alone_len._sc_host[0]
        assert n == wav_len._sc_host[b] and tuple(alone.shape) == (1, n)
        assert torch.equal(alone[0].view(torch.int32), wav[b, :n].view(torch.int32)), f"utterance {b} at {r} Hz"
        assert not wav[b, n:].any()
    assert torch.equal(wav[0, :3001].cpu().view(torch.int32), xs[0].view(torch.int32))           # 16 kHz fp32 mono: the input's own bits
    assert torch.equal(wav[3, :2500].cpu(), (xs[3][:, 0] + xs[3][:, 1]) / 2)
    for b in (1, 2, 4):
        _check_against_fp64(wav[b, : wav_len._sc_host[b]], xs[b], rates[b])


def test_two_calls_give_the_same_bits(mixed):
    from speechclip_plus_amd.audio_prep import prep_audio
    xs, rates, wav, wav_len = mixed
    again, again_len = prep_audio(xs, rates, DEV)
    assert again_len._sc_host == wav_len._sc_host and torch.equal(again.view(torch.int32), wav.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 4. confinement
@pytest.mark.parametrize("dtype", (torch.int16, torch.float32), ids=("int16", "fp32"))
def test_poisoned_slack_and_output(dtype):
    from speechclip_plus_amd.audio_prep import RawAudioBatch, out_len, prep_audio, run
    rates, chs, frames = [48000, 11025, 16000, 48000], [2, 1, 2, 1], [5000, 3000, 1500, 3]
    xs = [_noise(n, c, dtype, seed=40 + i) for i, (n, c) in enumerate(zip(frames, chs))]
    slack = 257                                                       # samples of poison in front of, between and behind the utterances
    if dtype == torch.int16:
        poison = lambda n: torch.full((n,), 0x7FFF, dtype=torch.int16)     # as pairs the bits of an fp32 NaN; as samples full scale
    else:
        poison = lambda n: torch.full((n,), float("nan"))
    parts, offsets, at = [poison(slack)], [], slack
    for x in xs:
        offsets.append(at)
        parts += [x.reshape(-1), poison(slack)]
        at += x.numel() + slack
    raw = RawAudioBatch(torch.cat(parts), frames, chs, rates, offsets=offsets)
    n_out = [out_len(n, r) for n, r in zip(frames, rates)]
    out = torch.full((4, max(n_out) + 300), float("nan"), device=DEV)
    wav, wav_len = run(raw, DEV, out=out)
    assert wav is out and wav_len._sc_host == n_out
    assert not bool(torch.isnan(wav).any())
    clean, _ = prep_audio(xs, rates, DEV)
    for b, n in enumerate(n_out):
        assert not wav[b, n:].any() and torch.equal(wav[b, n:], torch.zeros_like(wav[b, n:]))
        assert torch.equal(wav[b, :n].view(torch.int32), clean[b, :n].view(torch.int32)), f"utterance {b}: the slack reached the output"


# ---------------------------------------------------------------------------------------------------- 5. long utterance
def test_the_end_of_a_310_second_utterance():
    """m P passes 2^31 at 304 s (P = 441): the last 1 000 outputs against the float64 restatement evaluated at those indices"""
    from speechclip_plus_amd.audio_prep import prep_audio
    sr, n = 44100, 310 * 44100
    x = _noise(n, 1, torch.int16, seed=310)
    wav, wav_len = prep_audio([x], sr, DEV)
    n_out = 310 * 16000
    assert wav_len._sc_host == [n_out] and tuple(wav.shape) == (1, n_out) and (n_out - 1000) * 441 > 2 ** 31
    _check_against_fp64(wav[0, n_out - 1000:], x, sr, start=n_out - 1000, stop=n_out)
    _check_against_fp64(wav[0, :1000], x, sr, start=0, stop=1000)


# ---------------------------------------------------------------------------------------------------- 6. end to end
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_encode_speech_on_raw_pcm_equals_the_pre_resampled_call(model):
    from speechclip_plus_amd.audio_prep import prep_audio
    pcm = (_noise(int(0.4 * 48000), 2, torch.float32, 60) * 6000).to(torch.int16)
    with torch.no_grad():
        raw = model.encode_speech([pcm], sample_rate=48000)["parallel_audio_feat"]
        wav, wav_len = prep_audio([pcm], 48000, DEV)
        pre = model.encode_speech([wav[0, : wav_len._sc_host[0]]])["parallel_audio_feat"]
        assert wav_len._sc_host == [6400] and tuple(raw.shape) == tuple(pre.shape) and bool(torch.isfinite(raw).all())
        assert torch.equal(raw.view(torch.int32), pre.view(torch.int32))
        # without a rate the call is today's: the samples as they are, the same bits on every run
        same = [torch.randn(5000, generator=torch.Generator().manual_seed(61)) * 0.3, torch.randn(3300, generator=torch.Generator().manual_seed(62)) * 0.3]
        first = model.encode_speech(same)["parallel_audio_feat"]
        second = model.encode_speech(same, sample_rate=None)["parallel_audio_feat"]
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))
        # ... and the 16 kHz pass-through feeds the encoder the very same samples
        third = model.encode_speech(same, sample_rate=16000)["parallel_audio_feat"]
        assert torch.equal(first.view(torch.int32), third.view(torch.int32))
        hs_raw = model.feature_extractor_s3prl([pcm], sample_rate=48000)[0]
        hs_pre = model.feature_extractor_s3prl([wav[0, :6400]])[0]
        assert torch.equal(hs_raw, hs_pre)


def test_forward_on_a_collated_raw_batch_equals_the_pre_resampled_batch(model):
    from speechclip_plus_amd.audio_prep import prep_audio
    from speechclip_plus_amd.data import collate_general, transfer_batch_to_device
    g = torch.Generator().manual_seed(63)
    specs = [(48000, 2, 0.40), (44100, 1, 0.35), (16000, 1, 0.30), (22050, 2, 0.45)]
    pcm = [(_noise(int(s * sr), ch, torch.float32, 70 + i) * 6000).to(torch.int16) for i, (sr, ch, s) in enumerate(specs)]
    images = [torch.randn(512, generator=g) for _ in specs]
    rows = [{"wav": p, "wav_sr": sr, "image": im, "id": b // 2} for b, (p, (sr, _, _), im) in enumerate(zip(pcm, specs, images))]
    batch = collate_general(rows)
    assert batch["wav"].dtype == torch.int16 and batch["wav"].dim() == 1 and "wav_len" not in batch
    on_dev = transfer_batch_to_device(batch, DEV)
    assert on_dev["wav"].is_cuda and all(on_dev[k]._sc_host == batch[k]._sc_host for k in ("wav_frames", "wav_ch", "wav_sr"))
    pre_rows = []
    for b, (p, (sr, _, _), im) in enumerate(zip(pcm, specs, images)):
        wav, wav_len = prep_audio([p], sr, DEV)
        pre_rows.append({"wav": wav[0, : wav_len._sc_host[0]].cpu(), "image": im, "id": b // 2})
    on_dev_pre = transfer_batch_to_device(collate_general(pre_rows), DEV)
    assert on_dev_pre["wav"].dtype == torch.float32 and on_dev_pre["wav"].dim() == 2 and "wav_sr" not in on_dev_pre
    with torch.no_grad():
        _, _, others_raw = model(on_dev)
        _, _, others_pre = model(on_dev_pre)
    a, b = others_raw["parallel_audio_feat"], others_pre["parallel_audio_feat"]
    assert tuple(a.shape) == (4, 512) and bool(torch.isfinite(a).all())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(others_raw["image_feat"], others_pre["image_feat"])
