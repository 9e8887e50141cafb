"""Raw-audio input, host side (speechclip_plus_amd/audio_prep.py): geometry, the coefficient table against the closed form, the closed
form against an analytic sine and an independent resampler, the pass-through, the accepted input forms and the collate route.  The
closed form (include/speechclip_hip.h, "Raw-audio input"): P = sr / gcd, Q = 16000 / gcd, c = 0.99 min(P, Q), W = 6,
y[m] = sum_j x[j] (c / P) sinc(u) cos^2(pi u / 2W) over |u| < W with u = c (j - m P / Q) / P."""
import math
import os
import re
import wave

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000)
PQ_TAPS = {8000: (1, 2, 13), 11025: (441, 640, 13), 22050: (441, 320, 17), 32000: (2, 1, 25), 44100: (441, 160, 34), 48000: (3, 1, 37),
           96000: (6, 1, 73)}


def _sine(sr, seconds=0.25, f=1000.0):
    return torch.from_numpy(np.sin(2 * np.pi * f * np.arange(int(sr * seconds)) / sr).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbol_declared_bound_and_exported():
    from speechclip_plus_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    decl = re.search(r"int sc_audio_resample\(([^;]*)\);", header)
    lib = _lib.lib()
    assert decl is not None and hasattr(lib, "sc_audio_resample")
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["sc_audio_resample"]) == 16
    assert lib.sc_abi_version() == 7                                   # the change is additive
    assert "audio_prep.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "audio_prep.hip"))
    assert callable(ops.audio_resample)
    # argument checks answer before any launch: a null source, and a table past 64 KB
    assert lib.sc_audio_resample(None, 8, 1, None, 1, None, None, 3, 1, 37, 2048, None, 8, 1, 8, None) != 0
    assert lib.sc_audio_resample(1 << 12, 8, 1, 1 << 12, 1, 1 << 12, 1 << 12, 441, 4000, 13, 2048, 1 << 12, 8, 1, 8, None) != 0
    assert b"65536" in lib.sc_last_error()


# ---------------------------------------------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize("sr", RATES)
def test_geometry_and_out_len(sr):
    from speechclip_plus_amd.audio_prep import out_len, resample_geometry, tile_outputs
    P, Q, taps = resample_geometry(sr)
    assert (P, Q, taps) == PQ_TAPS[sr]
    assert P * 16000 == Q * sr and math.gcd(P, Q) == 1
    for n in (1, 2, P - 1, P, P + 1, 10 * P + 3):
        if n < 1:
            continue
        want = -((-n * Q) // P)                                         # ceil(n Q / P)
        assert out_len(n, sr) == want and (want - 1) * P < n * Q <= want * P
    assert out_len(P, sr) == Q and out_len(P + 1, sr) == Q + -(-Q // P)
    tile = tile_outputs(sr)
    assert tile % 256 == 0 and 256 <= tile <= 2048 and ((tile - 1) * P + Q - 1) // Q + taps + 2 <= 8192


def test_geometry_of_the_target_rate_and_integer_types():
    from speechclip_plus_amd.audio_prep import out_len, resample_geometry
    assert resample_geometry(16000) == (1, 1, 1) and out_len(12345, 16000) == 12345
    assert all(isinstance(v, int) for v in resample_geometry(44100)) and isinstance(out_len(7, 44100), int)
    assert out_len(310 * 44100, 44100) == 310 * 16000                 # far past 2^31 / 441, in python integers


# ---------------------------------------------------------------------------------------------------- 2. table
@pytest.mark.parametrize("sr", RATES)
def test_table_is_the_closed_form_rounded_once(sr):
    from speechclip_plus_amd.audio_prep import resample_geometry, resample_table
    P, Q, taps = resample_geometry(sr)
    table, first = resample_table(sr)
    assert table.dtype == torch.float32 and tuple(table.shape) == (Q, taps) and first.dtype == torch.int32 and tuple(first.shape) == (Q,)
    assert table.numel() * 4 <= 33 * 1024 + 512
    assert resample_table(sr)[0] is table                              # cached per rate and device
    c, W = 0.99 * min(P, Q), 6
    got = table.double().numpy()
    for i in range(Q):
        k = first[i].item() + np.arange(-1, taps + 1)                   # one tap before the row and one behind it as well
        u = c * (k - i * P / Q) / P
        inside = np.abs(u) < W
        assert np.all(np.abs(np.abs(u) - W) > 1e-9)                     # no rate here puts a tap on |u| = W, where float64 could not decide
        h = (c / P) * np.sinc(u) * np.cos(np.pi * u / (2 * W)) ** 2
        # every phase's taps cover exactly |u| < W: the tap before the first lies outside, the taps inside form one run from t = 0
        n_in = int(inside[1:-1].sum())
        assert not inside[0] and inside[1] and np.all(inside[1: 1 + n_in]) and not np.any(inside[1 + n_in:]), (sr, i)
        want = np.where(inside[1:-1], h[1:-1], 0.0)
        assert np.all(got[i, n_in:] == 0.0)
        err = np.abs(got[i] - want)
        # one fp32 rounding per coefficient (+ 1e-15: sin(pi u) of the two float64 evaluations near a zero crossing)
        assert np.all(err <= np.abs(want) * 2.0 ** -24 + 1e-15), (sr, i, err.max())
    assert max(int((table[i] != 0).sum()) for i in range(Q)) <= taps and np.any(got[:, taps - 1] != 0.0)


# ---------------------------------------------------------------------------------------------------- 3. sine
@pytest.mark.parametrize("sr", RATES)
def test_sine_against_the_analytic_16k_sine(sr):
    """bound 2e-3: a property of the filter (twice the worst value measured on the closed form, 1.0e-3 at 11 025 Hz)"""
    from speechclip_plus_amd.audio_prep import resample_reference
    y = resample_reference(_sine(sr), sr, torch.float64)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000)
    err = np.abs(y.numpy() - want)[200:-200].max()
    print(f"sine 1 kHz at {sr} Hz: max abs error on interior outputs {err:.2e}")
    assert y.dtype == torch.float64 and len(y) == 4000 and err <= 2e-3


# ---------------------------------------------------------------------------------------------------- 4. independent resampler
@pytest.mark.parametrize("sr", RATES)
def test_against_scipy_resample_poly(sr):
    """bound 5e-3 (about twice the 2.4e-3 measured at 8 kHz): the definition is a resampler, nothing finer"""
    from scipy.signal import resample_poly
    from speechclip_plus_amd.audio_prep import resample_geometry, resample_reference
    P, Q, _ = resample_geometry(sr)
    rng = np.random.default_rng(20)
    f, a, p = rng.uniform(50, 3000, 20), rng.uniform(0.2, 1.0, 20), rng.uniform(0, 2 * np.pi, 20)
    t = np.arange(sr // 4) / sr
    x = (a[:, None] * np.sin(2 * np.pi * f[:, None] * t[None, :] + p[:, None])).sum(0)
    x = (x / np.abs(x).max()).astype(np.float32)                       # full scale
    y = resample_reference(x, sr, torch.float64).numpy()
    z = resample_poly(x.astype(np.float64), Q, P)
    assert len(z) == len(y)
    err = np.abs(y - z)[200:-200].max()
    print(f"20 sines at {sr} Hz: max abs difference from scipy.signal.resample_poly on interior outputs {err:.2e}")
    assert err <= 5e-3


# ---------------------------------------------------------------------------------------------------- 5. pass-through
def test_pass_through_at_16k():
    from speechclip_plus_amd.audio_prep import prep_audio, resample_reference
    g = torch.Generator().manual_seed(5)
    x = torch.randn(777, generator=g)
    for dt in (torch.float32, torch.float64):
        assert torch.equal(resample_reference(x, 16000, dt), x.to(dt))
    pcm = torch.randint(-32768, 32768, (501,), generator=g).to(torch.int16)
    pcm[:2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    assert torch.equal(resample_reference(pcm, 16000, torch.float32), pcm.float() / 32768.0)
    st = torch.randn(300, 2, generator=g)
    assert torch.equal(resample_reference(st, 16000, torch.float32), (st[:, 0] + st[:, 1]) / 2)
    st16 = torch.randint(-32768, 32768, (300, 2), generator=g).to(torch.int16)
    assert torch.equal(resample_reference(st16, 16000, torch.float32), (st16[:, 0].float() / 32768 + st16[:, 1].float() / 32768) / 2)
    # the whole call on the host: the fp32 restatement, padded, with host lengths
    wav, wav_len = prep_audio([x, pcm, st.numpy()], 16000, "cpu")
    assert wav.dtype == torch.float32 and tuple(wav.shape) == (3, 777) and wav_len.tolist() == [777, 501, 300] == wav_len._sc_host
    assert torch.equal(wav[0], x) and torch.equal(wav[1, :501], pcm.float() / 32768.0) and torch.equal(wav[2, :300], (st[:, 0] + st[:, 1]) / 2)
    assert not wav[1, 501:].any() and not wav[2, 300:].any()


def test_host_path_resamples_and_pads():
    from speechclip_plus_amd.audio_prep import out_len, prep_audio, resample_reference
    a, b = _sine(48000, 0.05), (_sine(44100, 0.02) * 20000).to(torch.int16)
    wav, wav_len = prep_audio([a, b], [48000, 44100], "cpu")
    assert wav_len._sc_host == [out_len(len(a), 48000), out_len(len(b), 44100)] == [800, 320] and tuple(wav.shape) == (2, 800)
    assert torch.equal(wav[0], resample_reference(a, 48000, torch.float32)) and not wav[1, 320:].any()
    assert (wav[1, :320].double() - resample_reference(b, 44100, torch.float64)).abs().max() < 1e-5


# ---------------------------------------------------------------------------------------------------- 6. input forms
def test_wav_file_reads_back_as_its_array(tmp_path):
    from speechclip_plus_amd.audio_prep import as_entries
    pcm = np.random.default_rng(6).integers(-32768, 32768, (1234, 2)).astype(np.int16)
    path = tmp_path / "stereo_22050.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(22050)
        f.writeframes(pcm.astype("<i2").tobytes())
    (from_file, sr_file), (from_array, sr_array) = as_entries([str(path), pcm], 22050)
    assert sr_file == sr_array == 22050 and from_file.dtype == torch.int16 and torch.equal(from_file, from_array)
    assert torch.equal(as_entries([path], 16000)[0][0], from_array) and as_entries([path], 16000)[0][1] == 22050     # the header's rate
    mono = as_entries([pcm[:, 0].copy(), torch.zeros(9)], [8000, 48000])
    assert [tuple(t.shape) for t, _ in mono] == [(1234, 1), (9, 1)] and [r for _, r in mono] == [8000, 48000]


def test_every_refusal_names_the_item(tmp_path):
    from speechclip_plus_amd.audio_prep import as_entries
    ok = torch.zeros(10)
    wide = tmp_path / "wide.wav"
    with wave.open(str(wide), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(3)
        f.setframerate(16000)
        f.writeframes(bytes(30))
    not_wav = tmp_path / "not.wav"
    not_wav.write_bytes(b"ID3 this is no RIFF file")
    cases = [(torch.zeros(10, dtype=torch.float64), 16000, "dtype"), (np.zeros(10, dtype=np.int32), 16000, "dtype"),
             (torch.zeros(10, dtype=torch.uint8), 16000, "dtype"), (str(wide), 16000, "24-bit"), (str(not_wav), 16000, "WAV"),
             (ok, 3999, "3999"), (ok, 192001, "192001"), (ok, 44101, "table"), (ok, 16000.0, "int"), (ok, None, "int"),
             (torch.zeros(0), 16000, "empty"), (torch.zeros(0, 2), 16000, "empty"), (torch.zeros(10, 9), 16000, "channels"),
             (torch.zeros(2, 3, 4), 16000, "shape"), ({"no": "audio"}, 16000, "dict")]
    for bad, sr, word in cases:
        with pytest.raises(ValueError, match="audio item 1") as e:
            as_entries([ok, bad], [16000, sr])
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError, match="2 sample rates for 1"):
        as_entries([ok], [16000, 16000])
    with pytest.raises(ValueError, match="empty audio batch"):
        as_entries([], 16000)
    with pytest.raises(ValueError, match="list"):
        as_entries(ok, 16000)


def test_collate_without_wav_sr_is_unchanged():
    from speechclip_plus_amd.data import collate_general
    rows = [{"wav": torch.tensor([1.0, 2.0, 3.0]), "image": torch.tensor([0.5, -0.5]), "id": 4},
            {"wav": torch.tensor([4.0]), "image": torch.tensor([1.5, 2.5]), "id": 9}]
    out = collate_general(rows)
    assert list(out.keys()) == ["wav", "image", "id", "wav_len"]
    assert torch.equal(out["wav"], torch.tensor([[1.0, 2.0, 3.0], [4.0, 0.0, 0.0]])) and out["wav"].dtype == torch.float32
    assert torch.equal(out["image"], torch.tensor([[0.5, -0.5], [1.5, 2.5]]))
    assert torch.equal(out["id"], torch.tensor([4, 9])) and out["id"].dtype == torch.int64
    assert torch.equal(out["wav_len"], torch.tensor([3, 1])) and out["wav_len"].dtype == torch.int64 and out["wav_len"]._sc_host == [3, 1]


def test_collate_with_wav_sr_packs_and_keeps_host_twins():
    from speechclip_plus_amd.audio_prep import RawAudioBatch
    from speechclip_plus_amd.data import collate_general, transfer_batch_to_device
    a = torch.tensor([[100, -100], [200, -200], [300, -300]], dtype=torch.int16)
    b = torch.tensor([7, 8, 9, 10, 11], dtype=torch.int16)
    rows = [{"wav": a, "wav_sr": 48000, "image": torch.zeros(2), "id": 0}, {"wav": b, "wav_sr": 16000, "image": torch.ones(2), "id": 1}]
    out = collate_general(rows)
    assert "wav_len" not in out and set(out) == {"wav", "wav_frames", "wav_ch", "wav_sr", "image", "id"}
    assert out["wav"].dtype == torch.int16 and out["wav"].tolist() == [100, -100, 200, -200, 300, -300, 7, 8, 9, 10, 11]
    for key, want in (("wav_frames", [3, 5]), ("wav_ch", [2, 1]), ("wav_sr", [48000, 16000])):
        assert out[key].dtype == torch.int64 and out[key].tolist() == want == out[key]._sc_host
    moved = transfer_batch_to_device(out, "cpu")
    assert all(moved[k]._sc_host == out[k]._sc_host for k in ("wav_frames", "wav_ch", "wav_sr"))
    raw = RawAudioBatch(moved["wav"], moved["wav_frames"], moved["wav_ch"], moved["wav_sr"])
    assert raw.offsets == [0, 6] and torch.equal(raw.entry(0), a) and torch.equal(raw.entry(1).reshape(-1), b)
    # one fp32 utterance makes the packed buffer fp32; the int16 one becomes x / 32768, which is exact
    mixed = collate_general([rows[0], {"wav": torch.tensor([0.25, -0.5]), "wav_sr": 8000, "image": torch.ones(2), "id": 1}])
    assert mixed["wav"].dtype == torch.float32 and torch.equal(mixed["wav"][:6], a.reshape(-1).float() / 32768.0)
    with pytest.raises(ValueError, match="audio item 1"):
        collate_general([rows[0], {"wav": b, "wav_sr": 44101, "image": torch.ones(2), "id": 1}])


def test_public_entry_points_take_sample_rate():
    import inspect
    from speechclip_plus_amd import KWClip_GeneralTransformer
    for name in ("processWavs", "encode_speech", "extract_keywords", "feature_extractor_s3prl"):
        p = inspect.signature(getattr(KWClip_GeneralTransformer, name)).parameters
        assert "sample_rate" in p and p["sample_rate"].default is None, name
    wav = [torch.zeros(5), torch.zeros(3)]
    got = KWClip_GeneralTransformer.processWavs(None, wav)              # without a rate: today's path, the same objects
    assert got[0] is wav and got[1] == [5, 3]
