"""Raw-audio input of the speech encoder: PCM of any rate, ``int16`` or ``float32``, mono or interleaved multi-channel -> the 16 kHz mono
fp32 batch every entry point here expects.  The reference gets there through ``librosa.load(path, sr=16_000)``
(avssl/data/base_dataset.py:81, example.py:21): decode, to float, to mono, resample.  This module is everything behind the decoder, as
host geometry / coefficient tables plus one HIP kernel (csrc/audio_prep.hip).

The resampler is the project's own, stated in closed form.  ``g = gcd(sr, 16000)``, ``P = sr / g``, ``Q = 16000 / g``,
``c = 0.99 min(P, Q)``, ``W = 6``, ``x[j] = 0`` outside ``0 <= j < n``, ``u = c (j - m P / Q) / P``:

    y[m] = sum_j x[j] (c / P) sinc(u) cos^2(pi u / (2 W))    over |u| < W,        n_out = ceil(n Q / P)

a Hann-windowed sinc with six zero crossings and roll-off 0.99 - the default filter of torchaudio's ``resample``.  It is NOT librosa's
``soxr_hq``: neither librosa, soxr nor torchaudio was available to run against, so no bit parity with the reference's loader is claimed;
the yardstick is the closed form in float64 (``resample_reference``).  ``sr == 16000`` is an exact pass-through (no filter).  Before the
filter, in librosa's order: ``int16`` becomes ``x / 32768``, channels are averaged in fp32 as ``(x0 + x1 + ...) / ch``.

  resample_geometry / out_len   P, Q, taps per output and the output length, in integers
  resample_table                the polyphase table [Q, taps] fp32 (computed in float64, rounded once) and each phase's first tap
  resample_reference            the torch restatement of the closed form: the float64 yardstick of the tests, and in fp32 the path taken
                                when there is no GPU
  as_entries / pack             validation of a list of arrays / tensors / 16-bit WAV paths; the packed ragged buffer (RawAudioBatch)
  run / prep_audio              one pinned H2D copy on the "h2d" stream + one launch per distinct rate; no device synchronisation

Not built: compressed formats and WAV files that are not 16-bit PCM; the data sets' ``normalize_waveform`` layer-norm; writing the
resampled samples straight into the conv front end's operand (the way image_prep writes the patch GEMM's) - a later fusion.
"""
import math
import os
import wave
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .data import attach_host_lengths

TARGET_SR = 16000
ZEROS = 6                          # W: zero crossings on each side
ROLLOFF_NUM, ROLLOFF_DEN = 99, 100  # c = 0.99 min(P, Q)
MIN_SR, MAX_SR = 4000, 192000
MAX_CH = 8
MAX_TABLE_BYTES = 64 * 1024        # [Q, taps] fp32: the kernel holds it in LDS
DESC_WORDS = 5                     # int64 per utterance (include/speechclip_hip.h, "Raw-audio input")
MAX_TILE = 2048                    # outputs per workgroup ...
WINDOW_FLOATS = 8192               # ... as long as the tile's input window stays below this (32 KiB of LDS)
_GEOM_CACHE = {}
_TABLE64_CACHE = {}
_TABLE_CACHE = {}


# --------------------------------------------------------------------------------------------------------- geometry and tables
def _check_rate(sr, what: str = "sample rate") -> int:
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)):
        raise ValueError(f"{what}: an int in Hz, got {sr!r}")
    sr = int(sr)
    if sr < MIN_SR or sr > MAX_SR:
        raise ValueError(f"{what} {sr} Hz: supported rates are {MIN_SR} .. {MAX_SR} Hz")
    return sr


def _phases(P: int, Q: int) -> Tuple[np.ndarray, np.ndarray]:
    """(first [Q], count [Q]) int64: phase i = m mod Q reads x[(m div Q) P + k] for first[i] <= k < first[i] + count[i], exactly the k
    with |u| < W.  u = c (k - i P / Q) / P = 99 (k Q - i P) / (100 max(P, Q)), so |u| < 6 is 99 |k Q - i P| < 600 max(P, Q): integers."""
    bound = (ZEROS * ROLLOFF_DEN * max(P, Q) - 1) // ROLLOFF_NUM          # the largest |k Q - i P| inside the window
    ip = np.arange(Q, dtype=np.int64) * P
    first = -((bound - ip) // Q)                                          # ceil((i P - bound) / Q)
    last = (ip + bound) // Q
    return first, last - first + 1


def resample_geometry(sr: int) -> Tuple[int, int, int]:
    """(P, Q, taps): ``sr / gcd``, ``16000 / gcd`` and the largest number of source samples one output reads; integer arithmetic only"""
    sr = _check_rate(sr)
    hit = _GEOM_CACHE.get(sr)
    if hit is None:
        g = math.gcd(sr, TARGET_SR)
        P, Q = sr // g, TARGET_SR // g
        hit = _GEOM_CACHE[sr] = (P, Q, 1 if P == Q else int(_phases(P, Q)[1].max()))
    return hit


def check_rate(sr: int, what: str = "sample rate") -> int:
    """the limits of one source rate, named: 4 000 .. 192 000 Hz and a coefficient table of at most 64 KB"""
    sr = _check_rate(sr, what)
    P, Q, taps = resample_geometry(sr)
    if (P, Q) != (1, 1) and Q * taps * 4 > MAX_TABLE_BYTES:
        raise ValueError(f"{what} {sr} Hz: the coefficient table [Q = {Q}, taps = {taps}] fp32 needs {Q * taps * 4} bytes, the limit is "
                         f"{MAX_TABLE_BYTES} (a rate that shares a larger divisor with {TARGET_SR})")
    return sr


def out_len(n: int, sr: int) -> int:
    """ceil(n Q / P): the number of 16 kHz samples ``n`` samples at ``sr`` become"""
    P, Q, _ = resample_geometry(sr)
    return (int(n) * Q + P - 1) // P


def tile_outputs(sr: int) -> int:
    """outputs per workgroup of the kernel at this rate: the largest multiple of 256 up to MAX_TILE whose input window fits"""
    P, Q, taps = resample_geometry(sr)
    tile = MAX_TILE
    while tile > 256 and ((tile - 1) * P + Q - 1) // Q + taps + 2 > WINDOW_FLOATS:
        tile -= 256
    return tile


def _table64(sr: int) -> Tuple[np.ndarray, np.ndarray]:
    """(h [Q, taps] float64, first [Q] int32): the closed form's coefficients, zero behind a phase's own tap count"""
    sr = check_rate(sr)
    hit = _TABLE64_CACHE.get(sr)
    if hit is None:
        P, Q, taps = resample_geometry(sr)
        if (P, Q) == (1, 1):
            h, first = np.ones((1, 1)), np.zeros(1, dtype=np.int32)
        else:
            first, count = _phases(P, Q)
            t = np.arange(taps, dtype=np.int64)[None, :]
            n = (first[:, None] + t) * Q - (np.arange(Q, dtype=np.int64) * P)[:, None]          # k Q - i P
            u = (ROLLOFF_NUM * n).astype(np.float64) / float(ROLLOFF_DEN * max(P, Q))
            h = (ROLLOFF_NUM * min(P, Q) / (ROLLOFF_DEN * P)) * np.sinc(u) * np.cos(np.pi * u / (2 * ZEROS)) ** 2
            h = np.where(t < count[:, None], h, 0.0)
            first = first.astype(np.int32)
        h.setflags(write=False)
        first.setflags(write=False)
        hit = _TABLE64_CACHE[sr] = (h, first)
    return hit


def resample_table(sr: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(table [Q, taps] fp32, first [Q] int32) on ``device`` (default: the host).  Output m = q Q + i is
    ``sum_t table[i, t] x[q P + first[i] + t]``; the coefficients are computed in float64 and rounded once; cached per rate and device."""
    device = torch.device("cpu" if device is None else device)
    key = (int(sr), str(device))
    hit = _TABLE_CACHE.get(key)
    if hit is None:
        h, first = _table64(sr)
        hit = (torch.from_numpy(h.astype(np.float32)).to(device), torch.from_numpy(first.copy()).to(device))
        _TABLE_CACHE[key] = hit
    return hit


def _mono_f32(x: torch.Tensor) -> torch.Tensor:
    """[frames, ch] or [frames], int16 or fp32 -> [frames] fp32: x / 32768, then (x0 + x1 + ...) / ch in channel order"""
    f = x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x.to(torch.float32)
    if f.dim() == 1:
        return f
    s = f[:, 0].clone() if f.shape[1] > 1 else f[:, 0]
    for c in range(1, f.shape[1]):
        s = s + f[:, c]
    return s / float(f.shape[1]) if f.shape[1] > 1 else s


def resample_reference(x, sr: int, dtype: torch.dtype = torch.float64, start: int = 0, stop: Optional[int] = None, return_abs: bool = False):
    """The closed form restated in torch on the device ``x`` lives on: outputs ``start .. stop - 1`` (default: all ``out_len(n, sr)``) of
    one utterance ``x`` ([frames] or [frames, ch], int16 or fp32).  Conversion and down-mix are in fp32, as defined; the filter runs in
    ``dtype``: float64 with the unrounded coefficients is the tests' yardstick, float32 with ``resample_table`` the path without a GPU.
    ``return_abs``: also ``sum_j |h_j x_j|`` per output (the scale of the kernel's rounding error)."""
    x = _one_entry(x, "resample_reference")
    mono = _mono_f32(x)
    n = int(mono.shape[0])
    P, Q, taps = resample_geometry(check_rate(sr))
    total = out_len(n, sr)
    stop = total if stop is None else min(int(stop), total)
    start = max(int(start), 0)
    if (P, Q) == (1, 1):
        y = mono[start:stop].to(dtype)
        return (y, y.abs()) if return_abs else y
    if dtype == torch.float64:
        h = torch.from_numpy(_table64(sr)[0].copy()).to(mono.device)
        first = torch.from_numpy(_table64(sr)[1].astype(np.int64)).to(mono.device)
    else:
        h, first = resample_table(sr, mono.device)
        h, first = h.to(dtype), first.long()
    m = torch.arange(start, max(stop, start), dtype=torch.int64, device=mono.device)
    q = torch.div(m, Q, rounding_mode="floor")
    ph = m - q * Q
    base = q * P + first[ph]
    src = mono.to(dtype)
    acc = torch.zeros(m.shape[0], dtype=dtype, device=mono.device)
    mag = torch.zeros_like(acc)
    zero = torch.zeros((), dtype=dtype, device=mono.device)
    for t in range(taps):                                       # ascending j, as the kernel
        j = base + t
        xv = torch.where((j >= 0) & (j < n), src[j.clamp(0, n - 1)], zero)
        term = h[ph, t] * xv
        acc = acc + term
        if return_abs:
            mag = mag + term.abs()
    return (acc, mag) if return_abs else acc


# --------------------------------------------------------------------------------------------------------- inputs
def _read_wav(path, what: str) -> Tuple[torch.Tensor, int]:
    try:
        with wave.open(os.fspath(path), "rb") as f:
            ch, width, sr, frames, comp = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes(), f.getcomptype()
            data = f.readframes(frames)
    except (wave.Error, EOFError, OSError) as e:
        raise ValueError(f"{what}: {path!r} does not read as a PCM WAV file ({e})") from None
    if width != 2 or comp != "NONE":
        raise ValueError(f"{what}: {path!r} holds {8 * width}-bit samples ({comp}); only 16-bit PCM WAV files are read")
    pcm = np.frombuffer(data, dtype="<i2").astype(np.int16)
    return torch.from_numpy(pcm[: (len(pcm) // ch) * ch].reshape(-1, ch).copy()), sr


def _one_entry(x, what: str) -> torch.Tensor:
    """one array / tensor -> [frames, ch] int16 or fp32 torch tensor (host or device), validated"""
    if isinstance(x, np.ndarray):
        if x.dtype not in (np.int16, np.float32):
            raise ValueError(f"{what}: samples are int16 or float32, got dtype {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x) if x.flags.writeable else np.array(x))
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}: a 1-D or [frames, channels] tensor or numpy array, or a path to a 16-bit PCM WAV file, got {type(x)}")
    if x.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"{what}: samples are int16 or float32, got dtype {x.dtype}")
    if x.dim() == 1:
        x = x.unsqueeze(1)
    if x.dim() != 2:
        raise ValueError(f"{what}: shape [frames] or [frames, channels], got {tuple(x.shape)}")
    if x.shape[1] < 1 or x.shape[1] > MAX_CH:
        raise ValueError(f"{what}: {x.shape[1]} channels in shape {tuple(x.shape)} ([frames, channels]); 1 .. {MAX_CH} are supported")
    if x.shape[0] < 1:
        raise ValueError(f"{what}: empty (no frames)")
    return x


def as_entries(wavs, sample_rate) -> List[Tuple[torch.Tensor, int]]:
    """a list of utterances -> validated (``[frames, ch]`` int16 / fp32 tensor, rate) pairs; every rule is enforced here, before any
    launch.  Items: 1-D (mono) or ``[frames, channels]`` tensors / numpy arrays, or paths of 16-bit PCM WAV files (their rate and channel
    count come from the header; ``sample_rate`` applies to the arrays).  ``sample_rate``: one int, or one per item."""
    if not isinstance(wavs, (list, tuple)):
        raise ValueError(f"raw audio comes as a list, got {type(wavs)}")
    if len(wavs) == 0:
        raise ValueError("empty audio batch: a non-empty list of utterances")
    if isinstance(sample_rate, (list, tuple, np.ndarray, torch.Tensor)):
        rates = [int(r) if isinstance(r, (int, np.integer)) and not isinstance(r, bool) else (r.item() if isinstance(r, torch.Tensor) else r)
                 for r in (sample_rate.tolist() if isinstance(sample_rate, (np.ndarray, torch.Tensor)) else sample_rate)]
        if len(rates) != len(wavs):
            raise ValueError(f"{len(rates)} sample rates for {len(wavs)} utterances")
    else:
        rates = [sample_rate] * len(wavs)
    out = []
    for i, (x, sr) in enumerate(zip(wavs, rates)):
        what = f"audio item {i}"
        if isinstance(x, (str, os.PathLike)):
            x, sr = _read_wav(x, what)
        out.append((_one_entry(x, what), check_rate(sr, f"{what}: sample rate")))
    return out


def _host_ints(v, name: str) -> List[int]:
    if isinstance(v, torch.Tensor):
        host = getattr(v, "_sc_host", None)
        if host is None:
            if v.is_cuda:
                raise ValueError(f"{name} on the device needs its host twin (data.transfer_batch_to_device keeps it): reading it back would "
                                 "synchronise")
            host = v.tolist()
        v = host
    return [int(a) for a in v]


class RawAudioBatch:
    """B utterances of unequal lengths, channel counts and rates as one packed 1-D buffer of ``int16`` or ``float32`` samples: utterance b
    is ``packed[offset[b] : offset[b] + frames[b] ch[b]]`` read as [frames, ch] (interleaved).  ``frames`` / ``ch`` / ``sr`` are HOST
    data: lists, or int64 [B] tensors that live on the host or carry a host twin.  ``offsets`` (in samples) default to back-to-back."""

    def __init__(self, packed: torch.Tensor, frames, ch, sr, offsets: Optional[Sequence[int]] = None):
        self.frames, self.ch, self.sr = _host_ints(frames, "wav_frames"), _host_ints(ch, "wav_ch"), _host_ints(sr, "wav_sr")
        if not isinstance(packed, torch.Tensor) or packed.dtype not in (torch.int16, torch.float32) or packed.dim() != 1:
            raise ValueError("packed raw audio must be a 1-D int16 or float32 tensor, got "
                             f"{getattr(packed, 'dtype', type(packed))} {tuple(getattr(packed, 'shape', ()))}")
        B = len(self.frames)
        if B < 1 or len(self.ch) != B or len(self.sr) != B:
            raise ValueError(f"raw audio batch: {B} frame counts, {len(self.ch)} channel counts, {len(self.sr)} rates (equal and >= 1)")
        sizes = [n * c for n, c in zip(self.frames, self.ch)]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        self.offsets = [int(o) for o in offsets]
        if len(self.offsets) != B:
            raise ValueError(f"{len(self.offsets)} offsets for {B} utterances")
        for b, (n, c, r, o) in enumerate(zip(self.frames, self.ch, self.sr, self.offsets)):
            if n < 1 or c < 1 or c > MAX_CH:
                raise ValueError(f"audio item {b}: {n} frames of {c} channels (frames >= 1, channels 1 .. {MAX_CH})")
            check_rate(r, f"audio item {b}: sample rate")
            if o < 0 or o + n * c > packed.numel():
                raise ValueError(f"audio item {b}: {n} x {c} samples at offset {o} do not fit the packed buffer of {packed.numel()} samples")
        self.packed = packed
        self._stage = None                 # pack(): the pinned buffer ``packed`` is a view of, with room for run()'s descriptors

    def __len__(self):
        return len(self.frames)

    def entry(self, b: int) -> torch.Tensor:
        return self.packed[self.offsets[b]: self.offsets[b] + self.frames[b] * self.ch[b]].reshape(self.frames[b], self.ch[b])


def _pin_here() -> bool:
    """where data.collate_general pins: a GPU is there and this is not a DataLoader worker"""
    import torch.utils.data
    return torch.cuda.is_available() and torch.utils.data.get_worker_info() is None


def pack(entries: Sequence[Tuple[torch.Tensor, int]], pin_memory: bool = False) -> RawAudioBatch:
    """validated entries -> one RawAudioBatch: int16 if every utterance is, else fp32 (int16 items become x / 32768, which is exact, so
    the result's bits do not depend on what else is in the batch).  Host entries pack on the host (pinned if asked and possible, with
    room behind the samples for what ``run`` uploads with them), a batch with device entries on their device."""
    i16 = all(t.dtype == torch.int16 for t, _ in entries)
    dtype = torch.int16 if i16 else torch.float32
    frames, ch, sr = [int(t.shape[0]) for t, _ in entries], [int(t.shape[1]) for t, _ in entries], [r for _, r in entries]
    dev = next((t.device for t, _ in entries if t.is_cuda), torch.device("cpu"))
    total, stage = sum(n * c for n, c in zip(frames, ch)), None
    if dev.type == "cpu":
        # one buffer [samples | room for run()'s descriptors and lengths]: pinned, it is what the single H2D copy reads
        nbytes = total * (2 if i16 else 4)
        stage = torch.empty((nbytes + 15) // 16 * 16 + (DESC_WORDS + 1) * 8 * len(entries), dtype=torch.uint8,
                            pin_memory=bool(pin_memory) and _pin_here())
        packed = stage[:nbytes].view(dtype)
    else:
        packed = torch.empty(total, dtype=dtype, device=dev)
    at = 0
    for t, _ in entries:
        flat = t.reshape(-1)
        if flat.dtype != dtype:
            flat = flat.to(torch.float32) / 32768.0
        packed[at: at + flat.numel()].copy_(flat)
        at += flat.numel()
    raw = RawAudioBatch(packed, frames, ch, sr)
    raw._stage = stage
    return raw


# --------------------------------------------------------------------------------------------------------- device
def run(raw: RawAudioBatch, device, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``raw`` -> (wav [B, Lmax] fp32 at 16 kHz, zero behind each utterance; wav_len [B] int64 with its host twin) on ``device``.  On a
    GPU: host samples and the descriptors travel in ONE pinned copy on the "h2d" stream (device-resident samples: the descriptors
    alone), the current stream waits for its event, then one launch per distinct rate writes every element of ``wav``.  No device
    synchronisation.  Without a GPU: ``resample_reference`` in fp32.  ``out``: the caller's buffer [B, >= Lmax] (tests)."""
    device = torch.device(device)
    B = len(raw)
    n_out = [out_len(n, r) for n, r in zip(raw.frames, raw.sr)]
    Lmax = max(n_out)
    if out is not None and (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < Lmax or out.stride(1) != 1):
        raise ValueError(f"out must be fp32 [{B}, >= {Lmax}] with unit column stride, got {out.dtype} {tuple(out.shape)}")
    if device.type != "cuda":
        wav = torch.zeros(B, Lmax, dtype=torch.float32) if out is None else out.zero_()
        for b in range(B):
            wav[b, : n_out[b]] = resample_reference(raw.entry(b).cpu(), raw.sr[b], torch.float32)
        return wav.to(device), attach_host_lengths(torch.tensor(n_out, dtype=torch.long).to(device), n_out)
    from . import ops
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    esz = raw.packed.element_size()
    groups = {}
    for b, r in enumerate(raw.sr):
        groups.setdefault(r, []).append(b)
    order = [b for bs in groups.values() for b in bs]
    aux = np.empty(DESC_WORDS * B + B, dtype=np.int64)                    # [descriptors, grouped by rate | n_out per utterance]
    aux[: DESC_WORDS * B].reshape(B, DESC_WORDS)[:] = [(raw.offsets[b] * esz, raw.frames[b], raw.ch[b], n_out[b], b) for b in order]
    aux[DESC_WORDS * B:] = n_out
    main = torch.cuda.current_stream(device)
    cs = ops.shared_stream("h2d", device, priority=-1)
    if raw.packed.is_cuda:
        stage = torch.from_numpy(aux).pin_memory()
        with torch.cuda.stream(cs):                  # allocated on the copy stream's pool: nothing queued elsewhere still reads the block
            aux_d = stage.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        src = raw.packed if raw.packed.device == device else raw.packed.to(device, non_blocking=True)
    else:
        pcm_bytes = raw.packed.numel() * esz
        aux_at = (pcm_bytes + 15) // 16 * 16
        stage = raw._stage                           # pack()'s own buffer: the samples sit in it already, with room for the descriptors
        if stage is None or not stage.is_pinned() or stage.numel() < aux_at + aux.nbytes:
            stage = None
        if stage is None and raw.packed.is_pinned():
            # pinned samples without room behind them (a collated batch given to forward as it is): two copies, no staging on the host
            aux_h = torch.from_numpy(aux).pin_memory()
            with torch.cuda.stream(cs):
                src, aux_d = raw.packed.to(device, non_blocking=True), aux_h.to(device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
            src.record_stream(main)
        else:
            if stage is None:                        # pageable samples: staged through pinned memory (a copy on the host)
                stage = torch.empty(aux_at + aux.nbytes, dtype=torch.uint8, pin_memory=True)
                stage[:pcm_bytes].view(raw.packed.dtype).copy_(raw.packed)
            stage[aux_at: aux_at + aux.nbytes].view(torch.int64).copy_(torch.from_numpy(aux))
            with torch.cuda.stream(cs):
                buf = torch.empty(aux_at + aux.nbytes, dtype=torch.uint8, device=device)
                buf.copy_(stage[: aux_at + aux.nbytes], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
            buf.record_stream(main)
            src, aux_d = buf[:pcm_bytes].view(raw.packed.dtype), buf[aux_at:].view(torch.int64)
    main.wait_event(ev)
    aux_d.record_stream(main)
    desc = aux_d[: DESC_WORDS * B].view(B, DESC_WORDS)
    wav = torch.empty(B, Lmax, dtype=torch.float32, device=device) if out is None else out
    at = 0
    for r, bs in groups.items():
        P, Q, taps = resample_geometry(r)
        table, first = resample_table(r, device) if (P, Q) != (1, 1) else (None, None)
        ops.audio_resample(src, desc[at: at + len(bs)], table, first, P, Q, taps, tile_outputs(r), wav)
        at += len(bs)
    return wav, attach_host_lengths(aux_d[DESC_WORDS * B:], n_out)


def prep_audio(wavs, sample_rate, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """a list of utterances (``as_entries``) at ``sample_rate`` (one int, or one per item) -> (wav [B, Lmax] fp32, 16 kHz mono,
    zero-padded; wav_len [B] int64 carrying its host twin) on ``device`` - what ``encode_speech`` and the encoder take."""
    if isinstance(wavs, RawAudioBatch):
        return run(wavs, device)
    return run(pack(as_entries(wavs, sample_rate), pin_memory=torch.device(device).type == "cuda"), device)
