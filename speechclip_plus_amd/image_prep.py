"""Raw-image input of the frozen CLIP image tower: CLIP's preprocessing - bicubic ``Resize(224)`` of a PIL image, ``CenterCrop(224)``,
``ToTensor``, ``Normalize`` (avssl/module/clip_official.py:153-166 ``prep_image``; the data sets' ``clip_image_transform``,
avssl/data/base_dataset.py:93-106) - as host geometry / coefficient tables plus two HIP kernels (csrc/image_prep.hip).

Pillow's 8-bit resampling is integer arithmetic (22-bit fixed-point coefficients, a horizontal pass, a ``uint8`` intermediate image,
a vertical pass), so the device result is held to EQUALITY with Pillow's, not to a tolerance.  This module is the host half:

  clip_resize_geometry    the resize / crop rule (torchvision's ``Resize(int)`` and ``CenterCrop``)
  pil_bicubic_coeffs      Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` in float64
  norm_lut                what ``ToTensor`` + ``Normalize`` give for each of the 256 byte values, per channel
  reference_transform     the numpy twin of the kernels (tests and documentation of the contract only: NOT a fallback)
  as_entries / plan       validation of a list of images and the per-batch descriptor / coefficient tables the kernels read
  run                     upload (one pinned copy on the "h2d" stream) + the two launches; no device synchronisation

Everything above ``run`` is pure numpy / torch-CPU and imports without a GPU.
"""
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD

N_PX = 224
PRECISION_BITS = 22                # Pillow's 8-bit fixed point: coefficients are round(w * 2^22)
MAX_KSIZE = 65                     # taps per output on either axis: the shorter side is at most 16 x 224 pixels
MAX_SHORT_SIDE = 16 * N_PX
DESC_WORDS = 8                     # int64 per image (include/speechclip_hip.h, "Raw-image input")
_COEFF_CACHE = {}
_WINDOW_CACHE = {}
_PLAN_CACHE = {}
_LUT = None


# --------------------------------------------------------------------------------------------------------- geometry and tables
def clip_resize_geometry(w: int, h: int, n_px: int = N_PX) -> Tuple[int, int, int, int]:
    """(out_w, out_h, crop_left, crop_top) of ``Resize(n_px)`` + ``CenterCrop(n_px)`` on a w x h image.

    Resize: the shorter side becomes n_px, the longer ``int(n_px * long / short)``.  Crop: ``int(round((out - n_px) / 2.0))`` with
    Python's ``round`` (halves go to even).  Both rules are restated from torchvision's published code
    (``transforms.functional.resize`` / ``center_crop``); neither torchvision nor the ``clip`` package was available to execute
    them against when this was written, so the fixture under tests/golden pins the rule as restated, not torchvision's output."""
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"image size {w} x {h}: both sides must be >= 1")
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = n_px, int(n_px * long / short)
    out_w, out_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return out_w, out_h, int(round((out_w - n_px) / 2.0)), int(round((out_h - n_px) / 2.0))


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_coeffs(in_size: int, out_size: int):
    """-> (bounds [out, 2] int32: first tap, tap count; coef [out, ksize] int32: 22-bit fixed point, zero behind the count).
    Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter (a = -0.5), in float64, the taps summed one
    after the other as the C loop does.  Cached per (in_size, out_size): a data set has a handful of sizes."""
    key = (int(in_size), int(out_size))
    hit = _COEFF_CACHE.get(key)
    if hit is not None:
        return hit
    in_size, out_size = key
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [_bicubic((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, n)
        for x, v in enumerate(w):
            coef[xx, x] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
    bounds.setflags(write=False)
    coef.setflags(write=False)
    _COEFF_CACHE[key] = (bounds, coef)
    return bounds, coef


def _window(in_size: int, out_size: int, first: int, n_px: int = N_PX):
    """the table of outputs first .. first + n_px - 1 of the (in_size -> out_size) pass; ``in_size == out_size`` (Pillow skips the
    pass) is the one-tap identity, coefficient 2^22: (2^21 + p 2^22) >> 22 = p"""
    key = (in_size, out_size, first, n_px)
    hit = _WINDOW_CACHE.get(key)
    if hit is None:
        if in_size == out_size:
            bounds = np.stack([np.arange(first, first + n_px), np.ones(n_px, dtype=np.int64)], axis=1).astype(np.int32)
            coef = np.full((n_px, 1), 1 << PRECISION_BITS, dtype=np.int32)
        else:
            b, c = pil_bicubic_coeffs(in_size, out_size)
            bounds, coef = b[first: first + n_px].copy(), c[first: first + n_px].copy()
        hit = _WINDOW_CACHE[key] = (bounds, coef)
    return hit


def norm_lut() -> torch.Tensor:
    """[3, 256] fp32: ``ToTensor`` + ``Normalize(CLIP_IMAGE_MEAN, CLIP_IMAGE_STD)`` of every byte value, made with torch on the CPU;
    the kernel looks values up in it, so the result does not depend on the device's division"""
    global _LUT
    if _LUT is None:
        v = torch.arange(256, dtype=torch.uint8).float().div(255)
        _LUT = torch.stack([v.sub(CLIP_IMAGE_MEAN[c]).div(CLIP_IMAGE_STD[c]) for c in range(3)]).contiguous()
    return _LUT


def _clip8(acc: np.ndarray) -> np.ndarray:
    return np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _resample_axis0(img: np.ndarray, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """one pass along axis 0 of img [n_in, ...] uint8: int32 accumulation, arithmetic shift, clip to a byte"""
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.uint8)
    for i, (first, n) in enumerate(bounds):
        k = coef[i, :n].astype(np.int32).reshape((n,) + (1,) * (img.ndim - 1))
        out[i] = _clip8((img[first: first + n].astype(np.int32) * k).sum(axis=0, dtype=np.int32))
    return out


def reference_transform(img_u8_hwc, n_px: int = N_PX):
    """(uint8 [n_px, n_px, 3], fp32 [3, n_px, n_px]) numpy arrays: the host twin of the two kernels, in Pillow's order - the horizontal
    pass if the width changes, the uint8 intermediate, the vertical pass if the height changes, the crop, the LUT.  For tests and as
    the statement of the contract; the product path has no CPU fallback."""
    img = np.ascontiguousarray(np.asarray(img_u8_hwc))
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"reference_transform: uint8 [H, W, 3], got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    out_w, out_h, left, top = clip_resize_geometry(w, h, n_px)
    if out_w != w:
        b, c = pil_bicubic_coeffs(w, out_w)
        img = np.ascontiguousarray(_resample_axis0(img.transpose(1, 0, 2), b, c).transpose(1, 0, 2))
    if out_h != h:
        b, c = pil_bicubic_coeffs(h, out_h)
        img = _resample_axis0(img, b, c)
    u8 = np.ascontiguousarray(img[top: top + n_px, left: left + n_px])
    lut = norm_lut().numpy()
    f32 = np.stack([lut[c][u8[:, :, c]] for c in range(3)]).astype(np.float32)
    return u8, f32


# --------------------------------------------------------------------------------------------------------- inputs
def attach_host_sizes(image_hw: torch.Tensor, host: Optional[Sequence] = None) -> torch.Tensor:
    """``image_hw`` [B, 2] with its host twin attached (``_sc_host``: a list of (h, w)), as data.attach_host_lengths does for wav_len:
    the tables are host decisions, and reading a device tensor back would synchronise every step"""
    if host is None:
        if image_hw.is_cuda:
            raise ValueError("attach_host_sizes: a device tensor needs the host values passed in (reading it back would synchronise)")
        host = image_hw.tolist()
    image_hw._sc_host = [(int(h), int(w)) for h, w in host]
    return image_hw


class RawImageBatch:
    """B images of unequal sizes as one packed ``uint8`` buffer: image b is ``packed[offset[b] : offset[b] + 3 h_b w_b]`` read as
    [h_b, w_b, 3] (RGB, interleaved).  ``hw``: the sizes as HOST data - a list of (h, w), or an int64 [B, 2] tensor that lives on
    the host or carries a host twin (``attach_host_sizes``).  ``offsets`` default to back-to-back."""

    def __init__(self, packed: torch.Tensor, hw, offsets: Optional[Sequence[int]] = None):
        if isinstance(hw, torch.Tensor):
            host = getattr(hw, "_sc_host", None)
            if host is None:
                if hw.is_cuda:
                    raise ValueError("image_hw on the device needs its host twin (data.transfer_batch_to_device keeps it; "
                                     "image_prep.attach_host_sizes attaches one): reading it back would synchronise")
                if hw.dim() != 2 or hw.shape[1] != 2:
                    raise ValueError(f"image_hw must be [B, 2] (height, width), got {tuple(hw.shape)}")
                host = hw.tolist()
            hw = host
        self.hw = [(int(h), int(w)) for h, w in hw]
        if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 1:
            raise ValueError("packed raw images must be a 1-D uint8 tensor, got "
                             f"{getattr(packed, 'dtype', type(packed))} {tuple(getattr(packed, 'shape', ()))}")
        if len(self.hw) < 1:
            raise ValueError("empty image batch")
        sizes = [3 * h * w for h, w in self.hw]
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        self.offsets = [int(o) for o in offsets]
        if len(self.offsets) != len(self.hw):
            raise ValueError(f"{len(self.offsets)} offsets for {len(self.hw)} images")
        for (h, w), o, n in zip(self.hw, self.offsets, sizes):
            check_size(w, h)
            if o < 0 or o + n > packed.numel():
                raise ValueError(f"image of {h} x {w} x 3 bytes at offset {o} does not fit the packed buffer of {packed.numel()} bytes")
        self.packed = packed

    def __len__(self):
        return len(self.hw)


def check_size(w: int, h: int, n_px: int = N_PX) -> None:
    """the size limits of one image, named: H, W >= 1 and at most MAX_KSIZE taps per output on both axes"""
    if h < 1 or w < 1:
        raise ValueError(f"image of height {h}, width {w}: H, W >= 1")
    out_w, out_h, _, _ = clip_resize_geometry(w, h, n_px)
    for n_in, n_out, axis in ((w, out_w, "width"), (h, out_h, "height")):
        ksize = int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
        if ksize > MAX_KSIZE:
            raise ValueError(f"image {w} x {h}: the {axis} pass needs ksize = {ksize} taps, the limit is ksize <= {MAX_KSIZE} "
                             f"(a downscale of at most 16: the shorter side at most {MAX_SHORT_SIDE} = 16 x {n_px} pixels)")


def _as_hwc_u8(img) -> torch.Tensor:
    """one list entry -> uint8 [H, W, 3] torch tensor (host or device), validated"""
    if isinstance(img, (str, os.PathLike)):
        try:
            from PIL import Image
        except ImportError as e:
            raise ValueError(f"image path {img!r}: opening files needs PIL, which does not import ({e})") from None
        with Image.open(img) as f:
            img = f.convert("RGB")
    if not isinstance(img, (torch.Tensor, np.ndarray)) and hasattr(img, "convert") and hasattr(img, "mode"):        # a PIL image
        if img.mode != "RGB":
            img = img.convert("RGB")                       # base_dataset.py:104
        img = np.array(img)
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise ValueError(f"raw images are uint8 [H, W, 3], got dtype {img.dtype}")
        img = torch.from_numpy(img if img.flags.writeable and img.flags.c_contiguous else np.array(img))
    if not isinstance(img, torch.Tensor):
        raise ValueError(f"raw image entries are uint8 [H, W, 3] tensors, numpy arrays, PIL images or paths, got {type(img)}")
    if img.dtype != torch.uint8:
        raise ValueError(f"raw images are uint8 [H, W, 3], got dtype {img.dtype}")
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"raw images are uint8 [H, W, 3] (three interleaved channels), got shape {tuple(img.shape)}")
    check_size(int(img.shape[1]), int(img.shape[0]))
    return img


def as_entries(images) -> List[torch.Tensor]:
    """a list of raw images -> validated uint8 [H, W, 3] tensors; every rule is enforced here, before any launch"""
    if not isinstance(images, (list, tuple)):
        raise ValueError(f"raw images come as a list, got {type(images)}")
    if len(images) == 0:
        raise ValueError("empty image batch: a non-empty list of images")
    return [_as_hwc_u8(img) for img in images]


def pack_host(entries: Sequence[torch.Tensor]) -> RawImageBatch:
    """host uint8 [H, W, 3] tensors -> RawImageBatch on the host (data.collate_general)"""
    hw = [(int(t.shape[0]), int(t.shape[1])) for t in entries]
    return RawImageBatch(torch.cat([t.reshape(-1) for t in entries]), hw)


# --------------------------------------------------------------------------------------------------------- per-batch tables
class _SizeEntry:
    """what one (w, h) contributes to a Plan - both windows, the intermediate's row range - checked once and cached per size"""

    def __init__(self, w: int, h: int, n_px: int):
        out_w, out_h, left, top = clip_resize_geometry(w, h, n_px)
        hb, hc = _window(w, out_w, left, n_px)
        vb, vc = _window(h, out_h, top, n_px)
        row0 = int(vb[:, 0].min())
        rows = int((vb[:, 0] + vb[:, 1]).max()) - row0
        # the bounds the kernels rely on: every tap of every output lies inside the source / the intermediate
        assert hb[:, 0].min() >= 0 and (hb[:, 0] + hb[:, 1]).max() <= w and hb[:, 1].min() >= 1 and hb[:, 1].max() <= hc.shape[1]
        assert row0 >= 0 and row0 + rows <= h and vb[:, 1].min() >= 1 and vb[:, 1].max() <= vc.shape[1]
        assert hc.shape[1] <= MAX_KSIZE and vc.shape[1] <= MAX_KSIZE
        vrel = vb.copy()
        vrel[:, 0] -= row0
        self.hkey, self.vkey = ("h", w, out_w, left), ("v", h, out_h, top)
        self.hb, self.hc, self.vrel, self.vc = hb.reshape(-1), hc.reshape(-1), vrel.reshape(-1), vc.reshape(-1)
        self.row0, self.rows, self.ksize = row0, rows, hc.shape[1] | (vc.shape[1] << 32)


_SIZE_CACHE = {}


def _size_entry(w: int, h: int, n_px: int) -> _SizeEntry:
    key = (w, h, n_px)
    e = _SIZE_CACHE.get(key)
    if e is None:
        e = _SIZE_CACHE[key] = _SizeEntry(w, h, n_px)
    return e


class Plan:
    """what the kernels read for one batch of sizes: ``tab`` int32 = [descriptors: B x 8 int64 | coefficient tables], the
    intermediate image's byte count and the largest row count.  Descriptor of image b (int64): source byte offset, source width,
    intermediate byte offset, intermediate rows, first source row of the intermediate, horizontal table offset, vertical table
    offset (int32 units into ``tab``), ksize_h | ksize_v << 32.  A table = bounds [n_px][2] then coef [n_px][ksize]."""

    def __init__(self, hw: Sequence[Tuple[int, int]], offsets: Sequence[int], n_px: int = N_PX):
        B = len(hw)
        desc = []
        parts, where, cursor = [], {}, 2 * DESC_WORDS * B          # int32 units

        def table(key, bounds, coef):
            nonlocal cursor
            if key not in where:
                where[key] = cursor
                parts.extend([bounds, coef])
                cursor += bounds.size + coef.size
            return where[key]

        mid_off, self.max_rows, self.src_end = 0, 0, 0
        for b, ((h, w), off) in enumerate(zip(hw, offsets)):
            e = _size_entry(w, h, n_px)
            desc.append((off, w, mid_off, e.rows, e.row0, table(e.hkey, e.hb, e.hc), table(e.vkey, e.vrel, e.vc), e.ksize))
            mid_off += e.rows * n_px * 3
            self.max_rows = max(self.max_rows, e.rows)
            self.src_end = max(self.src_end, off + 3 * h * w)
        self.B, self.n_px, self.mid_bytes = B, n_px, mid_off
        self.tab = torch.from_numpy(np.concatenate([np.array(desc, dtype=np.int64).view(np.int32).reshape(-1)] + parts))
        self._pinned = None

    def pinned(self) -> torch.Tensor:
        """``tab`` in pinned memory (made once: the table is read-only, so every upload of this plan reads the same host buffer)"""
        if self._pinned is None:
            self._pinned = self.tab.pin_memory()
        return self._pinned


def plan_ints(hw: Sequence[Tuple[int, int]], n_px: int = N_PX) -> int:
    """int32 count of the Plan's ``tab`` for these sizes (it does not depend on the offsets)"""
    seen, n = set(), 2 * DESC_WORDS * len(hw)
    for h, w in hw:
        e = _size_entry(w, h, n_px)
        for key, size in ((e.hkey, e.hb.size + e.hc.size), (e.vkey, e.vrel.size + e.vc.size)):
            if key not in seen:
                seen.add(key)
                n += size
    return n


def plan(hw: Sequence[Tuple[int, int]], offsets: Sequence[int], n_px: int = N_PX) -> Plan:
    """the batch's Plan, cached per (sizes, offsets): a loader repeats a handful of size combinations only by chance, but the
    per-size windows underneath are cached as well, so a new combination costs the concatenation alone"""
    key = (tuple(hw), tuple(offsets), n_px)
    p = _PLAN_CACHE.get(key)
    if p is None:
        if len(_PLAN_CACHE) >= 256:
            _PLAN_CACHE.clear()
        p = _PLAN_CACHE[key] = Plan(hw, offsets, n_px)
    return p


# --------------------------------------------------------------------------------------------------------- device
def run(images, device, pixels: bool = True, seg=None, patch: int = 0, Kp: int = 0,
        out: Optional[torch.Tensor] = None, A: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None):
    """Resize + crop + normalise ``images`` (a list of raw images, or a RawImageBatch) on ``device`` -> (pixels, A):
    pixels fp32 [B, 3, 224, 224] if ``pixels``, and A [seg.rows, Kp] bf16 - the patch GEMM's operand, as ops.vit_patchify of those
    pixels gives it - if ``seg`` is given.  Host images and the tables travel in ONE pinned copy on the "h2d" stream; the current
    stream waits for its event.  No device synchronisation.  ``out`` / ``A`` / ``mid``: caller's buffers (tests)."""
    from . import ops
    device = torch.device(device)
    if isinstance(images, RawImageBatch):
        raw, entries = images, None
    else:
        raw, entries = None, as_entries(images)
    if device.type != "cuda":
        raise RuntimeError("the CLIP image preprocessing runs on the HIP kernels: there is no CPU path (image_prep.reference_transform "
                           "is the test twin)")
    main = torch.cuda.current_stream(device)
    cs = ops.shared_stream("h2d", device, priority=-1)
    if raw is not None and (raw.packed.is_cuda or raw.packed.is_pinned()):
        # the packed bytes are on the device already (data.transfer_batch_to_device) or pinned: no staging copy on the host
        pl = plan(raw.hw, raw.offsets)
        with torch.cuda.stream(cs):                  # allocated on the copy stream's pool: nothing queued elsewhere still reads the block
            tab = pl.pinned().to(device, non_blocking=True)
            src = raw.packed if raw.packed.is_cuda else raw.packed.to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        if src is not raw.packed:
            src.record_stream(main)
        elif src.device != device:
            src = src.to(device, non_blocking=True)
    else:
        # one buffer [host images | tables | device images]: the first two parts are one pinned copy, device entries are copied behind
        if raw is not None:
            hw, dev_parts = raw.hw, []
            host_parts = [(i, raw.packed[o: o + 3 * h * w]) for i, ((h, w), o) in enumerate(zip(raw.hw, raw.offsets))]
        else:
            hw = [(int(t.shape[0]), int(t.shape[1])) for t in entries]
            host_parts = [(i, t) for i, t in enumerate(entries) if not t.is_cuda]
            dev_parts = [(i, t) for i, t in enumerate(entries) if t.is_cuda]
        offsets, cursor = [0] * len(hw), 0
        for i, t in host_parts:
            offsets[i] = cursor
            cursor += t.numel()
        tab_at = (cursor + 15) // 16 * 16
        n_tab = plan_ints(hw)
        cursor = host_end = tab_at + (4 * n_tab + 15) // 16 * 16
        for i, t in dev_parts:
            offsets[i] = cursor
            cursor += t.numel()
        pl = plan(hw, offsets)
        assert pl.tab.numel() == n_tab
        stage = torch.empty(host_end, dtype=torch.uint8, pin_memory=True)
        for i, t in host_parts:
            stage[offsets[i]: offsets[i] + t.numel()].copy_(t.reshape(-1))
        stage[tab_at: tab_at + 4 * n_tab].view(torch.int32).copy_(pl.tab)
        with torch.cuda.stream(cs):                  # allocated on the copy stream's pool: nothing queued elsewhere still reads the block
            buf = torch.empty(cursor, dtype=torch.uint8, device=device)
            buf[:host_end].copy_(stage, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        buf.record_stream(main)
        for i, t in dev_parts:
            buf[offsets[i]: offsets[i] + t.numel()].copy_(t.reshape(-1), non_blocking=True)
        tab, src = buf[tab_at: tab_at + 4 * n_tab].view(torch.int32), buf
    main.wait_event(ev)
    tab.record_stream(main)
    lut = _device_lut(device)
    if mid is None:
        mid = torch.empty(pl.mid_bytes, dtype=torch.uint8, device=device)
    ops.image_resample_h(src, tab, mid, pl)
    if pixels and out is None:
        out = torch.empty(pl.B, 3, pl.n_px, pl.n_px, dtype=torch.float32, device=device)
    if seg is not None and A is None:
        A = torch.empty(seg.rows, Kp, dtype=torch.bfloat16, device=device)
    ops.image_resample_v_norm(mid, tab, lut, pl, out if pixels else None, A if seg is not None else None, seg, patch, Kp)
    return (out if pixels else None), (A if seg is not None else None)


_DEV_LUT = {}


def _device_lut(device) -> torch.Tensor:
    key = str(device)
    if key not in _DEV_LUT:
        _DEV_LUT[key] = norm_lut().to(device)
    return _DEV_LUT[key]
