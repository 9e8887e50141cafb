"""Shared by the raw-image tests and tests/golden/make_golden_image_prep.py: the source sizes and the integer hash that makes the source
pixels.  No library RNG: the digests in tests/golden/image_prep.json hold under any numpy."""
import hashlib
import json
import os

import numpy as np

KINDS = ("noise", "smooth", "blocks")
# (W, H): landscape, portrait, out 336 / crop 56, crop 37.5 -> 38, crop 36.5 -> 36 (upscale), no pass, crop only, 225 x 224, upscale with
# 4-5 taps, extreme aspect, 1023 x 767, ksize 63
SIZES = [(500, 375), (375, 500), (500, 333), (275, 206), (61, 46), (224, 224), (224, 300), (225, 224), (100, 80), (31, 977), (1023, 767),
         (3000, 2001)]
CASES = [(w, h, KINDS[i % 3]) for i, (w, h) in enumerate(SIZES)]


def hash32(x: np.ndarray) -> np.ndarray:
    """lowbias32 on uint32 arrays (wrap-around arithmetic)"""
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def make_source(w: int, h: int, kind: str, seed: int = 0) -> np.ndarray:
    """uint8 [h, w, 3].  noise: a hash of the element index; smooth: integer ramps and a slow triangle wave; blocks: 0 / 255 squares of 8
    pixels per channel (bicubic overshoots at their edges, so both passes clip)"""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), np.arange(3, dtype=np.int64), indexing="ij")
    if kind == "noise":
        v = hash32(((y * w + x) * 3 + c + 0x9E3779B1 * (seed + 1)) & 0xFFFFFFFF) & np.uint32(255)
    elif kind == "smooth":
        tri = np.abs(((x * 3 + y * 5 + c * 37 + seed) % 256) - 128)
        v = ((x * 255) // max(w - 1, 1) + (y * 255) // max(h - 1, 1) + tri) // 3 + c * 20
        v = np.clip(v, 0, 255)
    elif kind == "blocks":
        v = (hash32((((y // 8) * 4099 + (x // 8)) * 3 + c + 0x85EBCA6B * (seed + 1)) & 0xFFFFFFFF) & np.uint32(1)) * np.uint32(255)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(v.astype(np.uint8))


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_fixture() -> dict:
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.json")) as f:
        return json.load(f)


_SOURCES = {}
_REFS = {}


def source(i: int) -> np.ndarray:
    """case i's source pixels (made once per process, shared, read-only)"""
    if i not in _SOURCES:
        w, h, kind = CASES[i]
        a = make_source(w, h, kind, seed=i)
        a.setflags(write=False)
        _SOURCES[i] = a
    return _SOURCES[i]


def reference(i: int):
    """image_prep.reference_transform of case i (computed once per process, shared, read-only)"""
    if i not in _REFS:
        from speechclip_plus_amd.image_prep import reference_transform
        u8, f32 = reference_transform(source(i))
        u8.setflags(write=False)
        f32.setflags(write=False)
        _REFS[i] = (u8, f32)
    return _REFS[i]
