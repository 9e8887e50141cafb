"""Writes tests/golden/image_prep.json: what Pillow + torch make of CLIP's preprocessing (bicubic Resize(224) of the shorter side,
CenterCrop(224), ToTensor, Normalize) on the cases of tests/image_prep_cases.py.  Per case: the source size and kind, the resize / crop
geometry, the sha256 of Pillow's resized-and-cropped uint8 [224, 224, 3] and of the normalised fp32 [3, 224, 224] tensor's bytes
(digests, not images: noise does not compress).  The geometry is the rule of torchvision's Resize(int) / CenterCrop restated
(speechclip_plus_amd/image_prep.clip_resize_geometry): torchvision itself is not needed and was not run.

    python tests/golden/make_golden_image_prep.py
"""
import json
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from image_prep_cases import CASES, make_source, sha256  # noqa: E402
from speechclip_plus_amd.clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD  # noqa: E402
from speechclip_plus_amd.image_prep import clip_resize_geometry  # noqa: E402


def main():
    cases = []
    for i, (w, h, kind) in enumerate(CASES):
        src = make_source(w, h, kind, seed=i)
        out_w, out_h, left, top = clip_resize_geometry(w, h)
        img = Image.fromarray(src, "RGB")
        if (out_w, out_h) != (w, h):                         # torchvision's resize returns the image itself at equal size
            img = img.resize((out_w, out_h), Image.BICUBIC)
        u8 = np.array(img)[top: top + 224, left: left + 224].copy()
        assert u8.shape == (224, 224, 3)
        t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255)           # ToTensor
        mean, std = torch.tensor(CLIP_IMAGE_MEAN).view(3, 1, 1), torch.tensor(CLIP_IMAGE_STD).view(3, 1, 1)
        t = t.sub(mean).div(std)                                                          # Normalize
        cases.append({"w": w, "h": h, "kind": kind, "seed": i, "geometry": [out_w, out_h, left, top], "source_sha256": sha256(src),
                      "u8_sha256": sha256(u8), "f32_sha256": sha256(t.numpy())})
    out = {"pillow": PIL.__version__, "torch": torch.__version__.split("+")[0], "n_px": 224, "cases": cases}
    with open(os.path.join(HERE, "image_prep.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote image_prep.json:", len(cases), "cases, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
