"""Generates tests/golden/recipes_cascaded.json: for the three config/speechCLIP/**/spchclp_c.yaml recipes of the reference (the
original SpeechCLIP cascaded model), the values load_config gives the keys the built-in cascaded_base_config / cascaded_large_config
hold - ``keyword.number`` among them, which tests/golden/recipes.json does not store.  The reduced-vocabulary table is recorded as its
path (as the yaml writes it) and its row count.  Settings only.  tests/test_cascaded_cpu.py checks the built-ins against these values,
so the reference checkout is needed only to regenerate the file:

    python tests/golden/make_recipe_cascaded_fixture.py <reference checkout>
"""
import glob
import json
import os
import sys

import numpy as np
import yaml

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from speechclip_plus_amd import cascaded_base_config, cascaded_large_config, load_config  # noqa: E402

VOCAB_KEY = "clip.reduce_subword_embbedding"


def flat(c, pre=""):
    out = {}
    for k, v in c.items():
        if hasattr(v, "items"):
            out.update(flat(v, pre + k + "."))
        else:
            out[pre + k] = v
    return out


def main(ref: str) -> None:
    keys = set(flat(cascaded_base_config())) | set(flat(cascaded_large_config()))
    cfg_root = os.path.join(ref, "config")
    out = {}
    for path in sorted(glob.glob(os.path.join(cfg_root, "speechCLIP", "**", "spchclp_c.yaml"), recursive=True)):
        fy = flat(load_config(path, reference_root=ref))              # the table as the reference ships it: must exist
        rec = {k: v for k, v in fy.items() if k in keys and k != VOCAB_KEY}
        rec[VOCAB_KEY] = {"path": yaml.safe_load(open(path))["clip"]["reduce_subword_embbedding"], "rows": int(len(np.load(fy[VOCAB_KEY])))}
        out[os.path.relpath(path, cfg_root)] = rec
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recipes_cascaded.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{dst}: {len(out)} recipes")


if __name__ == "__main__":
    main(sys.argv[1])
