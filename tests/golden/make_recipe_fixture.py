"""Generates tests/golden/recipes.json: for every yaml recipe under the reference's config/, the values that load_config gives the
keys the built-in configs hold (speechclip_plus_amd.config: base / large parallel, cascaded+ base, hybrid+ large), with the
reduced-vocabulary table of a recipe recorded as its path (as the yaml writes it) and its row count.  tests/test_host_cpu.py checks
the built-in configs and load_config against these values, so the reference checkout is needed only to regenerate the file:

    python tests/golden/make_recipe_fixture.py <reference checkout>
"""
import glob
import json
import os
import sys

import numpy as np
import yaml

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from speechclip_plus_amd import (base_parallel_config, cascaded_plus_base_config, hybrid_plus_large_config,  # noqa: E402
                                 large_parallel_config, load_config)

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
    keys = set()
    for builtin in (base_parallel_config(), large_parallel_config(), cascaded_plus_base_config(), hybrid_plus_large_config()):
        keys |= set(flat(builtin))
    cfg_root = os.path.join(ref, "config")
    out = {}
    for path in sorted(glob.glob(os.path.join(cfg_root, "**", "*.yaml"), recursive=True)):
        fy = flat(load_config(path, reference_root=ref))              # the table as the reference ships it: must exist
        rec = {k: v for k, v in fy.items() if k in keys and k != VOCAB_KEY}
        if isinstance(fy.get(VOCAB_KEY), str):
            rec[VOCAB_KEY] = {"path": yaml.safe_load(open(path))["clip"]["reduce_subword_embbedding"], "rows": int(len(np.load(fy[VOCAB_KEY])))}
        out[os.path.relpath(path, cfg_root)] = rec
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "recipes.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{dst}: {len(out)} recipes")


if __name__ == "__main__":
    main(sys.argv[1])
