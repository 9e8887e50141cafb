#!/usr/bin/env python3
"""Writes tests/golden/split_weights_small.npz: per small case the distances d(emulation, all sites + w_split) and d(emulation, all
sites + bf16 weights) from the fp32 oracle (tests/split_cases.py).  CPU only, this repository's oracle only; about a minute."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
import split_cases  # noqa: E402

if __name__ == "__main__":
    out = {}
    for case in split_cases.CASES:
        d_split, d_bf16 = split_cases.rehearse(case)
        print(f"{case}: d(split emulation) {d_split:.6g}  d(bf16 emulation) {d_bf16:.6g}  ratio {d_bf16 / d_split:.3f}")
        out[case] = np.asarray([d_split, d_bf16], dtype=np.float64)
    np.savez(split_cases.FIXTURE, **out)
    print("wrote", split_cases.FIXTURE)
