#!/usr/bin/env python3
"""Generate tests/golden/kw_neighbors.npz: the reference's keyword detokenisation on small seeded inputs.

Needs the reference checkout (it does not travel with the package).  Like make_golden.py it imports the reference's LEAF file
avssl/util/model_utils.py by path and runs both of its functions - extract_fixed_keyword_neighbors and
extract_dynamic_keyword_neighbors - on the CPU with a stub model object, for both retrieve methods.  The fixture stores inputs and
outputs only (a few hundred KB): the token table, the keyword embeddings, and per utterance the neighbour ids, the decoded tokens
and the scores as they came out of the reference.  No reference text is copied.

    python tests/golden/make_golden_kwneighbors.py [path of the reference checkout]

Shapes: V = 300 reduced sub-words of a 1000-token vocabulary, E = 32, K = 5.
  fixed    7 utterances x 4 keywords, dev_batch_size 3 (the last batch holds one utterance)
  dynamic  batches of 3, 3 and 1 utterances with up to 5 keywords, counts between 0 and the batch's maximum

The stub's tokenizer decodes an original token id to itself, so the "token" of an entry is the ORIGINAL id of the neighbour:
the reduced -> original mapping is part of what the fixture pins.  The table goes in as float64 holding float32 values: the
reference then takes the pseudo-inverse in float64 (torch.linalg.pinv follows its input) and the cosine in float64, which is the
accuracy the 1e-6 score tolerance of the tests is meant against.  ``fixed_gold`` records the caption label the reference attached
to every entry: entry i + x gets gold_texts[x] (model_utils.py:122), the reference bug docs/parity.md lists.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
V, VOCAB, E, K, NKW, BS = 300, 1000, 32, 5, 4, 3


def load_leaf(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Identity:
    def __getitem__(self, i):
        return int(i)


def stub_model(reduced_ids, keyword_num):
    clip = _NS(tokenizer=_NS(decoder=_Identity()), selected_text_emb_ids=reduced_ids,
               reducedl2Original={n: int(o) for n, o in enumerate(reduced_ids.tolist())})
    return _NS(config=_NS(data=_NS(dev_batch_size=BS)), clip=clip, subword_embd_dim=E, keyword_num=keyword_num)


def unpack(entries, n_max):
    """list of {"gold", "neighbors"} -> tokens [U, n_max, K] int64 (-1 = no such keyword), scores [U, n_max, K] float64, counts, gold"""
    U = len(entries)
    tok = np.full((U, n_max, K), -1, dtype=np.int64)
    sc = np.full((U, n_max, K), -np.inf, dtype=np.float64)
    cnt = np.zeros(U, dtype=np.int64)
    for u, e in enumerate(entries):
        cnt[u] = len(e["neighbors"])
        for i in range(cnt[u]):
            for r, (t, s) in enumerate(e["neighbors"][f"keyword_{i}"]):
                tok[u, i, r], sc[u, i, r] = t, s
    return tok, sc, cnt, np.array([e["gold"] for e in entries], dtype=np.int64)


def main():
    mu = load_leaf("avssl/util/model_utils.py", "ref_model_utils")
    g = torch.Generator().manual_seed(20260)
    table = 0.01 * torch.randn(V, E, generator=g)
    reduced_ids = torch.randperm(VOCAB, generator=g)[:V]
    table64 = table.double()

    def keywords(n):
        """half table rows (what the hard quantiser emits), half free Gaussian embeddings of the table's scale"""
        rows = table[torch.randint(0, V, (n,), generator=g)].clone()
        free = 0.01 * torch.randn(n, E, generator=g)
        pick = torch.rand(n, generator=g) < 0.5
        return torch.where(pick.unsqueeze(1), rows, free)

    out = {"table": table.numpy(), "reduced_ids": reduced_ids.numpy(), "K": np.int64(K), "dev_batch_size": np.int64(BS)}
    # ---- fixed
    U = 7
    kw_fixed = keywords(U * NKW).view(U, NKW, E)
    gold = list(range(100, 100 + U))                      # "captions": an integer label per utterance
    out["fixed_keywords"] = kw_fixed.numpy()
    out["fixed_gold_in"] = np.array(gold)
    # ---- dynamic: batches of 3, 3, 1 utterances
    sizes, counts = [3, 3, 1], [[2, 5, 0], [1, 3, 3], [4]]
    kw_dyn, flat_counts = [], []
    for b, (n, c) in enumerate(zip(sizes, counts)):
        kw_dyn.append([keywords(n * max(c)).view(n, max(c), E)])
        flat_counts += c
        out[f"dyn_keywords_{b}"] = kw_dyn[-1][0].numpy()
    gold_dyn = list(range(200, 200 + sum(sizes)))
    out["dyn_counts"] = np.array(flat_counts)
    out["dyn_gold_in"] = np.array(gold_dyn)
    for method in ("cosine", "pseudo_inverse"):
        res = mu.extract_fixed_keyword_neighbors(stub_model(reduced_ids, NKW), K, method, table64, kw_fixed, gold)
        tok, sc, cnt, gl = unpack(res, NKW)
        assert (cnt == NKW).all() and len(res) == U
        out[f"fixed_{method}_tokens"], out[f"fixed_{method}_scores"], out[f"fixed_{method}_gold"] = tok, sc, gl
        res = mu.extract_dynamic_keyword_neighbors(stub_model(reduced_ids, None), K, method, [None] * len(sizes), table64, kw_dyn,
                                                   gold_dyn, flat_counts)
        tok, sc, cnt, gl = unpack(res, max(flat_counts))
        assert cnt.tolist() == flat_counts and gl.tolist() == gold_dyn
        out[f"dyn_{method}_tokens"], out[f"dyn_{method}_scores"] = tok, sc
        for name in (f"fixed_{method}_scores", f"dyn_{method}_scores"):
            s = out[name]
            fin = np.isfinite(s[..., 0])
            gaps = (s[fin][:, :-1] - s[fin][:, 1:]).min()
            print(f"{name}: |score| <= {np.abs(s[fin]).max():.3f}, smallest gap between listed neighbours {gaps:.2e}")
            assert gaps > 1e-5, "listed neighbours closer than 10 x the 1e-6 score tolerance: pick another seed (the id check must not hinge on rounding)"
    path = os.path.join(HERE, "kw_neighbors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
