"""GPU: ops.rank_best / ops.rank_ahead (csrc/rank.hip) alone - the accumulate contract, the ranges and the removed-row mask.

THE INVARIANT: a split-bf16 score depends only on its row of A, its row of B and the fixed K order.  So "best" over every (A range,
B range) pair followed by "ahead" over every pair gives, bit for bit, the keys and counts ``ops.rank_counts`` gives on the whole of A
against the whole of B - and with a mask, on the gallery with the dead rows physically deleted.  Every expectation is exact.

THE ORACLE.  ``rank_best`` / ``rank_ahead`` and ``rank_counts`` are three entries of ONE kernel, so holding one against another is
the code under test compared with itself.  On Gaussian data the expectation therefore comes from no rank kernel: ``_oracle`` takes
the [nA, nB] fp32 score matrix from ``ops.cosine_scores_split`` on the same rows - the GEMM, another kernel, whose bits are the
tile's (tests/test_gpu_wide_search.py: "both routes agree bit for bit") -, copies it to the CPU, cuts it to [:nA, :nB] and applies
tests/rank_cases.py's rule: exact integers for ``ahead``, the fp32 maximum as fp64 for ``best``.  Both ``_parts(...)`` and
``ops.rank_counts(...)`` are held against it with no tolerance, and against each other bit for bit.  Integer data (exact scores)
is held against the same rule on an int64 product the CPU computes.

Shapes: E = 64 and E = 100 (pads to 128); nA in {1, 127, 128, 129, 300}, nB in {1, 129, 257, 300}: one tile and several, 1-row and
1-column tails; B cut into ranges of 100 rows (tile tails inside the gallery) and 1 + 256 + 43 rows, each range split on its own."""
import functools

import pytest
import torch

import rank_cases as rk
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ES, NAS, NBS = (64, 100), (1, 127, 128, 129, 300), (1, 129, 257, 300)
RAW = ("key_a", "key_b", "ahead_a", "ahead_b")


def _ranges(n: int, sizes):
    """consecutive (start, stop) ranges of the given sizes (an int: equal ranges, the last may be short) covering [0, n)"""
    if isinstance(sizes, int):
        return [(r, min(n, r + sizes)) for r in range(0, n, sizes)]
    assert sum(sizes) == n
    out, r = [], 0
    for s in sizes:
        out.append((r, r + s))
        r += s
    return out


def _parts(A, B, a_ids, b_ids, a_ranges=None, b_ranges=None, live=None, slabs=None, init=None, best_calls=1, ahead_calls=1):
    """"best" over every (A range, B range) pair, then "ahead" over every pair; every range split on its own.  ``init``: the four
    buffers' initial contents (None: zeros).  -> the four raw int32 vectors on the CPU"""
    from speechclip_plus_amd import ops
    nA, nB = A.shape[0], B.shape[0]
    a_ranges = [(0, nA)] if a_ranges is None else a_ranges
    b_ranges = [(0, nB)] if b_ranges is None else b_ranges
    a_sp = [ops.split3_bf16(A[a0:a1].contiguous().to(DEV), 0) for a0, a1 in a_ranges]
    b_sp = [ops.split3_bf16(B[b0:b1].contiguous().to(DEV), 1) for b0, b1 in b_ranges]
    ai, bi = a_ids.to(DEV), b_ids.to(DEV)
    lv = None if live is None else live.to(DEV)
    buf = {k: torch.zeros(nA if k.endswith("_a") else nB, dtype=torch.int32) for k in RAW} if init is None else {k: v.clone() for k, v in init.items()}
    buf = {k: v.to(DEV) for k, v in buf.items()}

    def every_pair(fn, extra):
        for (a0, a1), asp in zip(a_ranges, a_sp):
            for (b0, b1), bsp in zip(b_ranges, b_sp):
                fn(asp, bsp, ai[a0:a1], bi[b0:b1], a1 - a0, b1 - b0, buf["key_a"][a0:a1], buf["key_b"][b0:b1],
                   *(buf[k][a0:a1] if k.endswith("_a") else buf[k][b0:b1] for k in extra),
                   b_live=None if lv is None else lv[b0:b1], slabs=slabs)
    for _ in range(best_calls):
        every_pair(ops.rank_best, ())
    for _ in range(ahead_calls):
        every_pair(ops.rank_ahead, ("ahead_a", "ahead_b"))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in buf.items()}


def _oracle(A, B, a_ids, b_ids):
    """the rule of tests/rank_cases.py on the fp32 scores the GEMM writes for the same rows (no rank kernel runs) -> its dict"""
    from speechclip_plus_amd import ops
    b_split = ops.split3_bf16(B.to(DEV), 1)
    scores = ops.cosine_scores_split(A.to(DEV), None, b_split, b_split.shape[0])
    torch.cuda.synchronize()
    return rk.both_directions(scores.cpu()[: A.shape[0], : B.shape[0]].double(), a_ids, b_ids)


def _whole(A, B, a_ids, b_ids, slabs=None):
    """``ops.rank_counts`` on one (A, B) pair -> (best_a fp32, ahead_a int32, best_b, ahead_b) on the CPU"""
    from speechclip_plus_amd import ops
    out = ops.rank_counts(ops.split3_bf16(A.to(DEV), 0), ops.split3_bf16(B.to(DEV), 1), a_ids.to(DEV), b_ids.to(DEV), A.shape[0], B.shape[0],
                          slabs=slabs)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def _value(key):
    from speechclip_plus_amd import ops
    return ops._rank_key_value(key)


def _same_bits(got, want, cols=None):
    """the raw vectors of ``_parts`` against ``_whole``'s tuple, bit for bit; ``cols``: the live columns ``want`` was computed on"""
    kb, ab = (got["key_b"], got["ahead_b"]) if cols is None else (got["key_b"][cols], got["ahead_b"][cols])
    return (torch.equal(_value(got["key_a"]).view(torch.int32), want[0].view(torch.int32)) and torch.equal(got["ahead_a"], want[1])
            and torch.equal(_value(kb).view(torch.int32), want[2].view(torch.int32)) and torch.equal(ab, want[3]))


def _finished(got, n_b, n_a, cols=None):
    """mutual_ranks' convention on the raw vectors of ``_parts`` (or on ``_whole``'s tuple): a query whose best is not finite never
    hits -> tests/rank_cases.py's dict"""
    if isinstance(got, tuple):
        best_a, ahead_a, best_b, ahead_b = got
    else:
        best_a, ahead_a, best_b, ahead_b = _value(got["key_a"]), got["ahead_a"], _value(got["key_b"]), got["ahead_b"]
    ahead_a = torch.where(torch.isfinite(best_a), ahead_a.long(), torch.full((), n_b, dtype=torch.int64))
    ahead_b = torch.where(torch.isfinite(best_b), ahead_b.long(), torch.full((), n_a, dtype=torch.int64))
    if cols is not None:
        ahead_b, best_b = ahead_b[cols], best_b[cols]
    return {"ahead_AB": ahead_a, "best_AB": best_a, "ahead_BA": ahead_b, "best_BA": best_b}


def _assert_equals_reference(got, ref):
    for key in ("ahead_AB", "ahead_BA"):
        bad = (got[key] != ref[key]).nonzero().flatten()[:5]
        assert torch.equal(got[key], ref[key]), (key, bad.tolist(), got[key][bad].tolist(), ref[key][bad].tolist())
    for key in ("best_AB", "best_BA"):
        assert torch.equal(got[key].double(), ref[key]), key             # exact integers (or -inf): the fp32 value IS the reference


def _assert_both_equal_the_oracle(got, want, ref, n_b, n_a, cols=None):
    """``_parts``' vectors and ``_whole``'s tuple (computed on the live columns ``cols``) each equal the oracle ``ref`` exactly, and
    each other bit for bit"""
    _assert_equals_reference(_finished(got, n_b, n_a, cols), ref)
    _assert_equals_reference(_finished(want, n_b, n_a), ref)
    assert _same_bits(got, want, cols)


@functools.lru_cache(maxsize=None)
def _gauss(nA, nB, E):
    g = torch.Generator().manual_seed(1000 * nA + 10 * nB + E)
    a_ids, b_ids = rk.caption_ids(nA, nB, seed=nA + nB)
    return torch.randn(nA, E, generator=g), torch.randn(nB, E, generator=g), a_ids, b_ids


@functools.lru_cache(maxsize=None)
def _ints(nA, nB, E):
    q, gal = sc_cases.int_case(nA, nB, E, seed=nA + nB + E)
    a_ids, b_ids = rk.caption_ids(nA, nB, seed=nA)
    return q, gal, a_ids, b_ids


# ---------------------------------------------------------------------------------------------------- 1. one pair, no mask
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("nB", NBS)
@pytest.mark.parametrize("nA", NAS)
def test_one_pair_without_a_mask_is_rank_counts_bit_for_bit(nA, nB, E):
    A, B, a_ids, b_ids = _gauss(nA, nB, E)
    want, ref = _whole(A, B, a_ids, b_ids, 1), _oracle(A, B, a_ids, b_ids)
    for S in (1, 2, 3, None, None):                                   # the default twice: a second run gives the same bits
        _assert_both_equal_the_oracle(_parts(A, B, a_ids, b_ids, slabs=S), want, ref, nB, nA)


# ---------------------------------------------------------------------------------------------------- 2. B in ranges
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("sizes", (100, (1, 256, 43)), ids=("100s", "1+256+43"))
@pytest.mark.parametrize("nA", NAS)
def test_ranges_of_b_accumulate_to_the_whole_gallery(nA, sizes, E):
    nB = 300
    A, B, a_ids, b_ids = _gauss(nA, nB, E)
    _assert_both_equal_the_oracle(_parts(A, B, a_ids, b_ids, b_ranges=_ranges(nB, sizes)), _whole(A, B, a_ids, b_ids),
                                  _oracle(A, B, a_ids, b_ids), nB, nA)
    q, gal, a_ids, b_ids = _ints(nA, nB, E)
    got = _parts(q.float(), gal.float(), a_ids, b_ids, b_ranges=_ranges(nB, sizes))
    _assert_equals_reference(_finished(got, nB, nA), rk.both_directions(q.long() @ gal.long().t(), a_ids, b_ids))


# ---------------------------------------------------------------------------------------------------- 3. A in halves
@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("nB", NBS)
@pytest.mark.parametrize("nA", (127, 129, 300))
def test_two_halves_of_a_accumulate_in_the_b_side_buffers(nA, nB, E):
    A, B, a_ids, b_ids = _gauss(nA, nB, E)
    halves = _ranges(nA, (nA // 2, nA - nA // 2))
    want, ref = _whole(A, B, a_ids, b_ids), _oracle(A, B, a_ids, b_ids)
    _assert_both_equal_the_oracle(_parts(A, B, a_ids, b_ids, a_ranges=halves), want, ref, nB, nA)
    _assert_both_equal_the_oracle(_parts(A, B, a_ids, b_ids, a_ranges=halves, b_ranges=_ranges(nB, 100)), want, ref, nB, nA)


# ---------------------------------------------------------------------------------------------------- 4. placement across ranges
@functools.lru_cache(maxsize=None)
def _placed():
    """integer data, 130 x 300 x 64, for ranges of 100 rows.  Query 0 (a row of threes, id 5000): its correct rows are 250 (a row of
    threes: score 576) and 40 (a row of ones: 192); row 10 (a row of twos: 384, another id) is its highest wrong candidate and lies
    in an EARLIER range than 250; row 150 repeats row 250 under another id - a wrong candidate in another range that ties with the
    best correct one.  Query 5's id is in no range."""
    q, gal, a_ids, b_ids = (t.clone() for t in _ints(130, 300, 64))
    a_ids[0] = 5000
    a_ids[5] = 10 ** 12
    b_ids[250], b_ids[40], b_ids[10], b_ids[150] = 5000, 5000, 6000, 6001
    q[0], gal[250], gal[40], gal[10] = 3, 3, 1, 2
    gal[150] = gal[250]
    return q, gal, a_ids, b_ids


def test_best_and_ties_in_other_ranges_and_an_absent_id():
    q, gal, a_ids, b_ids = _placed()
    score = q.long() @ gal.long().t()
    ref = rk.both_directions(score, a_ids, b_ids)
    wrong = score[0].clone()
    wrong[b_ids == 5000] = -10 ** 9
    assert score[0, 250] == 576 == score[0, 150] and int(wrong[:100].argmax()) == 10 and score[0, 10] == 384    # the scenario holds
    assert ref["best_AB"][0] == 576 and ref["ahead_AB"][0] == 1 and ref["ahead_AB"][5] == 300 and not bool((b_ids == 10 ** 12).any())
    for sizes in (100, (1, 256, 43)):
        got = _parts(q.float(), gal.float(), a_ids, b_ids, b_ranges=_ranges(300, sizes))
        _assert_equals_reference(_finished(got, 300, 130), ref)


def test_nan_inf_and_zero_rows_in_different_ranges():
    A, B, a_ids, b_ids, ref = rk.degenerate_case()                  # 130 x 140: B's NaN row 33 and inf row 129, A's rows 7, 64, 100
    got = _parts(A, B, a_ids, b_ids, a_ranges=_ranges(130, 50), b_ranges=_ranges(140, 50))
    _assert_equals_reference(_finished(got, 140, 130), ref)


# ---------------------------------------------------------------------------------------------------- 5. the mask
@functools.lru_cache(maxsize=None)
def _masked():
    """``_placed`` with a mask for ranges of 100 rows: row 250 - query 0's best correct row - is dead, so row 40 counts; both correct
    rows of query 1's id are dead; range 100 .. 199 is dead altogether; a few more rows are dead here and there.  The dead rows hold
    NaN and 1e30 in the float gallery the kernel sees.  -> (A fp32, B fp32, a_ids, b_ids, live bool, int64 scores)"""
    q, gal, a_ids, b_ids = (t.clone() for t in _placed())
    a_ids[1] = 7000
    b_ids[20], b_ids[260] = 7000, 7000
    live = torch.ones(300, dtype=torch.bool)
    live[[250, 20, 260, 0, 99, 200, 299]] = False
    live[100:200] = False
    B = gal.float()
    dead = (~live).nonzero().flatten()
    B[dead[::2]] = float("nan")
    B[dead[1::2]] = 1e30
    return q.float(), B, a_ids, b_ids, live, q.long() @ gal.long().t()


@pytest.mark.parametrize("sizes", (300, 100, (1, 256, 43)), ids=("whole", "100s", "1+256+43"))
def test_dead_rows_are_no_candidates_and_no_queries(sizes):
    A, B, a_ids, b_ids, live, score = _masked()
    n_live = int(live.sum())
    ref = rk.both_directions(score[:, live], a_ids, b_ids[live])
    assert ref["best_AB"][0] == 192 and ref["ahead_AB"][1] == n_live          # the next correct row counts; no correct row is left
    init = {k: torch.zeros(130 if k.endswith("_a") else 300, dtype=torch.int32) for k in RAW}
    init["key_b"][~live], init["ahead_b"][~live] = 0x12345678, -777             # sentinels in the dead columns' slots
    got = _parts(A, B, a_ids, b_ids, b_ranges=_ranges(300, sizes), live=live, init=init)
    assert bool((got["key_b"][~live] == 0x12345678).all()) and bool((got["ahead_b"][~live] == -777).all())
    _assert_equals_reference(_finished(got, n_live, 130, cols=live), ref)
    as_bytes = _parts(A, B, a_ids, b_ids, b_ranges=_ranges(300, sizes), live=live.to(torch.uint8) * 3, init=init)   # any non-zero byte is live
    assert all(torch.equal(as_bytes[k], got[k]) for k in RAW)


@pytest.mark.parametrize("E", ES)
def test_a_mask_equals_the_gallery_without_the_dead_rows(E):
    A, B, a_ids, b_ids = _gauss(300, 300, E)
    live = torch.rand(300, generator=torch.Generator().manual_seed(E)) > 0.3
    live[100:200] = False                                             # a fully dead range
    want, ref, n_live = _whole(A, B[live], a_ids, b_ids[live]), _oracle(A, B[live], a_ids, b_ids[live]), int(live.sum())
    poisoned = B.clone()
    poisoned[~live] = float("nan")
    for sizes in (300, 100, (1, 256, 43)):
        for gallery in (B, poisoned):
            _assert_both_equal_the_oracle(_parts(A, gallery, a_ids, b_ids, b_ranges=_ranges(300, sizes), live=live), want, ref, n_live, 300,
                                          cols=live)


@pytest.mark.parametrize("nA,nB", ((129, 257), (300, 300)))
def test_a_mask_of_ones_equals_no_mask(nA, nB):
    A, B, a_ids, b_ids = _gauss(nA, nB, 100)
    ones = torch.ones(nB, dtype=torch.bool)
    want, ref = _whole(A, B, a_ids, b_ids), _oracle(A, B, a_ids, b_ids)
    for sizes in (nB, 100):
        _assert_both_equal_the_oracle(_parts(A, B, a_ids, b_ids, b_ranges=_ranges(nB, sizes), live=ones), want, ref, nB, nA)


# ---------------------------------------------------------------------------------------------------- 6. the accumulate contract
def test_ahead_twice_doubles_and_best_twice_changes_nothing():
    A, B, a_ids, b_ids = _gauss(300, 300, 64)
    b_ranges = _ranges(300, 100)
    once = _parts(A, B, a_ids, b_ids, b_ranges=b_ranges)
    assert int(once["ahead_a"].sum()) > 0 and int(once["ahead_b"].sum()) > 0
    best_twice = _parts(A, B, a_ids, b_ids, b_ranges=b_ranges, best_calls=2)
    assert all(torch.equal(best_twice[k], once[k]) for k in RAW)
    ahead_twice = _parts(A, B, a_ids, b_ids, b_ranges=b_ranges, ahead_calls=2)
    assert torch.equal(ahead_twice["key_a"], once["key_a"]) and torch.equal(ahead_twice["key_b"], once["key_b"])
    assert torch.equal(ahead_twice["ahead_a"], 2 * once["ahead_a"]) and torch.equal(ahead_twice["ahead_b"], 2 * once["ahead_b"])
    only_best = _parts(A, B, a_ids, b_ids, b_ranges=b_ranges, ahead_calls=0)
    assert torch.equal(only_best["key_a"], once["key_a"]) and not bool(only_best["ahead_a"].any()) and not bool(only_best["ahead_b"].any())
