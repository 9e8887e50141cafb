"""GPU: retrieval.mutual_ranks_sharded / mutual_recall_sharded and KWClip_GeneralTransformer.validation_epoch_end(group=...), whole
calls.  THE INVARIANT: a score depends only on its row of A, its row of B and the fixed K order, so for every partition into shards -
on one device or over the ranks of a process group -

    mutual_ranks_sharded(A, ShardedGalleryIndex(B, shard_rows=r, ids=b_ids), a_ids) == mutual_ranks(A, B, a_ids, b_ids)

in all four vectors: the same integers, the same 32 bits in every best score.  With removed rows the right-hand side runs on the
surviving rows.  No tolerance anywhere in this file."""
import functools
import os
import queue
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NA, N, E = 200, 300, 100
KEYS = ("ahead_AB", "ahead_BA", "best_AB", "best_BA")
REMOVED = (0, 99, 100, 128, 255, 256, 299)                            # first and last rows of shards at every shard size, and rows inside


@functools.lru_cache(maxsize=None)
def _case():
    """-> (A [NA, E], B [N, E], a_ids [NA], b_ids [N]) on the CPU, never modified.  B: ids 0 .. 124 at rows 0 .. 124 and again at rows
    125 .. 249 (two correct rows per id, in different shards at most shard sizes), rows 250 .. 299 with ids A does not know.  A: 5 rows
    per id for ids 0 .. 38, each made from the id's first row of B plus noise; its last five rows carry an id B does not hold.  Row 7 of
    B is repeated at row 132 (id 7 again: two correct candidates that tie) and at row 130 (id 5: a wrong candidate that ties with the
    best correct one, from another shard)."""
    g = torch.Generator().manual_seed(22)
    B = torch.randn(N, E, generator=g)
    b_ids = torch.cat([torch.arange(125), torch.arange(125), 1000 + torch.arange(50)])
    a_ids = torch.arange(NA) // 5                                     # ids 0 .. 39
    a_ids[-5:] = 5000                                                 # an id B does not hold
    A = B[a_ids.clamp(max=124)] + 0.7 * torch.randn(NA, E, generator=g)        # a query looks like its image
    B[132] = B[7]
    B[130] = B[7]
    return A, B, a_ids, b_ids


def _cpu(out):
    torch.cuda.synchronize()
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _same(got, want):
    """the same integers, the same 32 bits in every best score"""
    return all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape for k in KEYS) and \
        all(torch.equal(got[k], want[k]) for k in ("ahead_AB", "ahead_BA")) and \
        all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in ("best_AB", "best_BA"))


def _whole(A, B, a_ids, b_ids, cosine, live=None):
    """``mutual_ranks`` on the rows of B that ``live`` keeps, scattered back to B's rows with -1 / -inf at the others -> the CPU"""
    from speechclip_plus_amd import mutual_ranks
    keep = torch.ones(B.shape[0], dtype=torch.bool) if live is None else live
    out = _cpu(mutual_ranks(A.to(DEV), B[keep].to(DEV), a_ids.to(DEV), b_ids[keep].to(DEV), cosine=cosine))
    ahead, best = torch.full((B.shape[0],), -1, dtype=torch.int64), torch.full((B.shape[0],), float("-inf"))
    ahead[keep], best[keep] = out["ahead_BA"], out["best_BA"]
    return {"ahead_AB": out["ahead_AB"], "best_AB": out["best_AB"], "ahead_BA": ahead, "best_BA": best}


@functools.lru_cache(maxsize=None)
def _want(cosine: bool):
    return _whole(*_case(), cosine)


def _index(shard_rows, cosine):
    from speechclip_plus_amd import ShardedGalleryIndex
    _, B, _, b_ids = _case()
    return ShardedGalleryIndex(B.to(DEV), shard_rows=shard_rows, cosine=cosine, ids=b_ids.to(DEV))


# ---------------------------------------------------------------------------------------------------- 1. the invariant
@pytest.mark.parametrize("cosine", (False, True), ids=("dot", "cosine"))
@pytest.mark.parametrize("shard_rows", (1, 100, 128, 129, N, N + 1))
def test_sharded_ranks_equal_mutual_ranks_on_the_whole_gallery(shard_rows, cosine):
    from speechclip_plus_amd import mutual_ranks_sharded
    A, B, a_ids, b_ids = _case()
    index = _index(shard_rows, cosine)
    assert len(index.shards) == -(-N // shard_rows)
    got = _cpu(mutual_ranks_sharded(A.to(DEV), index, a_ids.to(DEV), cosine=cosine))
    assert set(got) == set(KEYS) | {"n_A", "n_B_live"} and (got["n_A"], got["n_B_live"]) == (NA, N)
    want = _want(cosine)
    assert _same(got, want)
    assert 0 < int((want["ahead_AB"] == 0).sum()) < NA and bool((want["ahead_AB"][-5:] == N).all())       # hits, misses, an absent id


@pytest.mark.parametrize("cosine", (False, True), ids=("dot", "cosine"))
@pytest.mark.parametrize("shard_rows", (100, 128, N))
def test_removed_rows_then_restored(shard_rows, cosine):
    from speechclip_plus_amd import mutual_ranks_sharded
    A, B, a_ids, b_ids = _case()
    index = _index(shard_rows, cosine)
    index.remove(list(REMOVED))
    live = torch.ones(N, dtype=torch.bool)
    live[list(REMOVED)] = False
    got = _cpu(mutual_ranks_sharded(A.to(DEV), index, a_ids.to(DEV), cosine=cosine))
    assert (got["n_A"], got["n_B_live"]) == (NA, N - len(REMOVED))
    assert _same(got, _whole(A, B, a_ids, b_ids, cosine, live))
    assert bool((got["ahead_BA"][~live] == -1).all()) and bool(torch.isneginf(got["best_BA"][~live]).all())
    assert not _same(got, _want(cosine))                              # row 0 was query 0's best candidate: the removal shows
    index.restore([0, 99])
    live[[0, 99]] = True
    assert _same(_cpu(mutual_ranks_sharded(A.to(DEV), index, a_ids.to(DEV), cosine=cosine)), _whole(A, B, a_ids, b_ids, cosine, live))
    index.restore()
    assert _same(_cpu(mutual_ranks_sharded(A.to(DEV), index, a_ids.to(DEV), cosine=cosine)), _want(cosine))


# ---------------------------------------------------------------------------------------------------- 2. recall
@pytest.mark.parametrize("shard_rows", (100, N + 1))
def test_recall_dictionaries_equal_mutual_recall(shard_rows):
    from speechclip_plus_amd import mutual_recall, mutual_recall_sharded
    A, B, a_ids, b_ids = _case()
    ks = [1, 5, 10, 400]                                              # 400: more than either side's candidates
    index = _index(shard_rows, False)
    for stats in (False, True):
        want = mutual_recall(A.to(DEV), B.to(DEV), a_ids.to(DEV), b_ids.to(DEV), ks, rank_stats=stats)
        assert mutual_recall_sharded(A.to(DEV), index, a_ids.to(DEV), ks, rank_stats=stats) == want
    assert set(want[0]) == {f"recall@{k}" for k in ks} | {"median_rank", "mean_rank"} and 0.0 < want[0]["recall@1"] < 100.0
    index.remove(list(REMOVED))
    live = torch.ones(N, dtype=torch.bool)
    live[list(REMOVED)] = False
    want = mutual_recall(A.to(DEV), B[live].to(DEV), a_ids.to(DEV), b_ids[live].to(DEV), ks, rank_stats=True)
    assert mutual_recall_sharded(A.to(DEV), index, a_ids.to(DEV), ks, rank_stats=True) == want


# ---------------------------------------------------------------------------------------------------- 3. empty operands
def test_an_empty_a_and_an_empty_gallery_are_legal():
    from speechclip_plus_amd import ShardedGalleryIndex, mutual_ranks_sharded, mutual_recall_sharded
    A, B, a_ids, b_ids = _case()
    none = torch.zeros(0, dtype=torch.int64)
    got = _cpu(mutual_ranks_sharded(torch.zeros(0, E, device=DEV), _index(100, False), none.to(DEV)))
    assert (got["n_A"], got["n_B_live"]) == (0, N) and got["ahead_AB"].shape == got["best_AB"].shape == (0,)
    assert got["ahead_BA"].tolist() == [0] * N and bool(torch.isneginf(got["best_BA"]).all())   # no candidate: ahead = their number, 0
    empty = ShardedGalleryIndex(torch.zeros(0, E, device=DEV), shard_rows=100, ids=none.to(DEV))
    got = _cpu(mutual_ranks_sharded(A.to(DEV), empty, a_ids.to(DEV)))
    assert (got["n_A"], got["n_B_live"]) == (NA, 0) and got["ahead_BA"].shape == got["best_BA"].shape == (0,)
    assert got["ahead_AB"].tolist() == [0] * NA and bool(torch.isneginf(got["best_AB"]).all())
    AB, BA, mean = mutual_recall_sharded(A.to(DEV), empty, a_ids.to(DEV), [1])
    assert AB == {"recall@1": 100.0}                                  # ``recall_from_ranks``' reading of ahead = 0 candidates < 1


# ---------------------------------------------------------------------------------------------------- 4. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_two_ranks(worker):
    """``worker(rank, world, port, out)`` in two freshly spawned children -> {rank: what it put after its rank}.  A rank that died is
    noticed at once, not at the timeout; a rank left waiting in a collective for one that died is killed."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got, waited = {}, 0
    try:
        while len(got) < 2:
            try:
                item = out.get(timeout=1)
                got[item[0]] = item[1:]
            except queue.Empty:
                waited += 1
                assert all(p.exitcode in (None, 0) for p in procs) and waited < 240, [p.exitcode for p in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    return got


def _init_rank(rank, world, port):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


RANK_ROWS, RANK_QUERIES, RANK_REMOVED, RANK_KS = (300, 212), (5, 3), (3, 350), [1, 5, 10]


@functools.lru_cache(maxsize=None)
def _rank_case():
    """512 gallery rows whose ids repeat every 200 rows (the correct rows of an id lie on both ranks), 8 queries that look like a row
    of theirs; the last query's id is in no row.  Row 3 - the row query 0 was made from - and row 350 are removed: one in each range."""
    g = torch.Generator().manual_seed(23)
    B = torch.randn(512, E, generator=g)
    b_ids = torch.arange(512) % 200
    a_ids = torch.tensor([3, 150, 77, 199, 0, 42, 180, 999])
    A = B[torch.tensor([3, 350, 277, 199, 400, 42, 380, 5])] + 0.5 * torch.randn(8, E, generator=g)
    return A, B, a_ids, b_ids


def _ranks_worker(rank, world, port, out):
    dist = _init_rank(rank, world, port)
    from speechclip_plus_amd import ShardedGalleryIndex, mutual_ranks_sharded, mutual_recall_sharded
    A, B, a_ids, b_ids = _rank_case()
    r0, q0 = sum(RANK_ROWS[:rank]), sum(RANK_QUERIES[:rank])
    r1, q1 = r0 + RANK_ROWS[rank], q0 + RANK_QUERIES[rank]
    index = ShardedGalleryIndex(B[r0:r1].to(DEV), cosine=True, ids=b_ids[r0:r1].to(DEV), group=dist.group.WORLD)
    index.remove(list(RANK_REMOVED))
    ranks = mutual_ranks_sharded(A[q0:q1].to(DEV), index, a_ids[q0:q1].to(DEV), cosine=True)
    recall = mutual_recall_sharded(A[q0:q1].to(DEV), index, a_ids[q0:q1].to(DEV), RANK_KS, cosine=True, rank_stats=True)
    torch.cuda.synchronize()
    # by value: torch tensors travel as fds the exiting rank may close
    out.put((rank, ranks["n_A"], ranks["n_B_live"], {k: ranks[k].cpu().numpy() for k in KEYS}, recall))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_each_with_its_own_rows_and_queries():
    """gloo rendezvous, both ranks on cuda:0 (a 1-GPU box cannot host an RCCL world): rank 0 holds 300 rows and 5 queries, rank 1 212
    rows and 3 queries, one removed row in each range; every rank's slices equal the single-process result on the surviving rows and
    both ranks report its recall dictionaries"""
    from speechclip_plus_amd import mutual_recall
    got = _run_two_ranks(_ranks_worker)
    A, B, a_ids, b_ids = _rank_case()
    live = torch.ones(512, dtype=torch.bool)
    live[list(RANK_REMOVED)] = False
    want = _whole(A, B, a_ids, b_ids, True, live)
    assert want["ahead_AB"][7] == 510 and int((want["ahead_AB"] == 0).sum()) >= 4                 # the absent id; most queries find theirs
    want_recall = mutual_recall(A.to(DEV), B[live].to(DEV), a_ids.to(DEV), b_ids[live].to(DEV), RANK_KS, cosine=True, rank_stats=True)
    for rank in (0, 1):
        n_a, n_live, vecs, recall = got[rank]
        assert (n_a, n_live) == (8, 510)
        r0, q0 = sum(RANK_ROWS[:rank]), sum(RANK_QUERIES[:rank])
        mine = {"ahead_AB": want["ahead_AB"][q0: q0 + RANK_QUERIES[rank]], "best_AB": want["best_AB"][q0: q0 + RANK_QUERIES[rank]],
                "ahead_BA": want["ahead_BA"][r0: r0 + RANK_ROWS[rank]], "best_BA": want["best_BA"][r0: r0 + RANK_ROWS[rank]]}
        assert _same({k: torch.from_numpy(v) for k, v in vecs.items()}, mine), rank
        assert recall == want_recall, rank


# ---------------------------------------------------------------------------------------------------- 5. the model hook
def _bare_model():
    """the hook reads ``config`` and ``recall_at`` only: no encoder is built"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    cfg = base_parallel_config()
    cfg.retrieval.fused_ranks = True
    model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
    torch.nn.Module.__init__(model)
    model.config, model.recall_at, model.cascaded_branch = cfg, cfg.retrieval.recall_at, None
    return model


BATCHES = ((10, 12), (7, 11))                                         # the validation batches of rank 0 and of rank 1


@functools.lru_cache(maxsize=None)
def _outputs():
    """40 samples in 4 uneven batches, on the CPU: ids 0 .. 24, then 0 .. 14 again - an image id seen on rank 0 comes back on rank 1
    with ANOTHER embedding, which is the one kept -, one id twice on rank 0 and one twice on rank 1"""
    g = torch.Generator().manual_seed(24)
    ids = torch.arange(40) % 25
    ids[5], ids[39] = ids[2], ids[23]
    img = torch.randn(40, E, generator=g)
    audio = img + 0.8 * torch.randn(40, E, generator=g)
    outputs, r0 = [], 0
    for n in BATCHES[0] + BATCHES[1]:
        outputs.append({"id": ids[r0: r0 + n], "parallel_audio_feat": audio[r0: r0 + n], "image_feat": img[r0: r0 + n]})
        r0 += n
    return outputs


def _on_device(outputs):
    return [{"others": {k: v.to(DEV) for k, v in o.items()}} for o in outputs]


def _validation_worker(rank, world, port, out):
    dist = _init_rank(rank, world, port)
    mine = _outputs()[:2] if rank == 0 else _outputs()[2:]
    result = _bare_model().validation_epoch_end(_on_device(mine), group=dist.group.WORLD)
    torch.cuda.synchronize()
    out.put((rank, result))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_validation_epoch_end_over_two_ranks_equals_the_single_process_call():
    got = _run_two_ranks(_validation_worker)
    want = _bare_model().validation_epoch_end(_on_device(_outputs()))
    assert set(want[0]) == {"recall@1", "recall@5", "recall@10"} and 0.0 < want[0]["recall@1"] < 100.0
    for rank in (0, 1):
        assert got[rank] == (want,), (rank, got[rank], want)
