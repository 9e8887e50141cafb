"""GPU: retrieval.ShardedGalleryIndex / search_sharded, the whole call.  THE INVARIANT: a score depends only on its query row, its
gallery row and the fixed K order, so for every partition into shards

    search_sharded(q, ShardedGalleryIndex(g, shard_rows=r, ...), k, ...) == search(q, GalleryIndex(g, ...), k, ...)

- the same idx everywhere, the same 32 bits in every non-NaN value, NaN where NaN.  No tolerance anywhere in this file.

Data: E = 64, 130 queries, 700 gallery rows; rows duplicated across the boundaries of every shard size (ties across shards), ids with
collisions, so the filter bites in every shard."""
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
NQ, N, E = 130, 700, 64
SHARD_ROWS = (40, 128, 300, N)


@functools.lru_cache(maxsize=None)
def _case():
    """-> (q [NQ, E], gal [N, E], q_ids [NQ], g_ids [N]) on the CPU, never modified"""
    g = torch.Generator().manual_seed(21)
    q, gal = torch.randn(NQ, E, generator=g), torch.randn(N, E, generator=g)
    for r in (40, 128, 300, 600):                                     # equal rows on both sides of a shard boundary, at every shard size
        gal[r] = gal[r - 1]
    gal[41] = gal[39]
    gal[650] = gal[5]                                                 # ... and far apart
    return q, gal, torch.arange(NQ, dtype=torch.int64) % 37, (torch.arange(N, dtype=torch.int64) * 7) % 37


def _same(got, want):
    """the same rows in the same places, the same 32 bits in every non-NaN value, NaN where NaN"""
    (gv, gi), (wv, wi) = got, want
    assert gv.dtype == wv.dtype == torch.float32 and gi.dtype == wi.dtype == torch.int64 and gv.shape == wv.shape == gi.shape == wi.shape
    nan = torch.isnan(wv)
    return (torch.equal(gi, wi) and torch.equal(torch.isnan(gv), nan)
            and torch.equal(gv.view(torch.int32).masked_fill(nan, 0), wv.view(torch.int32).masked_fill(nan, 0)))


def _cpu(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


@functools.lru_cache(maxsize=None)
def _want(k: int, filtered: bool, cosine: bool):
    """``search`` on the whole gallery, once per (k, filtered, cosine), on the CPU"""
    from speechclip_plus_amd import GalleryIndex, search
    q, gal, q_ids, g_ids = _case()
    index = GalleryIndex(gal.to(DEV), cosine=cosine, ids=g_ids.to(DEV) if filtered else None)
    return _cpu(search(q.to(DEV), index, k, cosine=cosine, query_ids=q_ids.to(DEV) if filtered else None))


def _sharded(shard_rows, k, filtered, cosine, gal=None, queries=None):
    from speechclip_plus_amd import ShardedGalleryIndex, search_sharded
    q, g, q_ids, g_ids = _case()
    index = ShardedGalleryIndex((g if gal is None else gal).to(DEV), shard_rows=shard_rows, cosine=cosine, ids=g_ids.to(DEV) if filtered else None)
    q = q if queries is None else queries
    return index, _cpu(search_sharded(q.to(DEV), index, k, cosine=cosine, query_ids=q_ids[: q.shape[0]].to(DEV) if filtered else None))


# ---------------------------------------------------------------------------------------------------- 1. the invariant
@pytest.mark.parametrize("cosine", (False, True), ids=("dot", "cosine"))
@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids"))
@pytest.mark.parametrize("shard_rows", SHARD_ROWS)
@pytest.mark.parametrize("k", (5, 32, 33, 100))
def test_sharded_search_equals_search_on_the_whole_gallery(k, shard_rows, filtered, cosine):
    index, got = _sharded(shard_rows, k, filtered, cosine)
    assert len(index.shards) == -(-N // shard_rows) and index.row0 == list(range(0, N, shard_rows))
    assert len(index) == index.N == index.n_live == N and index.E == E and index.cosine == cosine
    assert sum(s.N for s in index.shards) == N
    assert _same(got, _want(k, filtered, cosine))


def test_ties_across_a_shard_boundary_keep_the_lower_global_row_first():
    """row 40 equals row 39 (and 41): with shards of 40 rows they lie in different shards and score the same against every query"""
    want = _want(100, False, False)
    seen = 0
    for i in range(NQ):
        row = want[1][i].tolist()
        if 39 in row and row.index(39) + 2 < 100:
            p = row.index(39)
            assert row[p + 1: p + 3] == [40, 41] and want[0][i, p] == want[0][i, p + 2]
            seen += 1
    assert seen, "some list holds the three equal rows"
    assert _same(_sharded(40, 100, False, False)[1], want)


@pytest.mark.parametrize("k", (32, 100))
def test_removed_rows_in_two_different_shards(k):
    from speechclip_plus_amd import GalleryIndex, search, search_sharded
    q, gal, q_ids, g_ids = _case()
    plain = _want(k, True, True)
    gone = [int(plain[1][0, 0]), int(plain[1][1, 0]), 3, 699, 128]   # leaders of two lists and rows of the first, the last and a middle shard
    whole = GalleryIndex(gal.to(DEV), cosine=True, ids=g_ids.to(DEV)).remove(gone)
    want = _cpu(search(q.to(DEV), whole, k, cosine=True, query_ids=q_ids.to(DEV)))
    assert not _same(want, plain)
    index, _ = _sharded(128, k, True, True)
    assert index.remove(gone) is index and index.n_live == N - len(set(gone))
    assert len({r // 128 for r in gone}) >= 3, "the removed rows lie in different shards"
    got = _cpu(search_sharded(q.to(DEV), index, k, cosine=True, query_ids=q_ids.to(DEV)))
    assert _same(got, want) and not bool(torch.isin(got[1], torch.tensor(gone)).any())
    index.restore([gone[0], 699])
    whole.restore([gone[0], 699])
    assert index.n_live == whole.n_live
    assert _same(_cpu(search_sharded(q.to(DEV), index, k, cosine=True, query_ids=q_ids.to(DEV))),
                 _cpu(search(q.to(DEV), whole, k, cosine=True, query_ids=q_ids.to(DEV))))
    assert index.restore() is index and index.n_live == N
    assert _same(_cpu(search_sharded(q.to(DEV), index, k, cosine=True, query_ids=q_ids.to(DEV))), plain)
    with pytest.raises(IndexError, match=r"rows outside \[0, 700\)"):
        index.remove([N])


@pytest.mark.parametrize("k", (5, 100))
def test_a_nan_row_leads_every_list_as_in_search(k):
    from speechclip_plus_amd import GalleryIndex, search
    q, gal = _case()[:2]
    gal = gal.clone()
    gal[333, 7] = float("nan")
    want = _cpu(search(q.to(DEV), GalleryIndex(gal.to(DEV)), k))
    assert bool((want[1][:, 0] == 333).all()) and bool(torch.isnan(want[0][:, 0]).all())
    for shard_rows in (128, 300):
        assert _same(_sharded(shard_rows, k, False, False, gal=gal)[1], want)


@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids"))
@pytest.mark.parametrize("k", (32, 100))
def test_three_query_chunks(monkeypatch, k, filtered):
    from speechclip_plus_amd import retrieval
    S = -(-N // 128)
    assert retrieval.SHARD_LISTS_BYTES // (S * k * 8) > NQ, "the stock constant gives one chunk here"
    monkeypatch.setattr(retrieval, "SHARD_LISTS_BYTES", S * k * 8 * 50)          # 50 queries per chunk: 50, 50 and 30
    assert _same(_sharded(128, k, filtered, False)[1], _want(k, filtered, False))


def test_short_and_empty_operands():
    from speechclip_plus_amd import ShardedGalleryIndex, search, search_sharded
    q, gal = _case()[:2]
    _, (vals, idx) = _sharded(128, 64, False, False, gal=gal[:40])                # fewer rows than k: fillers behind them
    assert bool((idx[:, 40:] == -1).all()) and bool(torch.isneginf(vals[:, 40:]).all())
    assert _same((vals, idx), _cpu(search(q.to(DEV), gal[:40].to(DEV), 64)))
    for k in (5, 64):
        index = ShardedGalleryIndex(gal[:0].to(DEV))                             # no gallery row at all: one empty shard
        vals, idx = search_sharded(q[:5].to(DEV), index, k)
        assert len(index) == 0 and tuple(idx.shape) == (5, k) and bool((idx == -1).all()) and bool(torch.isneginf(vals).all())
    _, (vals, idx) = _sharded(128, 64, False, False, queries=q[:0])               # no query
    assert tuple(vals.shape) == tuple(idx.shape) == (0, 64)


# ---------------------------------------------------------------------------------------------------- 2. hard_negatives, retrieve
@pytest.mark.parametrize("k", (7, 64))
def test_hard_negatives_with_a_sharded_index(k):
    from speechclip_plus_amd import GalleryIndex, ShardedGalleryIndex, hard_negatives
    q, gal, q_ids, g_ids = (t.to(DEV) for t in _case())
    want = _cpu(hard_negatives(q, GalleryIndex(gal, cosine=True, ids=g_ids), q_ids, None, k, cosine=True))
    got = _cpu(hard_negatives(q, ShardedGalleryIndex(gal, shard_rows=300, cosine=True, ids=g_ids), q_ids, None, k, cosine=True))
    assert _same(got, want)
    assert bool((g_ids.cpu()[got[1]] != q_ids.cpu().unsqueeze(1)).all())
    with pytest.raises(ValueError, match="its own ids"):
        hard_negatives(q, ShardedGalleryIndex(gal, shard_rows=300), q_ids, None, k)


@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_retrieve_with_a_sharded_index(model):
    from speechclip_plus_amd import GalleryIndex, ShardedGalleryIndex
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(9, 512, generator=g).to(DEV)
    gallery = torch.randn(300, 512, generator=g).to(DEV)
    q_ids, g_ids = (torch.arange(9) % 4).to(DEV), (torch.arange(300) % 4).to(DEV)
    for k in (7, 64):
        want = _cpu(model.retrieve(emb, GalleryIndex(gallery, cosine=True, ids=g_ids), k=k))
        got = _cpu(model.retrieve(emb, ShardedGalleryIndex(gallery, shard_rows=128, cosine=True, ids=g_ids), k=k))
        assert _same(got, want)
        want = _cpu(model.retrieve(emb, GalleryIndex(gallery, cosine=True, ids=g_ids), k=k, query_ids=q_ids))
        got = _cpu(model.retrieve(emb, ShardedGalleryIndex(gallery, shard_rows=128, cosine=True, ids=g_ids), k=k, query_ids=q_ids))
        assert _same(got, want) and bool((g_ids.cpu()[got[1]] != q_ids.cpu().unsqueeze(1)).all())
    with pytest.raises(ValueError, match="brings its own ids"):
        model.retrieve(emb, ShardedGalleryIndex(gallery, shard_rows=128, cosine=True, ids=g_ids), k=7, query_ids=q_ids, gallery_ids=g_ids)


# ---------------------------------------------------------------------------------------------------- 3. beyond search's limit
def test_top_100_of_a_gallery_beyond_the_wide_limit():
    """N = 262 144 + 200 rows at k = 100: ``search`` refuses, the default ``shard_rows`` gives two shards.  The gallery is 0.01 x Gaussian
    but for 100 planted rows c_j q / |q|^2 (score c_j against q, up to rounding; c_j = 100 - j / 2, far apart and far above the
    rest, whose scores are of the size 0.01 |q|): the expected list is the planted order."""
    from speechclip_plus_amd import ShardedGalleryIndex, search, search_sharded
    from speechclip_plus_amd.retrieval import wide_max_gallery
    lim = wide_max_gallery()
    n, k = lim + 200, 100
    g = torch.Generator().manual_seed(5)
    q = torch.randn(1, E, generator=g)
    unit = q[0] / float(q[0] @ q[0])
    gal = (0.01 * torch.randn(n, E, generator=g)).to(DEV)
    fixed = [0, lim - 1, lim, n - 1]                                  # both ends of both shards
    places = fixed + [p for p in torch.randperm(n, generator=g)[:200].tolist() if p not in fixed][: k - 4]
    order = torch.randperm(k, generator=g).tolist()                   # which c_j each planted place gets
    c = torch.tensor([100.0 - 0.5 * order[j] for j in range(k)])
    gal[torch.tensor(places, device=DEV)] = (c.unsqueeze(1) * unit.unsqueeze(0)).to(DEV)
    expected = [places[j] for j in sorted(range(k), key=lambda j: order[j])]
    queries = torch.cat([q, 2.0 * q, 0.5 * q]).to(DEV)                # nQ = 3: positive multiples keep the order
    with pytest.raises(ValueError, match="at most N = 262144"):
        search(queries, gal, k)
    index = ShardedGalleryIndex(gal)
    assert len(index.shards) == 2 and index.row0 == [0, lim] and len(index) == n
    vals, idx = _cpu(search_sharded(queries, index, k))
    assert idx.tolist() == [expected] * 3
    assert bool((vals[:, :-1] > vals[:, 1:]).all())
    narrow = _cpu(search(queries, gal, 32))                           # k <= 32 has no limit: the first 32 entries, bit for bit
    assert _same((vals[:, :32].contiguous(), idx[:, :32].contiguous()), narrow)


# ---------------------------------------------------------------------------------------------------- 4. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_ROWS, RANK_QUERIES, RANK_K = (300, 212), (5, 3), 40


def _rank_case():
    q, gal, q_ids, g_ids = _case()
    return q[:8], gal[:512], q_ids[:8], g_ids[:512]


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from speechclip_plus_amd import ShardedGalleryIndex, search_sharded
    q, gal, q_ids, g_ids = _rank_case()
    r0, q0 = sum(RANK_ROWS[:rank]), sum(RANK_QUERIES[:rank])
    r1, q1 = r0 + RANK_ROWS[rank], q0 + RANK_QUERIES[rank]
    index = ShardedGalleryIndex(gal[r0:r1].to(DEV), cosine=True, ids=g_ids[r0:r1].to(DEV), group=dist.group.WORLD)
    vals, idx = search_sharded(q[q0:q1].to(DEV), index, RANK_K, cosine=True, query_ids=q_ids[q0:q1].to(DEV))
    torch.cuda.synchronize()
    # by value: torch tensors travel as fds the exiting rank may close
    out.put((rank, len(index), index.row0, len(index.shards), index.n_live, vals.cpu().numpy(), idx.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_each_with_its_own_rows_and_queries():
    """gloo rendezvous, both ranks on cuda:0 (a 1-GPU box cannot host an RCCL world): rank 0 holds 300 rows and 5 queries, rank 1 212
    rows and 3 queries, with ids; every rank's lists equal ``search`` of its queries against the whole 512-row gallery"""
    from speechclip_plus_amd import GalleryIndex, search
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    got, waited = {}, 0
    try:
        while len(got) < 2:
            try:
                item = out.get(timeout=1)
                got[item[0]] = item[1:]
            except queue.Empty:                                       # a rank that died is noticed at once, not at the timeout
                waited += 1
                assert all(p.exitcode in (None, 0) for p in procs) and waited < 240, [p.exitcode for p in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:                                               # a rank left waiting in a collective for one that died
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    q, gal, q_ids, g_ids = _rank_case()
    want = _cpu(search(q.to(DEV), GalleryIndex(gal.to(DEV), cosine=True, ids=g_ids.to(DEV)), RANK_K, cosine=True, query_ids=q_ids.to(DEV)))
    for rank, q0 in ((0, 0), (1, 5)):
        n, row0, shards, n_live, vals, idx = got[rank]
        assert (n, row0, shards, n_live) == (512, [sum(RANK_ROWS[:rank])], 1, 512)
        q1 = q0 + RANK_QUERIES[rank]
        assert _same((torch.from_numpy(vals), torch.from_numpy(idx)), (want[0][q0:q1], want[1][q0:q1])), rank
