"""Which error a bad ``search`` / ``search_compact`` / index call reports, and in which order, without a GPU: one table of calls, each
with the exception type and a pattern of its text.  ``search`` checks in this order: k > 1024; the CompactGalleryIndex branch (its
own message per case); k > 32: route="fused" / slabs=, then an unknown route; queries; gallery (only when the call is filtered or
k > 32); the filter; the device; k > 32: the 262 144-row limit; the index build; E; k >= 1; k <= 32: an unknown route.  Where two
errors apply, the earlier one is reported - the accidental differences between the k <= 32 and the k > 32 path included (a gallery
that is no tensor is a RuntimeError on the unfiltered k <= 32 path and a ValueError everywhere else).

The checks behind the device test are reached with tensors whose ``is_cuda`` is faked and indexes built bare: every such call raises
before anything is allocated on a device or launched."""
import pytest
import torch

Q, G = torch.zeros(3, 64), torch.zeros(5, 64)                        # CPU tensors: a call that passes every format check ends in
QI, GI = torch.arange(3), torch.arange(5)                            # "device tensors only"
LIVE = torch.ones(5, dtype=torch.bool)


class _Fake(torch.Tensor):
    is_cuda = True


def _fake(t):
    return t.as_subclass(_Fake)


def _bare(cls, **fields):
    obj = cls.__new__(cls)
    for name, value in fields.items():
        setattr(obj, name, value)
    return obj


def _compact(**fields):
    from speechclip_plus_amd import CompactGalleryIndex
    return _bare(CompactGalleryIndex, **{"N": 5, "E": 64, **fields})


def _index(N=5, E=64):
    """a GalleryIndex that passes the device test and holds no rows"""
    from speechclip_plus_amd import GalleryIndex
    return _bare(GalleryIndex, N=N, E=E, Ep=64, ids=None, live=None, cosine=False, split=_fake(torch.zeros(128, 384, dtype=torch.bfloat16)))


def _search(*args, **kwargs):
    from speechclip_plus_amd import search
    return search(*args, **kwargs)


def _search_compact(*args, **kwargs):
    from speechclip_plus_amd import search_compact
    return search_compact(*args, **kwargs)


def _hard_negatives(*args, **kwargs):
    from speechclip_plus_amd import hard_negatives
    return hard_negatives(*args, **kwargs)


def _gallery_index(*args, **kwargs):
    from speechclip_plus_amd import GalleryIndex
    return GalleryIndex(*args, **kwargs)


def _compact_index(*args, **kwargs):
    from speechclip_plus_amd import CompactGalleryIndex
    return CompactGalleryIndex(*args, **kwargs)


DEVICE = "search runs on the HIP kernels: device tensors only"
K_RANGE = r"search: 1 <= k <= 1024 \(k {}\)"
FUSED_WIDE = r'search: k = 40 with route="fused" / slabs= - the fused kernel keeps at most 32'
ROUTE = r"""search: route = 'nonsense' \("fused" or "composition"\)"""
QUERIES = r"search: queries must be a \[nQ, E\] tensor"
GALLERY = r"search: gallery must be a \[N, E\] tensor or a GalleryIndex"

# (name, call, args, kwargs, exception, pattern)
CASES = [
    # ---- 1. k > 1024 comes first
    ("k 2000 on a compact index", _search, lambda: (Q, _compact(), 2000), {}, ValueError, K_RANGE.format(2000)),
    ("k 2000, route fused, 3-d queries", _search, lambda: (torch.zeros(2, 3, 64), G, 2000), {"route": "fused"}, ValueError, K_RANGE.format(2000)),
    ("k 1025", _search, lambda: (Q, G, 1025), {}, ValueError, K_RANGE.format(1025)),
    # ---- 2. the compact branch, one message per case
    ("k 40 on a compact index", _search, lambda: (Q, _compact(), 40), {}, ValueError, "search: k = 40 on a CompactGalleryIndex - its certificate"),
    ("k 40 on a compact index with a filter and a route", _search, lambda: (Q, _compact(), 40),
     {"query_ids": QI, "route": "fused"}, ValueError, "search: k = 40 on a CompactGalleryIndex"),
    ("k 33 on a compact index, 1-d queries", _search, lambda: (torch.zeros(64), _compact(), 33), {}, ValueError, "search: k = 33 on a CompactGalleryIndex"),
    ("compact index with ids", _search, lambda: (Q, _compact(), 2), {"query_ids": QI, "gallery_ids": GI}, ValueError,
     "search: a CompactGalleryIndex takes no filter arguments here"),
    ("compact index with a filter and a route", _search, lambda: (Q, _compact(), 2), {"live": LIVE, "route": "fused"}, ValueError,
     "takes no filter arguments here"),
    ("compact index with route=", _search, lambda: (Q, _compact(), 2), {"route": "composition"}, ValueError,
     "search: route applies to a GalleryIndex or a tensor, not to a CompactGalleryIndex"),
    ("compact index with route=, 1-d queries", _search, lambda: (torch.zeros(64), _compact(), 2), {"route": "fused"}, ValueError,
     "search: route applies to a GalleryIndex or a tensor"),
    ("compact index, 1-d queries", _search, lambda: (torch.zeros(64), _compact(), 2), {}, ValueError,
     r"search_compact: queries must be a \[nQ, E\] tensor"),
    # ---- 3. k > 32: route="fused" / slabs=, then an unknown route, both before queries
    ("k 40 fused, 3-d queries", _search, lambda: (torch.zeros(2, 3, 64), G, 40), {"route": "fused"}, ValueError, FUSED_WIDE),
    ("k 40 slabs", _search, lambda: (Q, G, 40), {"slabs": 2}, ValueError, FUSED_WIDE),
    ("k 40 slabs and an unknown route", _search, lambda: (Q, G, 40), {"slabs": 1, "route": "nonsense"}, ValueError, FUSED_WIDE),
    ("k 40 unknown route", _search, lambda: (Q, G, 40), {"route": "nonsense"}, ValueError, ROUTE),
    ("k 40 unknown route, 3-d queries", _search, lambda: (torch.zeros(2, 3, 64), G, 40), {"route": "nonsense"}, ValueError, ROUTE),
    ("k 40 unknown route, one-sided id", _search, lambda: (Q, G, 40), {"route": "nonsense", "query_ids": QI}, ValueError, ROUTE),
    # ---- 4. queries
    ("k 2, 1-d queries", _search, lambda: (torch.zeros(64), G, 2), {}, ValueError, QUERIES),
    ("k 40, queries no tensor", _search, lambda: ([[0.0] * 64], G, 40), {}, ValueError, QUERIES),
    ("k 2, 3-d queries and a one-sided id", _search, lambda: (torch.zeros(2, 3, 64), G, 2), {"query_ids": QI}, ValueError, QUERIES),
    ("k 40, 1-d queries and a 3-d gallery", _search, lambda: (torch.zeros(64), torch.zeros(5, 2, 64), 40), {}, ValueError, QUERIES),
    # ---- 5. gallery: checked when the call is filtered or k > 32, else left to the device test
    ("k 2, gallery no tensor", _search, lambda: (Q, [[0.0] * 64], 2), {}, RuntimeError, DEVICE),
    ("k 2, 3-d gallery", _search, lambda: (Q, torch.zeros(5, 2, 64), 2), {}, RuntimeError, DEVICE),
    ("k 2, gallery no tensor, filtered", _search, lambda: (Q, [[0.0] * 64], 2), {"live": LIVE}, ValueError, GALLERY),
    ("k 2, 3-d gallery, one-sided id", _search, lambda: (Q, torch.zeros(5, 2, 64), 2), {"gallery_ids": GI}, ValueError, GALLERY),
    ("k 40, gallery no tensor", _search, lambda: (Q, None, 40), {}, ValueError, GALLERY),
    ("k 40, 3-d gallery, one-sided id", _search, lambda: (Q, torch.zeros(5, 2, 64), 40), {"query_ids": QI}, ValueError, GALLERY),
    # ---- 6. the filter, before the device
    ("k 40, one-sided id", _search, lambda: (Q, G, 40), {"query_ids": QI}, ValueError, "search: ids on one side only - give query_ids and gallery_ids"),
    ("k 2, one-sided id", _search, lambda: (Q, G, 2), {"gallery_ids": GI}, ValueError, "search: ids on one side only"),
    ("k 2, bad live dtype", _search, lambda: (Q, G, 2), {"live": torch.ones(5)}, ValueError, r"search: live must be torch\.bool or torch\.uint8, not torch\.float32"),
    ("k 40, bad live dtype", _search, lambda: (Q, G, 40), {"live": torch.ones(5)}, ValueError, "search: live must be"),
    ("k 2, bad id length", _search, lambda: (Q, G, 2), {"query_ids": torch.arange(4), "gallery_ids": GI}, ValueError,
     r"search: query_ids has shape \(4,\), expected \(3,\)"),
    ("k 0, bad live shape", _search, lambda: (Q, G, 0), {"live": torch.ones(4, dtype=torch.bool)}, ValueError, r"search: live has shape \(4,\), expected \(5,\)"),
    ("k 2, ids on the CPU", _search, lambda: (Q, G, 2), {"query_ids": QI, "gallery_ids": GI}, RuntimeError, DEVICE + r" \(query_ids\)"),
    ("k 40, live on the CPU", _search, lambda: (Q, G, 40), {"live": LIVE}, RuntimeError, DEVICE + r" \(live\)"),
    ("an index's own ids are the gallery's", _search, lambda: (Q, _bare(type(_index()), N=5, E=64, ids=GI.int(), live=None, split=Q), 2),
     {"query_ids": QI}, ValueError, "search: gallery_ids must be torch.int64, not torch.int32"),
    # ---- 7. the device, before the row limit, E, k >= 1 and the k <= 32 route
    ("k 2 on the CPU", _search, lambda: (Q, G, 2), {}, RuntimeError, DEVICE + "$"),
    ("k 40 on the CPU", _search, lambda: (Q, G, 40), {}, RuntimeError, DEVICE + "$"),
    ("k 0 on the CPU", _search, lambda: (Q, G, 0), {}, RuntimeError, DEVICE + "$"),
    ("k 2, unknown route, on the CPU", _search, lambda: (Q, G, 2), {"route": "nonsense"}, RuntimeError, DEVICE + "$"),
    ("k 2, other E, on the CPU", _search, lambda: (Q, torch.zeros(5, 32), 2), {}, RuntimeError, DEVICE + "$"),
    ("device queries, CPU index", _search, lambda: (_fake(Q), _bare(type(_index()), N=5, E=64, ids=None, live=None, split=Q), 2), {},
     RuntimeError, DEVICE + "$"),
    # ---- 8. k > 32: the row limit, before E
    ("k 40, 300 000 rows, other E", _search, lambda: (_fake(Q), _index(N=300000, E=32), 40), {}, ValueError,
     r"search: k = 40 against 300000 gallery rows - 128 query rows of scores no longer fit the score scratch; 32 < k <= 1024 serves at most "
     r"N = 262144 gallery rows"),
    # ---- 10. E, before k >= 1
    ("k 40, other E", _search, lambda: (_fake(Q), _index(E=32), 40), {}, AssertionError, r"torch\.Size\(\[3, 64\]\), 32"),
    ("k 0, other E", _search, lambda: (_fake(Q), _index(E=32), 0), {}, AssertionError, r"torch\.Size\(\[3, 64\]\), 32"),
    # ---- 11. k >= 1, before the k <= 32 route
    ("k 0", _search, lambda: (_fake(Q), _index(), 0), {}, ValueError, K_RANGE.format(0)),
    ("k -3, unknown route", _search, lambda: (_fake(Q), _index(), -3), {"route": "nonsense"}, ValueError, K_RANGE.format(-3)),
    # ---- 12. k <= 32: an unknown route comes last
    ("k 2, unknown route", _search, lambda: (_fake(Q), _index(), 2), {"route": "nonsense"}, ValueError, ROUTE),
    ("k 2, unknown route and slabs", _search, lambda: (_fake(Q), _index(), 2), {"route": "nonsense", "slabs": 2}, ValueError, ROUTE),
    # ---- search_compact: queries, gallery (filtered only), the filter, the device, fallback
    ("compact: 1-d queries, bad fallback", _search_compact, lambda: (torch.zeros(64), G, 2), {"fallback": "maybe"}, ValueError,
     r"search_compact: queries must be a \[nQ, E\] tensor"),
    ("compact: gallery no tensor", _search_compact, lambda: (Q, None, 2), {}, RuntimeError, "search_compact runs on the HIP kernels: device tensors only$"),
    ("compact: gallery no tensor, filtered", _search_compact, lambda: (Q, None, 2), {"live": LIVE}, ValueError,
     r"search_compact: gallery must be a \[N, E\] tensor or a CompactGalleryIndex"),
    ("compact: one-sided id, bad fallback", _search_compact, lambda: (Q, G, 2), {"query_ids": QI, "fallback": "maybe"}, ValueError,
     "search_compact: ids on one side only - give query_ids and gallery_ids"),
    ("compact: bad live dtype", _search_compact, lambda: (Q, G, 2), {"live": torch.ones(5)}, ValueError, "search_compact: live must be"),
    ("compact: ids on the CPU", _search_compact, lambda: (Q, G, 2), {"query_ids": QI, "gallery_ids": GI}, RuntimeError,
     r"search_compact runs on the HIP kernels: device tensors only \(query_ids\)"),
    ("compact: bad fallback on the CPU", _search_compact, lambda: (Q, G, 2), {"fallback": "maybe"}, RuntimeError,
     "search_compact runs on the HIP kernels: device tensors only$"),
    ("compact: bad fallback, other E", _search_compact, lambda: (_fake(Q), _compact(coarse=_fake(Q), live=None, E=32), 2), {"fallback": "maybe"},
     ValueError, r"""search_compact: fallback = 'maybe' \("exact" or "none"\)"""),
    ("compact: other E, k above depth", _search_compact, lambda: (_fake(Q), _compact(coarse=_fake(Q), live=None, E=32), 9), {"depth": 8},
     AssertionError, r"torch\.Size\(\[3, 64\]\), 32"),
    ("compact: k above depth", _search_compact, lambda: (_fake(Q), _compact(coarse=_fake(Q), live=None), 9), {"depth": 8}, AssertionError,
     "k = 9, depth = 8: 1 <= k <= depth <= 32"),
    # ---- hard_negatives
    ("hard_negatives: no a_ids", _hard_negatives, lambda: (Q, G, None, GI, 2), {}, ValueError, "hard_negatives: a_ids is required"),
    ("hard_negatives: no b_ids", _hard_negatives, lambda: (Q, _index(), QI, None, 2), {}, ValueError, "hard_negatives: b_ids is required unless"),
    ("hard_negatives: k 40 on a compact index", _hard_negatives, lambda: (_fake(Q), _compact(coarse=_fake(Q), live=None), QI, GI, 40), {},
     RuntimeError, r"search_compact runs on the HIP kernels: device tensors only \(query_ids\)"),
    # ---- the two constructors: the same checks under the class's own name
    ("GalleryIndex: 1-d gallery", _gallery_index, lambda: (torch.zeros(64),), {}, ValueError, r"^GalleryIndex: gallery must be a \[N, E\] tensor"),
    ("GalleryIndex: on the CPU, bad ids", _gallery_index, lambda: (G,), {"ids": GI.int()}, RuntimeError,
     "^GalleryIndex runs on the HIP kernels: device tensors only$"),
    ("GalleryIndex: bad ids dtype", _gallery_index, lambda: (_fake(G),), {"ids": GI.int()}, ValueError, "^GalleryIndex: ids must be torch.int64, not torch.int32"),
    ("GalleryIndex: bad ids length", _gallery_index, lambda: (_fake(G),), {"ids": torch.arange(4)}, ValueError,
     r"^GalleryIndex: ids has shape \(4,\), expected \(5,\)"),
    ("GalleryIndex: ids on the CPU", _gallery_index, lambda: (_fake(G),), {"ids": GI}, RuntimeError,
     r"^GalleryIndex runs on the HIP kernels: device tensors only \(ids\)"),
    ("CompactGalleryIndex: 3-d gallery", _compact_index, lambda: (torch.zeros(5, 2, 64),), {}, ValueError,
     r"^CompactGalleryIndex: gallery must be a \[N, E\] tensor"),
    ("CompactGalleryIndex: on the CPU, bad ids", _compact_index, lambda: (G,), {"ids": GI.int()}, RuntimeError,
     "^CompactGalleryIndex runs on the HIP kernels: device tensors only$"),
    ("CompactGalleryIndex: bad ids dtype", _compact_index, lambda: (_fake(G),), {"ids": GI.float()}, ValueError,
     "^CompactGalleryIndex: ids must be torch.int64, not torch.float32"),
    ("CompactGalleryIndex: ids on the CPU", _compact_index, lambda: (_fake(G),), {"ids": GI}, RuntimeError,
     r"^CompactGalleryIndex runs on the HIP kernels: device tensors only \(ids\)"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_error_reported_and_its_precedence(case):
    _, call, args, kwargs, exception, pattern = case
    with pytest.raises(exception, match=pattern) as info:
        call(*args(), **kwargs)
    assert type(info.value) is exception                             # not a subclass: the type itself is part of the behaviour
