"""Hierarchical agglomeration of the fragment graph on the device (include/pea_agglo.h: pea_agglo_merge) -- the merge loop that the
reference's validation and inference loops run on the host with waterz,

  scripts_ac3ac4/main.py:316-324, scripts_ac3ac4/inference.py:211-220 -waterz    waterz.agglomerate(affs, [t], fragments=.., ..)
  scripts_cvppp/utils/seg_waterz.py, scripts_bbbc039v1/utils/seg_waterz.py       seg_waterz(affs, mask)

as launches of csrc/pea_k_agglo.hip between pea.region_adjacency and pea.project_node_labels: stitched affinities -> fragments ->
agglomerated segmentation -> scores never leave the device.  The result is defined by the header's round rule: where no two live edges
share a score it is the partition of "pop the cheapest edge, merge while below the threshold, rescore" (waterz without queue
discretisation); the tie rule among equal scores is this library's, not waterz's.  The number of rounds depends on
the data, so with rounds=None a call enqueues a batch of rounds, reads how many live edges are still below the threshold (one
synchronisation per batch) and resumes with a doubling batch until none is; with an explicit `rounds` nothing is read back, the call
can be captured with pea.graphed, and completeness is left in stats.  utils/seg_waterz.py carries the reference's names.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _on_device, _ptr, _stream
from .rag import RegionAdjacency, _device_of, project_node_labels, region_adjacency
from .segscore import labels_int32
from .ws import distance_transform_watershed

FIRST_BATCH = 32  # rounds of the first batch with rounds=None
WATERSHED = "watershed"
OFFSETS_3D = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
OFFSETS_2D = [[-1, 0], [0, -1]]
_RAG_VALUE = {"mean": "mean", "min": "min", "max": "max"}  # the column of the RAG that a linkage takes as its cost


class Agglomeration(object):
    """root    int32 [B, max_id + 1] ([max_id + 1] for one image): the smallest fragment id of every id's cluster (waterz's convention)
    labels  int32, the same shape: the clusters 1 .. n in ascending root id, 0 for an id that is not present: what
            pea.project_node_labels takes
    counts  int32 [B] (0-dim): n
    stats   int64 [B, 8] ([8]): the columns _lib.AGGLO_STAT_COLUMNS
    complete  no live edge is below the threshold (reads stats: one synchronisation)
    resume(threshold, rounds=None) -> Agglomeration: more rounds from where this one stands, at the same or a higher threshold"""

    def __init__(self, run, root, labels, counts, stats):
        self._run, self.root, self.labels, self.counts, self.stats = run, root, labels, counts, stats

    def __repr__(self):
        return "Agglomeration(ids=%d, threshold=%r)" % (self.root.shape[-1], self._run.threshold)

    def stat(self, name):
        return self.stats[..., _lib.AGGLO_STAT_COLUMNS.index(name)]

    @property
    def complete(self):
        s = self.stat("mergeable")
        if int(s.min()) < 0:
            raise _lib.PeaLibraryError("pea_agglo_merge refused the resumed call on the device: it does not go with the record in its workspace")
        return int(s.max()) == 0

    def resume(self, threshold, rounds=None):
        return self._run.call(threshold, rounds, True)


class _Run(object):
    """one graph on one private workspace: the descriptor, the buffers and the calls on them"""

    def __init__(self, uv, n_edges, n_stride, value, weight, node_size, max_id, linkage, ignore_zero, batched):
        dev = uv.device
        self.keep = (uv, n_edges, value, weight, node_size)
        self.dev, self.batched, self.threshold = dev, batched, None
        B, E = int(uv.shape[0]), int(uv.shape[1])
        d = self.d = _lib.PeaAggloDesc()
        d.B, d.max_id, d.max_edges, d.n_edges_stride, d.linkage = B, int(max_id), E, int(n_stride), _lib.AGGLO_LINKAGES[linkage]
        self.base_flags = _lib.AGGLO_IGNORE_ZERO if ignore_zero else 0
        L = self.L = _lib.lib()
        d.flags, d.rounds, d.threshold = self.base_flags, 0, 0.0
        rc = L.pea_agglo_validate(ctypes.byref(d))
        if rc:
            raise ValueError("invalid agglomeration descriptor (%s): B=%d, max_id=%d, max_edges=%d" % (L.pea_strerror(rc).decode(), B, d.max_id, E))
        self.nb = int(L.pea_agglo_workspace_bytes(ctypes.byref(d)))
        with _on_device(dev):
            self.work = torch.empty(self.nb // 8, dtype=torch.int64, device=dev)
        self.started = False

    def _once(self, threshold, rounds, resume):
        d, dev = self.d, self.dev
        B, N = d.B, d.max_id + 1
        d.threshold, d.rounds, d.flags = float(threshold), int(rounds), self.base_flags | (_lib.AGGLO_RESUME if resume else 0)
        uv, n_edges, value, weight, node_size = self.keep
        with _on_device(dev):
            out = {"root": torch.empty((B, N), dtype=torch.int32, device=dev), "labels": torch.empty((B, N), dtype=torch.int32, device=dev),
                   "counts": torch.empty((B,), dtype=torch.int32, device=dev), "stats": torch.empty((B, _lib.AGGLO_STATS), dtype=torch.int64, device=dev)}
            io = _lib.PeaAggloBuffers()
            io.uv, io.n_edges, io.value, io.weight = uv.data_ptr(), n_edges.data_ptr(), value.data_ptr(), (weight.data_ptr() if weight is not None else None)
            io.node_size = node_size.data_ptr() if node_size is not None else None
            for k, t in out.items():
                setattr(io, k, t.data_ptr())
            _lib.check(self.L.pea_agglo_merge(ctypes.byref(d), ctypes.byref(io), _ptr(self.work), self.nb, _stream()), "pea_agglo_merge")
        self.started = True
        return out

    def call(self, threshold, rounds, resume):
        threshold = float(np.float32(threshold))
        if threshold != threshold:
            raise ValueError("threshold is a NaN")
        if resume and not self.started:
            raise ValueError("nothing to resume")
        if resume and threshold < self.threshold:
            raise ValueError("a resumed call may not lower the threshold: %r after %r" % (threshold, self.threshold))
        if rounds is not None and not 0 <= int(rounds) <= _lib.AGGLO_MAX_ROUNDS:
            raise ValueError("rounds must be None or lie in 0 .. %d, got %r" % (_lib.AGGLO_MAX_ROUNDS, rounds))
        self.threshold = threshold
        if rounds is not None:
            out = self._once(threshold, rounds, resume)
        else:
            cap = self.d.max_id + 1  # a round that can merge does merge: more rounds than ids cannot be needed
            batch, done = FIRST_BATCH, 0
            while True:
                n = min(batch, _lib.AGGLO_MAX_ROUNDS)
                out = self._once(threshold, n, resume)
                done += n
                left = out["stats"][:, 2]
                if int(left.min()) < 0:  # (the one synchronisation of the batch)
                    raise _lib.PeaLibraryError("pea_agglo_merge refused the resumed call on the device")
                if int(left.max()) == 0:
                    break
                if done > cap + FIRST_BATCH:
                    raise _lib.PeaLibraryError("the agglomeration is not complete after %d rounds on %d ids" % (done, cap))
                resume, batch = True, batch * 2
        t = out if self.batched else {k: v[0] for k, v in out.items()}
        return Agglomeration(self, t["root"], t["labels"], t["counts"], t["stats"])


def _rag_edge_count(rag):
    """the largest edge count of a RegionAdjacency's images from its stats alone: 64 bytes per image come to the host, the tables stay
    on the device.  Only a RAG whose table or rows overflowed goes through its own reader, which rebuilds a default-sized one once at
    four times the size and raises for a size that the caller named"""
    stats = rag.tensors["stats"].cpu()
    if bool((stats < 0).any()) or bool((stats[:, 1:3] != 0).any()):
        n = rag.n_edges
        return max(n) if rag._batched else n
    return int(stats[:, 0].max())


def _check_common(linkage, thresholds=None):
    if linkage not in _lib.AGGLO_LINKAGES:
        raise ValueError("linkage must be one of %s, got %r" % (sorted(_lib.AGGLO_LINKAGES), linkage))
    if thresholds is not None:
        ts = [float(t) for t in thresholds]
        if not ts:
            raise ValueError("thresholds is empty")
        if any(t != t for t in ts) or any(b < a for a, b in zip(ts, ts[1:])):
            raise ValueError("thresholds must be ascending (merges below a threshold are a prefix of those below a higher one), got %r" % (ts,))
        return ts
    return None


def _graph_tensors(x, dtype, dev, name):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    x = x.detach().to(device=dev, dtype=dtype)
    return x if x.is_contiguous() else x.contiguous()


def agglomerate_graph(rag_or_uv, value=None, weight=None, *, threshold, linkage="mean", n_edges=None, max_id=None, node_size=None,
                      ignore_zero=False, rounds=None, batched=False):
    """Agglomerate a weighted graph -> Agglomeration (root, labels, counts, stats), all on the device.

    rag_or_uv  a pea.RegionAdjacency (its device tables are used as they are: uv, the edge counts in its stats, node_size, and as
               the cost its mean / min / max column by linkage, weighted by its sample count), or uv: integer [E, 2] ([B, E, 2] with
               batched=True), u < v
    value      float [E] ([B, E]): the cost of every row;  weight  integer [E]: the samples behind it (linkage="mean" only)
    threshold  a pair merges only while its score is strictly below it
    linkage    "mean" (the weighted mean of the parts), "min" (single linkage), "max" (complete linkage)
    n_edges    how many rows of every image count (None: all), an integer, a list or an int64 tensor [B]
    max_id     the largest id (None: uv.max(), one round trip to the host)
    node_size  int64 [max_id + 1]: ids of size 0 get label 0 and are not counted
    rounds     None: run to completion (a synchronisation per batch of rounds); an integer: enqueue exactly that many rounds and
               return without reading anything back -- stats[..., 2] > 0 then says that the partition is a refinement of the final one"""
    _check_common(linkage)
    if isinstance(rag_or_uv, RegionAdjacency):
        rag = rag_or_uv
        if value is not None or weight is not None:
            raise ValueError("a RegionAdjacency brings its own values and weights")
        rows = None
        if rounds is None:
            rows = max(1, _rag_edge_count(rag))
        t = rag.tensors
        stats = t["stats"]
        uv, val, cnt = t["uv"], t[_RAG_VALUE[linkage]], t["count"]
        if rows is not None and rows < int(uv.shape[1]):  # the rows that hold edges, dense: the tables are sized from the rows
            uv, val, cnt = uv[:, :rows].contiguous(), val[:, :rows].contiguous(), cnt[:, :rows].contiguous()
        val = val if val.dtype == torch.float64 else val.to(torch.float64)
        run = _Run(uv, stats, _lib.RAG_STATS, val, cnt, t["node_size"], rag.n_nodes - 1, linkage, ignore_zero, True)
        run.batched = rag._batched
        return run.call(threshold, rounds, False)
    if value is None:
        raise TypeError("value is required with a uv table")
    if linkage == "mean" and weight is None:
        raise TypeError("linkage='mean' needs the weight of every row")
    dev = _device_of(rag_or_uv, value, weight)
    uv = _graph_tensors(rag_or_uv, torch.int32, dev, "uv")
    want = 3 if batched else 2
    if uv.dim() != want or int(uv.shape[-1]) != 2 or int(uv.shape[-2]) < 1:
        raise ValueError("uv must be %s with E >= 1, got %s" % ("[B, E, 2]" if batched else "[E, 2]", tuple(uv.shape)))
    uv = uv if batched else uv[None]
    B, E = int(uv.shape[0]), int(uv.shape[1])
    val = _graph_tensors(value, torch.float64, dev, "value")
    wt = _graph_tensors(weight, torch.int64, dev, "weight")
    for x, name in ((val, "value"), (wt, "weight")):
        if x is not None and tuple(x.shape) != tuple(uv.shape[1:-1] if not batched else uv.shape[:-1]):
            raise ValueError("%s %s does not go with uv %s" % (name, tuple(x.shape), tuple(uv.shape)))
    val = val.reshape(B, E)
    wt = None if wt is None else wt.reshape(B, E)
    if max_id is None:
        max_id = max(0, int(uv.max()))
    if n_edges is None:
        n_edges = E
    if isinstance(n_edges, (int, np.integer)):
        n_edges = [int(n_edges)] * B
    ne = _graph_tensors(n_edges if isinstance(n_edges, torch.Tensor) else np.asarray(n_edges, np.int64), torch.int64, dev, "n_edges").reshape(-1)
    if int(ne.numel()) != B:
        raise ValueError("n_edges must hold one count per image, got %d for %d" % (int(ne.numel()), B))
    ns = _graph_tensors(node_size, torch.int64, dev, "node_size")
    if ns is not None:
        ns = ns.reshape(B, -1)
        if int(ns.shape[1]) != int(max_id) + 1:
            raise ValueError("node_size must hold max_id + 1 = %d sizes per image, got %d" % (int(max_id) + 1, int(ns.shape[1])))
    run = _Run(uv, ne, 1, val, wt, ns, max_id, linkage, ignore_zero, bool(batched))
    return run.call(threshold, rounds, False)


def _prepare(affs, fragments, offsets):
    """arguments first, then the device -> (affs float32 [K, ...] on the device, fragments int32, offsets, came as numpy)"""
    if not isinstance(affs, (np.ndarray, torch.Tensor)):
        raise TypeError("affs must be a numpy array or a torch.Tensor, got %s" % type(affs).__name__)
    ndim = len(affs.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("affs must be [K, Y, X] or [K, Z, Y, X], got %s" % (tuple(affs.shape),))
    if fragments is None:
        raise TypeError("fragments is required: a label image, or fragments=\"watershed\" for the distance-transform watershed on the device")
    made = isinstance(fragments, str)
    if made and fragments != WATERSHED:
        raise ValueError("fragments=%r: the only named way to make them is %r" % (fragments, WATERSHED))
    if not made:
        if not isinstance(fragments, (np.ndarray, torch.Tensor)):
            raise TypeError("fragments must be a numpy array, a torch.Tensor or %r" % WATERSHED)
        if tuple(fragments.shape) != tuple(affs.shape[1:]):
            raise ValueError("fragments %s does not go with affs %s" % (tuple(fragments.shape), tuple(affs.shape)))
    offs = (OFFSETS_3D if ndim == 3 else OFFSETS_2D) if offsets is None else [[int(v) for v in o] for o in offsets][:ndim]
    if int(affs.shape[0]) < ndim or len(offs) != ndim or any(len(o) != ndim for o in offs):
        raise ValueError("the agglomeration takes the %d local channels of affs with one offset of %d steps each, got %s and %r"
                         % (ndim, ndim, tuple(affs.shape), offsets))
    as_numpy = isinstance(affs, np.ndarray)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("the agglomeration runs on an MI355X only (no CPU fallback), and no GPU is visible")
        affs = torch.from_numpy(np.ascontiguousarray(affs[:ndim], dtype=np.float32)).cuda()
    elif not affs.is_cuda:
        raise RuntimeError("affs is on %s: the agglomeration runs on an MI355X only (no CPU fallback)" % affs.device)
    affs = affs.detach().to(torch.float32)
    if made:
        i, j = (1, 2) if ndim == 3 else (0, 1)  # the reference's boundary map (utils/lmc.py)
        frag = distance_transform_watershed(torch.maximum(1 - affs[i], 1 - affs[j]).contiguous(), .25, 2.)[0]
    else:
        frag = labels_int32(fragments, "fragments", affs.device)
    return affs[:ndim].contiguous(), frag, offs, as_numpy


def agglomerate(affs, thresholds, fragments=None, linkage="mean", offsets=None, rounds=None, max_id=None, capacity=None, max_edges=None):
    """waterz.agglomerate on the device: yields one segmentation (int32, ids 1 .. n in ascending order of the clusters' smallest
    fragment id, 0 where the fragments are 0) per threshold, served from ONE run resumed at every next threshold.

    affs        [K >= 3, Z, Y, X] ([K >= 2, Y, X]), tensor or numpy (then numpy comes back): the first three (two) channels are the
                local ones, offsets (-1, 0, 0), (0, -1, 0), (0, 0, -1) unless `offsets` names others
    thresholds  ascending; the cost of an edge is 1 - a over its boundary samples (mean, min or max by linkage)
    fragments   a label image of the spatial shape, 0 = background; "watershed": made on the device as utils/lmc.py makes them
    rounds      None: every threshold runs to completion; an integer: that many rounds per threshold and no synchronisation (with
                max_id, capacity and max_edges named, usable under pea.graphed)"""
    ts = _check_common(linkage, thresholds)
    a, frag, offs, as_numpy = _prepare(affs, fragments, offsets)

    def gen():
        rag = region_adjacency(frag, a, offs, one_minus=True, ignore_zero=True, max_id=max_id, capacity=capacity, max_edges=max_edges)
        out = None
        for t in ts:
            out = agglomerate_graph(rag, threshold=t, linkage=linkage, ignore_zero=True, rounds=rounds) if out is None else out.resume(t, rounds)
            seg = project_node_labels(frag, out.labels)
            yield seg.cpu().numpy() if as_numpy else seg

    return gen()
