"""The region adjacency graph of a fragment image or volume on the device (include/pea_rag.h: pea_rag_build, pea_rag_project): what
the reference's utils/lmc.py computes with elf between the fragments and the multicut solver,

  rag        = feats.compute_rag(fragments)                                   the sorted unique pairs of touching fragments
  costs      = feats.compute_affinity_features(rag, 1 - affs, offsets)[:, 0]   the mean of (1 - a) over each pair's boundary
  edge_sizes = feats.compute_boundary_mean_and_length(rag, boundary)[:, 1]     the boundary length of each pair
  seg        = feats.project_node_labels_to_pixels(rag, node_labels)           seg[p] = node_labels[fragments[p]]

as eight launches of csrc/pea_k_rag.hip, none per edge; the stitched affinity volume stays on the device and a table of a few hundred
kilobytes comes back.  Every number is bit-reproducible (integer and fixed-point sums).  utils/lmc.py carries the reference's names.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..affinity_op import _on_device, _ptr, _stream, stream_workspace
from .segscore import default_capacity as _default_capacity, labels_int32

CAPACITY_CAP = 1 << 22  # of the default capacity: edges grow with the voxels, so the ceiling is higher than the score tables'


def default_capacity(S):
    """slots per image when the caller names none: the rule of harness/segscore.py -- the power of two at or above S / 32, at least
    256 -- with a ceiling of 2^22 (64 bytes and two words per slot and image).  The default max_edges is half of it.  A table that
    turns out too small is retried once at four times the size when the results are read (RegionAdjacency)."""
    return _default_capacity(S, CAPACITY_CAP)


def _workspace(dev, nb):
    return stream_workspace("rag", dev, nb, _lib.lib().pea_rag_workspace_init, "pea_rag_workspace_init")


def probs_to_costs(probs, beta=.5):
    """the reference's utils/mc_baselines.py:99-105: probabilities of a boundary -> multicut costs,
    log((1 - p') / p') + log((1 - beta) / beta) with p' = 0.998 p + 0.001, in float64"""
    p_min = 0.001
    p_max = 1. - p_min
    costs = (p_max - p_min) * np.asarray(probs, dtype=np.float64) + p_min
    return np.log((1. - costs) / costs) + np.log((1. - beta) / beta)


def transform_probabilities_to_costs(probs, beta=.5, edge_sizes=None, weighting_exponent=1.):
    """probs_to_costs, and with edge_sizes: costs *= (edge_sizes / edge_sizes.max()) ** weighting_exponent.  A constant factor in what
    is called an edge's size cancels in that quotient.  The weighting is elf's transform_probabilities_to_costs as its documentation
    states it; elf and nifty are installed neither where this was written nor where it is tested, so this line is not checked
    against them."""
    costs = probs_to_costs(probs, beta)
    if edge_sizes is not None:
        sizes = np.asarray(edge_sizes, dtype=np.float64)
        if sizes.shape != costs.shape:
            raise ValueError("edge_sizes %s and probs %s differ in shape" % (sizes.shape, costs.shape))
        if sizes.size:
            costs = costs * (sizes / sizes.max()) ** weighting_exponent
    return costs


def _rag_args(fragments, affs, offsets, boundary, batched):
    """shapes and dtypes, before any device is looked for -> (frag shape [B, Z, Y, X], ndim, K, offsets as K x 3)"""
    for x, name in ((fragments, "fragments"), (affs, "affs"), (boundary, "boundary")):
        if x is not None and not isinstance(x, (np.ndarray, torch.Tensor)):
            raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    if fragments is None:
        raise TypeError("fragments is required")
    shape = tuple(int(v) for v in fragments.shape)
    lead = 1 if batched else 0
    ndim = len(shape) - lead
    if ndim not in (2, 3):
        raise ValueError("fragments must be %s, got %s" % ("[B, Y, X] or [B, Z, Y, X]" if batched else "[Y, X] or [Z, Y, X]", shape))
    if min(shape) < 1:
        raise ValueError("fragments has an empty dimension: %s" % (shape,))
    B = shape[0] if batched else 1
    sp = shape[lead:]
    K, offs = 0, []
    if affs is not None:
        if offsets is None:
            raise ValueError("affs needs offsets: one (%s) per channel" % ("dz, dy, dx" if ndim == 3 else "dy, dx"))
        ashape = tuple(int(v) for v in affs.shape)
        if len(ashape) != len(shape) + 1 or ashape[lead + 1:] != sp or (batched and ashape[0] != B):
            raise ValueError("affs %s does not go with fragments %s: expected %s" % (ashape, shape, ("[B, K" if batched else "[K") + ", ...]"))
        K = ashape[lead]
        offs = [[int(v) for v in o] for o in offsets]
        if len(offs) != K or any(len(o) != ndim for o in offs):
            raise ValueError("offsets must hold %d offsets of %d steps each (one per channel of affs), got %r" % (K, ndim, offsets))
        if not 1 <= K <= _lib.RAG_MAX_K:
            raise ValueError("affs has %d channels: pea_rag_build takes 1 .. %d" % (K, _lib.RAG_MAX_K))
        offs = [[0] * (3 - ndim) + o for o in offs]
    elif offsets is not None:
        raise ValueError("offsets without affs")
    if boundary is not None and tuple(int(v) for v in boundary.shape) != shape:
        raise ValueError("boundary %s and fragments %s differ in shape" % (tuple(boundary.shape), shape))
    S = int(np.prod(sp))
    if S >= 2 ** 31:
        raise ValueError("an image of %d voxels: pea_rag_build serves fewer than 2^31 per image" % S)
    return (B,) + (1,) * (3 - ndim) + sp, ndim, K, offs


def _device_of(*xs):
    dev = None
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            if dev is not None and x.device != dev:
                raise RuntimeError("the arguments lie on %s and %s" % (dev, x.device))
            dev = x.device
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("region_adjacency runs on an MI355X only (no CPU fallback), and no GPU is visible")
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _f32_on(x, dev):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not x.dtype.is_floating_point:
        raise TypeError("affs and boundary must hold floating-point values, got %s" % x.dtype)
    x = x.detach().to(device=dev, dtype=torch.float32)
    return x if x.is_contiguous() else x.contiguous()


def _launch(F, A, Bd, shape4, ndim, K, offs, flags, max_id, capacity, max_edges, want_nodes=True):
    d = _lib.PeaRagDesc()
    d.ndim, d.B, d.K, d.max_id, d.capacity, d.max_edges, d.flags = ndim, shape4[0], K, int(max_id), int(capacity), int(max_edges), flags
    d.dims[:] = list(shape4[1:])
    for k, o in enumerate(offs):
        d.offsets[k][:] = o
    L = _lib.lib()
    rc = L.pea_rag_validate(ctypes.byref(d))
    if rc:
        raise ValueError("invalid region-adjacency descriptor (%s): shape %s, K=%d, max_id=%d, capacity=%d (a power of two >= %d), max_edges=%d"
                         % (L.pea_strerror(rc).decode(), shape4, K, d.max_id, d.capacity, _lib.RAG_MIN_CAPACITY, d.max_edges))
    dev = F.device
    B, E, M = d.B, int(max_edges), int(max_id) + 1
    with _on_device(dev):
        t = {"uv": torch.empty((B, E, 2), dtype=torch.int32, device=dev),
             "size": torch.empty((B, E), dtype=torch.int64, device=dev),
             "count": torch.empty((B, E), dtype=torch.int64, device=dev),
             "mean": torch.empty((B, E), dtype=torch.float64, device=dev),
             "bmean": torch.empty((B, E), dtype=torch.float64, device=dev),
             "min": torch.empty((B, E), dtype=torch.float32, device=dev),
             "max": torch.empty((B, E), dtype=torch.float32, device=dev),
             "node_size": torch.empty((B, M), dtype=torch.int64, device=dev) if want_nodes else None,
             "stats": torch.empty((B, _lib.RAG_STATS), dtype=torch.int64, device=dev)}
        io = _lib.PeaRagBuffers()
        io.fragments, io.affs, io.boundary = F.data_ptr(), (A.data_ptr() if A is not None else None), (Bd.data_ptr() if Bd is not None else None)
        for name, ten in t.items():
            setattr(io, name, ten.data_ptr() if ten is not None else None)
        nb = int(L.pea_rag_workspace_bytes(ctypes.byref(d)))
        work = _workspace(dev, nb)
        _lib.check(L.pea_rag_build(ctypes.byref(d), ctypes.byref(io), _ptr(work), nb, _stream()), "pea_rag_build")
    return t


class RegionAdjacency(object):
    """The device tables of one region_adjacency call.  Nothing is copied to the host until a value is asked for; `.tensors` holds the
    device tensors as pea_rag_build wrote them ([B, max_edges, ...], rows past the edge count zero; 'stats' [B, 8]).

    The properties copy once and give numpy arrays cut to the edge count -- for a single image the array, for batched=True a list
    over the batch: .uv int32 [n, 2] sorted by (u, v); .sizes, .counts int64 [n]; .mean, .boundary_mean float64 [n]; .min, .max
    float32 [n]; .node_sizes int64 [n_nodes]; .stats a dict of integers (a list of dicts); .n_nodes = max_id + 1; .n_edges.

    The first read checks stats: if the table or the edge rows overflowed and capacity and max_edges were the defaults, the call is
    repeated ONCE at four times both; an overflow of a size the caller named, or a second one, raises RuntimeError naming the
    parameter to enlarge."""

    def __init__(self, tensors, relaunch, n_nodes, capacity, max_edges, batched, defaults):
        self.tensors, self.n_nodes, self.capacity, self.max_edges = tensors, int(n_nodes), int(capacity), int(max_edges)
        self._relaunch, self._batched, self._defaults = relaunch, batched, defaults
        self._host = None

    def _rows(self):
        if self._host is None:
            stats = self.tensors["stats"].cpu().numpy()
            if self._defaults and (stats[:, 1:3] != 0).any():
                self.capacity, self.max_edges = 4 * self.capacity, 4 * self.max_edges
                self.tensors = self._relaunch(self.capacity, self.max_edges)
                stats = self.tensors["stats"].cpu().numpy()
            if (stats < 0).any():
                raise RuntimeError("pea_rag_build ran on a workspace that was never prepared")
            if (stats[:, 2] != 0).any():
                raise RuntimeError("the edge table overflowed at capacity %d (voxel pairs dropped per image: %s): pass a larger capacity"
                                   % (self.capacity, stats[:, 2].tolist()))
            if (stats[:, 1] != 0).any():
                raise RuntimeError("%s edges found but max_edges is %d: pass a larger max_edges" % (stats[:, 0].tolist(), self.max_edges))
            host = {k: v.cpu().numpy() for k, v in self.tensors.items() if v is not None and k != "stats"}
            host["stats"] = stats
            self._host = host
        return self._host

    def _per_image(self, name):
        h = self._rows()
        vals = [h[name][b, :int(h["stats"][b, 0])] for b in range(h["stats"].shape[0])]
        return vals if self._batched else vals[0]

    uv = property(lambda self: self._per_image("uv"))
    sizes = property(lambda self: self._per_image("size"))
    counts = property(lambda self: self._per_image("count"))
    mean = property(lambda self: self._per_image("mean"))
    min = property(lambda self: self._per_image("min"))
    max = property(lambda self: self._per_image("max"))
    boundary_mean = property(lambda self: self._per_image("bmean"))

    @property
    def n_edges(self):
        n = [int(v) for v in self._rows()["stats"][:, 0]]
        return n if self._batched else n[0]

    @property
    def node_sizes(self):
        h = self._rows()["node_size"]
        return list(h) if self._batched else h[0]

    @property
    def stats(self):
        s = self._rows()["stats"]
        out = [dict(zip(_lib.RAG_STAT_COLUMNS[:6], (int(v) for v in row[:6]))) for row in s]
        return out if self._batched else out[0]

    def costs(self, beta=0.5, weighting_exponent=1.0):
        """transform_probabilities_to_costs(mean, beta, edge_sizes=sizes, weighting_exponent): the multicut costs of the edges, float64
        (mean is the mean of 1 - a where the call had one_minus=True, as the reference's mc_baseline has it)"""
        m, s = self.mean, self.sizes
        if self._batched:
            return [transform_probabilities_to_costs(a, beta, b, weighting_exponent) for a, b in zip(m, s)]
        return transform_probabilities_to_costs(m, beta, s, weighting_exponent)

    def __repr__(self):
        return "RegionAdjacency(n_nodes=%d, capacity=%d, max_edges=%d)" % (self.n_nodes, self.capacity, self.max_edges)


def region_adjacency(fragments, affs=None, offsets=None, boundary=None, *, one_minus=False, ignore_zero=False, max_id=None, capacity=None,
                     max_edges=None, batched=False):
    """The region adjacency graph of a fragment image or volume with per-edge statistics -> RegionAdjacency.

    fragments    integer ids, [Y, X] or [Z, Y, X] (batched=True: [B, Y, X] or [B, Z, Y, X], every image on its own); a device tensor is
                 used as it is, a numpy array or CPU tensor is uploaded; int64 / uint64 are narrowed after one range check
                 (harness/segscore.py labels_int32: one host synchronisation for a device tensor of these dtypes).  Ids outside
                 0 .. max_id are no ids: their voxels take part in nothing (stats['no_id']).
    affs         [K, ...] ([B, K, ...]) floating point, with offsets: K offsets (dy, dx) / (dz, dy, dx), q = p + offset.  A sample on
                 a pair that is not an edge is skipped (stats['not_touching']), a non-finite one or |x| > 2^15 too (stats['skipped']).
                 A view that is not dense float32 is copied.
    boundary     the shape of fragments: every voxel pair (p, q) of an edge adds boundary[p] + boundary[q]; .boundary_mean
    one_minus    the sample is 1 - affs (float32, as numpy's 1 - affs)
    ignore_zero  id 0 is background and takes part in no edge (default: an ordinary node, as elf's compute_rag has it)
    max_id       the largest id.  None costs one fragments.max() round trip to the host; with max_id, capacity and max_edges all
                 given the call has no host synchronisation and can be captured with pea.graphed.
    capacity     table slots per image, a power of two >= 64; None: default_capacity(voxels per image)
    max_edges    rows of the edge outputs per image; None: half the capacity"""
    shape4, ndim, K, offs = _rag_args(fragments, affs, offsets, boundary, bool(batched))
    dev = _device_of(fragments, affs, boundary)
    F = labels_int32(fragments, "fragments", dev)
    A, Bd = _f32_on(affs, dev), _f32_on(boundary, dev)
    if max_id is None:
        max_id = max(0, int(F.max()))
    if not 0 <= int(max_id) <= 2 ** 31 - 2:
        raise ValueError("max_id must lie in 0 .. 2^31 - 2, got %r" % (max_id,))
    S = shape4[1] * shape4[2] * shape4[3]
    defaults = capacity is None and max_edges is None
    cap = default_capacity(S) if capacity is None else int(capacity)
    me = max(1, cap // 2) if max_edges is None else int(max_edges)
    flags = (_lib.RAG_ONE_MINUS if one_minus else 0) | (_lib.RAG_IGNORE_ZERO if ignore_zero else 0)

    def launch(c, e):
        return _launch(F, A, Bd, shape4, ndim, K, offs, flags, max_id, c, e)

    return RegionAdjacency(launch(cap, me), launch, int(max_id) + 1, cap, me, bool(batched), defaults)


def project_node_labels(fragments, node_labels, count_bad=False):
    """seg[p] = node_labels[fragments[p]] (elf's project_node_labels_to_pixels) as one streaming launch, int32 in and out: no int64
    index copy of the volume.  fragments: integer ids of any shape, tensor or numpy; node_labels: one integer label per node.  A voxel
    whose id is no node gives 0.  A numpy `fragments` gives a numpy array back, a tensor a device tensor.
    count_bad=True: -> (seg, n_bad) with n_bad a device int64 tensor [1], the voxels that had no node."""
    for x, name in ((fragments, "fragments"), (node_labels, "node_labels")):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    if len(node_labels.shape) != 1 or int(node_labels.shape[0]) < 1:
        raise ValueError("node_labels must be a vector of at least one label, got shape %s" % (tuple(node_labels.shape),))
    if int(np.prod(fragments.shape)) < 1:
        raise ValueError("fragments is empty: %s" % (tuple(fragments.shape),))
    as_numpy = isinstance(fragments, np.ndarray)
    dev = _device_of(fragments, node_labels)
    F, N = labels_int32(fragments, "fragments", dev), labels_int32(node_labels, "node_labels", dev)
    L = _lib.lib()
    with _on_device(dev):
        seg = torch.empty(F.shape, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev) if count_bad else None
        _lib.check(L.pea_rag_project(F.numel(), _ptr(F), _ptr(N), N.numel(), _ptr(seg), _ptr(bad), _stream()), "pea_rag_project")
    out = seg.cpu().numpy() if as_numpy else seg
    return (out, bad) if count_bad else out
