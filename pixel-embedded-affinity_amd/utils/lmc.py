"""The reference's utils/lmc.py (scripts_ac3ac4/, scripts_cvppp/, scripts_bbbc039v1/) under its own names: mc_baseline and
multicut_multi, with everything between the fragments and the solver, and the projection after it, on the device (harness/rag.py,
include/pea_rag.h).  The affinity volume is read where the stitcher left it; what goes to the host is the edge table.

What stays the caller's, on the host:
  * the fragments, unless fragments="watershed" asks for them.  The reference makes them per plane with elf's
    distance_transform_watershed when none are given; here `fragments` is required, and the string "watershed" makes them on the
    device with the reference's parameters (threshold=.25, sigma_seeds=2.: harness/ws.py distance_transform_watershed on the boundary
    map, ids stacked plane by plane), so the chain stitcher -> boundary map -> fragments -> RAG -> costs never leaves the device.
  * the solver.  `solver` is a callable (n_nodes, uvs, costs) -> node_labels, which is the signature of the reference's
    utils/mc_baselines.py multicut(n_nodes, uvs, costs).  The default builds exactly that from nifty (UndirectedGraph, insertEdges,
    multicutObjective, kernighanLinFactory(warmStartGreedy=True)) and raises where nifty is not installed.
"""
import numpy as np
import torch

from ..harness.segscore import labels_int32
from ..harness.rag import probs_to_costs, project_node_labels, region_adjacency, transform_probabilities_to_costs
from ..harness.ws import distance_transform_watershed

__all__ = ["mc_baseline", "multicut_multi", "probs_to_costs", "transform_probabilities_to_costs", "boundary_map", "nifty_multicut"]

OFFSETS_3D = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
OFFSETS_2D = [[-1, 0], [0, -1]]
WATERSHED = "watershed"  # fragments=WATERSHED: make them on the device as the reference does when none are given


def nifty_multicut(n_nodes, uvs, costs):
    """the reference's mc_baselines.multicut(n_nodes, uvs, costs) without a time limit: Kernighan-Lin, warm-started greedily"""
    try:
        import nifty
        import nifty.graph.opt.multicut as nmc
    except ImportError as ex:
        raise ImportError("the default multicut solver needs nifty, which is not installed (%s): pass solver=, a callable "
                          "(n_nodes, uvs, costs) -> node_labels" % ex)
    graph = nifty.graph.UndirectedGraph(n_nodes)
    graph.insertEdges(uvs)
    obj = nmc.multicutObjective(graph, costs)
    return obj.kernighanLinFactory(warmStartGreedy=True).create(obj).optimize()


def _check(affs, offsets, fragments):
    """-> ndim; argument errors before any device is looked for"""
    if fragments is None:
        raise TypeError("fragments is required: pass a label image, or fragments=\"watershed\" for the reference's distance-transform "
                        "watershed (threshold=.25, sigma_seeds=2.) on the device")
    made = isinstance(fragments, str)
    if made and fragments != WATERSHED:
        raise ValueError("fragments=%r: the only named way to make them is %r" % (fragments, WATERSHED))
    for x, name in ((affs, "affs"),) + (() if made else ((fragments, "fragments"),)):
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise TypeError("%s must be a numpy array or a torch.Tensor, got %s" % (name, type(x).__name__))
    if made:  # the fragments will have the spatial shape of affs
        ndim = len(affs.shape) - 1
        if ndim not in (2, 3):
            raise ValueError("affs must be [K, Y, X] or [K, Z, Y, X] to make the fragments, got %s" % (tuple(affs.shape),))
        if len(offsets) != int(affs.shape[0]) or any(len(o) != ndim for o in offsets):
            raise ValueError("affs has %d channels and needs as many offsets of %d steps, got %r" % (int(affs.shape[0]), ndim, offsets))
        if int(affs.shape[0]) < ndim:
            raise ValueError("the boundary map needs the in-plane channels %s of affs, which has %d" % (boundary_channels(ndim), int(affs.shape[0])))
        return ndim
    ndim = len(fragments.shape)
    if ndim not in (2, 3):
        raise ValueError("fragments must be [Y, X] or [Z, Y, X], got %s" % (tuple(fragments.shape),))
    if len(affs.shape) != ndim + 1 or tuple(affs.shape[1:]) != tuple(fragments.shape):
        raise ValueError("affs %s does not go with fragments %s: expected [K, ...]" % (tuple(affs.shape), tuple(fragments.shape)))
    if len(offsets) != int(affs.shape[0]) or any(len(o) != ndim for o in offsets):
        raise ValueError("affs has %d channels and needs as many offsets of %d steps, got %r" % (int(affs.shape[0]), ndim, offsets))
    if int(affs.shape[0]) < ndim:
        raise ValueError("the boundary map needs the in-plane channels %s of affs, which has %d" % (boundary_channels(ndim), int(affs.shape[0])))
    return ndim


def boundary_channels(ndim):
    """the two channels the reference's boundary map is taken from: 1, 2 of a volume (y and x), 0, 1 of an image"""
    return (1, 2) if ndim == 3 else (0, 1)


def boundary_map(affs):
    """np.maximum((1 - affs)[i], (1 - affs)[j]) with (i, j) = boundary_channels: the reference's boundary_input, tensor or numpy in
    and the same kind out"""
    i, j = boundary_channels(len(affs.shape) - 1)
    if isinstance(affs, np.ndarray):
        return np.maximum(1 - affs[i], 1 - affs[j])
    return torch.maximum(1 - affs[i], 1 - affs[j])


def _multicut(affs, offsets, fragments, solver):
    _check(affs, offsets, fragments)
    made = isinstance(fragments, str)
    as_numpy = isinstance(affs if made else fragments, np.ndarray)
    if isinstance(affs, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("mc_baseline runs on an MI355X only (no CPU fallback), and no GPU is visible")
        affs = torch.from_numpy(np.ascontiguousarray(affs)).cuda()
    affs = affs.detach().to(torch.float32)
    if made:
        frag = distance_transform_watershed(boundary_map(affs).contiguous(), .25, 2.)[0]
    else:
        frag = labels_int32(fragments, "fragments", affs.device)
    rag = region_adjacency(frag, affs, offsets, boundary_map(affs), one_minus=True)
    costs = rag.costs()
    node_labels = (solver or nifty_multicut)(rag.n_nodes, rag.uv, costs)
    node_labels = np.asarray(node_labels)
    if node_labels.shape != (rag.n_nodes,):
        raise ValueError("the solver returned %s labels for %d nodes" % (node_labels.shape, rag.n_nodes))
    seg = project_node_labels(frag, node_labels)
    return seg.cpu().numpy() if as_numpy else seg


def _ndim(affs, fragments):
    """the spatial dimensions of the call: those of the fragments, of affs where the fragments are still to be made"""
    if isinstance(fragments, str):
        return len(getattr(affs, "shape", ())) - 1
    return len(getattr(fragments, "shape", ())) if fragments is not None else 0


def mc_baseline(affs, fragments=None, solver=None):
    """The reference's mc_baseline: affs [3, Z, Y, X] with the offsets (-1, 0, 0), (0, -1, 0), (0, 0, -1) ([2, Y, X] with (-1, 0),
    (0, -1)), tensor or numpy, and fragments of the spatial shape (or "watershed": made on the device) -> the segmentation, int32 (a
    numpy array where fragments -- affs, with "watershed" -- was one, else a device tensor).  The costs are transform_probabilities_to_costs(mean of 1 - a over each edge, edge_sizes = its boundary
    length); solver(n_nodes, uvs, costs) -> node_labels runs on the host."""
    ndim = _ndim(affs, fragments)
    return _multicut(affs, OFFSETS_3D if ndim == 3 else OFFSETS_2D, fragments, solver)


def multicut_multi(affs, offsets=None, fragments=None, solver=None):
    """The reference's multicut_multi: mc_baseline with the offsets of the caller (default: mc_baseline's), one per channel and of any
    reach -- a long-range sample on a pair of fragments that do not touch is left out, as elf's compute_affinity_features leaves it
    out."""
    ndim = _ndim(affs, fragments)
    if offsets is None:
        offsets = OFFSETS_3D if ndim == 3 else OFFSETS_2D
    return _multicut(affs, offsets, fragments, solver)
