"""ctypes binding of libpea_hip.so (the C ABI declared in include/pea.h).

The library is the product: there is NO CPU fallback.  If the shared object is missing or cannot be
loaded, every op raises PeaLibraryError loudly.  `build()` compiles it in-tree with hipcc for gfx950
(cross-compiles without a GPU), so the .so travels with the repository snapshot.
"""
import ctypes
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO_PATH = os.environ.get("PEA_HIP_LIB") or os.path.join(CSRC, "libpea_hip.so")  # PEA_HIP_LIB: debugging override
HEADER = os.path.join(HERE, "..", "include", "pea.h")
HEADER_INFER = os.path.join(HERE, "..", "include", "pea_infer.h")
HEADER_MULTI = os.path.join(HERE, "..", "include", "pea_multi.h")
HEADER_FLIP = os.path.join(HERE, "..", "include", "pea_flip.h")
HEADER_MULTI_LABELS = os.path.join(HERE, "..", "include", "pea_multi_labels.h")
HEADER_HEAD16 = os.path.join(HERE, "..", "include", "pea_head16.h")
HEADER_METRICS = os.path.join(HERE, "..", "include", "pea_metrics.h")
HEADER_FGMASK = os.path.join(HERE, "..", "include", "pea_fgmask.h")
HEADER_DISC = os.path.join(HERE, "..", "include", "pea_disc.h")
HEADER_CROP = os.path.join(HERE, "..", "include", "pea_crop.h")
HEADER_DIST = os.path.join(HERE, "..", "include", "pea_dist.h")
HEADER_SEGSCORE = os.path.join(HERE, "..", "include", "pea_segscore.h")
HEADER_INSTSCORE = os.path.join(HERE, "..", "include", "pea_instscore.h")
HEADER_CC = os.path.join(HERE, "..", "include", "pea_cc.h")
HEADER_RAG = os.path.join(HERE, "..", "include", "pea_rag.h")
HEADER_WS = os.path.join(HERE, "..", "include", "pea_ws.h")
HEADER_MWS = os.path.join(HERE, "..", "include", "pea_mws.h")
HEADER_AGGLO = os.path.join(HERE, "..", "include", "pea_agglo.h")
HEADER_MERGE = os.path.join(HERE, "..", "include", "pea_merge.h")

PEA_ABI_VERSION = 2
PEA_MAX_K = 32
PEA_MULTI_MAX_N, PEA_MULTI_MAX_K = 4, 12  # include/pea_multi.h
E_UNSUPPORTED = -3
BORDER_CIRCULAR, BORDER_CROP_ZERO, BORDER_REPLICATE = 0, 1, 2
F32, F16, BF16 = 0, 1, 2
NORM_BX, NORM_CROPPED, NORM_FULL = 0, 1, 2
FLAG_RELU_AFFS, FLAG_ONE_MINUS, FLAG_HALF_SHIFT, FLAG_CLAMP01, FLAG_ACCUMULATE_DE = 1, 2, 4, 8, 16  # activation of the affs output (include/pea.h)
FLAG_MASK_F32 = 32  # the mask of the training forwards holds f32 values (include/pea.h PEA_FLAG_MASK_F32)
FLAG_LOSS_ACT = 64  # the loss of the training forwards is taken on the activated map (include/pea.h PEA_FLAG_LOSS_ACT)
FLAG_LOSS_BCE = 128  # with FLAG_LOSS_ACT | FLAG_CLAMP01: that loss is the weighted binary cross-entropy (include/pea.h PEA_FLAG_LOSS_BCE)
RULES_U8, RULES_I32, RULES_I64, RULES_F32 = 0, 1, 2, 3  # element type of the rules table (include/pea_flip.h PEA_RULES_*)
TGT_PADDING, TGT_BOTH_FOREGROUND, TGT_MASK_INSIDE, TGT_ACCUMULATE = 1, 2, 4, 8
METRICS_COLS = 5  # mse, bce, tp, fp, fn (include/pea_metrics.h PEA_METRICS_COLS)
MET_RELU, MET_DIVIDE, MET_STORE, MET_MASK_F32 = 1, 2, 4, 8  # include/pea_metrics.h PEA_MET_*
FG_LABELS_I32, FG_LABELS_U8 = 0, 1  # element type of the label image (include/pea_fgmask.h PEA_FG_LABELS_*)
FG_SKIP_EMPTY_CLASS = 1  # include/pea_fgmask.h PEA_FG_SKIP_EMPTY_CLASS
FG_STATS = 5  # loss, S0 / n0, S1 / n1, n0, n1 (include/pea_fgmask.h PEA_FG_STATS)
DISC_MAX_IDS, DISC_MAX_D = 4096, 64  # include/pea_disc.h PEA_DISC_MAX_IDS, PEA_DISC_MAX_D
DISC_BACKGROUND, DISC_NEED_GRAD = 1, 2  # include/pea_disc.h PEA_DISC_*
DIST_MAX_D = 64  # include/pea_dist.h PEA_DIST_MAX_D
DIST_BORDER_ZERO_VECTOR = 3  # include/pea_dist.h: a value of PeaDistDesc.border beside BORDER_REPLICATE
DIST_INVERT = 1  # include/pea_dist.h PEA_DIST_INVERT
SEG_MIN_CAPACITY, SEG_COLS = 64, 19  # include/pea_segscore.h PEA_SEG_MIN_CAPACITY, PEA_SEG_COLS
# the columns of pea_seg_scores' out [B][SEG_COLS] in order (include/pea_segscore.h PEA_SEG_<NAME>)
SEG_COLUMNS = ("n_overflow", "n_bad", "best_dice", "best_dice_rev", "sbd", "diff_fg", "fgbg_dice", "voi_split", "voi_merge", "are",
               "are_precision", "are_recall", "sum_nij2", "sum_ai2", "sum_bj2", "n_prime", "n_pred_ids", "n_gt_ids", "n_pairs")
INST_MIN_CAPACITY, INST_MAX_ID, INST_COLS = 64, 65535, 18  # include/pea_instscore.h PEA_INST_MIN_CAPACITY, PEA_INST_MAX_ID, PEA_INST_COLS
# the columns of pea_inst_scores' out [B][INST_COLS] in order (include/pea_instscore.h PEA_INST_<NAME>)
INST_COLUMNS = ("n_overflow", "n_bad", "aji", "aji_inter", "aji_union", "dq", "sq", "pq", "tp", "fp", "fn", "sum_iou", "pixel_f1", "pix_tp",
                "pix_fp", "pix_fn", "n_pred_ids", "n_gt_ids")
CC_IN_U8, CC_IN_I32 = 0, 1  # element type of the input of pea_cc_label (include/pea_cc.h PEA_CC_IN_*)
RAG_ONE_MINUS, RAG_IGNORE_ZERO = 1, 2  # include/pea_rag.h PEA_RAG_ONE_MINUS, PEA_RAG_IGNORE_ZERO
RAG_MAX_K, RAG_MIN_CAPACITY, RAG_STATS = 32, 64, 8  # include/pea_rag.h PEA_RAG_MAX_K, PEA_RAG_MIN_CAPACITY, PEA_RAG_STATS
# the columns of pea_rag_build's stats [B][RAG_STATS] in order (include/pea_rag.h PEA_RAG_N_<NAME>)
RAG_STAT_COLUMNS = ("edges", "edges_dropped", "pairs_dropped", "no_id", "not_touching", "skipped", "reserved0", "reserved1")
WS_STACK_IDS, WS_FIELD, WS_MAX_RADIUS = 1, 2, 32  # include/pea_ws.h PEA_WS_STACK_IDS, PEA_WS_FIELD, PEA_WS_MAX_RADIUS
MWS_MAX_K, MWS_MAX_ROUNDS, MWS_RESUME, MWS_STATS = 32, 65536, 1, 8  # include/pea_mws.h PEA_MWS_MAX_K, PEA_MWS_MAX_ROUNDS, PEA_MWS_RESUME, PEA_MWS_STATS
MWS_INPUTS = {"affs": 0, "elf": 1, "weights": 2}  # include/pea_mws.h PEA_MWS_IN_AFFS, PEA_MWS_IN_ELF, PEA_MWS_IN_WEIGHTS
# the columns of pea_mws_segment's stats [B][MWS_STATS] in order (include/pea_mws.h PEA_MWS_<NAME>)
MWS_STAT_COLUMNS = ("rounds", "undecided", "merges", "exclusions", "missing_stride", "missing_mask", "missing_nan", "missing_outside")
AGGLO_RESUME, AGGLO_IGNORE_ZERO = 1, 2  # include/pea_agglo.h PEA_AGGLO_RESUME, PEA_AGGLO_IGNORE_ZERO
AGGLO_LINKAGES = {"mean": 0, "min": 1, "max": 2}  # include/pea_agglo.h PEA_AGGLO_MEAN, PEA_AGGLO_MIN, PEA_AGGLO_MAX
AGGLO_MAX_ROUNDS, AGGLO_MAX_EDGES, AGGLO_STATS = 65536, 1 << 30, 8  # include/pea_agglo.h PEA_AGGLO_MAX_ROUNDS, PEA_AGGLO_MAX_EDGES, PEA_AGGLO_STATS
# the columns of pea_agglo_merge's stats [B][AGGLO_STATS] in order (include/pea_agglo.h PEA_AGGLO_<NAME>)
AGGLO_STAT_COLUMNS = ("rounds", "live", "mergeable", "merges", "clusters", "no_edge", "bad_value", "reserved")
MERGE_RELABEL, MERGE_MAX_PASSES, MERGE_MAX_WINDOW, MERGE_STATS = 1, 8, 45, 8  # include/pea_merge.h PEA_MERGE_RELABEL, PEA_MERGE_MAX_PASSES, PEA_MERGE_MAX_WINDOW, PEA_MERGE_STATS
# the columns of pea_merge_small's stats [B][MERGE_STATS] in order (include/pea_merge.h PEA_MERGE_<NAME>)
MERGE_STAT_COLUMNS = ("candidates", "merges", "negative", "few", "out_of_range", "chain", "reserved", "reserved")
DISC_STATS = 5  # loss, var, dist, reg, n_bad; then var_b, dist_b, reg_b, C_b per image (include/pea_disc.h PEA_DISC_STATS)

EXPORTS = ("pea_version", "pea_strerror", "pea_desc_validate", "pea_workspace_bytes", "pea_workspace_init", "pea_reload_env",
           "pea_affinity_infer", "pea_affinity_fwd", "pea_affinity_bwd", "pea_affinity_fwd_ex", "pea_affinity_bwd_ex", "pea_affinity_bwd_ex2", "pea_inv_norm",
           "pea_cross_supported", "pea_affinity_bwd_dual", "pea_affinity_bwd_dual_ex", "pea_affinity_fwd_dual_ex", "pea_scale_inplace", "pea_scale_inplace_multi", "pea_weighted_sum",
           "pea_fill_border_relu", "pea_head_workspace_bytes", "pea_head_fwd", "pea_head_bwd",
           "pea_targets_workspace_bytes", "pea_gen_targets", "pea_stitch_add", "pea_stitch_finalize",
           "pea_label_weights", "pea_affinity_fwd_bwd_labels", "pea_affinity_fwd_bwd_labels_ex", "pea_labels_scratch_bytes",
           "pea_affinity_fwd_bwd_labels_dual")
# the entry points of include/pea_infer.h (the fused 3D window inference); include/pea.h and EXPORTS stay as they are
EXPORTS_INFER = ("pea_infer_stitch_supported", "pea_affinity_infer_stitch")
# the entry points of include/pea_multi.h (up to four self losses per launch: the deep-supervision scales)
EXPORTS_MULTI = ("pea_multi_supported", "pea_affinity_fwd_multi", "pea_affinity_bwd_multi")
# the entry point of include/pea_flip.h (the per-sample un-flip of the EMA embedding, rules read on the device)
EXPORTS_FLIP = ("pea_consistency_unflip",)
# the entry points of include/pea_multi_labels.h (up to four self losses per launch straight from label images)
EXPORTS_MULTI_LABELS = ("pea_multi_labels_supported", "pea_multi_labels_scratch_bytes", "pea_affinity_fwd_bwd_labels_multi")
# the entry points of include/pea_head16.h (the embedding head on f16 / bf16 features)
EXPORTS_HEAD16 = ("pea_head_supported_t", "pea_head_fwd_t", "pea_head_bwd_t")
# the entry points of include/pea_metrics.h (the validation pixel metrics: MSE, BCE and the F1 counts in one data launch)
EXPORTS_METRICS = ("pea_metrics_validate", "pea_metrics_workspace_bytes", "pea_affs_metrics")
# the entry points of include/pea_fgmask.h (the foreground-mask loss of the BBBC039V1 step and the validation mask)
EXPORTS_FGMASK = ("pea_fgmask_validate", "pea_fgmask_workspace_bytes", "pea_fgmask_loss_fwd", "pea_fgmask_loss_bwd", "pea_fgmask_argmax")
# the entry points of include/pea_disc.h (the discriminative instance loss: segment means by label)
EXPORTS_DISC = ("pea_disc_validate", "pea_disc_workspace_bytes", "pea_disc_workspace_init", "pea_disc_context_bytes", "pea_disc_loss_fwd",
                "pea_disc_loss_bwd")
# the entry point of include/pea_crop.h (the reference's 3D border rule on an activated map: 0 where the pair does not exist)
EXPORTS_CROP = ("pea_affs_crop_zero",)
# the entry points of include/pea_dist.h (distance-form affinities of the raw embedding: forward and vjp)
EXPORTS_DIST = ("pea_dist_validate", "pea_dist_affinity", "pea_dist_affinity_vjp")
# the entry points of include/pea_segscore.h (the segmentation scores of the validation loops from one contingency table per image)
EXPORTS_SEGSCORE = ("pea_seg_validate", "pea_seg_workspace_bytes", "pea_seg_workspace_init", "pea_seg_scores", "pea_seg_table")
# the entry points of include/pea_instscore.h (the instance scores of the BBBC039V1 validation loop: AJI, PQ, pixel F1)
EXPORTS_INSTSCORE = ("pea_inst_validate", "pea_inst_workspace_bytes", "pea_inst_workspace_init", "pea_inst_scores")
# the entry points of include/pea_cc.h (connected components: label, size filter, mask)
EXPORTS_CC = ("pea_cc_validate", "pea_cc_workspace_bytes", "pea_cc_label")
# the entry points of include/pea_rag.h (the region adjacency graph with affinity and boundary statistics; the projection)
EXPORTS_RAG = ("pea_rag_validate", "pea_rag_workspace_bytes", "pea_rag_workspace_init", "pea_rag_build", "pea_rag_project")
# the entry points of include/pea_ws.h (the watershed fragments: distance transform, seeds, flood)
EXPORTS_WS = ("pea_ws_validate", "pea_ws_seeds_workspace_bytes", "pea_ws_flood_workspace_bytes", "pea_ws_seeds", "pea_ws_flood")
# the entry points of include/pea_mws.h (the mutex watershed)
EXPORTS_MWS = ("pea_mws_validate", "pea_mws_workspace_bytes", "pea_mws_segment")
# the entry points of include/pea_agglo.h (the hierarchical agglomeration of the fragment graph: waterz's merge loop)
EXPORTS_AGGLO = ("pea_agglo_validate", "pea_agglo_workspace_bytes", "pea_agglo_merge")
# the entry points of include/pea_merge.h (the small-segment merges and the renumbering: merge_func, relabel)
EXPORTS_MERGE = ("pea_merge_validate", "pea_merge_workspace_bytes", "pea_merge_small")


class PeaLibraryError(RuntimeError):
    """libpea_hip.so is missing / unloadable, or a pea_* call returned an error."""


class PeaDesc(ctypes.Structure):
    """mirror of `struct PeaDesc` in include/pea.h"""
    _fields_ = [("abi", ctypes.c_int32), ("ndim", ctypes.c_int32), ("B", ctypes.c_int32),
                ("D", ctypes.c_int32), ("dims", ctypes.c_int32 * 3), ("K", ctypes.c_int32),
                ("border", ctypes.c_int32), ("dtype", ctypes.c_int32), ("norm", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("eps", ctypes.c_float),
                ("offsets", (ctypes.c_int32 * 3) * PEA_MAX_K), ("lam", ctypes.c_float * PEA_MAX_K),
                ("target_bstride", ctypes.c_int64), ("weight_bstride", ctypes.c_int64),
                ("mask_bstride", ctypes.c_int64)]


class PeaMultiFwd(ctypes.Structure):
    """mirror of `struct PeaMultiFwd` in include/pea_multi.h"""
    _fields_ = [("desc", ctypes.POINTER(PeaDesc)), ("e", ctypes.c_void_p), ("target", ctypes.c_void_p), ("weight", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("affs", ctypes.c_void_p), ("g_out", ctypes.c_void_p), ("loss_out", ctypes.c_void_p)]


class PeaMultiBwd(ctypes.Structure):
    """mirror of `struct PeaMultiBwd` in include/pea_multi.h"""
    _fields_ = [("desc", ctypes.POINTER(PeaDesc)), ("e", ctypes.c_void_p), ("g", ctypes.c_void_p), ("dloss", ctypes.c_void_p),
                ("de", ctypes.c_void_p)]


class PeaMultiLabels(ctypes.Structure):
    """mirror of `struct PeaMultiLabels` in include/pea_multi_labels.h"""
    _fields_ = [("desc", ctypes.POINTER(PeaDesc)), ("e", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("label_dims", ctypes.c_int32 * 3),
                ("label_step", ctypes.c_int32 * 3), ("wtab", ctypes.c_void_p), ("affs", ctypes.c_void_p), ("loss_out", ctypes.c_void_p),
                ("dloss", ctypes.c_void_p), ("de", ctypes.c_void_p)]


class PeaMetricsDesc(ctypes.Structure):
    """mirror of `struct PeaMetricsDesc` in include/pea_metrics.h"""
    _fields_ = [("B", ctypes.c_int32), ("C", ctypes.c_int32), ("CP", ctypes.c_int32), ("dims", ctypes.c_int32 * 3),
                ("pred_dims", ctypes.c_int32 * 3), ("origin", ctypes.c_int32 * 3), ("flags", ctypes.c_uint32),
                ("clip_lo", ctypes.c_float), ("clip_hi", ctypes.c_float)]


class PeaFgDesc(ctypes.Structure):
    """mirror of `struct PeaFgDesc` in include/pea_fgmask.h"""
    _fields_ = [("B", ctypes.c_int32), ("Y", ctypes.c_int32), ("X", ctypes.c_int32), ("logits_dtype", ctypes.c_int32),
                ("labels_type", ctypes.c_int32), ("flags", ctypes.c_uint32), ("origin", ctypes.c_int32 * 2),
                ("out_dims", ctypes.c_int32 * 2)]


class PeaDiscDesc(ctypes.Structure):
    """mirror of `struct PeaDiscDesc` in include/pea_disc.h"""
    _fields_ = [("B", ctypes.c_int32), ("D", ctypes.c_int32), ("S", ctypes.c_int64), ("num_ids", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("delta_v", ctypes.c_float), ("delta_d", ctypes.c_float), ("alpha", ctypes.c_float),
                ("beta", ctypes.c_float), ("gamma", ctypes.c_float)]


class PeaDistDesc(ctypes.Structure):
    """mirror of `struct PeaDistDesc` in include/pea_dist.h"""
    _fields_ = [("B", ctypes.c_int32), ("D", ctypes.c_int32), ("dims", ctypes.c_int32 * 3), ("K", ctypes.c_int32),
                ("offsets", (ctypes.c_int32 * 3) * PEA_MAX_K), ("dtype", ctypes.c_int32), ("border", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("delta_v", ctypes.c_float), ("delta_d", ctypes.c_float)]


class PeaSegDesc(ctypes.Structure):
    """mirror of `struct PeaSegDesc` in include/pea_segscore.h"""
    _fields_ = [("B", ctypes.c_int32), ("S", ctypes.c_int64), ("capacity", ctypes.c_int64), ("flags", ctypes.c_uint32)]


class PeaInstDesc(ctypes.Structure):
    """mirror of `struct PeaInstDesc` in include/pea_instscore.h"""
    _fields_ = [("B", ctypes.c_int32), ("S", ctypes.c_int64), ("capacity", ctypes.c_int64), ("max_id", ctypes.c_int32),
                ("match_iou", ctypes.c_double), ("flags", ctypes.c_uint32)]


class PeaCcDesc(ctypes.Structure):
    """mirror of `struct PeaCcDesc` in include/pea_cc.h"""
    _fields_ = [("ndim", ctypes.c_int32), ("B", ctypes.c_int32), ("dims", ctypes.c_int32 * 3), ("in_type", ctypes.c_int32),
                ("connectivity", ctypes.c_int32), ("min_size", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class PeaRagDesc(ctypes.Structure):
    """mirror of `struct PeaRagDesc` in include/pea_rag.h"""
    _fields_ = [("ndim", ctypes.c_int32), ("B", ctypes.c_int32), ("dims", ctypes.c_int32 * 3), ("K", ctypes.c_int32),
                ("offsets", (ctypes.c_int32 * 3) * RAG_MAX_K), ("max_id", ctypes.c_int32), ("capacity", ctypes.c_int64),
                ("max_edges", ctypes.c_int64), ("flags", ctypes.c_uint32)]


class PeaRagBuffers(ctypes.Structure):
    """mirror of `struct PeaRagBuffers` in include/pea_rag.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("fragments", "affs", "boundary", "uv", "size", "count", "mean", "bmean", "min", "max",
                                               "node_size", "stats")]


class PeaWsDesc(ctypes.Structure):
    """mirror of `struct PeaWsDesc` in include/pea_ws.h"""
    _fields_ = [("N", ctypes.c_int32), ("Y", ctypes.c_int32), ("X", ctypes.c_int32), ("threshold", ctypes.c_float),
                ("sigma_seeds", ctypes.c_float), ("sigma_weights", ctypes.c_float), ("alpha", ctypes.c_float),
                ("maxima_connectivity", ctypes.c_int32), ("seed_connectivity", ctypes.c_int32), ("min_size", ctypes.c_int32),
                ("flags", ctypes.c_uint32)]


class PeaMwsDesc(ctypes.Structure):
    """mirror of `struct PeaMwsDesc` in include/pea_mws.h"""
    _fields_ = [("B", ctypes.c_int32), ("Z", ctypes.c_int32), ("Y", ctypes.c_int32), ("X", ctypes.c_int32), ("K", ctypes.c_int32),
                ("n_attractive", ctypes.c_int32), ("offsets", (ctypes.c_int32 * 3) * MWS_MAX_K), ("strides", ctypes.c_int32 * 3),
                ("input", ctypes.c_int32), ("rounds", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class PeaAggloDesc(ctypes.Structure):
    """mirror of `struct PeaAggloDesc` in include/pea_agglo.h"""
    _fields_ = [("B", ctypes.c_int32), ("max_id", ctypes.c_int32), ("max_edges", ctypes.c_int64), ("n_edges_stride", ctypes.c_int64),
                ("linkage", ctypes.c_int32), ("rounds", ctypes.c_int32), ("threshold", ctypes.c_float), ("flags", ctypes.c_uint32)]


class PeaMergeDesc(ctypes.Structure):
    """mirror of `struct PeaMergeDesc` in include/pea_merge.h"""
    _fields_ = [("B", ctypes.c_int32), ("Y", ctypes.c_int32), ("X", ctypes.c_int32), ("max_id", ctypes.c_int32), ("n_passes", ctypes.c_int32),
                ("threshold", ctypes.c_int32 * MERGE_MAX_PASSES), ("window", ctypes.c_int32 * MERGE_MAX_PASSES), ("flags", ctypes.c_uint32)]


class PeaAggloBuffers(ctypes.Structure):
    """mirror of `struct PeaAggloBuffers` in include/pea_agglo.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("uv", "n_edges", "value", "weight", "node_size", "root", "labels", "counts", "stats")]


HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]
OBJ_DIR = os.path.join(CSRC, "build")


def sources():
    """the translation units of the library (csrc/pea_host.h lists what each holds)"""
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def build(force=False, verbose=False, jobs=None):
    """Compile csrc/*.hip -> csrc/libpea_hip.so for gfx950: one object per file, compiled in parallel, one link.
    Serialised across processes by a lock file: the ranks of a multi-GPU job all import the package at once, and if the library
    is stale each of them would otherwise write the same object files."""
    import fcntl
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(OBJ_DIR, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            return _build_locked(force, verbose, jobs)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(force, verbose, jobs):
    srcs = sources()
    hdrs = [HEADER, HEADER_INFER, HEADER_MULTI, HEADER_FLIP, HEADER_MULTI_LABELS, HEADER_HEAD16, HEADER_METRICS, HEADER_FGMASK, HEADER_DISC, HEADER_CROP, HEADER_DIST, HEADER_SEGSCORE, HEADER_INSTSCORE, HEADER_CC, HEADER_RAG, HEADER_WS, HEADER_MWS, HEADER_AGGLO, HEADER_MERGE] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    newest_hdr = max(os.path.getmtime(h) for h in hdrs)
    if not force and os.path.exists(SO_PATH) and os.path.getmtime(SO_PATH) >= max([newest_hdr] + [os.path.getmtime(x) for x in srcs]):
        return SO_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise PeaLibraryError("hipcc not found: cannot build libpea_hip.so")
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs, todo = [], []
    for src in srcs:
        obj = os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(newest_hdr, os.path.getmtime(src)):
            todo.append((src, obj))
    jobs = jobs or min(len(todo) or 1, max(1, (os.cpu_count() or 2) - 1))
    running = []

    def reap(block_until):
        while len(running) > block_until:
            for i, (p, src, obj) in enumerate(running):
                if p.poll() is not None:
                    running.pop(i)
                    if p.returncode != 0:
                        for q, _, _ in running:
                            q.kill()
                        raise PeaLibraryError("hipcc failed on %s (rc %d)" % (src, p.returncode))
                    os.replace(obj + ".tmp", obj)
                    break
            else:
                import time
                time.sleep(0.05)

    for src, obj in todo:
        cmd = [hipcc] + HIPCC_FLAGS + ["-c", "-o", obj + ".tmp", src]
        if verbose:
            print(" ".join(cmd))
        running.append((subprocess.Popen(cmd, cwd=CSRC), src, obj))
        reap(jobs - 1)
    reap(0)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_PATH + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    os.replace(SO_PATH + ".tmp", SO_PATH)
    return SO_PATH


_lib = None


def lib():
    """Load the library (after torch, so both bind to the same HIP runtime, libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise PeaLibraryError(
            "%s not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback." % SO_PATH)
    import torch  # noqa: F401  (loads torch's bundled libamdhip64 first)
    try:
        L = ctypes.CDLL(SO_PATH)
    except OSError as ex:
        raise PeaLibraryError("cannot load %s: %s" % (SO_PATH, ex))
    for name in EXPORTS + EXPORTS_INFER + EXPORTS_MULTI + EXPORTS_FLIP + EXPORTS_MULTI_LABELS + EXPORTS_HEAD16 + EXPORTS_METRICS + EXPORTS_FGMASK + EXPORTS_DISC + EXPORTS_CROP + EXPORTS_DIST + EXPORTS_SEGSCORE + EXPORTS_INSTSCORE + EXPORTS_CC + EXPORTS_RAG + EXPORTS_WS + EXPORTS_MWS + EXPORTS_AGGLO + EXPORTS_MERGE:
        if not hasattr(L, name):
            raise PeaLibraryError("%s does not export %s" % (SO_PATH, name))
    vp, dp = ctypes.c_void_p, ctypes.POINTER(PeaDesc)
    L.pea_version.restype = ctypes.c_int
    L.pea_strerror.restype = ctypes.c_char_p
    L.pea_strerror.argtypes = [ctypes.c_int]
    L.pea_desc_validate.restype = ctypes.c_int
    L.pea_desc_validate.argtypes = [dp]
    L.pea_workspace_bytes.restype = ctypes.c_size_t
    L.pea_workspace_bytes.argtypes = [dp]
    L.pea_workspace_init.restype = ctypes.c_int
    L.pea_workspace_init.argtypes = [vp, ctypes.c_size_t, vp]
    L.pea_reload_env.restype = None
    L.pea_reload_env.argtypes = []
    L.pea_affinity_infer.restype = ctypes.c_int
    L.pea_affinity_infer.argtypes = [dp, vp, vp, vp, vp]
    L.pea_affinity_fwd.restype = ctypes.c_int
    L.pea_affinity_fwd.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_affinity_bwd.restype = ctypes.c_int
    L.pea_affinity_bwd.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp]
    L.pea_affinity_fwd_ex.restype = ctypes.c_int
    L.pea_affinity_fwd_ex.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_affinity_bwd_ex.restype = ctypes.c_int
    L.pea_affinity_bwd_ex.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pea_affinity_bwd_ex2.restype = ctypes.c_int
    L.pea_affinity_bwd_ex2.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pea_cross_supported.restype = ctypes.c_int
    L.pea_cross_supported.argtypes = [dp, ctypes.c_int]
    L.pea_inv_norm.restype = ctypes.c_int
    L.pea_inv_norm.argtypes = [dp, vp, vp, vp]
    L.pea_affinity_bwd_dual_ex.restype = ctypes.c_int
    L.pea_affinity_bwd_dual_ex.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pea_affinity_fwd_dual_ex.restype = ctypes.c_int
    L.pea_affinity_fwd_dual_ex.argtypes = [dp, dp] + [vp] * 14 + [ctypes.c_size_t, vp]
    L.pea_affinity_bwd_dual.restype = ctypes.c_int
    L.pea_affinity_bwd_dual.argtypes = [dp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pea_scale_inplace.restype = ctypes.c_int
    L.pea_scale_inplace.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp, vp]
    L.pea_targets_workspace_bytes.restype = ctypes.c_size_t
    L.pea_targets_workspace_bytes.argtypes = [dp]
    L.pea_gen_targets.restype = ctypes.c_int
    L.pea_gen_targets.argtypes = [dp, vp, ctypes.c_uint, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_scale_inplace_multi.restype = ctypes.c_int
    L.pea_scale_inplace_multi.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int, vp, vp]
    L.pea_weighted_sum.restype = ctypes.c_int
    L.pea_weighted_sum.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, vp, vp]
    L.pea_label_weights.restype = ctypes.c_int
    L.pea_label_weights.argtypes = [dp, vp, ctypes.c_uint, vp, vp, ctypes.c_size_t, vp]
    L.pea_affinity_fwd_bwd_labels.restype = ctypes.c_int
    L.pea_affinity_fwd_bwd_labels.argtypes = [dp, vp, vp, vp, vp, ctypes.c_uint, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_affinity_fwd_bwd_labels_ex.restype = ctypes.c_int
    L.pea_affinity_fwd_bwd_labels_ex.argtypes = [dp, vp, vp, vp, vp, ctypes.c_uint, vp, vp, vp, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp]
    L.pea_labels_scratch_bytes.restype = ctypes.c_size_t
    L.pea_labels_scratch_bytes.argtypes = [dp]
    L.pea_affinity_fwd_bwd_labels_dual.restype = ctypes.c_int
    L.pea_affinity_fwd_bwd_labels_dual.argtypes = [dp, dp, vp, vp, vp, vp, ctypes.c_uint, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_stitch_add.restype = ctypes.c_int
    L.pea_stitch_add.argtypes = [vp, vp, vp, vp] + [ctypes.c_int] * 10 + [vp]
    L.pea_stitch_finalize.restype = ctypes.c_int
    L.pea_stitch_finalize.argtypes = [vp, vp, ctypes.c_int, ctypes.c_size_t, vp]
    L.pea_fill_border_relu.restype = ctypes.c_int
    L.pea_fill_border_relu.argtypes = [vp] + [ctypes.c_int] * 7 + [vp]
    L.pea_head_workspace_bytes.restype = ctypes.c_size_t
    L.pea_head_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    L.pea_head_fwd.restype = ctypes.c_int
    L.pea_head_fwd.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp]
    L.pea_head_bwd.restype = ctypes.c_int
    L.pea_head_bwd.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_infer_stitch_supported.restype = ctypes.c_int
    L.pea_infer_stitch_supported.argtypes = [dp, ctypes.c_int]
    L.pea_affinity_infer_stitch.restype = ctypes.c_int
    L.pea_affinity_infer_stitch.argtypes = [dp, vp, ctypes.c_int, vp, vp, vp] + [ctypes.c_int] * 6 + [vp]
    L.pea_multi_supported.restype = ctypes.c_int
    L.pea_multi_supported.argtypes = [ctypes.POINTER(dp), ctypes.c_int]
    L.pea_affinity_fwd_multi.restype = ctypes.c_int
    L.pea_affinity_fwd_multi.argtypes = [ctypes.POINTER(PeaMultiFwd), ctypes.c_int, vp, ctypes.c_size_t, vp]
    L.pea_affinity_bwd_multi.restype = ctypes.c_int
    L.pea_affinity_bwd_multi.argtypes = [ctypes.POINTER(PeaMultiBwd), ctypes.c_int, vp]
    L.pea_multi_labels_supported.restype = ctypes.c_int
    L.pea_multi_labels_supported.argtypes = [ctypes.POINTER(PeaMultiLabels), ctypes.c_int, ctypes.c_uint]
    L.pea_multi_labels_scratch_bytes.restype = ctypes.c_size_t
    L.pea_multi_labels_scratch_bytes.argtypes = [ctypes.POINTER(PeaMultiLabels), ctypes.c_int]
    L.pea_affinity_fwd_bwd_labels_multi.restype = ctypes.c_int
    L.pea_affinity_fwd_bwd_labels_multi.argtypes = [ctypes.POINTER(PeaMultiLabels), ctypes.c_int, ctypes.c_uint, vp, ctypes.c_size_t, vp,
                                                    ctypes.c_size_t, vp]
    L.pea_consistency_unflip.restype = ctypes.c_int
    L.pea_consistency_unflip.argtypes = [ctypes.c_int] * 6 + [vp, vp, vp, ctypes.c_int, ctypes.c_int, vp]
    L.pea_head_supported_t.restype = ctypes.c_int
    L.pea_head_supported_t.argtypes = [ctypes.c_int] * 4
    L.pea_head_fwd_t.restype = ctypes.c_int
    L.pea_head_fwd_t.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp]
    L.pea_head_bwd_t.restype = ctypes.c_int
    L.pea_head_bwd_t.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp, vp,
                                 ctypes.c_size_t, vp]
    L.pea_metrics_validate.restype = ctypes.c_int
    L.pea_metrics_validate.argtypes = [ctypes.POINTER(PeaMetricsDesc)]
    L.pea_metrics_workspace_bytes.restype = ctypes.c_size_t
    L.pea_metrics_workspace_bytes.argtypes = []
    L.pea_affs_metrics.restype = ctypes.c_int
    L.pea_affs_metrics.argtypes = [ctypes.POINTER(PeaMetricsDesc), vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    fp = ctypes.POINTER(PeaFgDesc)
    L.pea_fgmask_validate.restype = ctypes.c_int
    L.pea_fgmask_validate.argtypes = [fp]
    L.pea_fgmask_workspace_bytes.restype = ctypes.c_size_t
    L.pea_fgmask_workspace_bytes.argtypes = []
    L.pea_fgmask_loss_fwd.restype = ctypes.c_int
    L.pea_fgmask_loss_fwd.argtypes = [fp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_fgmask_loss_bwd.restype = ctypes.c_int
    L.pea_fgmask_loss_bwd.argtypes = [fp, vp, vp, vp, vp, vp, vp]
    L.pea_fgmask_argmax.restype = ctypes.c_int
    L.pea_fgmask_argmax.argtypes = [fp, vp, vp, vp]
    dd = ctypes.POINTER(PeaDiscDesc)
    L.pea_disc_validate.restype = ctypes.c_int
    L.pea_disc_validate.argtypes = [dd]
    L.pea_disc_workspace_bytes.restype = ctypes.c_size_t
    L.pea_disc_workspace_bytes.argtypes = [dd]
    L.pea_disc_workspace_init.restype = ctypes.c_int
    L.pea_disc_workspace_init.argtypes = [vp, ctypes.c_size_t, vp]
    L.pea_disc_context_bytes.restype = ctypes.c_size_t
    L.pea_disc_context_bytes.argtypes = [dd]
    L.pea_disc_loss_fwd.restype = ctypes.c_int
    L.pea_disc_loss_fwd.argtypes = [dd, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_disc_loss_bwd.restype = ctypes.c_int
    L.pea_disc_loss_bwd.argtypes = [dd, vp, vp, vp, vp, vp, vp]
    L.pea_affs_crop_zero.restype = ctypes.c_int
    L.pea_affs_crop_zero.argtypes = [dp, vp, vp]
    ds = ctypes.POINTER(PeaDistDesc)
    L.pea_dist_validate.restype = ctypes.c_int
    L.pea_dist_validate.argtypes = [ds]
    L.pea_dist_affinity.restype = ctypes.c_int
    L.pea_dist_affinity.argtypes = [ds, vp, vp, vp]
    L.pea_dist_affinity_vjp.restype = ctypes.c_int
    L.pea_dist_affinity_vjp.argtypes = [ds, vp, vp, vp, vp, vp]
    sg = ctypes.POINTER(PeaSegDesc)
    L.pea_seg_validate.restype = ctypes.c_int
    L.pea_seg_validate.argtypes = [sg]
    L.pea_seg_workspace_bytes.restype = ctypes.c_size_t
    L.pea_seg_workspace_bytes.argtypes = [sg]
    L.pea_seg_workspace_init.restype = ctypes.c_int
    L.pea_seg_workspace_init.argtypes = [vp, ctypes.c_size_t, vp]
    L.pea_seg_scores.restype = ctypes.c_int
    L.pea_seg_scores.argtypes = [sg, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_seg_table.restype = ctypes.c_int
    L.pea_seg_table.argtypes = [sg, vp, vp, ctypes.c_int32, vp, vp, vp, vp, ctypes.c_int64, vp, ctypes.c_size_t, vp]
    it = ctypes.POINTER(PeaInstDesc)
    L.pea_inst_validate.restype = ctypes.c_int
    L.pea_inst_validate.argtypes = [it]
    L.pea_inst_workspace_bytes.restype = ctypes.c_size_t
    L.pea_inst_workspace_bytes.argtypes = [it]
    L.pea_inst_workspace_init.restype = ctypes.c_int
    L.pea_inst_workspace_init.argtypes = [vp, ctypes.c_size_t, vp]
    L.pea_inst_scores.restype = ctypes.c_int
    L.pea_inst_scores.argtypes = [it, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    cc = ctypes.POINTER(PeaCcDesc)
    L.pea_cc_validate.restype = ctypes.c_int
    L.pea_cc_validate.argtypes = [cc]
    L.pea_cc_workspace_bytes.restype = ctypes.c_size_t
    L.pea_cc_workspace_bytes.argtypes = [cc]
    L.pea_cc_label.restype = ctypes.c_int
    L.pea_cc_label.argtypes = [cc, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    rg = ctypes.POINTER(PeaRagDesc)
    L.pea_rag_validate.restype = ctypes.c_int
    L.pea_rag_validate.argtypes = [rg]
    L.pea_rag_workspace_bytes.restype = ctypes.c_size_t
    L.pea_rag_workspace_bytes.argtypes = [rg]
    L.pea_rag_workspace_init.restype = ctypes.c_int
    L.pea_rag_workspace_init.argtypes = [vp, ctypes.c_size_t, vp]
    L.pea_rag_build.restype = ctypes.c_int
    L.pea_rag_build.argtypes = [rg, ctypes.POINTER(PeaRagBuffers), vp, ctypes.c_size_t, vp]
    L.pea_rag_project.restype = ctypes.c_int
    L.pea_rag_project.argtypes = [ctypes.c_int64, vp, vp, ctypes.c_int64, vp, vp, vp]
    ws = ctypes.POINTER(PeaWsDesc)
    L.pea_ws_validate.restype = ctypes.c_int
    L.pea_ws_validate.argtypes = [ws]
    L.pea_ws_seeds_workspace_bytes.restype = ctypes.c_size_t
    L.pea_ws_seeds_workspace_bytes.argtypes = [ws]
    L.pea_ws_flood_workspace_bytes.restype = ctypes.c_size_t
    L.pea_ws_flood_workspace_bytes.argtypes = [ws]
    L.pea_ws_seeds.restype = ctypes.c_int
    L.pea_ws_seeds.argtypes = [ws, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.pea_ws_flood.restype = ctypes.c_int
    L.pea_ws_flood.argtypes = [ws, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    mw = ctypes.POINTER(PeaMwsDesc)
    L.pea_mws_validate.restype = ctypes.c_int
    L.pea_mws_validate.argtypes = [mw]
    L.pea_mws_workspace_bytes.restype = ctypes.c_size_t
    L.pea_mws_workspace_bytes.argtypes = [mw]
    L.pea_mws_segment.restype = ctypes.c_int
    L.pea_mws_segment.argtypes = [mw, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    ag = ctypes.POINTER(PeaAggloDesc)
    L.pea_agglo_validate.restype = ctypes.c_int
    L.pea_agglo_validate.argtypes = [ag]
    L.pea_agglo_workspace_bytes.restype = ctypes.c_size_t
    L.pea_agglo_workspace_bytes.argtypes = [ag]
    L.pea_agglo_merge.restype = ctypes.c_int
    L.pea_agglo_merge.argtypes = [ag, ctypes.POINTER(PeaAggloBuffers), vp, ctypes.c_size_t, vp]
    mg = ctypes.POINTER(PeaMergeDesc)
    L.pea_merge_validate.restype = ctypes.c_int
    L.pea_merge_validate.argtypes = [mg]
    L.pea_merge_workspace_bytes.restype = ctypes.c_size_t
    L.pea_merge_workspace_bytes.argtypes = [mg]
    L.pea_merge_small.restype = ctypes.c_int
    L.pea_merge_small.argtypes = [mg, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    if L.pea_version() != PEA_ABI_VERSION:
        raise PeaLibraryError("ABI mismatch: library %d, binding %d" % (L.pea_version(), PEA_ABI_VERSION))
    _lib = L
    return L


_RELOAD_HOOKS = []


def reload_env():
    """make the loaded library re-read the PEA_* switches (it reads them once) and drop what the Python layer remembered of them"""
    if _lib is not None:
        _lib.pea_reload_env()
    for hook in _RELOAD_HOOKS:
        hook()


def set_switch(name, value):
    """set (value) or clear (None) a PEA_* environment switch, then reload_env()"""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    reload_env()


def check(rc, what):
    if rc != 0:
        raise PeaLibraryError("%s failed: rc=%d (%s)" % (what, rc, lib().pea_strerror(rc).decode()))
