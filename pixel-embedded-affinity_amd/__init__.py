"""pixel-embedded-affinity_amd -- the MI355X-native embedding -> affinity hot path.

A drop-in for the one data-parallel hot path of weih527/Pixel-Embedded-Affinity: per-pixel embedding
-> K-offset affinity map -> class-balanced weighted-MSE loss -> gradient, as hand-written HIP for
gfx950 behind a C ABI (include/pea.h), with this thin Python layer mirroring the reference's own
function names so its main.py / inference.py call sites only change their import line
(see INTEGRATION.md).

Import name: the directory is not a valid Python identifier, so load it through
`__graft_entry__.load_package()` (registers it as `pixel_embedded_affinity_amd`).
"""
from . import _lib
from ._lib import PeaLibraryError, build
from .affinity_op import (AffinityMap, AffinitySpec, FusedAffinityMSE, Graphed, LabelsAffinityMSE, MultiAffinityMSE, MultiLabelsAffinityMSE, affinity_infer, backward,
                          check_label_ranges, graphed, unflip)
from .loss.loss import BCE_loss_func, BCELoss, MSELoss, WeightedBCE, WeightedMSE
from .loss.loss_embedding_mse import (ema_embedding_loss, ema_embedding_loss_from_labels, embedding2affs, embedding_loss,
                                      embedding_loss_from_labels, embedding_loss_from_labels_multi, embedding_loss_multi)
from .loss import embedding2affs_3d, embedding2affs_3d_l2, loss_embedding, loss_embedding_exp, loss_embedding_norm
from .loss.loss_embedding import (ema_embedding_loss as ema_embedding_loss_half_clamp, embedding2affs as embedding2affs_half_clamp,
                                  embedding_loss as embedding_loss_half_clamp)
from .loss.loss_embedding_exp import embedding2affs as embedding2affs_clamp, embedding_loss as embedding_loss_clamp
from .loss.loss_embedding_norm import (ema_embedding_loss as ema_embedding_loss_normalized, embedding2affs as embedding2affs_normalized,
                                       embedding_loss as embedding_loss_normalized)
from .loss.loss_embedding_mse_3d import (ema_embedding_loss_norm1, ema_embedding_loss_norm2, ema_embedding_loss_norm5,
                                         ema_embedding_loss_norm5_from_labels, embedding_loss_norm2,
                                         ema_embedding_loss_norm6, embedding_loss_norm6,
                                         embedding_loss_norm1, embedding_loss_norm1_from_labels, embedding_loss_norm1_from_labels_multi, embedding_loss_norm1_multi,
                                         embedding_loss_norm5,
                                         embedding_loss_norm5_from_labels, inf_embedding_loss_norm1, inf_embedding_loss_norm5)
from .utils.affinity_ours import gen_offsets, multi_offset
from .utils.postproc import affs_crop_zero_, fill_border_relu_, relu_
from .utils.targets import gen_affs_ours, gen_targets, seg_to_aff
from .harness.stitch import VolumeStitcher
from .harness.metrics import AffinityMetrics, affinity_metrics
from .harness.fgmask import ForegroundMaskCE, foreground_mask, foreground_mask_loss
from .harness.disc import DiscriminativeLoss, discriminative_loss_stats
from .loss.loss_discriminative import discriminative_loss
from .harness.dist import DistanceAffinities, distance_affinities
from .utils import emb2affs, embeddings_ours
from .harness.segscore import SegmentationScores, segmentation_scores
from .utils import evaluate, seg_scores
from .utils.evaluate import AbsDiffFGLabels, BestDice, Dice, DiffFGLabels, FGBGDice, SymmetricBestDice
from .utils.seg_scores import adapted_rand_error, variation_of_information
from .harness.instscore import InstanceScores, instance_scores
from .utils import metrics_bbbc
from .utils.metrics_bbbc import agg_jc_index, get_fast_pq, pixel_f1, remap_label
from .harness.cc import ConnectedComponents, connected_components, remove_small_components
from .utils import postprocessing
from .utils.postprocessing import remove_samll_object
from .harness.rag import RegionAdjacency, project_node_labels, region_adjacency
from .utils import lmc
from .utils.lmc import mc_baseline, multicut_multi, probs_to_costs, transform_probabilities_to_costs
from .harness.ws import (Watershed, WatershedSeeds, distance_transform_watershed, plateau_maxima, seeded_watershed, watershed_seeds)
from .utils import fragment
from .harness.mws import MutexWatershed, mutex_watershed
from .utils.seg_mutex import mutex_watershed as elf_mutex_watershed, seg_mutex
from .harness.agglo import Agglomeration, agglomerate, agglomerate_graph
from .utils.seg_waterz import seg_waterz
from .harness.merge import BBBC_MERGE_PASSES, CVPPP_MERGE_PASSES, MergedSegments, merge_small_objects
from .utils import merge_objects
from .utils.merge_objects import merge_func, merge_func_bbbc, merge_small_object
from .harness.handoff import AffsCollector
from .harness.head_loss import HeadAffinityMSE, head_embedding_loss
from .harness.train_step import CvpppTrainStep, convert_consistency_flip, label_pyramid, make_optimizer
from .model.unet2d_residual import ResidualUNet2D_deep
from .model.head import EmbeddingHead, OutConv, head16_supported, head_conv3d_block
from .harness.loss_section import (ac3ac4_loss_section, ac3ac4_loss_section_composed, ac3ac4_loss_section_from_labels,
                                   cvppp_loss_section, cvppp_loss_section_composed,
                                   cvppp_loss_section_from_labels, cvppp_label_weight_tables, cvppp_validation_section,
                                   deep_weight_factor,
                                   finish_pred_2d_, finish_pred_3d_)

__all__ = [
    "PeaLibraryError", "build", "backward", "graphed", "Graphed", "check_label_ranges", "AffinityMap", "AffinitySpec", "FusedAffinityMSE", "affinity_infer", "WeightedMSE", "WeightedBCE", "BCELoss", "MSELoss",
    "embedding_loss", "ema_embedding_loss", "embedding2affs", "embedding_loss_norm1", "embedding_loss_norm5",
    "ema_embedding_loss_norm1", "ema_embedding_loss_norm5", "inf_embedding_loss_norm1", "inf_embedding_loss_norm5",
    "gen_offsets", "multi_offset", "fill_border_relu_", "relu_", "cvppp_loss_section", "ac3ac4_loss_section",
    "deep_weight_factor", "finish_pred_2d_", "finish_pred_3d_", "gen_targets", "gen_affs_ours", "seg_to_aff", "VolumeStitcher", "embedding_loss_from_labels",
    "ema_embedding_loss_from_labels", "LabelsAffinityMSE", "cvppp_loss_section_from_labels", "cvppp_loss_section_composed", "ac3ac4_loss_section_composed",
    "ac3ac4_loss_section_from_labels",
    "embedding_loss_norm1_from_labels", "embedding_loss_norm5_from_labels", "ema_embedding_loss_norm5_from_labels",
    "loss_embedding", "loss_embedding_exp", "loss_embedding_norm", "embedding_loss_half_clamp", "ema_embedding_loss_half_clamp",
    "embedding2affs_half_clamp", "embedding_loss_clamp", "embedding2affs_clamp", "embedding_loss_normalized",
    "ema_embedding_loss_normalized", "embedding2affs_normalized",
    "embedding_loss_norm6", "ema_embedding_loss_norm6", "EmbeddingHead", "OutConv", "head_conv3d_block", "head16_supported", "cvppp_label_weight_tables", "cvppp_validation_section",
    "MultiAffinityMSE", "embedding_loss_multi", "embedding_loss_norm1_multi", "unflip", "convert_consistency_flip",
    "MultiLabelsAffinityMSE", "embedding_loss_from_labels_multi", "embedding_loss_norm1_from_labels_multi",
    "affinity_metrics", "AffinityMetrics",
    "BCE_loss_func", "foreground_mask_loss", "foreground_mask", "ForegroundMaskCE",
    "discriminative_loss", "discriminative_loss_stats", "DiscriminativeLoss",
    "embedding2affs_3d", "embedding2affs_3d_l2", "embedding_loss_norm2", "ema_embedding_loss_norm2", "affs_crop_zero_",
    "distance_affinities", "DistanceAffinities", "emb2affs", "embeddings_ours",
]
# The segmentation scores (include/pea_segscore.h) are public attributes of the package like everything above.  They are listed here
# and not in __all__, whose exact contents tests/test_dist_host.py pins: `from pixel_embedded_affinity_amd import *` does not bring
# them in, `pea.segmentation_scores` and `from pixel_embedded_affinity_amd import SymmetricBestDice` do.
SEGSCORE_EXPORTS = (
    "segmentation_scores", "SegmentationScores", "evaluate", "seg_scores", "DiffFGLabels", "BestDice", "FGBGDice", "Dice",
    "AbsDiffFGLabels", "SymmetricBestDice", "adapted_rand_error", "variation_of_information",
)
# likewise the instance scores of the BBBC039V1 validation loop (include/pea_instscore.h)
INSTSCORE_EXPORTS = ("instance_scores", "InstanceScores", "metrics_bbbc", "agg_jc_index", "get_fast_pq", "pixel_f1", "remap_label")
# likewise connected-component labelling (include/pea_cc.h) and the reference's remove_samll_object on it
CC_EXPORTS = ("connected_components", "ConnectedComponents", "remove_small_components", "postprocessing", "remove_samll_object")
# likewise the region adjacency graph (include/pea_rag.h) and the reference's utils/lmc.py on it
RAG_EXPORTS = ("region_adjacency", "RegionAdjacency", "project_node_labels", "lmc", "mc_baseline", "multicut_multi", "probs_to_costs",
               "transform_probabilities_to_costs")
# likewise the watershed fragments (include/pea_ws.h) and the reference's scripts_ac3ac4/utils/fragment.py on them
WS_EXPORTS = ("watershed_seeds", "WatershedSeeds", "seeded_watershed", "Watershed", "distance_transform_watershed", "plateau_maxima", "fragment")
# likewise the mutex watershed (include/pea_mws.h) and the reference's utils/seg_mutex.py on it; elf's own mutex_watershed(1 - affs, ..)
# is elf_mutex_watershed here and mutex_watershed in utils/seg_mutex.py, the module that the reference's call sites import from
MWS_EXPORTS = ("mutex_watershed", "MutexWatershed", "seg_mutex", "elf_mutex_watershed")
# likewise the hierarchical agglomeration of the fragment graph (include/pea_agglo.h) and the reference's seg_waterz on it; the module
# pea.utils.seg_waterz also carries relabel and waterz's own agglomerate(affs, thresholds, ..)
AGGLO_EXPORTS = ("agglomerate_graph", "agglomerate", "Agglomeration", "seg_waterz")
# likewise the small-segment merges and the renumbering (include/pea_merge.h) and the reference's merge_func on them; the module
# pea.utils.merge_objects also carries relabel (utils/postprocessing.py stays without them: tests/test_cc_host.py)
MERGE_EXPORTS = ("merge_small_objects", "MergedSegments", "CVPPP_MERGE_PASSES", "BBBC_MERGE_PASSES", "merge_objects", "merge_small_object",
                 "merge_func", "merge_func_bbbc")
