"""hotformerloc_amd: MI355X-native (gfx950) HOTFormerLoc hierarchical octree attention encoder.

Public surface (mirrors the reference's): `model_factory`, `ModelParams`, `Octree`, `Points`,
`merge_octrees`, and the `dwconv` op module.  See DESIGN.md / INTEGRATION.md.

Raw-submap post-processing on the device (the reference's open3d / CSF toolkit): `trim_radius`, `remove_outliers` (and
`knn_mean_distance`, the exact k-nearest-neighbour mean distance behind it; `estimate_normals` on the same search;
`remove_radius_outliers` / `radius_neighbour_counts` on its radius form, which `estimate_normals(radius=)` and
`compute_fpfh(radius=)` take as hybrid or radius-only neighbourhoods),
`remove_ground`, `voxel_downsample` /
`pnvlad_downsample` / `random_downsample`, `normalise_submaps`, chained by `prepare_submaps` / `prepare_submaps_fixed`;
every step has a numpy `*_host` twin that states its definition.

Towards a pose for a retrieved candidate: `estimate_normals`, then `compute_fpfh` (33-bin FPFH descriptors per point on the
same search) and `feature_correspondences` (nearest rows in descriptor space, optionally mutual) give the point pairs a
robust estimator needs; `ransac_registration` is that estimator (a deterministic RANSAC over `correspondence_pairs`:
`ransac_hypotheses`, `score_hypotheses`, select, a short polish) and hands `icp_refine(init=...)` its starting pose;
`global_registration` chains all of it from two raw clouds to a refined 6-DoF pose in one call.  The `*_host` twins define
every step.

Back to the ranking: `spectral_consistency` scores how many of a pair's correspondences agree with one rigid motion (the
leading eigenvalue of their length-consistency matrix, no pose estimated), `prune_correspondences` keeps the ones its
eigenvector trusts, and `rerank_candidates` re-orders the (Q, k) result of `FlatL2Index.search` by that score.

Where nearly every correspondence is wrong (95 % and more) drawn triples stop finding a pose: `consensus_registration`
makes its candidates from the correspondences' second-order compatibility instead (`consensus_hypotheses`: a bit-matrix
graph, one consensus set and one Kabsch solve per seed, nothing random) and scores, selects and polishes them as
`ransac_registration` does; `global_registration(estimator='consensus')` and `rerank_candidates(..., estimator='consensus')`
use it for the coarse pose.

Matching on fewer than all points: `iss_keypoints` (Intrinsic Shape Signatures: `iss_saliency`, then the non-maximum
suppression `iss_select`) keeps the few per cent of a cloud's points where the surface bends in all three directions;
`global_registration` and `rerank_candidates` take `salient_radius=` and `non_max_radius=` and then match, verify and
estimate the coarse pose on those rows only, while the ICP still refines on the full clouds.

Training losses: `make_loss_fn(params)` builds what a training config's `loss =` names, `TruncatedSmoothAP` or the two
batch-hard losses `BatchHardTripletLossWithMasks` / `BatchHardContrastiveLossWithMasks` (`batch_hard_mine` is their miner;
`batch_hard_*_host` are the numpy twins); `should_expand_batch` and `expand_batch_size` turn their statistics into the
reference's dynamic batch sizing.
"""

import os as _os

# hipBLASLt's default kernels for this model's GEMM shapes (tens of thousands of rows, N and K of a few
# hundred) are stream-K: workgroups wait on each other's partial tiles.  Two consequences measured on
# MI355X ("Linear layers"): (1) several such GEMMs running at once on different HIP
# streams can dead-lock once they fill the CUs (Oxford cfg, batch >= 48 with all pyramid depths on side
# streams), (2) the plain data-parallel schedule is ~6 % faster end to end on these skinny shapes.
# The library reads this switch when it is first used, i.e. at the first GEMM of the process.
_os.environ.setdefault('TENSILE_STREAMK_DATA_PARALLEL', '1')

from .params import ModelParams, load_config            # noqa: F401,E402
from .model_factory import model_factory                 # noqa: F401,E402
from .octree import Octree, Points, merge_octrees, build_batch_octree   # noqa: F401,E402
from .optim import FusedAdam                             # noqa: F401,E402
from .batch_masks import TupleIndex, batch_masks, batch_masks_host     # noqa: F401,E402
from .voxel import (voxel_downsample, normalise_submaps, prepare_submaps, voxel_downsample_host,   # noqa: F401,E402
                    normalise_submaps_host, voxel_occupancy, voxel_occupancy_host, pnvlad_downsample,
                    pnvlad_downsample_host, random_downsample, random_downsample_host, normalise_submaps_padded,
                    normalise_submaps_padded_host, prepare_submaps_fixed)
from .ground import remove_ground, remove_ground_host                                              # noqa: F401,E402
from .outliers import (remove_outliers, remove_outliers_host, knn_mean_distance, knn_mean_distance_host,   # noqa: F401,E402
                       trim_radius, trim_radius_host, radius_neighbour_counts, radius_neighbour_counts_host,
                       remove_radius_outliers, remove_radius_outliers_host)
from .tuples import (radius_lists, radius_counts, radius_lists_host, radius_counts_host,          # noqa: F401,E402
                     tuple_index_from_poses, truth_from_poses)
from .overlap import (pose_matrix, relative_pose, match_nearest_pose, transform_points, nn_distances,   # noqa: F401,E402
                      chamfer_distance, overlap_ratio, submap_overlap, transform_points_host, nn_distances_host,
                      chamfer_distance_host, overlap_ratio_host, submap_overlap_host, ChamferResult, SubmapOverlap)
from .registration import (icp_refine, icp_refine_host, icp_correspondences, icp_correspondences_host,  # noqa: F401,E402
                           evaluate_registration, evaluate_registration_host, kabsch_update, kabsch_update_host,
                           plane_update, plane_update_host, RegistrationResult)
from .normals import estimate_normals, estimate_normals_host                                            # noqa: F401,E402
from .keypoints import (iss_saliency, iss_saliency_host, iss_select, iss_select_host, iss_keypoints,    # noqa: F401,E402
                        iss_keypoints_host)
from .fpfh import (compute_fpfh, compute_fpfh_host, feature_correspondences,                            # noqa: F401,E402
                   feature_correspondences_host)
from .global_registration import (correspondence_pairs, correspondence_pairs_host, ransac_hypotheses,   # noqa: F401,E402
                                  ransac_hypotheses_host, score_hypotheses, score_hypotheses_host, ransac_registration,
                                  ransac_registration_host, global_registration, global_registration_host, RansacResult)
from .spectral import (spectral_consistency, spectral_consistency_host, prune_correspondences,          # noqa: F401,E402
                       prune_correspondences_host, rerank_candidates, rerank_candidates_host, SpectralResult, RerankResult)
from .consensus import (consensus_hypotheses, consensus_hypotheses_host, consensus_registration,        # noqa: F401,E402
                        consensus_registration_host)
from .losses import (BatchHardTripletLossWithMasks, BatchHardContrastiveLossWithMasks, batch_hard_mine,  # noqa: F401,E402
                     batch_hard_mine_host, batch_hard_triplet_host, batch_hard_contrastive_host, make_loss_fn)
from .training import expand_batch_size, should_expand_batch                                            # noqa: F401,E402

__version__ = '0.1.0'
