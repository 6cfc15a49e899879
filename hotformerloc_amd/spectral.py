"""Spectral geometric verification of submap pairs from point correspondences, and the re-ranking of retrieved candidates by
it, on the GPU.

`FlatL2Index.search` orders a query's candidates by descriptor distance alone.  The geometry chain of this package
(`estimate_normals` -> `compute_fpfh` -> `feature_correspondences`) gives putative point pairs for any (query, candidate);
this module scores how many of them agree with ONE rigid motion without estimating that motion: spectral matching (Leordeanu
& Hebert 2005) on the length-consistency matrix of PointDSC / SC2-PCR, used for re-ranking as in SpectralGV (Vidanapathirana
et al. 2023).  Parity with the SpectralGV repository is not claimed (it keeps the diagonal of the matrix and matches learned
local features): what is computed is stated here, and the `*_host` functions are this text in numpy.

    spectral_consistency   the leading eigenvalue of every pair's consistency matrix, the score, the eigenvector
    prune_correspondences  the `keep` correspondences of largest eigenvector weight per pair, for `ransac_registration`
    rerank_candidates      (Q, k) retrieved candidates -> the same candidates by descending score, optionally the pose of
                           every query's new top-1

Definition (DESIGN.md section 7p has the reasons).  `source`, `target` and `correspondences` are those of
`ransac_registration`, gathered once into fp32 point pairs (p_c, q_c), c = 0 .. C - 1 of each pair.  Options: sigma =
`distance_threshold` > 0 and K = `iterations` >= 1.

  Matrix entry, for i != j, all in fp32: d = p_i - p_j component-wise, a = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx dx))) (the d2
  chain of the pair scan and the correctly rounded root), b the same on q_i - q_j, e = a - b, m_ij = max(0, fmaf(-(e e), s,
  1)) with s = fp32(1 / float64(sigma)^2).  m_ii = 0: a lone correspondence supports nothing.  m_ij and m_ji carry the same
  bits.

  Iteration.  v_0 is all ones.  For k = 1 .. K: w_i = sum_j m_ij v_{k-1,j} as the fp32 chain acc = fmaf(m_ij, v_j, acc) from
  acc = 0 over j ascending; in float64 r = sum v_i w_i, n = sum v_i^2, s2 = sum w_i^2; lambda_k = r / n; v_k,i = w_i /
  fp32(sqrt(s2)), an fp32 division.  If s2 == 0 (C < 2, or no two correspondences are consistent) the pair ends with
  eigenvalue 0 and all weights 0.

  Result.  `eigenvalue` = lambda_K; `score` = lambda_K / max(N_source, 1), N_source the number of points of the pair's source
  cloud (not C: a candidate with five mutual matches must not score as high as one with five hundred); `weights` = v_K, fp32,
  non-negative and of unit norm, in the layout of the correspondences.

Deliberately absent: an early stop, a host read inside the loop, float atomics.  Two runs give the same bits, and so do two
values of any tiling constant: a row's sum runs over ascending j in one thread.

The device functions raise `NativeLibraryError` on CPU clouds and launch on the current stream (csrc/spectral.hip): K launches
of `hfl_spectral_matvec` (the hot path: 512 rows in the registers of a workgroup against all the pair's correspondences
streaming through LDS, the matrix never in memory; the normalisation of step k is done by step k + 1 as it loads v) and one of
`hfl_spectral_finish`.  The results are read once at the end.

The host twin emulates the fp32 steps as `registration.py` does (an fmaf through one float64 operation) and sums the three
float64 quantities in numpy's order: the weights of the two routes agree to the bit wherever that emulation's double rounding
and the order of the float64 sums do not show, and to a few fp32 ulps of the largest weight otherwise.
"""

import importlib
from collections import namedtuple

import numpy as np
import torch

from . import registration as reg
from .overlap import _as_numpy, _fmaf, _host_d2_32, _ragged

# the package binds the function `global_registration` under the module's name: `_Batch`, `_HostBatch` and `_corr_rows` are
# the module's
GR = importlib.import_module('hotformerloc_amd.global_registration')

SpectralResult = namedtuple('SpectralResult', ['eigenvalue', 'score', 'weights'])
SpectralResult.__doc__ = """What `spectral_consistency` returns.  eigenvalue: (P,) float64 numpy, lambda_K of the module
docstring; score: (P,) float64 numpy, eigenvalue / max(N_source, 1); weights: v_K in the layout of the correspondences, a list
of (C_i,) float32 arrays or their concatenation for the `(rows, offsets)` form -- device tensors from `spectral_consistency`,
numpy from `spectral_consistency_host`."""

RerankResult = namedtuple('RerankResult', ['indices', 'scores', 'order'])
RerankResult.__doc__ = """What `rerank_candidates` returns: indices (Q, k) int64, every query's candidates by descending score
(the earlier retrieval rank on a tie; unused slots, index -1, last) -- what `recall_from_indices` takes; scores (Q, k) float64
in that order, -1 for an unused slot; order (Q, k) int64, the permutation applied: indices = candidates[q, order[q]].  Device
tensors from `rerank_candidates`, numpy from `rerank_candidates_host`."""


# ----------------------------------------------------------------------------------------------------------------- arguments
def _options(distance_threshold, iterations, what):
    sigma = float(distance_threshold)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError('%s: distance_threshold must be a finite number > 0' % what)
    if int(iterations) != iterations or iterations < 1:
        raise ValueError('%s: iterations must be an integer >= 1' % what)
    with np.errstate(over='ignore'):
        inv_s2 = np.float32(1.0 / (np.float64(sigma) * np.float64(sigma)))
    if not (inv_s2 > 0.0 and np.isfinite(inv_s2)):
        raise ValueError('%s: 1 / distance_threshold^2 must be a finite float32 > 0' % what)
    return inv_s2, int(iterations)


def _split(flat, c_off, as_list):
    return [flat[c_off[i]:c_off[i + 1]] for i in range(c_off.shape[0] - 1)] if as_list else flat


# -------------------------------------------------------------------------------------------------------------- device route
def spectral_consistency(source, target, correspondences, *, distance_threshold=0.4, iterations=10):
    """The spectral consistency of the correspondences of P pairs, as the module's docstring defines it ->
    `SpectralResult`.  The arguments and their refusals are those of `ransac_registration`.  `iterations` + 1 launches on the
    current stream without a host read; eigenvalue and score are read once at the end, the weights stay on the device."""
    from . import ops
    what = 'spectral_consistency'
    inv_s2, iters = _options(distance_threshold, iterations, what)
    b = GR._Batch(source, target, correspondences, what)
    dev = b.device
    with torch.cuda.device(dev):
        tiles, tile_off = ops.spectral_tiles(np.diff(b.c_off))
        n_tiles = int(tiles.shape[0])
        tiles, tile_off = torch.from_numpy(tiles).to(dev), torch.from_numpy(tile_off).to(dev)
        n_source = torch.from_numpy(b.n_source.astype(np.int64)).to(dev)
        w = [torch.zeros(int(b.corr.shape[0]), dtype=torch.float32, device=dev) for _ in range(2)]
        partials = [torch.zeros((max(n_tiles, 1), ops.SPECTRAL_SUMS), dtype=torch.float64, device=dev) for _ in range(2)]
        w_in = p_in = None
        for k in range(iters):                                         # step k + 1 normalises what step k wrote
            w_in, p_in = ops.spectral_matvec(b.corr, b.c_dev, tiles, tile_off, float(inv_s2), w_in, p_in, w[k % 2],
                                             partials[k % 2])
        eigenvalue, score, weights = ops.spectral_finish(w_in, p_in, n_tiles, tile_off, b.corr, b.c_dev, n_source)
        eigenvalue, score = eigenvalue.cpu().numpy(), score.cpu().numpy()
    return SpectralResult(eigenvalue, score, _split(weights, b.c_off, isinstance(correspondences, list)))


def _prune(correspondences, weights, keep, to_rows, xp, what):
    as_list = isinstance(correspondences, list)
    if int(keep) != keep or keep < 0:
        raise ValueError('%s: keep must be an integer >= 0' % what)
    if isinstance(weights, list) != as_list:
        raise ValueError('%s: weights must come in the layout of the correspondences' % what)
    if not as_list and not (isinstance(correspondences, tuple) and len(correspondences) == 2):
        raise ValueError('%s: correspondences: a list of (C_i, 2) integer arrays or a (rows, offsets) tuple expected' % what)
    pairs = len(correspondences) if as_list else int(_as_numpy(correspondences[1]).shape[0]) - 1
    parts, c_off = GR._corr_rows(correspondences, pairs, what, to_rows)
    w_parts = [to_rows(x) for x in (weights if as_list else [weights])]
    if len(w_parts) != len(parts) or any(x.ndim != 1 or x.shape[0] != c.shape[0] for x, c in zip(w_parts, parts)):
        raise ValueError('%s: one weight per correspondence expected' % what)
    for x in w_parts:
        if x.dtype not in (torch.float32, np.dtype(np.float32)):
            raise TypeError('%s: float32 weights expected, got %s' % (what, x.dtype))
    n = int(c_off[-1])
    lengths = np.diff(c_off)
    if xp is np:
        rows, w = np.concatenate(parts, 0), np.concatenate(w_parts, 0)
        pair = np.repeat(np.arange(pairs, dtype=np.int64), lengths)
        order = np.lexsort((-w, pair))                                 # stable: the lower row of equal weights comes first
        rank = np.arange(n, dtype=np.int64) - c_off[:-1][pair[order]]
        mask = np.zeros(n, bool)
        mask[order[(rank < keep) & (w[order] > 0)]] = True
        kept, counts = rows[mask], np.bincount(pair[mask], minlength=pairs)
    else:
        dev = parts[0].device
        rows, w = torch.cat(parts, 0), torch.cat([x.to(dev) for x in w_parts], 0)
        pair = torch.repeat_interleave(torch.arange(pairs, device=dev), torch.from_numpy(lengths).to(dev))
        by_weight = torch.sort(w, descending=True, stable=True).indices
        order = by_weight[torch.sort(pair[by_weight], stable=True).indices]
        rank = torch.arange(n, device=dev) - torch.from_numpy(c_off[:-1].copy()).to(dev)[pair[order]]
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[order[(rank < keep) & (w[order] > 0)]] = True
        kept = rows[mask]
        counts = torch.bincount(pair[mask], minlength=pairs).cpu().numpy()
    off = np.zeros(pairs + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return _split(kept, off, True) if as_list else (kept, off)


def prune_correspondences(correspondences, weights, keep):
    """Per pair the `keep` correspondences of largest weight (`SpectralResult.weights`), the lower row of equal weights, a
    row of weight 0 never; returned in their original order and in the layout given -- a list of (C_i, 2) tensors, or
    `((C, 2) rows, (P + 1,) int64 numpy offsets)` -- so that it feeds `ransac_registration` directly.  Tensors stay on their
    device (two stable sorts and a mask, no kernel of its own); `prune_correspondences_host` is the numpy route."""
    return _prune(correspondences, weights, keep, torch.as_tensor, torch, 'prune_correspondences')


def prune_correspondences_host(correspondences, weights, keep):
    """`prune_correspondences` in numpy."""
    return _prune(correspondences, weights, keep, _as_numpy, np, 'prune_correspondences')


def rerank_candidates(query_clouds, database_clouds, candidates, *, nb_neighbors=30, mutual=False, distance_threshold=0.4,
                      iterations=10, register=False, keep=None, ransac_distance=0.8, icp_distance=0.8,
                      estimation='point_to_plane', hypotheses=4096, seed=0, edge_length_ratio=0.9, refine_iterations=3,
                      min_correspondences=3, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6,
                      estimator='ransac', consensus_distance=0.4, seeds=64, consensus_size=10,
                      covariance_epsilon=1e-3, normal_radius=None, feature_radius=None, salient_radius=None,
                      non_max_radius=None):
    """Re-rank the candidates of a search by spectral consistency.  `query_clouds`: a list of Q raw (N_i, 3) float32 GPU
    clouds; `database_clouds`: the list of the database's clouds, of which only the named ones are touched; `candidates`:
    the (Q, k) index tensor of `FlatL2Index.search`, -1 for an unused slot.  Normals and FPFH are computed once per
    distinct cloud (the queries and the union of the named database rows); one `feature_correspondences` (`mutual`) and one
    `spectral_consistency` call (`distance_threshold`, `iterations`) cover all Q k pairs, the query as the source.  ->
    `RerankResult`.  With `register`, every query's new top-1 pair also goes through `prune_correspondences` (where `keep`
    is given) -> `ransac_registration` -> `icp_refine` on the features already computed, with the options of
    `global_registration` (`estimator='consensus'` and its three options included; `estimation='generalized'` takes the
    query's normals as the source's, with `covariance_epsilon`): -> `(RerankResult, RansacResult,
    RegistrationResult)`, query frame -> candidate frame, one row per query; a query without a candidate is then a
    `ValueError`.  `normal_radius` and `feature_radius` as in `global_registration`, and so are `salient_radius` and
    `non_max_radius`: `iss_keypoints` once per distinct cloud; the matcher, the score, the pruning and the coarse
    estimator on the keypoints' rows (the query's number of keypoints takes the place of its size in the score); the ICP
    on the full clouds."""
    from .fpfh import compute_fpfh, feature_correspondences
    from .normals import estimate_normals
    normals_of, fpfh_of = GR._with_radii(estimate_normals, compute_fpfh, nb_neighbors, normal_radius, feature_radius,
                                         'rerank_candidates')
    return _rerank(query_clouds, database_clouds, candidates, normals_of, fpfh_of, feature_correspondences,
                   GR.correspondence_pairs, spectral_consistency, prune_correspondences,
                   GR._coarse_estimator(estimator, True, 'rerank_candidates', ransac_distance, refine_iterations,
                                        min_correspondences, hypotheses, seed, edge_length_ratio, consensus_distance, seeds,
                                        consensus_size),
                   reg.icp_refine, True, nb_neighbors, mutual, distance_threshold, iterations, register, keep,
                   dict(max_correspondence_distance=icp_distance, max_iterations=max_iterations,
                        relative_fitness=relative_fitness, relative_rmse=relative_rmse,
                        min_correspondences=min_correspondences, estimation=estimation,
                        covariance_epsilon=covariance_epsilon),
                   GR._keypoints_of(salient_radius, non_max_radius, True, 'rerank_candidates'))


def _rerank(queries, database, candidates, normals_of, fpfh_of, match, pairs_of, spectral, prune, coarse_of, icp,
            device_route, nb, mutual, sigma, iterations, register, keep, icp_kw, keypoints_of=None):
    what = 'rerank_candidates'
    if not isinstance(queries, list) or not isinstance(database, list) or not queries or not database:
        raise ValueError('%s: two lists of (N_i, 3) clouds expected' % what)
    if icp_kw['estimation'] not in reg.ESTIMATIONS:
        raise ValueError('%s: estimation must be one of %s, got %r' % (what, ', '.join(reg.ESTIMATIONS), icp_kw['estimation']))
    reg._epsilon(icp_kw['covariance_epsilon'], what)
    _options(sigma, iterations, what)
    if keep is not None and (int(keep) != keep or keep < 0):
        raise ValueError('%s: keep must be None or an integer >= 0' % what)
    cand = _as_numpy(candidates)
    if cand.ndim != 2 or cand.shape[0] != len(queries) or not np.issubdtype(cand.dtype, np.integer):
        raise ValueError('%s: (%d, k) integer candidates expected, got shape %s' % (what, len(queries), tuple(cand.shape)))
    cand = cand.astype(np.int64)
    if (cand < -1).any() or (cand >= len(database)).any():
        raise ValueError('%s: a candidate names a row outside the database (%d clouds)' % (what, len(database)))
    named = np.unique(cand[cand >= 0])
    _ragged(queries, what, device_route)                               # the refusals, before anything is computed
    if named.shape[0]:
        _ragged([database[i] for i in named], what, device_route)
    n_q, k = cand.shape
    slot_q, slot_j = np.nonzero(cand >= 0)                             # the pairs, query by query in retrieval order
    scores = np.full((n_q, k), -1.0, np.float64)
    corr = weights = normals = points = None
    place = np.full(len(database), -1, np.int64)
    place[named] = n_q + np.arange(named.shape[0])
    if slot_q.shape[0]:
        clouds = list(queries) + [database[i] for i in named]
        normals = normals_of(clouds, nb)
        features = fpfh_of(clouds, normals, nb)
        points, rows = GR._at_keypoints(clouds, features, keypoints_of, device_route)
        at_t = place[cand[slot_q, slot_j]]
        matched = match([rows[q] for q in slot_q], [rows[t] for t in at_t], mutual=mutual)
        corr = pairs_of(matched[0], matched[2] if mutual else None)
        res = spectral([points[q] for q in slot_q], [points[t] for t in at_t], corr, distance_threshold=sigma,
                       iterations=iterations)
        scores[slot_q, slot_j], weights = res.score, res.weights
    order = np.argsort(-scores, axis=1, kind='stable')                 # the earlier rank of equal scores; -1 slots last
    indices, scores = np.take_along_axis(cand, order, 1), np.take_along_axis(scores, order, 1)
    if device_route:
        dev = torch.as_tensor(queries[0]).device
        ranked = RerankResult(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (indices, scores, order)))
    else:
        ranked = RerankResult(indices, scores, order)
    if not register:
        return ranked
    if k == 0 or (indices[:, 0] < 0).any():
        raise ValueError('%s: register=True needs a candidate for every query' % what)
    pair_of = np.full((n_q, k), -1, np.int64)
    pair_of[slot_q, slot_j] = np.arange(slot_q.shape[0])
    top = pair_of[np.arange(n_q), order[:, 0]]
    top_corr = [corr[i] for i in top]
    if keep is not None:
        top_corr = prune(top_corr, [weights[i] for i in top], keep)
    src, dst = [clouds[q] for q in range(n_q)], [clouds[place[i]] for i in indices[:, 0]]
    coarse = coarse_of([points[q] for q in range(n_q)], [points[place[i]] for i in indices[:, 0]], top_corr)
    plane, generalized = icp_kw['estimation'] != 'point_to_point', icp_kw['estimation'] == 'generalized'
    fine = icp(src, dst, init=coarse.transforms, target_normals=[normals[place[i]] for i in indices[:, 0]] if plane else None,
               source_normals=[normals[q] for q in range(n_q)] if generalized else None, **icp_kw)
    return ranked, coarse, fine


# ---------------------------------------------------------------------------------------------------------------- host route
def _host_matrix(p, q, inv_s2):
    """(C, C) float32 M of one pair, the diagonal 0"""
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.sqrt(_host_d2_32(p, p)) - np.sqrt(_host_d2_32(q, q))    # float32 throughout; numpy's root is correctly rounded
        m = np.maximum(np.float32(0.0), _fmaf(-(e * e), np.full((), inv_s2, np.float32), np.full((), 1.0, np.float32)))
    np.fill_diagonal(m, np.float32(0.0))
    return m


def _host_power_iteration(m, iterations):
    """(lambda_K float64, v_K (C,) float32) of one pair's matrix"""
    n_corr = m.shape[0]
    v = np.ones(n_corr, np.float32)
    eigenvalue = 0.0
    for _ in range(iterations):
        w = np.zeros(n_corr, np.float32)
        for j in range(n_corr):                                        # the fp32 chain over ascending j; row j is column j
            w = _fmaf(m[j], v[j:j + 1], w)
        v64, w64 = v.astype(np.float64), w.astype(np.float64)
        r, n, s2 = (v64 * w64).sum(), (v64 * v64).sum(), (w64 * w64).sum()
        if not s2 > 0.0:
            return 0.0, np.zeros(n_corr, np.float32)
        eigenvalue = float(r / n)
        v = w / np.float32(np.sqrt(s2))
    return eigenvalue, v


def spectral_consistency_host(source, target, correspondences, *, distance_threshold=0.4, iterations=10):
    """`spectral_consistency` on the CPU: the module's definition in numpy, pair by pair, the matrix in memory (for tests
    and small sets of correspondences) -> `SpectralResult` of numpy arrays."""
    what = 'spectral_consistency'
    inv_s2, iters = _options(distance_threshold, iterations, what)
    b = GR._HostBatch(source, target, correspondences, what)
    eigenvalue, weights = np.zeros(b.pairs, np.float64), []
    for i in range(b.pairs):
        if b.p[i].shape[0] == 0:
            weights.append(np.zeros(0, np.float32))
            continue
        eigenvalue[i], v = _host_power_iteration(_host_matrix(b.p[i], b.q[i], inv_s2), iters)
        weights.append(v)
    score = eigenvalue / np.maximum(b.n_source, 1).astype(np.float64)
    as_list = isinstance(correspondences, list)
    return SpectralResult(eigenvalue, score, weights if as_list else np.concatenate(weights + [np.zeros(0, np.float32)]))


def rerank_candidates_host(query_clouds, database_clouds, candidates, *, nb_neighbors=30, mutual=False, distance_threshold=0.4,
                           iterations=10, register=False, keep=None, ransac_distance=0.8, icp_distance=0.8,
                           estimation='point_to_plane', hypotheses=4096, seed=0, edge_length_ratio=0.9, refine_iterations=3,
                           min_correspondences=3, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6,
                           estimator='ransac', consensus_distance=0.4, seeds=64, consensus_size=10,
                           covariance_epsilon=1e-3, normal_radius=None, feature_radius=None, salient_radius=None,
                           non_max_radius=None):
    """`rerank_candidates` on the CPU, from the numpy twins of every step (brute force: for tests and small clouds)."""
    from .fpfh import compute_fpfh_host, feature_correspondences_host
    from .normals import estimate_normals_host
    normals_of, fpfh_of = GR._with_radii(estimate_normals_host, compute_fpfh_host, nb_neighbors, normal_radius,
                                         feature_radius, 'rerank_candidates')
    return _rerank(query_clouds, database_clouds, candidates, normals_of, fpfh_of,
                   feature_correspondences_host, GR.correspondence_pairs_host, spectral_consistency_host,
                   prune_correspondences_host,
                   GR._coarse_estimator(estimator, False, 'rerank_candidates', ransac_distance, refine_iterations,
                                        min_correspondences, hypotheses, seed, edge_length_ratio, consensus_distance, seeds,
                                        consensus_size),
                   reg.icp_refine_host, False, nb_neighbors, mutual, distance_threshold, iterations, register, keep,
                   dict(max_correspondence_distance=icp_distance, max_iterations=max_iterations,
                        relative_fitness=relative_fitness, relative_rmse=relative_rmse,
                        min_correspondences=min_correspondences, estimation=estimation,
                        covariance_epsilon=covariance_epsilon),
                   GR._keypoints_of(salient_radius, non_max_radius, False, 'rerank_candidates'))
