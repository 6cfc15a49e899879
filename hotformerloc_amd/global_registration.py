"""Global registration of a ragged batch of submap pairs: RANSAC over point correspondences, feeding ICP, on the GPU.

`icp_refine` needs a starting pose.  A pair that came with surveyed poses has one (`SubmapOverlap.transforms`); a candidate
that `FlatL2Index.search` merely retrieved has none, and the identity fails once the revisit is turned or a few metres off.
`feature_correspondences` on `compute_fpfh` descriptors gives point pairs of which most are wrong; this module finds the
rigid pose most of the rest agree on.  open3d is not a dependency and parity with its `registration_ransac_based_on_
correspondence` is not claimed (it stops early on a confidence estimate and draws from a thread-dependent generator): what
is computed is stated here, and the `*_host` functions are this text in numpy.

    correspondence_pairs   the (C_i, 2) [source row, target row] pairs of a `feature_correspondences` result
    ransac_hypotheses      H candidate poses per pair from drawn triples of correspondences
    score_hypotheses       the inlier count of every candidate
    ransac_registration    draw (or take the caller's candidates), score, select, polish -> `RansacResult`
    global_registration    two raw clouds -> normals -> FPFH -> correspondences -> RANSAC -> ICP, in one call; with
                           `estimator='consensus'` the coarse pose comes from `consensus_registration` (`consensus.py`), which
                           shares the score -> select -> polish below (`_select_and_polish`)

The package exports the function `global_registration` under the name of this module; the module itself (`inlier_d2`,
`NO_HYPOTHESIS`) is `importlib.import_module('hotformerloc_amd.global_registration')`.

Definition (DESIGN.md section 7n has the reasons).  `source` and `target` come in the layouts of `overlap.py`;
`correspondences` is a list of (C_i, 2) integer arrays [source row, target row] local to the pair, or `((C, 2) rows,
(P + 1,) offsets)`.  The rows are gathered once into fp32 point pairs (p_c, q_c), c = 0 .. C - 1.  A row out of range is a
`ValueError`.

  Hypotheses, h = 0 .. H - 1 of pair number `pair`.  (x0, x1, x2, _) = philox4x32_10(counter = (h, pair, 0, 0), key = seed)
  (`augment.philox4x32_10`; the key is the seed's low and high 32 bits); the sample rows are i_k = (uint64(x_k) . C) >> 32,
  reported as `draws` in any case.  A hypothesis is INVALID when C < 3; or two of the three rows are equal; or the edge-length
  check fails: for the index pairs (0,1), (0,2), (1,2), in float64 with one rounding per operation, ls = (dx dx + dy dy) +
  dz dz between the source points and lt likewise between the target points, and both ls >= rho2 lt and lt >= rho2 ls are
  required, rho2 = float64(edge_length_ratio)^2 (a ratio of 0 disables the check); or the Kabsch solve reports rank < 2.  That
  solve is `kabsch_solve` of csrc/kabsch.h, the one of the ICP (`registration._host_kabsch_one`), on the 17 float64 sums of
  the three pairs added in the order 0, 1, 2 (n = 3, sum d^2 = 0).  The pose is rounded to fp32: twelve values, the row-major
  (R | t) `hfl_transform_points` takes.  An invalid hypothesis has a pose of twelve NaNs.

  Score.  For every correspondence p' = the fmaf chain of `hfl_transform_points` on p (acc = fmaf(r0, x, t); acc = fmaf(r1,
  y, acc); fmaf(r2, z, acc)) and d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) on p' - q, in fp32.  It is an inlier iff d2 <= D2,
  D2 the largest finite fp32 with sqrtf(D2) <= fp32(max_correspondence_distance) (`inlier_d2` finds it by stepping
  `nextafter` around the square).  The correctly rounded root is monotone, so this is the predicate of the ICP, sqrt(d2) <=
  fp32(tau), without a root per test.  count_h is the number of inliers, -1 for an invalid hypothesis.  Counts are integers:
  their value does not depend on the order of summation.  Where the caller gives poses and no flags, a hypothesis is valid
  iff its twelve values are finite.

  Select.  The largest count, the lowest h on a tie.  If every count is -1 the pair ends NO_HYPOTHESIS (status 5, beside the
  codes of `registration.py`) with the identity, fitness 0 and rmse NaN.

  Polish.  The evaluate / update loop of `icp_refine` with the correspondences fixed and no convergence rule.  T_0 =
  float64(the selected fp32 pose).  For k = 0 .. refine_iterations: the inliers of fp32(T_k) by the predicate above; the 17
  float64 sums n, Sp, Sq, Spq, sum d^2 over them (d = sqrtf(d2), as in the ICP); fitness = n / C and rmse = sqrt(sum d^2 /
  n).  n < min_correspondences: TOO_FEW, rmse NaN.  k == refine_iterations: MAX_ITERATIONS, the normal end.  A degenerate
  update (rank < 2): DEGENERATE.  Otherwise T_{k+1} = [R | t] . T_k in float64.  The returned figures always belong to the
  returned pose.

Deliberately absent: an early stop on confidence, a host read inside the loop, float atomics.  Two runs give the same
bits, and so do two values of any tiling constant.

The device functions raise `NativeLibraryError` on CPU clouds and launch on the current stream (csrc/global_registration.hip):
`hfl_ransac_hypotheses` (one thread per hypothesis), `hfl_ransac_score` (the hot path: 512 hypotheses in the registers of a
workgroup against 1024 correspondences in LDS, integer atomic adds between the tiles of a pair), `hfl_ransac_select`, and
per polish iteration `hfl_ransac_sums` and the `hfl_icp_solve` of the ICP itself, with relative thresholds 0 and the
correspondence offsets as its denominators.  The results are read once at the end.

The host twins emulate the fp32 steps as `registration.py` does (an fmaf through one float64 operation) and sum in numpy's
order: the two routes agree in draws, flags and counts wherever no d2 lies within rounding of D2 and no edge or rank ratio
within rounding of its threshold, and in poses to rounding.
"""

from collections import namedtuple

import numpy as np
import torch

from . import augment
from . import registration as reg
from .overlap import _as_numpy, _fmaf, _host_ragged, _ragged, _same_pairs
# the statuses of a `RansacResult` and the solver's constants are names of this module too
from .registration import DEGENERATE, MAX_ITERATIONS, RANK_TOL, RUNNING, TOO_FEW, JACOBI_SWEEPS, N_SUMS      # noqa: F401
from .registration import _host_kabsch_many

NO_HYPOTHESIS = 5                      # HFL_RANSAC_NO_HYPOTHESIS: every hypothesis of the pair was invalid
ESTIMATORS = ('ransac', 'consensus')   # who makes the candidates of the coarse pose: drawn triples, or `consensus.py`
_HOST_CHUNK = 1 << 21                  # (hypothesis, correspondence) tests of one temporary of the numpy route

RansacResult = namedtuple('RansacResult', ['transforms', 'fitness', 'inlier_rmse', 'inliers', 'hypothesis',
                                           'hypothesis_inliers', 'valid_hypotheses', 'status'])
RansacResult.__doc__ = """What `ransac_registration` returns, numpy arrays on the host.  transforms: (P, 4, 4) float64, source
frame -> target frame; fitness: (P,) float64, the share of the pair's correspondences that are inliers of that pose;
inlier_rmse: (P,) float64 over them, NaN where the pair is TOO_FEW or NO_HYPOTHESIS; inliers: (P,) int64, their number;
hypothesis: (P,) int64, the selected h, -1 for NO_HYPOTHESIS; hypothesis_inliers: (P,) int64, its count before the polish (-1
likewise); valid_hypotheses: (P,) int64; status: (P,) int64, one of MAX_ITERATIONS (the normal end), TOO_FEW, DEGENERATE,
NO_HYPOTHESIS."""


# ----------------------------------------------------------------------------------------------------------------- arguments
def _options(hypotheses, seed, edge_length_ratio, what):
    if int(hypotheses) != hypotheses or hypotheses < 1:
        raise ValueError('%s: hypotheses must be an integer >= 1' % what)
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError('%s: seed must be an integer of 64 bits, >= 0' % what)
    rho = float(edge_length_ratio)
    if not 0.0 <= rho <= 1.0:
        raise ValueError('%s: edge_length_ratio must be a number in [0, 1]' % what)
    return int(hypotheses), int(seed), float(np.float64(rho) * np.float64(rho))


def _polish_options(max_correspondence_distance, refine_iterations, min_correspondences, what):
    d, iters, _, _, min_corr = reg._options(max_correspondence_distance, refine_iterations, 0.0, 0.0, min_correspondences, what,
                                            'refine_iterations')
    return d, iters, min_corr


def inlier_d2(max_correspondence_distance):
    """D2 of the module docstring: the largest finite float32 whose correctly rounded float32 root is <= float32(tau)."""
    tau = np.float32(max_correspondence_distance)
    if not tau >= 0.0:
        raise ValueError('max_correspondence_distance must be a number >= 0')
    top = np.finfo(np.float32).max
    with np.errstate(over='ignore'):
        x = np.float32(min(tau * tau, top))
    while np.sqrt(x) > tau:
        x = np.nextafter(x, np.float32(-np.inf))
    while x < top and np.sqrt(np.nextafter(x, np.float32(np.inf))) <= tau:
        x = np.nextafter(x, np.float32(np.inf))
    return np.float32(x)


def _key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def _corr_rows(correspondences, pairs, what, to_rows):
    """(rows (C, 2) int64 as `to_rows` makes them, offsets (P + 1,) int64 numpy) of a list of (C_i, 2) integer arrays or a
    `(rows, offsets)` tuple"""
    as_list = isinstance(correspondences, list)
    if not as_list and not (isinstance(correspondences, tuple) and len(correspondences) == 2):
        raise ValueError('%s: correspondences: a list of (C_i, 2) integer arrays or a (rows, offsets) tuple expected' % what)
    parts = [to_rows(c) for c in (correspondences if as_list else [correspondences[0]])]
    for c in parts:
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError('%s: (C, 2) correspondence rows expected, got shape %s' % (what, tuple(c.shape)))
        if c.dtype not in (torch.int32, torch.int64, np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError('%s: int32 or int64 correspondence rows expected, got %s' % (what, c.dtype))
    if as_list:
        if len(parts) != pairs:
            raise ValueError('%s: %d sets of correspondences for %d pairs: they must pair up' % (what, len(parts), pairs))
        off = np.zeros(pairs + 1, np.int64)
        np.cumsum([c.shape[0] for c in parts], out=off[1:])
        return parts, off
    offsets = correspondences[1]
    off = _as_numpy(offsets)
    if off.ndim != 1 or off.shape[0] != pairs + 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError('%s: (%d,) integer correspondence offsets expected: they must pair up with the clouds'
                         % (what, pairs + 1))
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != parts[0].shape[0] or (np.diff(off) < 0).any():
        raise ValueError('%s: correspondence offsets must start at 0, not decrease, and end at the number of rows (%d)'
                         % (what, parts[0].shape[0]))
    return parts, off


def _poses_of(poses, pairs, what):
    """(P, H, 12) float32 as given (numpy or tensor) from (P, H, 3, 4)"""
    shape = tuple(poses.shape)
    if len(shape) != 4 or shape[0] != pairs or shape[1] < 1 or shape[2:] != (3, 4):
        raise ValueError('%s: (%d, H >= 1, 3, 4) poses expected, got shape %s' % (what, pairs, shape))
    if poses.dtype not in (torch.float32, np.dtype(np.float32)):
        raise TypeError('%s: float32 poses expected, got %s' % (what, poses.dtype))
    return poses.reshape(pairs, shape[1], 12)


def _valid_of(valid, pairs, n_hyp, what):
    shape = tuple(valid.shape)
    if shape != (pairs, n_hyp):
        raise ValueError('%s: (%d, %d) flags expected, got shape %s' % (what, pairs, n_hyp, shape))
    if valid.dtype not in (torch.bool, np.dtype(bool)):
        raise TypeError('%s: bool flags expected, got %s' % (what, valid.dtype))
    return valid


# -------------------------------------------------------------------------------------------------------------- device route
class _Batch:
    """The correspondences of a batch of pairs on the device, gathered once: (C, 6) fp32 point pairs, their offsets, the
    tile table and its per-pair offsets; `n_source`: every pair's number of source points (numpy), for `spectral.py`."""

    def __init__(self, source, target, correspondences, what):
        from . import ops
        s, s_off, _ = _ragged(source, what, True)
        t, t_off, _ = _ragged(target, what, True)
        _same_pairs(s_off, t_off, what)
        self.pairs = s_off.shape[0] - 1
        self.n_source = np.diff(s_off)
        self.device = dev = s.device
        if t.device != dev:
            raise ValueError('%s: source and target lie on different devices' % what)
        parts, self.c_off = _corr_rows(correspondences, self.pairs, what, lambda c: torch.as_tensor(c))
        with torch.cuda.device(dev):
            rows = torch.cat([c.to(dev).to(torch.int64) for c in parts], 0)
            lengths = torch.from_numpy(np.diff(self.c_off)).to(dev)
            pair = torch.repeat_interleave(torch.arange(self.pairs, device=dev), lengths)
            n_s, n_t = torch.from_numpy(np.diff(s_off)).to(dev)[pair], torch.from_numpy(np.diff(t_off)).to(dev)[pair]
            # the one compare, before anything launches
            if bool(((rows < 0) | (rows >= torch.stack([n_s, n_t], 1))).any()):
                raise ValueError('%s: a correspondence names a row outside its cloud' % what)
            at_s = torch.from_numpy(s_off).to(dev)[pair] + rows[:, 0]
            at_t = torch.from_numpy(t_off).to(dev)[pair] + rows[:, 1]
            self.corr = torch.cat([s[at_s], t[at_t]], 1).contiguous()
            self.c_dev = torch.from_numpy(self.c_off).to(dev)
            tiles, tile_off = ops.ransac_tiles(np.diff(self.c_off))
            self.n_tiles = int(tiles.shape[0])
            self.tiles, self.tile_off = torch.from_numpy(tiles).to(dev), torch.from_numpy(tile_off).to(dev)

    def device_poses(self, poses, valid, what):
        """the caller's candidates as ((P, H, 12) fp32, (P, H) uint8) on the device"""
        poses = _poses_of(torch.as_tensor(poses), self.pairs, what).to(self.device).contiguous()
        if valid is None:
            valid = torch.isfinite(poses).all(2)
        else:
            valid = _valid_of(torch.as_tensor(valid), self.pairs, int(poses.shape[1]), what).to(self.device)
        return poses, valid.to(torch.uint8).contiguous()


def ransac_hypotheses(source, target, correspondences, *, hypotheses=4096, seed=0, edge_length_ratio=0.9):
    """H candidate poses for each of P pairs, as the module's docstring defines them, on the device -> `(poses (P, H, 3, 4)
    float32, valid (P, H) bool, draws (P, H, 3) int32)`, device tensors.  An invalid hypothesis has a pose of NaNs."""
    from . import ops
    what = 'ransac_hypotheses'
    n_hyp, seed, rho2 = _options(hypotheses, seed, edge_length_ratio, what)
    b = _Batch(source, target, correspondences, what)
    with torch.cuda.device(b.device):
        poses, valid, draws = ops.ransac_hypotheses(b.corr, b.c_dev, n_hyp, seed, rho2)
    return poses.view(b.pairs, n_hyp, 3, 4), valid.to(torch.bool), draws


def score_hypotheses(source, target, correspondences, poses, max_correspondence_distance, valid=None):
    """The inlier counts of given candidates on the device -> (P, H) int32 device tensor, -1 where `valid` ((P, H) bool) is
    False; without `valid` a candidate counts as valid iff its twelve values are finite.  `poses`: (P, H, 3, 4) float32."""
    from . import ops
    what = 'score_hypotheses'
    dist, _, _ = _polish_options(max_correspondence_distance, 0, 0, what)
    b = _Batch(source, target, correspondences, what)
    with torch.cuda.device(b.device):
        poses, valid = b.device_poses(poses, valid, what)
        return ops.ransac_score(b.corr, b.c_dev, b.tiles, poses, valid, float(inlier_d2(dist)))


def ransac_registration(source, target, correspondences, *, max_correspondence_distance=0.8, hypotheses=4096, seed=0,
                        edge_length_ratio=0.9, refine_iterations=3, min_correspondences=3, poses=None):
    """RANSAC on the correspondences of P pairs, as the module's docstring defines it -> `RansacResult`.  `poses`: (P, H, 3,
    4) float32 candidates of the caller's own in place of the drawn ones (a yaw sweep round a surveyed pose, say); one
    with a value that is not finite counts as invalid.  Everything is enqueued on the current stream without a host read;
    the results are read once at the end."""
    from . import ops
    what = 'ransac_registration'
    n_hyp, seed, rho2 = _options(hypotheses, seed, edge_length_ratio, what)
    dist, iters, min_corr = _polish_options(max_correspondence_distance, refine_iterations, min_correspondences, what)
    d2_max = float(inlier_d2(dist))
    b = _Batch(source, target, correspondences, what)
    with torch.cuda.device(b.device):
        if poses is None:
            poses, valid, _ = ops.ransac_hypotheses(b.corr, b.c_dev, n_hyp, seed, rho2)
        else:
            poses, valid = b.device_poses(poses, None, what)
        return _select_and_polish(b, poses, valid, d2_max, iters, min_corr)


def _select_and_polish(b, poses, valid, d2_max, iters, min_corr):
    """Score, select and polish of the module docstring on the candidates (poses (P, H, 12) fp32, valid (P, H) uint8) of a
    `_Batch`, whoever made them (`ransac_registration`, `consensus_registration`) -> `RansacResult`.  Enqueued on the current
    stream of the batch's device, which the caller has made current; the one read comes at the end."""
    from . import ops
    counts = ops.ransac_score(b.corr, b.c_dev, b.tiles, poses, valid, d2_max)
    state, istate, chosen = ops.ransac_select(counts, poses)
    partials = torch.zeros((max(b.n_tiles, 1), ops.ICP_SUMS), dtype=torch.float64, device=b.device)
    _, _, inliers = reg._iterate_on_device(
        state, istate, iters, lambda st, ist: ops.ransac_sums(b.corr, b.c_dev, b.tiles, st, ist, d2_max, partials=partials),
        lambda st, ist, is_last: ops.icp_solve(st, ist, partials, b.tile_off, b.n_tiles, b.c_dev, min_corr, 0.0, 0.0,
                                               is_last, want_sums=True), count=True)
    transforms, fitness, rmse, _, status = reg._read_state(state, istate)
    chosen, inliers = chosen.cpu().numpy().astype(np.int64), inliers.cpu().numpy().astype(np.int64)
    return RansacResult(transforms, fitness, rmse, inliers, chosen[:, 0].copy(), chosen[:, 1].copy(), chosen[:, 2].copy(),
                        status)


def _pairs_of(idx, mask, xp):
    """the kept (C, 2) int64 rows of one pair, in ascending source row"""
    keep = idx >= 0 if mask is None else (idx >= 0) & mask
    if xp is np:
        rows = np.nonzero(keep)[0].astype(np.int64)
        return np.stack([rows, idx[rows].astype(np.int64)], 1)
    rows = torch.nonzero(keep)[:, 0]
    return torch.stack([rows, idx[rows].to(torch.int64)], 1)


def _correspondence_pairs(idx, mask, as_array, xp, what):
    as_list = isinstance(idx, list)
    if not as_list and not (isinstance(idx, tuple) and len(idx) == 2):
        raise ValueError('%s: a list of (N_i,) index arrays or an (idx, offsets) tuple expected' % what)
    if mask is not None and isinstance(mask, list) != as_list:
        raise ValueError('%s: mask must come in the layout of idx' % what)
    parts = [as_array(i) for i in (idx if as_list else [idx[0]])]
    masks = None if mask is None else [as_array(m) for m in (mask if as_list else [mask])]
    if masks is not None and (len(masks) != len(parts) or any(tuple(m.shape) != tuple(i.shape) for m, i in zip(masks, parts))):
        raise ValueError('%s: mask must hold one flag per row of idx' % what)
    for i, part in enumerate(parts):
        if part.ndim != 1 or part.dtype not in (torch.int32, torch.int64, np.dtype(np.int32), np.dtype(np.int64)):
            raise TypeError('%s: (N,) int32 or int64 target rows expected' % what)
        if masks is not None and masks[i].dtype not in (torch.bool, np.dtype(bool)):
            raise TypeError('%s: bool mask expected' % what)
    if as_list:
        return [_pairs_of(part, None if masks is None else masks[i], xp) for i, part in enumerate(parts)]
    offsets = idx[1]
    off = _as_numpy(offsets)
    off = off.astype(np.int64)
    if off.ndim != 1 or off.shape[0] < 2 or off[0] != 0 or off[-1] != parts[0].shape[0] or (np.diff(off) < 0).any():
        raise ValueError('%s: offsets must start at 0, not decrease, and end at the number of rows (%d)'
                         % (what, parts[0].shape[0]))
    per_pair = [_pairs_of(parts[0][s:e], None if masks is None else masks[0][s:e], xp) for s, e in zip(off[:-1], off[1:])]
    c_off = np.zeros(off.shape[0], np.int64)
    np.cumsum([p.shape[0] for p in per_pair], out=c_off[1:])
    return (xp.concatenate(per_pair, 0) if xp is np else torch.cat(per_pair, 0)), c_off


def correspondence_pairs(idx, mask=None):
    """The point pairs of a `feature_correspondences` result: a list of per-pair (N_i,) `idx` (and `mask`) -> a list of
    (C_i, 2) int64 rows [source row, target row] with idx >= 0 (and mask), in ascending source row; an `(idx (N,), offsets
    (P + 1,))` tuple (and the concatenated mask) -> `((C, 2) rows, (P + 1,) int64 numpy offsets)`.  Tensors stay on their
    device; `correspondence_pairs_host` is the numpy route."""
    return _correspondence_pairs(idx, mask, torch.as_tensor, torch, 'correspondence_pairs')


def correspondence_pairs_host(idx, mask=None):
    """`correspondence_pairs` in numpy."""
    return _correspondence_pairs(idx, mask, _as_numpy, np, 'correspondence_pairs')


def _coarse_estimator(estimator, device_route, what, ransac_distance, refine_iterations, min_correspondences, hypotheses,
                      seed, edge_length_ratio, consensus_distance, seeds, consensus_size):
    """The coarse step of `global_registration` and `rerank_candidates(register=True)` as one callable (source, target,
    correspondences) -> `RansacResult`: 'ransac' is `ransac_registration` with `hypotheses`, `seed` and `edge_length_ratio`,
    'consensus' is `consensus_registration` with `consensus_distance`, `seeds` and `consensus_size`; both score and polish
    with `ransac_distance`, `refine_iterations` and `min_correspondences`."""
    if estimator not in ESTIMATORS:
        raise ValueError('%s: estimator must be one of %s, got %r' % (what, ', '.join(ESTIMATORS), estimator))
    kw = dict(max_correspondence_distance=ransac_distance, refine_iterations=refine_iterations,
              min_correspondences=min_correspondences)
    if estimator == 'ransac':
        run = ransac_registration if device_route else ransac_registration_host
        kw.update(hypotheses=hypotheses, seed=seed, edge_length_ratio=edge_length_ratio)
    else:
        from .consensus import consensus_registration, consensus_registration_host
        run = consensus_registration if device_route else consensus_registration_host
        kw.update(distance_threshold=consensus_distance, seeds=seeds, consensus_size=consensus_size)
    return lambda source, target, correspondences: run(source, target, correspondences, **kw)


def _with_radii(normals_of, fpfh_of, nb, normal_radius, feature_radius, what):
    """`normals_of(clouds, nb)` and `fpfh_of(clouds, normals, nb)` with the radii of `global_registration` and
    `rerank_candidates` bound: None leaves a step at its k nearest points; `nb` None is radius-only and needs both"""
    if nb is None and (normal_radius is None or feature_radius is None):
        raise ValueError('%s: nb_neighbors=None is the radius-only neighbourhood and needs normal_radius and feature_radius'
                         % what)
    return (normals_of if normal_radius is None else lambda clouds, k: normals_of(clouds, k, radius=normal_radius),
            fpfh_of if feature_radius is None else lambda clouds, normals, k: fpfh_of(clouds, normals, k, radius=feature_radius))


def _keypoints_of(salient_radius, non_max_radius, device_route, what):
    """None when both radii are None, else `iss_keypoints` (or its numpy twin) with the two radii bound and the gammas and
    `min_neighbors` at their defaults: clouds -> the per-cloud keypoint rows.  Only one radius: `ValueError`."""
    from . import keypoints
    radii = keypoints.check_radii(salient_radius, non_max_radius, what)
    if radii is None:
        return None
    run = keypoints.iss_keypoints if device_route else keypoints.iss_keypoints_host
    return lambda clouds: run(clouds, *radii)


def _at_keypoints(clouds, features, keypoints_of, device_route):
    """(clouds, features) as they are when `keypoints_of` is None, else their rows at the keypoints of every cloud, which
    may be none: what the matcher, the verification and the coarse estimator then work on"""
    if keypoints_of is None:
        return clouds, features
    rows = keypoints_of(clouds)
    as_rows = torch.as_tensor if device_route else _as_numpy
    return [as_rows(c)[k] for c, k in zip(clouds, rows)], [f[k] for f, k in zip(features, rows)]


def global_registration(source, target, *, nb_neighbors=30, mutual=True, ransac_distance=0.8, icp_distance=0.8,
                        estimation='point_to_plane', hypotheses=4096, seed=0, edge_length_ratio=0.9, refine_iterations=3,
                        min_correspondences=3, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6,
                        estimator='ransac', consensus_distance=0.4, seeds=64, consensus_size=10, covariance_epsilon=1e-3,
                        normal_radius=None, feature_radius=None, salient_radius=None, non_max_radius=None):
    """From two lists of raw (N_i, 3) float32 GPU clouds to refined 6-DoF poses, source frame -> target frame, in one call:
    `estimate_normals` -> `compute_fpfh` -> `feature_correspondences` (`mutual`) -> `correspondence_pairs` ->
    `ransac_registration` (`ransac_distance` and its options) -> `icp_refine(init=...)` (`icp_distance`, `estimation`, its
    options; point-to-plane uses the target normals already estimated, 'generalized' those and the source normals, with
    `covariance_epsilon`).  -> `(RansacResult, RegistrationResult)`.  A pair
    that ends NO_HYPOTHESIS enters the ICP at the identity.  `estimator='consensus'` takes the coarse pose from
    `consensus_registration` (`consensus_distance`, `seeds`, `consensus_size`; `ransac_distance`, `refine_iterations` and
    `min_correspondences` as before) instead; `hypotheses`, `seed` and `edge_length_ratio` are then unused.
    `normal_radius` and `feature_radius` are the `radius` of `estimate_normals` and of `compute_fpfh` (hybrid
    neighbourhoods); `nb_neighbors=None` is radius-only and needs both.
    `salient_radius` and `non_max_radius` (both, or neither) put `iss_keypoints` in front of the matcher, with its other
    parameters at their defaults: `feature_correspondences` then sees the descriptor rows at the keypoints only, and the
    coarse estimator their points, so both work on a few per cent of the rows.  Normals and FPFH are still computed on
    all points -- an FPFH row needs the SPFH of all its neighbours, so nothing is saved there -- and `icp_refine` still
    gets the full clouds and normals.  A cloud without a keypoint gives its pair no correspondence: NO_HYPOTHESIS, and
    the ICP from the identity.  With both None every result keeps its bits."""
    from .fpfh import compute_fpfh, feature_correspondences
    from .normals import estimate_normals
    coarse = _coarse_estimator(estimator, True, 'global_registration', ransac_distance, refine_iterations, min_correspondences,
                               hypotheses, seed, edge_length_ratio, consensus_distance, seeds, consensus_size)
    normals_of, fpfh_of = _with_radii(estimate_normals, compute_fpfh, nb_neighbors, normal_radius, feature_radius,
                                      'global_registration')
    return _global(source, target, normals_of, fpfh_of, feature_correspondences, correspondence_pairs, coarse,
                   reg.icp_refine, True, nb_neighbors, mutual, icp_distance, estimation, min_correspondences, max_iterations,
                   relative_fitness, relative_rmse, covariance_epsilon,
                   _keypoints_of(salient_radius, non_max_radius, True, 'global_registration'))


def _global(source, target, normals_of, fpfh_of, match, pairs_of, coarse_of, icp, device_route, nb, mutual, icp_distance,
            estimation, min_corr, max_iterations, rel_f, rel_r, epsilon=1e-3, keypoints_of=None):
    what = 'global_registration'
    if not isinstance(source, list) or not isinstance(target, list) or not source or len(source) != len(target):
        raise ValueError('%s: two lists of (N_i, 3) clouds that pair up expected' % what)
    if estimation not in reg.ESTIMATIONS:
        raise ValueError('%s: estimation must be one of %s, got %r' % (what, ', '.join(reg.ESTIMATIONS), estimation))
    reg._epsilon(epsilon, what)
    _ragged(source, what, device_route), _ragged(target, what, device_route)   # the refusals, before anything is computed
    pairs = len(source)
    normals = normals_of(source + target, nb)
    features = fpfh_of(source + target, normals, nb)
    points, rows = _at_keypoints(source + target, features, keypoints_of, device_route)
    matched = match(rows[:pairs], rows[pairs:], mutual=mutual)
    corr = pairs_of(matched[0], matched[2] if mutual else None)
    coarse = coarse_of(points[:pairs], points[pairs:], corr)
    plane, generalized = estimation != 'point_to_point', estimation == 'generalized'
    fine = icp(source, target, init=coarse.transforms, max_correspondence_distance=icp_distance,
               max_iterations=max_iterations, relative_fitness=rel_f, relative_rmse=rel_r, min_correspondences=min_corr,
               estimation=estimation, target_normals=normals[pairs:] if plane else None,
               source_normals=normals[:pairs] if generalized else None, covariance_epsilon=epsilon)
    return coarse, fine


# ---------------------------------------------------------------------------------------------------------------- host route
class _HostBatch:
    """the (p, q) float32 point pairs of every pair, gathered once, and every pair's number of source points"""

    def __init__(self, source, target, correspondences, what):
        s, s_off, _ = _host_ragged(source, what)
        t, t_off, _ = _host_ragged(target, what)
        _same_pairs(s_off, t_off, what)
        self.pairs = s_off.shape[0] - 1
        self.n_source = np.diff(s_off)
        parts, self.c_off = _corr_rows(correspondences, self.pairs, what, _as_numpy)
        rows = np.concatenate(parts, 0).astype(np.int64)
        self.p, self.q = [], []
        for i in range(self.pairs):
            r = rows[self.c_off[i]:self.c_off[i + 1]]
            src, dst = s[s_off[i]:s_off[i + 1]], t[t_off[i]:t_off[i + 1]]
            if (r < 0).any() or (r[:, 0] >= src.shape[0]).any() or (r[:, 1] >= dst.shape[0]).any():
                raise ValueError('%s: a correspondence names a row outside its cloud' % what)
            self.p.append(np.ascontiguousarray(src[r[:, 0]]))
            self.q.append(np.ascontiguousarray(dst[r[:, 1]]))

    def host_poses(self, poses, valid, what):
        poses = _poses_of(_as_numpy(poses), self.pairs, what)
        if valid is None:
            return poses, np.isfinite(poses).all(2)
        return poses, _valid_of(_as_numpy(valid), self.pairs, poses.shape[1], what)


def _host_draws(pair, n_hyp, n_corr, seed):
    """(H, 3) int32 sample rows of one pair"""
    ctr = np.zeros((n_hyp, 4), np.uint32)
    ctr[:, 0] = np.arange(n_hyp, dtype=np.uint32)
    ctr[:, 1] = np.uint32(pair)
    x = augment.philox4x32_10(ctr, _key(seed))[:, :3].astype(np.uint64)
    return ((x * np.uint64(n_corr)) >> np.uint64(32)).astype(np.int32)


def _edge2(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _host_triple_checks(p, q, draws, rho2):
    """(ok (H,) bool: C >= 3, distinct rows and the edge check; the float64 points (a, b, d) of source and target at those
    hypotheses)"""
    i0, i1, i2 = draws[:, 0], draws[:, 1], draws[:, 2]
    ok = np.full(draws.shape[0], p.shape[0] >= 3) & (i0 != i1) & (i0 != i2) & (i1 != i2)
    at = np.nonzero(ok)[0]
    ps = [p[draws[at, k]].astype(np.float64) for k in range(3)]
    qs = [q[draws[at, k]].astype(np.float64) for k in range(3)]
    if rho2 > 0.0:
        edges = np.ones(at.shape[0], bool)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ls, lt = _edge2(ps[a], ps[b]), _edge2(qs[a], qs[b])
            edges &= (ls >= rho2 * lt) & (lt >= rho2 * ls)
        ok[at[~edges]] = False
        ps, qs = [x[edges] for x in ps], [x[edges] for x in qs]
    return ok, ps, qs


def _host_triple_sums(ps, qs):
    """the (n, 17) sums of the three pairs, added in the order 0, 1, 2"""
    sums = np.zeros((ps[0].shape[0], N_SUMS), np.float64)
    sums[:, 0] = 3.0
    for u in range(3):
        sums[:, 1 + u] = (ps[0][:, u] + ps[1][:, u]) + ps[2][:, u]
        sums[:, 4 + u] = (qs[0][:, u] + qs[1][:, u]) + qs[2][:, u]
        for v in range(3):
            sums[:, 7 + 3 * u + v] = (ps[0][:, u] * qs[0][:, v] + ps[1][:, u] * qs[1][:, v]) + ps[2][:, u] * qs[2][:, v]
    return sums


def _host_hypotheses_one(p, q, pair, n_hyp, seed, rho2):
    draws = _host_draws(pair, n_hyp, p.shape[0], seed)
    poses = np.full((n_hyp, 12), np.nan, np.float32)
    ok, ps, qs = _host_triple_checks(p, q, draws, rho2)
    at = np.nonzero(ok)[0]
    r, t, solved = _host_kabsch_many(_host_triple_sums(ps, qs))
    ok[at[~solved]] = False
    poses[at[solved]] = np.concatenate([r[solved], t[solved][:, :, None]], 2).reshape(-1, 12).astype(np.float32)
    return poses, ok, draws


def ransac_hypotheses_host(source, target, correspondences, *, hypotheses=4096, seed=0, edge_length_ratio=0.9):
    """`ransac_hypotheses` on the CPU: `(poses (P, H, 3, 4) float32, valid (P, H) bool, draws (P, H, 3) int32)` numpy."""
    what = 'ransac_hypotheses'
    n_hyp, seed, rho2 = _options(hypotheses, seed, edge_length_ratio, what)
    b = _HostBatch(source, target, correspondences, what)
    parts = [_host_hypotheses_one(b.p[i], b.q[i], i, n_hyp, seed, rho2) for i in range(b.pairs)]
    return (np.stack([x[0] for x in parts]).reshape(b.pairs, n_hyp, 3, 4), np.stack([x[1] for x in parts]),
            np.stack([x[2] for x in parts]))


def _host_d2(p, q, m):
    """(H, C) float32 d2 of the correspondences (p, q) under the (H, 12) float32 poses m"""
    with np.errstate(all='ignore'):
        x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
        d = [_fmaf(m[:, 4 * c + 2, None], z, _fmaf(m[:, 4 * c + 1, None], y, _fmaf(m[:, 4 * c, None], x, m[:, 4 * c + 3, None])))
             - q[None, :, c] for c in range(3)]
        return _fmaf(d[2], d[2], _fmaf(d[1], d[1], d[0] * d[0]))


def _host_counts_one(p, q, poses, valid, d2_max):
    counts = np.where(valid, 0, -1).astype(np.int32)
    rows = max(1, _HOST_CHUNK // max(p.shape[0], 1))
    for h0 in range(0, poses.shape[0], rows):
        sl = slice(h0, h0 + rows)
        n = (_host_d2(p, q, poses[sl]) <= d2_max).sum(1).astype(np.int32)
        counts[sl] = np.where(valid[sl], n, -1)
    return counts


def score_hypotheses_host(source, target, correspondences, poses, max_correspondence_distance, valid=None):
    """`score_hypotheses` on the CPU: (P, H) int32 numpy counts."""
    what = 'score_hypotheses'
    dist, _, _ = _polish_options(max_correspondence_distance, 0, 0, what)
    b = _HostBatch(source, target, correspondences, what)
    poses, valid = b.host_poses(poses, valid, what)
    d2_max = inlier_d2(dist)
    return np.stack([_host_counts_one(b.p[i], b.q[i], poses[i], valid[i], d2_max) for i in range(b.pairs)])


def _host_polish_sums(p, q, pose, d2_max):
    """the 17 sums of the inliers of fp32(pose) among the fixed correspondences"""
    moved = reg._host_move(p, pose)
    d = moved - q                                                      # float32 throughout
    d2 = _fmaf(d[:, 2], d[:, 2], _fmaf(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
    inl = d2 <= d2_max
    return reg._host_point_sums(moved[inl].astype(np.float64), q[inl].astype(np.float64), np.sqrt(d2[inl]).astype(np.float64))


def ransac_registration_host(source, target, correspondences, *, max_correspondence_distance=0.8, hypotheses=4096, seed=0,
                             edge_length_ratio=0.9, refine_iterations=3, min_correspondences=3, poses=None):
    """`ransac_registration` on the CPU: the module's definition in numpy, pair by pair -> `RansacResult`."""
    what = 'ransac_registration'
    n_hyp, seed, rho2 = _options(hypotheses, seed, edge_length_ratio, what)
    dist, iters, min_corr = _polish_options(max_correspondence_distance, refine_iterations, min_correspondences, what)
    d2_max = inlier_d2(dist)
    b = _HostBatch(source, target, correspondences, what)
    given = None if poses is None else b.host_poses(poses, None, what)
    return _host_select_and_polish(
        b, lambda i: _host_hypotheses_one(b.p[i], b.q[i], i, n_hyp, seed, rho2)[:2] if given is None else (given[0][i], given[1][i]),
        d2_max, iters, min_corr)


def _host_select_and_polish(b, candidates, d2_max, iters, min_corr):
    """`_select_and_polish` in numpy on a `_HostBatch`; `candidates(i)` -> (poses (H, 12) float32, valid (H,) bool) of pair i"""
    pose = np.tile(np.eye(4)[:3], (b.pairs, 1, 1))
    fitness, rmse = np.zeros(b.pairs, np.float64), np.full(b.pairs, np.nan, np.float64)
    inliers, status = np.zeros(b.pairs, np.int64), np.zeros(b.pairs, np.int64)
    chosen, chosen_count, n_valid = (np.full(b.pairs, -1, np.int64), np.full(b.pairs, -1, np.int64),
                                     np.zeros(b.pairs, np.int64))
    for i in range(b.pairs):
        p, q = b.p[i], b.q[i]
        cand, valid = candidates(i)
        counts = _host_counts_one(p, q, cand, valid, d2_max)
        n_valid[i] = int((counts >= 0).sum())
        best = int(counts.argmax())                                    # the first of equal maxima: the lowest h
        if counts[best] < 0:
            status[i] = NO_HYPOTHESIS
            continue
        chosen[i], chosen_count[i] = best, counts[best]
        pose[i], fitness[i], rmse[i], inliers[i], _, status[i] = reg._host_iterate(
            lambda m34: _host_polish_sums(p, q, m34, d2_max), p.shape[0], cand[best].astype(np.float64).reshape(3, 4), iters,
            min_corr, 0.0, 0.0, reg._host_kabsch_one)
    return RansacResult(reg._full(pose), fitness, rmse, inliers, chosen, chosen_count, n_valid, status)


def global_registration_host(source, target, *, nb_neighbors=30, mutual=True, ransac_distance=0.8, icp_distance=0.8,
                             estimation='point_to_plane', hypotheses=4096, seed=0, edge_length_ratio=0.9,
                             refine_iterations=3, min_correspondences=3, max_iterations=30, relative_fitness=1e-6,
                             relative_rmse=1e-6, estimator='ransac', consensus_distance=0.4, seeds=64, consensus_size=10,
                             covariance_epsilon=1e-3, normal_radius=None, feature_radius=None, salient_radius=None,
                             non_max_radius=None):
    """`global_registration` on the CPU, from the numpy twins of every step (brute force: for tests and small clouds)."""
    from .fpfh import compute_fpfh_host, feature_correspondences_host
    from .normals import estimate_normals_host
    coarse = _coarse_estimator(estimator, False, 'global_registration', ransac_distance, refine_iterations,
                               min_correspondences, hypotheses, seed, edge_length_ratio, consensus_distance, seeds,
                               consensus_size)
    normals_of, fpfh_of = _with_radii(estimate_normals_host, compute_fpfh_host, nb_neighbors, normal_radius, feature_radius,
                                      'global_registration')
    return _global(source, target, normals_of, fpfh_of, feature_correspondences_host,
                   correspondence_pairs_host, coarse, reg.icp_refine_host, False, nb_neighbors, mutual, icp_distance,
                   estimation, min_correspondences, max_iterations, relative_fitness, relative_rmse, covariance_epsilon,
                   _keypoints_of(salient_radius, non_max_radius, False, 'global_registration'))
