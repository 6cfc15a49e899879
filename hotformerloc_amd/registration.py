"""Rigid ICP registration, point-to-point, point-to-plane or generalized, of a ragged batch of submap pairs, on the GPU.

Retrieval names a place; the query scan is useful once it is registered against it.  `submap_overlap` aligns a ground submap
to an aerial one by the surveyed poses alone, so its Chamfer distance mixes pose error with real disagreement between the
clouds; `icp_refine` takes such an alignment (or the identity, for a retrieved top-1 candidate) and refines it against the
points themselves.  The reference has no such step and open3d is not a dependency: parity with open3d's `registration_icp`
(a float64 k-d tree search) is not claimed.  What is computed is stated here, and `icp_refine_host` is this text in numpy.

    icp_refine             a batch of P pairs run to convergence on the device, one read of the results at the end
    icp_correspondences    one evaluation: every source point's distance, target, inlier flag, and the 17 sums of a pair
    evaluate_registration  fitness and inlier rmse of a given alignment (the k = 0 evaluation alone)
    kabsch_update          the rigid update (R, t) of given sums
    plane_update           the point-to-plane update (R, t) of given sums, and the generalized one: the same 29 sums

Definition (DESIGN.md section 7i has the reasons).  Per pair, T_0 = init (float64 4 x 4, the identity by default;
`SubmapOverlap.transforms` feeds in directly).  For k = 0 .. max_iterations: evaluate, decide, update.

  Evaluate.  p' = fp32(T_k[:3]) . p for every ORIGINAL source point p, the fmaf chain of `hfl_transform_points`
  (acc = fmaf(r0, x, t); acc = fmaf(r1, y, acc); fmaf(r2, z, acc)); the cloud is never moved incrementally.  j(p') is the
  nearest target by d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32, the lowest index on a tie, and d = sqrt(d2) rounded
  once: what `hfl_nn_dist` computes.  A source point is an inlier when it has a target and d <= fp32(max_correspondence_
  distance), compared in fp32 (the convention of `hfl_pair_stats`).  n is the inlier count, fitness_k = n / N_source,
  rmse_k = sqrt(sum d^2 / n) with the sum in float64 over the stored fp32 d.

  Stop.  The first rule that holds ends the pair, and its pose stays T_k, so the returned fitness and rmse always belong to
  the returned pose:  n < min_correspondences: TOO_FEW, rmse = NaN;  k >= 1 and |fitness_k - fitness_{k-1}| < relative_fitness
  and |rmse_k - rmse_{k-1}| < relative_rmse: CONVERGED;  k == max_iterations: MAX_ITERATIONS.

  Update.  Over the inliers, in float64 (a product of two fp32 values is exact there): Sp = sum p', Sq = sum q, Spq = sum
  p' q^T, q = target[j(p')].  H = Spq - Sp Sq^T / n = U S V^T;  R = V diag(1, 1, det(V U^T)) U^T;  t = Sq / n - R Sp / n;
  T_{k+1} = [R | t] . T_k in float64.  Where the second-largest singular value of H is <= 1e-12 x the largest (collinear or
  coincident correspondences) the pair is DEGENERATE and its pose stays T_k.  The decomposition is a one-sided cyclic Jacobi
  with 12 sweeps over the column pairs (0,1), (0,2), (1,2) of G = H V; with u1, u2 / v1, v2 the normalised columns of G / the
  columns of V at the two largest column norms, R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T, which is the formula above
  without a division by the smallest singular value: det R = +1 always, and a planar cloud is no special case.

Point-to-plane (`estimation='point_to_plane'`, `target_normals` in the layout of `target`, for instance from
`estimate_normals`).  Point-to-point ICP on sparse lidar submaps slides along the ground and along trunks: source and target
sample the same surface at different places, so the nearest target point is not the same physical point; the distance to the
target's tangent plane does not care.  Evaluate, fitness, `inlier_rmse` (it stays the point-to-point distance rmse, as in
open3d), the stop rules, `iterations` and the status codes are exactly as above, so a result is comparable across the two
modes.  Only the update differs:

  Update.  Over the inliers, in float64 from the fp32 values p' (moved source), q = target[j(p')], n = target_normals[j(p')],
  every operation rounded once: r = ((p'x - qx) nx + (p'y - qy) ny) + (p'z - qz) nz, a = p' x n, J = (a, n) (6 entries),
  A = sum J J^T, g = sum J r.  A zero normal (the "no normal" marker of `normals.py`) contributes nothing.  The sums of a
  pair are `N_SUMS_PLANE` = 29: n, sum d^2, g (6), the upper triangle of A row-major (21).

  Solve.  A x = -g for x = (alpha, beta, gamma, tx, ty, tz) by an LDL^T factorisation in float64 without pivoting, in a
  fixed operation order (column by column, the inner sums from k = 0 upwards).  A pivot d_i <= 1e-12 A_ii (a NaN too): the
  pair is DEGENERATE and its pose stays T_k -- parallel normals, or too few correspondences for six unknowns.  Otherwise
  R = Rz(gamma) Ry(beta) Rx(alpha) (open3d's `TransformVector6dToMatrix4d`), t = (tx, ty, tz), T_{k+1} = [R | t] . T_k in
  float64; R is a product of three rotations, so det R = +1 by construction.

Generalized, or plane-to-plane (`estimation='generalized'`, after Segal, Haehnel and Thrun 2009; `source_normals` in the
layout of `source` and `target_normals` in the layout of `target`, both unit to fp32 rounding or zero for "no normal", which
is what `estimate_normals` returns and is not checked; `covariance_epsilon`, 1e-3 by default, 0 < epsilon <= 1).
Point-to-plane trusts the target's normal alone; here both clouds carry a local surface, a disc of covariance R diag(eps, 1,
1) R^T = I - (1 - eps) n n^T round its normal, and every residual is weighted by the inverse of the two covariances added up
(DESIGN.md section 7r has the reasons).  Parity with open3d's `registration_generalized_icp` is not claimed.  Evaluate,
fitness, `inlier_rmse` (the point-to-point distance rmse still), the stop rules, `iterations` and the status codes are
exactly as above; dist, idx and the inlier flags keep the bits of the call without normals.  Only the update differs:

  Moved source normal.  a = fp32(R_k) . n_s, the chain of the evaluation without the translation (acc = r0 * x; acc =
  fmaf(r1, y, acc); fmaf(r2, z, acc)), not renormalised.  b = target_normals[j(p')].

  Row.  In float64 from the fp32 values p', q, a, b, every operation rounded once, keep = 1 - eps:
    C_ii = 2 - keep (a_i a_i + b_i b_i),  C_ij = -(keep (a_i a_j + b_i b_j)) for i < j         (a zero normal: its term is I)
    K00 = C11 C22 - C12 C12, K01 = C02 C12 - C01 C22, K02 = C01 C12 - C02 C11, K11 = C00 C22 - C02 C02,
    K12 = C01 C02 - C00 C12, K22 = C00 C11 - C01 C01;  rcp = 1 / ((C00 K00 + C01 K01) + C02 K02);  M_ij = K_ij rcp, symmetric
    r = p' - q;  w_i = (M_i0 r_0 + M_i1 r_1) + M_i2 r_2;  with i1 = i + 1 mod 3, i2 = i + 2 mod 3:
    g_i = p'_i1 w_i2 - p'_i2 w_i1 (i < 3),  g_{3+i} = w_i;  T_ij = p'_i1 M_i2,j - p'_i2 M_i1,j (row i of [p']x M);
    A_ij = p'_j1 T_i,j2 - p'_j2 T_i,j1 (i <= j < 3),  A_i,3+j = T_ij,  A_3+i,3+j = M_ij (i <= j).
  The eigenvalues of C lie in [2 eps, 2] for unit or zero normals, so C is positive definite and cond(C) <= 1 / eps.  These
  are g = J^T M r and A = J^T M J for J = (-[p']x | I) (3 x 6); with M = n n^T they are the point-to-plane row.

  Sums and solve.  The `N_SUMS_PLANE` = 29 sums in the layout of point-to-plane -- n, sum d^2, g (6), the upper triangle of A
  row-major (21) -- and its solve as it stands (LDL^T, R = Rz Ry Rx, `PIVOT_TOL`): `plane_update` solves either.  M is
  positive definite in every row, so three non-collinear inliers determine the pose, and a flat target under vertical normals,
  DEGENERATE for point-to-plane, is not degenerate here.

`iterations` is the k at which the pair stopped: the number of updates its pose received.  An empty source cloud is TOO_FEW
with fitness NaN (0 / 0), an empty target cloud TOO_FEW with fitness 0.

Layouts are those of `overlap.py`: a list of (N_i, 3) float32 clouds or `(points (N, 3), offsets (P + 1,))`.  Coordinates
must be finite; this is not checked.  The device functions raise `NativeLibraryError` on CPU tensors and launch on the
current stream: an iteration is two launches (csrc/registration.hip) -- `hfl_icp_correspond` moves the source, finds the
correspondences and reduces them to per-workgroup sums in a fixed order, `hfl_icp_solve` adds those, decides and updates --
and the loop is max_iterations + 1 such pairs of launches with no host read; a pair that has stopped costs its workgroups
one load.  No atomics, one writer per element: two runs give the same bits.

The host twins emulate the fp32 steps (fmaf through one float64 operation rounded to fp32, which differs from a fused
operation only by a double rounding in about one of 2^29 cases) and sum in numpy's order; the device sums run in the order
of `hfl_pair_stats`.  The two routes therefore agree in correspondences and counts wherever no two candidates and no
threshold lie within rounding of each other, and in poses to rounding.
"""

from collections import namedtuple

import numpy as np
import torch

from . import _native
from .overlap import _as_numpy, _fmaf, _host_argmin32, _host_ragged, _matrices, _ragged, _same_pairs

RUNNING, CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE = range(5)     # HFL_ICP_*: a pair's status
N_SUMS = 17                            # n, Sp (3), Sq (3), Spq (9, row-major: p' down, q across), sum d^2
N_SUMS_PLANE = 29                      # n, sum d^2, g (6), the upper triangle of A row-major (21)
JACOBI_SWEEPS = 12                     # KABSCH_SWEEPS of csrc/kabsch.h
RANK_TOL = 1e-12                       # second singular value <= RANK_TOL x the largest: DEGENERATE
PIVOT_TOL = 1e-12                      # a pivot of the LDL^T <= PIVOT_TOL x its diagonal entry of A: DEGENERATE
ESTIMATIONS = ('point_to_point', 'point_to_plane', 'generalized')

RegistrationResult = namedtuple('RegistrationResult', ['transforms', 'fitness', 'inlier_rmse', 'iterations', 'status'])
RegistrationResult.__doc__ = """What `icp_refine` returns, numpy arrays on the host.  transforms: (P, 4, 4) float64, source
frame -> target frame; fitness: (P,) float64, the share of source points with a target within the distance; inlier_rmse:
(P,) float64 over those points, NaN where the pair is TOO_FEW; iterations: (P,) int64, the updates the pose received; status:
(P,) int64, one of CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE."""


# ----------------------------------------------------------------------------------------------------------------- arguments
def _init_matrices(init, pairs, what):
    if init is None:
        return np.tile(np.eye(4)[:3], (pairs, 1, 1))
    return _matrices(init, pairs, what)


def _options(max_correspondence_distance, max_iterations, relative_fitness, relative_rmse, min_correspondences, what,
             iterations_name='max_iterations'):
    """the options of the ICP, and of the RANSAC polish, which calls its iteration count `refine_iterations`"""
    d = float(max_correspondence_distance)
    if not d >= 0.0:
        raise ValueError('%s: max_correspondence_distance must be a number >= 0' % what)
    if int(max_iterations) != max_iterations or max_iterations < 0:
        raise ValueError('%s: %s must be an integer >= 0' % (what, iterations_name))
    if int(min_correspondences) != min_correspondences or min_correspondences < 0:
        raise ValueError('%s: min_correspondences must be an integer >= 0' % what)
    return d, int(max_iterations), float(relative_fitness), float(relative_rmse), int(min_correspondences)


def _epsilon(covariance_epsilon, what):
    eps = float(covariance_epsilon)
    if not 0.0 < eps <= 1.0:
        raise ValueError('%s: covariance_epsilon must lie in (0, 1], got %r' % (what, covariance_epsilon))
    return eps


def _estimation(estimation, target_normals, what, source_normals=None, covariance_epsilon=1e-3):
    """True where the sums are the 29 of point-to-plane (that estimator and the generalized one); the target's normals go
    with those two and with no other, the source's with the generalized one alone"""
    if estimation not in ESTIMATIONS:
        raise ValueError('%s: estimation must be one of %s, got %r' % (what, ', '.join(ESTIMATIONS), estimation))
    _epsilon(covariance_epsilon, what)
    plane, generalized = estimation != 'point_to_point', estimation == 'generalized'
    if plane and target_normals is None:
        raise ValueError('%s: estimation=%r needs target_normals' % (what, estimation))
    if not plane and target_normals is not None:
        raise ValueError("%s: target_normals go with estimation='point_to_plane' or 'generalized'" % what)
    if generalized and source_normals is None:
        raise ValueError("%s: estimation='generalized' needs source_normals" % what)
    if not generalized and source_normals is not None:
        raise ValueError("%s: source_normals go with estimation='generalized'" % what)
    return plane


def _normals_of(target, target_normals, t_off, what, ragged, side='target'):
    """the (M, 3) float32 normals of the target batch: a list like `target`, or the packed array under the target's offsets;
    with `side='source'` the same of the source batch"""
    if isinstance(target, list) != isinstance(target_normals, list):
        raise ValueError('%s: %s_normals must come in the layout of %s' % (what, side, side))
    nrm, n_off, _ = ragged(target_normals if isinstance(target_normals, list) else (target_normals, t_off), what)
    if not np.array_equal(n_off, t_off):
        raise ValueError('%s: %s_normals must hold one normal per %s point, cloud by cloud' % (what, side, side))
    return nrm


def _full(m34):
    """(P, 3, 4) -> (P, 4, 4) with the row 0 0 0 1"""
    out = np.zeros((m34.shape[0], 4, 4), np.float64)
    out[:, :3] = m34
    out[:, 3, 3] = 1.0
    return out


# -------------------------------------------------------------------------------------------------------------- device route
def _device_state(m34, device):
    """(state (P, 16) float64, istate (P, 2) int32) on the device: the (P, 3, 4) poses, every pair RUNNING at iteration 0"""
    pairs = m34.shape[0]
    st = np.zeros((pairs, 16), np.float64)
    st[:, :12] = m34.reshape(pairs, 12)
    return torch.from_numpy(st).to(device), torch.zeros((pairs, 2), dtype=torch.int32, device=device)


def _iterate_on_device(state, istate, iters, evaluate, solve, count=False):
    """The loop of the estimator, enqueued without a host read: for k = 0 .. iters, `evaluate(state, istate)` reduces the
    correspondences of every RUNNING pair to partials and `solve(state, istate, is_last)` decides and updates -> what the
    last `evaluate` and the last `solve` returned and, with `count` (`solve` must then return the pairs' sums), the (P,)
    float64 n of the evaluation each pair stopped at, else None.  ICP and the RANSAC polish differ in the two callables."""
    n = torch.zeros(state.shape[0], dtype=torch.float64, device=state.device) if count else None
    found = sums = None
    for k in range(iters + 1):
        running = istate[:, 1] == RUNNING if count else None
        found = evaluate(state, istate)
        sums = solve(state, istate, k == iters)
        if count:
            n = torch.where(running, sums[:, 0], n)
    return found, sums, n


def _read_state(state, istate):
    """the one read at the end: `(transforms (P, 4, 4), fitness, rmse, iterations, status)`, numpy"""
    state, istate = state.cpu().numpy(), istate.cpu().numpy().astype(np.int64)
    return (_full(state[:, :12].reshape(-1, 3, 4)), state[:, 12].copy(), state[:, 13].copy(), istate[:, 0].copy(),
            istate[:, 1].copy())


class _Batch:
    """A batch of pairs on the device with everything an iteration needs: both clouds, their offsets, the tile table of the
    source clouds and its per-pair offsets, the partials."""

    def __init__(self, source, target, what, target_normals=None, source_normals=None, epsilon=1e-3):
        from . import ops
        self.s, self.s_off, _ = _ragged(source, what, True)
        self.t, self.t_off, _ = _ragged(target, what, True)
        _same_pairs(self.s_off, self.t_off, what)
        self.plane = target_normals is not None                    # the 29 sums and their solve: point-to-plane, generalized
        on_device = lambda b, w: _ragged(b, w, True)               # noqa: E731
        self.normals = _normals_of(target, target_normals, self.t_off, what, on_device) if self.plane else None
        self.s_normals = None if source_normals is None else \
            _normals_of(source, source_normals, self.s_off, what, on_device, 'source')
        self.epsilon = epsilon
        self.pairs = self.s_off.shape[0] - 1
        dev = self.s.device
        tiles, tile_off = ops.pair_tiles(np.diff(self.s_off))
        self.n_tiles = int(tiles.shape[0])
        with torch.cuda.device(dev):
            self.s_dev, self.t_dev = torch.from_numpy(self.s_off).to(dev), torch.from_numpy(self.t_off).to(dev)
            self.tiles, self.tile_off = torch.from_numpy(tiles).to(dev), torch.from_numpy(tile_off).to(dev)
            self.partials = torch.zeros((max(self.n_tiles, 1), ops.ICP_PLANE_SUMS if self.plane else ops.ICP_SUMS),
                                        dtype=torch.float64, device=dev)

    def state(self, m34):
        return _device_state(m34, self.s.device)

    def correspond(self, state, istate, max_dist, want_rows=False):
        from . import ops
        return ops.icp_correspond(self.s, self.s_dev, self.t, self.t_dev, self.tiles, state, istate, max_dist,
                                  partials=self.partials, want_rows=want_rows, target_normals=self.normals,
                                  source_normals=self.s_normals, epsilon=self.epsilon)

    def solve(self, state, istate, min_corr, rel_fitness, rel_rmse, is_last, want_sums=False):
        from . import ops
        return ops.icp_solve(state, istate, self.partials, self.tile_off, self.n_tiles, self.s_dev, min_corr, rel_fitness,
                             rel_rmse, is_last, want_sums=want_sums, plane=self.plane)


def icp_refine(source, target, init=None, max_correspondence_distance=0.8, max_iterations=30, relative_fitness=1e-6,
               relative_rmse=1e-6, min_correspondences=3, estimation='point_to_point', target_normals=None,
               source_normals=None, covariance_epsilon=1e-3):
    """ICP of P (source, target) pairs, as the module's docstring defines it -> `RegistrationResult`.  `init`: (P, 4, 4) or
    (P, 3, 4) float64, numpy or tensor, source frame -> target frame; None is the identity.  `estimation`:
    'point_to_point', or 'point_to_plane' with `target_normals` in the layout of `target` (a list of (M_i, 3) float32, or the
    packed (M, 3) tensor under the target's offsets), or 'generalized' with those and `source_normals` in the layout of
    `source`, and `covariance_epsilon` in (0, 1].  The whole loop is enqueued on the current stream without a host read; the
    results are read once at the end."""
    what = 'icp_refine'
    dist, iters, rel_f, rel_r, min_corr = _options(max_correspondence_distance, max_iterations, relative_fitness, relative_rmse,
                                                   min_correspondences, what)
    _estimation(estimation, target_normals, what, source_normals, covariance_epsilon)
    b = _Batch(source, target, what, target_normals, source_normals, float(covariance_epsilon))
    with torch.cuda.device(b.s.device):
        state, istate = b.state(_init_matrices(init, b.pairs, what))
        _iterate_on_device(state, istate, iters, lambda st, ist: b.correspond(st, ist, dist),
                           lambda st, ist, is_last: b.solve(st, ist, min_corr, rel_f, rel_r, is_last))
        return RegistrationResult(*_read_state(state, istate))


def _sums_of_normals(target_normals, source_normals, covariance_epsilon, what):
    """which sums `icp_correspondences` is asked for, by the normals it is given -> epsilon"""
    if source_normals is not None and target_normals is None:
        raise ValueError('%s: source_normals go with target_normals (the generalized sums)' % what)
    return _epsilon(covariance_epsilon, what)


def _evaluate(source, target, transforms, max_correspondence_distance, min_correspondences, what, want_rows,
              target_normals=None, source_normals=None, covariance_epsilon=1e-3):
    dist, _, _, _, min_corr = _options(max_correspondence_distance, 0, 0.0, 0.0, min_correspondences, what)
    eps = _sums_of_normals(target_normals, source_normals, covariance_epsilon, what)
    b = _Batch(source, target, what, target_normals, source_normals, eps)
    with torch.cuda.device(b.s.device):
        state, istate = b.state(_matrices(transforms, b.pairs, what))
        (_, d, j), sums, _ = _iterate_on_device(
            state, istate, 0, lambda st, ist: b.correspond(st, ist, dist, want_rows=want_rows),
            lambda st, ist, is_last: b.solve(st, ist, min_corr, 0.0, 0.0, is_last, want_sums=True))
    return d, j, sums, state, dist


def icp_correspondences(source, target, transforms, max_correspondence_distance, target_normals=None, source_normals=None,
                        covariance_epsilon=1e-3):
    """One evaluation at the given poses, on the device: `(dist (Ns,) float32, idx (Ns,) int32, inlier (Ns,) bool, sums
    (P, 17) float64)`.  dist and idx have the bits of `nn_distances(transform_points(source, transforms), target)`; inlier is
    `dist <= fp32(max_correspondence_distance)` where there is a target; sums are n, Sp, Sq, Spq (row-major) and sum d^2
    over a pair's inliers, in the device's fixed order.  With `target_normals` (the layout of `target`) the sums are the
    (P, 29) of the point-to-plane update -- n, sum d^2, g, the upper triangle of A -- and the rest keeps its bits; with
    `source_normals` (the layout of `source`) as well they are the (P, 29) of the generalized update at `covariance_epsilon`."""
    d, j, sums, _, dist = _evaluate(source, target, transforms, max_correspondence_distance, 0, 'icp_correspondences', True,
                                    target_normals, source_normals, covariance_epsilon)
    return d, j, (j >= 0) & (d <= float(np.float32(dist))), sums


def evaluate_registration(source, target, transforms, max_correspondence_distance, min_correspondences=3):
    """`(fitness (P,), inlier_rmse (P,))` float64 on the device: what iteration 0 of `icp_refine` reports for `init =
    transforms`, without iterating."""
    _, _, _, state, _ = _evaluate(source, target, transforms, max_correspondence_distance, min_correspondences,
                                  'evaluate_registration', False)
    return state[:, 12].contiguous(), state[:, 13].contiguous()


def kabsch_update(sums, min_correspondences=3):
    """The update step of `hfl_icp_solve` on given sums (P, 17) float64 on the device -> `(R (P, 3, 3), t (P, 3), status
    (P,) int32)` on the device.  status is RUNNING where (R, t) is the update, TOO_FEW where n < min_correspondences and
    DEGENERATE where H has rank < 2; there R = I and t = 0."""
    return _update_on_device(sums, min_correspondences, N_SUMS, 'kabsch_update', False)


def _update_on_device(sums, min_correspondences, n_sums, what, plane):
    from . import ops
    sums = torch.as_tensor(sums)
    if not sums.is_cuda:
        raise _native.NativeLibraryError('%s runs on the GPU and takes GPU tensors (%s_host is the CPU route)' % (what, what))
    if sums.dtype != torch.float64 or sums.dim() != 2 or sums.shape[1] != n_sums or sums.shape[0] < 1:
        raise TypeError('%s: (P >= 1, %d) float64 sums expected, got %s %s' % (what, n_sums, sums.dtype, tuple(sums.shape)))
    pairs = int(sums.shape[0])
    with torch.cuda.device(sums.device):
        state, istate = _device_state(_init_matrices(None, pairs, what), sums.device)   # (R | t) . I = (R | t), exactly
        one_each = torch.arange(pairs + 1, dtype=torch.int64, device=sums.device)       # one tile, one source point per pair
        ops.icp_solve(state, istate, sums.contiguous(), one_each, pairs, one_each, int(min_correspondences), 0.0, 0.0, False,
                      plane=plane)
    pose = state[:, :12].reshape(pairs, 3, 4)
    return pose[:, :, :3].contiguous(), pose[:, :, 3].contiguous(), istate[:, 1].contiguous()


def plane_update(sums, min_correspondences=6):
    """The update step of `hfl_icp_solve_plane` on given sums (P, 29) float64 on the device -> `(R (P, 3, 3), t (P, 3),
    status (P,) int32)` on the device: the twin of `kabsch_update`.  status is RUNNING where (R, t) is the update, TOO_FEW
    where n < min_correspondences and DEGENERATE where a pivot of the LDL^T fails; there R = I and t = 0.  The sums of the
    generalized estimator have the same layout and are solved by the same call."""
    return _update_on_device(sums, min_correspondences, N_SUMS_PLANE, 'plane_update', True)


# ---------------------------------------------------------------------------------------------------------------- host route
def _host_move(points, m34):
    """the fmaf chain of `hfl_transform_points` with the float32 rounding of one (3, 4) float64 pose"""
    m = m34.astype(np.float32)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    out = np.empty_like(points)
    for c in range(3):
        out[:, c] = _fmaf(m[c, 2], z, _fmaf(m[c, 1], y, _fmaf(m[c, 0], x, m[c, 3])))
    return out


def _host_nn32(q, t):
    """(dist (n,) float32, idx (n,) int32) of one pair with the arithmetic of `hfl_nn_dist`, brute force"""
    dist2, idx = _host_argmin32(q, t)
    return np.sqrt(dist2), idx                                         # float32 sqrt, correctly rounded; sqrt(+inf) = +inf


def _host_plane_sums(p, q, n, d):
    """the 29 sums of given inlier rows, float64 (n, 3) each and the distances (n,)"""
    sums = np.zeros(N_SUMS_PLANE, np.float64)
    sums[0] = p.shape[0]
    sums[1] = (d * d).sum()
    e = p - q
    r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
    jac = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                    p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], 1)
    sums[2:8] = (jac * r[:, None]).sum(0)
    slot = 8
    for a in range(6):
        for b in range(a, 6):
            sums[slot] = (jac[:, a] * jac[:, b]).sum()
            slot += 1
    return sums


def _host_turn(normals, m34):
    """the moved source normals: `_host_move` without the translation, acc = r0 * x first"""
    m = m34.astype(np.float32)
    x, y, z = normals[:, 0], normals[:, 1], normals[:, 2]
    out = np.empty_like(normals)
    for c in range(3):
        out[:, c] = _fmaf(m[c, 2], z, _fmaf(m[c, 1], y, m[c, 0] * x))
    return out


def _host_generalized_rows(p, q, a, b, d, epsilon):
    """The (n, 29) terms of given inlier rows under the generalized estimator, the row of the module's docstring operation for
    operation (`icp_generalized_row` of csrc/registration.hip): float64 (n, 3) moved source points p, targets q, moved source
    normals a and target normals b, the distances d (n,); their sum over the rows is the pair's 29 sums."""
    p, q, a, b = ([np.asarray(x, np.float64)[:, i] for i in range(3)] for x in (p, q, a, b))
    d = np.asarray(d, np.float64)
    keep = np.float64(1.0) - np.float64(epsilon)
    c = [[None] * 3 for _ in range(3)]
    for i in range(3):
        c[i][i] = 2.0 - keep * (a[i] * a[i] + b[i] * b[i])
        for j in range(i + 1, 3):
            c[i][j] = c[j][i] = -(keep * (a[i] * a[j] + b[i] * b[j]))
    k00, k01, k02 = c[1][1] * c[2][2] - c[1][2] * c[1][2], c[0][2] * c[1][2] - c[0][1] * c[2][2], \
        c[0][1] * c[1][2] - c[0][2] * c[1][1]
    k11, k12, k22 = c[0][0] * c[2][2] - c[0][2] * c[0][2], c[0][1] * c[0][2] - c[0][0] * c[1][2], \
        c[0][0] * c[1][1] - c[0][1] * c[0][1]
    rcp = 1.0 / ((c[0][0] * k00 + c[0][1] * k01) + c[0][2] * k02)
    m = [[k00 * rcp, k01 * rcp, k02 * rcp], [None, k11 * rcp, k12 * rcp], [None, None, k22 * rcp]]
    m[1][0], m[2][0], m[2][1] = m[0][1], m[0][2], m[1][2]
    r = [p[i] - q[i] for i in range(3)]
    w = [(m[i][0] * r[0] + m[i][1] * r[1]) + m[i][2] * r[2] for i in range(3)]
    rows = np.zeros((d.shape[0], N_SUMS_PLANE), np.float64)
    rows[:, 0] = 1.0
    rows[:, 1] = d * d
    slot = 8
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        rows[:, 2 + i] = p[i1] * w[i2] - p[i2] * w[i1]
        rows[:, 5 + i] = w[i]
        t = [p[i1] * m[i2][j] - p[i2] * m[i1][j] for j in range(3)]
        for j in range(i, 3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            rows[:, slot] = p[j1] * t[j2] - p[j2] * t[j1]
            slot += 1
        for j in range(3):
            rows[:, slot] = t[j]
            slot += 1
    for i in range(3):
        for j in range(i, 3):
            rows[:, slot] = m[i][j]
            slot += 1
    return rows


def _host_point_sums(p, q, d):
    """the 17 sums of given inlier rows, float64 (n, 3) each and the distances (n,); zeros where there is no row"""
    sums = np.zeros(N_SUMS, np.float64)
    sums[0] = p.shape[0]
    sums[1:4], sums[4:7] = p.sum(0), q.sum(0)
    sums[7:16] = (p[:, :, None] * q[:, None, :]).sum(0).reshape(9)
    sums[16] = (d * d).sum()
    return sums


def _host_evaluate_one(src, dst, m34, max_dist32, normals=None, s_normals=None, epsilon=1e-3):
    """one pair, one evaluation: (dist float32, idx int32, inlier bool, sums (17,) float64, or (29,) with the target's
    normals: those of point-to-plane, or with the source's normals too those of the generalized estimator)"""
    moved = _host_move(src, m34)
    dist, idx = _host_nn32(moved, dst)
    inl = (idx >= 0) & (dist <= max_dist32)
    p, q, d = moved[inl].astype(np.float64), dst[idx[inl]].astype(np.float64), dist[inl].astype(np.float64)
    if s_normals is not None:
        a = _host_turn(s_normals, m34)[inl].astype(np.float64).reshape(-1, 3)
        b = normals[idx[inl]].astype(np.float64).reshape(-1, 3)
        sums = _host_generalized_rows(p.reshape(-1, 3), q.reshape(-1, 3), a, b, d, epsilon).sum(0)
        sums[1] = (d * d).sum()                                        # in the order of the other two modes: the same rmse bits
        return dist, idx, inl, sums
    if normals is not None:
        return dist, idx, inl, _host_plane_sums(p, q, normals[idx[inl]].astype(np.float64).reshape(-1, 3), d)
    return dist, idx, inl, _host_point_sums(p, q, d)


def _rotate_many(g, v, p, q):
    """`jacobi_rotate<p, q>` of csrc/jacobi3.h on every row at once; a row whose columns are orthogonal already is left"""
    alpha = g[0][p] * g[0][p] + g[1][p] * g[1][p] + g[2][p] * g[2][p]
    beta = g[0][q] * g[0][q] + g[1][q] * g[1][q] + g[2][q] * g[2][q]
    gamma = g[0][p] * g[0][q] + g[1][p] * g[1][q] + g[2][p] * g[2][q]
    skip = gamma == 0.0
    zeta = (beta - alpha) / (2.0 * gamma)
    t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    c = 1.0 / np.sqrt(1.0 + t * t)
    s = c * t
    for i in range(3):
        gp, gq, vp, vq = g[i][p], g[i][q], v[i][p], v[i][q]
        g[i][p], g[i][q] = np.where(skip, gp, c * gp - s * gq), np.where(skip, gq, s * gp + c * gq)
        v[i][p], v[i][q] = np.where(skip, vp, c * vp - s * vq), np.where(skip, vq, s * vp + c * vq)


def _pick(cols, j):
    """cols[j[n]][n]: the run-time pick of a column"""
    return np.where(j == 0, cols[0], np.where(j == 1, cols[1], cols[2]))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _host_kabsch_many(sums, want_ratio=False):
    """(R (n, 3, 3), t (n, 3), solved (n,) bool) of (n, 17) sums; solved is False where H has rank < 2, and R and t mean
    nothing there.  `kabsch_solve` of csrc/kabsch.h, line by line, every float64 operation on all rows at once: the one
    transcription, for the ICP, the RANSAC polish and the hypotheses alike.  With `want_ratio` also the (n,) rank ratios the
    decision was taken on, second over largest singular value (NaN where H is 0 or not finite)"""
    n_rows = sums.shape[0]
    with np.errstate(all='ignore'):
        s = [sums[:, k].astype(np.float64) for k in range(N_SUMS)]
        n = s[0]
        g = [[s[7 + 3 * a + b] - s[1 + a] * s[4 + b] / n for b in range(3)] for a in range(3)]
        v = [[np.full(n_rows, np.float64(a == b)) for b in range(3)] for a in range(3)]
        for _ in range(JACOBI_SWEEPS):
            _rotate_many(g, v, 0, 1)
            _rotate_many(g, v, 0, 2)
            _rotate_many(g, v, 1, 2)
        w = [np.sqrt(g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j]) for j in range(3)]
        i1 = np.where((w[0] >= w[1]) & (w[0] >= w[2]), 0, np.where(w[1] >= w[2], 1, 2))
        ja, jb = np.where(i1 == 0, 1, 0), np.where(i1 == 2, 1, 2)
        i2 = np.where(_pick(w, ja) >= _pick(w, jb), ja, jb)
        w1, w2 = _pick(w, i1), _pick(w, i2)
        solved = w2 > RANK_TOL * w1
        u1, u2 = [_pick(g[i], i1) / w1 for i in range(3)], [_pick(g[i], i2) / w2 for i in range(3)]
        v1, v2 = [_pick(v[i], i1) for i in range(3)], [_pick(v[i], i2) for i in range(3)]
        u3, v3 = _cross(u1, u2), _cross(v1, v2)
        mp, mq = [s[1 + a] / n for a in range(3)], [s[4 + a] / n for a in range(3)]
        r = [[v1[a] * u1[b] + v2[a] * u2[b] + v3[a] * u3[b] for b in range(3)] for a in range(3)]
        t = [mq[a] - (r[a][0] * mp[0] + r[a][1] * mp[1] + r[a][2] * mp[2]) for a in range(3)]
        ratio = w2 / w1
    out = (np.stack([np.stack(row, 1) for row in r], 1).reshape(n_rows, 3, 3), np.stack(t, 1).reshape(n_rows, 3), solved)
    return out + (ratio,) if want_ratio else out


def _host_kabsch_one(s):
    """(R (3, 3), t (3,)) of one pair's sums, or None where H has rank < 2: `_host_kabsch_many` on one row"""
    r, t, solved = _host_kabsch_many(np.asarray(s, np.float64).reshape(1, N_SUMS))
    return (r[0], t[0]) if solved[0] else None


def kabsch_update_host(sums, min_correspondences=3):
    """`kabsch_update` on the CPU: `(R (P, 3, 3) float64, t (P, 3) float64, status (P,) int32)` numpy arrays."""
    return _update_on_host(sums, min_correspondences, N_SUMS, 'kabsch_update', _host_kabsch_one)


def _update_on_host(sums, min_correspondences, n_sums, what, solve_one):
    sums = np.asarray(_as_numpy(sums), dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != n_sums or sums.shape[0] < 1:
        raise TypeError('%s: (P >= 1, %d) float64 sums expected, got shape %s' % (what, n_sums, sums.shape))
    pairs = sums.shape[0]
    r, t, status = np.tile(np.eye(3), (pairs, 1, 1)), np.zeros((pairs, 3), np.float64), np.zeros(pairs, np.int32)
    for p in range(pairs):
        if sums[p, 0] < min_correspondences:
            status[p] = TOO_FEW
            continue
        solved = solve_one(sums[p])
        if solved is None:
            status[p] = DEGENERATE
        else:
            r[p], t[p] = solved
    return r, t, status


def _host_plane_one(s):
    """(R (3, 3), t (3,)) of one pair's 29 sums, or None where a pivot fails: `plane_solve` of csrc/registration.hip, line by
    line, on numpy float64 scalars"""
    with np.errstate(all='ignore'):
        s = [np.float64(x) for x in s]
        a = [[np.float64(0.0)] * 6 for _ in range(6)]                  # the lower triangle becomes L
        slot = 8
        for i in range(6):
            for j in range(i, 6):
                a[i][j] = a[j][i] = s[slot]
                slot += 1
        d = [np.float64(0.0)] * 6
        for j in range(6):
            diag = a[j][j]
            dj = diag
            for k in range(j):
                dj = dj - a[j][k] * a[j][k] * d[k]
            if not dj > PIVOT_TOL * diag:
                return None
            d[j] = dj
            for i in range(j + 1, 6):
                v = a[i][j]
                for k in range(j):
                    v = v - a[i][k] * a[j][k] * d[k]
                a[i][j] = v / dj
        x = [np.float64(0.0)] * 6
        for i in range(6):                                             # L y = -g
            v = -s[2 + i]
            for k in range(i):
                v = v - a[i][k] * x[k]
            x[i] = v
        x = [x[i] / d[i] for i in range(6)]
        for i in range(5, -1, -1):                                     # L^T x = z
            v = x[i]
            for k in range(i + 1, 6):
                v = v - a[k][i] * x[k]
            x[i] = v
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        r = np.array([[cb * cg, sa * sb * cg - ca * sg, ca * sb * cg + sa * sg],
                      [cb * sg, sa * sb * sg + ca * cg, ca * sb * sg - sa * cg],
                      [-sb, sa * cb, ca * cb]], np.float64)
    return r, np.array(x[3:], np.float64)


def plane_update_host(sums, min_correspondences=6):
    """`plane_update` on the CPU: `(R (P, 3, 3) float64, t (P, 3) float64, status (P,) int32)` numpy arrays; the sums of the
    generalized estimator as well."""
    return _update_on_host(sums, min_correspondences, N_SUMS_PLANE, 'plane_update', _host_plane_one)


def _host_batch(source, target, what, target_normals=None, source_normals=None):
    """per pair (source, target), then the target's normals where given, then the source's"""
    s, s_off, _ = _host_ragged(source, what)
    t, t_off, _ = _host_ragged(target, what)
    _same_pairs(s_off, t_off, what)
    pairs = s_off.shape[0] - 1
    if target_normals is None:
        return [(s[s_off[p]:s_off[p + 1]], t[t_off[p]:t_off[p + 1]]) for p in range(pairs)], s_off
    n = _normals_of(target, target_normals, t_off, what, _host_ragged)
    if source_normals is None:
        return [(s[s_off[p]:s_off[p + 1]], t[t_off[p]:t_off[p + 1]], n[t_off[p]:t_off[p + 1]]) for p in range(pairs)], s_off
    a = _normals_of(source, source_normals, s_off, what, _host_ragged, 'source')
    return [(s[s_off[p]:s_off[p + 1]], t[t_off[p]:t_off[p + 1]], n[t_off[p]:t_off[p + 1]], a[s_off[p]:s_off[p + 1]])
            for p in range(pairs)], s_off


def _host_figures(sums, n_source, min_corr):
    """(fitness, rmse, too few) of one evaluation, from the 17 sums or the 29"""
    n, sum_d2 = sums[0], sums[1] if sums.shape[0] == N_SUMS_PLANE else sums[16]
    with np.errstate(all='ignore'):
        fitness = np.float64(n) / np.float64(n_source)                 # an empty source cloud: 0 / 0 = NaN
        few = n < min_corr
        rmse = np.float64(np.nan) if (few or n <= 0) else np.sqrt(sum_d2 / n)
    return float(fitness), float(rmse), bool(few)


def _host_iterate(evaluate, n_rows, pose0, iters, min_corr, rel_f, rel_r, solve_one):
    """Evaluate, decide, update on one pair, as the module's docstring defines them -> `(pose (3, 4), fitness, rmse, n, k,
    status)`, the figures and the inlier count n of the evaluation the pair stopped at.  `evaluate(pose)` gives the sums of
    the inliers under a (3, 4) float64 pose, `n_rows` is the denominator of the fitness, `solve_one(sums)` the update or
    None.  The RANSAC polish runs it with both relative thresholds 0: abs(x) < 0 never holds, so it cannot end CONVERGED."""
    pose, prev = pose0, None
    for k in range(iters + 1):
        sums = evaluate(pose)
        fitness, rmse, few = _host_figures(sums, n_rows, min_corr)
        if few:
            status = TOO_FEW
        elif k >= 1 and abs(fitness - prev[0]) < rel_f and abs(rmse - prev[1]) < rel_r:
            status = CONVERGED
        elif k == iters:
            status = MAX_ITERATIONS
        else:
            solved = solve_one(sums)
            status = DEGENERATE if solved is None else RUNNING
        if status != RUNNING:
            return pose, fitness, rmse, int(sums[0]), k, status
        r, t = solved
        pose = np.concatenate([r @ pose[:, :3], (r @ pose[:, 3] + t)[:, None]], 1)    # (R | t) . T_k, the row 0 0 0 1 implied
        prev = (fitness, rmse)


def icp_refine_host(source, target, init=None, max_correspondence_distance=0.8, max_iterations=30, relative_fitness=1e-6,
                    relative_rmse=1e-6, min_correspondences=3, estimation='point_to_point', target_normals=None,
                    source_normals=None, covariance_epsilon=1e-3):
    """`icp_refine` on the CPU: the module's definition in numpy, pair by pair -> `RegistrationResult`."""
    what = 'icp_refine'
    dist, iters, rel_f, rel_r, min_corr = _options(max_correspondence_distance, max_iterations, relative_fitness, relative_rmse,
                                                   min_correspondences, what)
    plane = _estimation(estimation, target_normals, what, source_normals, covariance_epsilon)
    solve_one = _host_plane_one if plane else _host_kabsch_one
    batch, _ = _host_batch(source, target, what, target_normals, source_normals)
    eps = float(covariance_epsilon)
    pose = _init_matrices(init, len(batch), what).copy()
    fitness, rmse = np.zeros(len(batch), np.float64), np.zeros(len(batch), np.float64)
    iterations, status = np.zeros(len(batch), np.int64), np.zeros(len(batch), np.int64)
    for p, (src, dst, *nrm) in enumerate(batch):
        pose[p], fitness[p], rmse[p], _, iterations[p], status[p] = _host_iterate(
            lambda m34: _host_evaluate_one(src, dst, m34, np.float32(dist), *nrm, epsilon=eps)[3], src.shape[0], pose[p], iters,
            min_corr, rel_f, rel_r, solve_one)
    return RegistrationResult(_full(pose), fitness, rmse, iterations, status)


def icp_correspondences_host(source, target, transforms, max_correspondence_distance, target_normals=None,
                             source_normals=None, covariance_epsilon=1e-3):
    """`icp_correspondences` on the CPU: `(dist float32, idx int32, inlier bool, sums (P, 17) float64)` numpy arrays; with
    `target_normals` the sums are (P, 29), those of the generalized estimator where `source_normals` are given too."""
    what = 'icp_correspondences'
    dist = _options(max_correspondence_distance, 0, 0.0, 0.0, 0, what)[0]
    eps = _sums_of_normals(target_normals, source_normals, covariance_epsilon, what)
    batch, _ = _host_batch(source, target, what, target_normals, source_normals)
    m = _matrices(transforms, len(batch), what)
    parts = [_host_evaluate_one(pair[0], pair[1], m[p], np.float32(dist), *pair[2:], epsilon=eps)
             for p, pair in enumerate(batch)]
    return (np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts]), np.concatenate([x[2] for x in parts]),
            np.stack([x[3] for x in parts]))


def evaluate_registration_host(source, target, transforms, max_correspondence_distance, min_correspondences=3):
    """`evaluate_registration` on the CPU: `(fitness (P,), inlier_rmse (P,))` float64 numpy arrays."""
    what = 'evaluate_registration'
    dist, _, _, _, min_corr = _options(max_correspondence_distance, 0, 0.0, 0.0, min_correspondences, what)
    batch, _ = _host_batch(source, target, what)
    m = _matrices(transforms, len(batch), what)
    figures = [_host_figures(_host_evaluate_one(src, dst, m[p], np.float32(dist))[3], src.shape[0], min_corr)
               for p, (src, dst) in enumerate(batch)]
    return np.array([f[0] for f in figures], np.float64), np.array([f[1] for f in figures], np.float64)
