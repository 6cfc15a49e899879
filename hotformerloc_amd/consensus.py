"""Consensus registration of a ragged batch of submap pairs: pose hypotheses from the second-order compatibility of point
correspondences, on the GPU.

`ransac_registration` draws random triples of correspondences; a triple helps only if all three are right, which happens with
probability (inlier share)^3 -- 1.25e-4 at 5 % inliers, so that 4 096 hypotheses hold half a good triple on average.  FPFH
matches between a ground scan and an aerial submap, or between two forest revisits, lie there.  This module makes its
hypotheses from the structure of the correspondences instead, as the core of SC2-PCR does (Chen et al., CVPR 2022): two
correspondences are COMPATIBLE when they preserve the length between them; two compatible correspondences that also share
many compatible third parties almost certainly belong to the same rigid motion; so every well-connected correspondence is a
seed, its best-supported partners form a consensus set, and one Kabsch solve over the set is a hypothesis.  Nothing is drawn:
there is no seed of a generator to tune.  Parity with the SC2-PCR repository is not claimed (it seeds by a non-maximum-
suppressed eigenvector, runs two stages and weights the SVD): what is computed is stated here, and the `*_host` functions are
this text in numpy.

    consensus_hypotheses     S candidate poses per pair, one per seed, with their seeds (and sets, supports, degrees)
    consensus_registration   those candidates -> score, select, polish as in `ransac_registration` -> `RansacResult`

`global_registration(estimator='consensus')` and `rerank_candidates(register=True, estimator='consensus')` take their coarse
pose from here.

Definition (DESIGN.md section 7q has the reasons).  `source`, `target` and `correspondences` are those of
`ransac_registration`, gathered once into fp32 point pairs (p_c, q_c), c = 0 .. C - 1 of each pair.  Options: d =
`distance_threshold` > 0, S = `seeds` >= 1, k1 = `consensus_size` in 3 .. 64.

  1. Compatibility.  For i != j, all in fp32: a = |p_i - p_j| and b = |q_i - q_j| as in `spectral.py` (the d2 fmaf chain of the
     pair scan and the correctly rounded root), e = a - b, B_ij = 1 iff |e| <= fp32(d).  B_ii = 0.  The expression is
     symmetric operation for operation: B_ij == B_ji.
  2. Degree.  deg_i = sum_j B_ij, an int32.
  3. Seeds.  The correspondences ordered by (deg descending, index ascending); slot h = 0 .. min(S, C) - 1 takes the h-th of
     that order as its seed s_h.  Slots h >= C are unused: seed -1, invalid.
  4. Second-order support of seed s.  For j != s: n_sj = B_sj sum_k B_sk B_jk, the number of correspondences compatible with
     both; zero where j is not compatible with s.
  5. Consensus set.  s itself and the k1 - 1 columns j of largest n_sj among those with n_sj >= 1, the lower j of equal
     ones; all of them if fewer qualify.  m = its size, the members in ascending order.  m < 3: the hypothesis is invalid.
  6. Pose.  The 17 float64 sums of `registration.py` over the members, added in ascending member order by one accumulator
     each (n = m, Sp, Sq, Spq, sum d^2 = 0), solved by `kabsch_solve` of csrc/kabsch.h (`registration._host_kabsch_many`), the
     solver of the ICP and of `ransac_hypotheses`; rank < 2 is invalid.  The pose is rounded to the twelve fp32 values of a
     hypothesis of `ransac_registration`; an invalid slot holds twelve NaNs, no members (-1) and support 0.  `support` is
     the n_sj of the weakest member of a valid set.
  7. `consensus_registration` is the score -> select -> polish part of `ransac_registration` on these S poses and flags,
     with the same semantics (largest count, lowest h, `NO_HYPOTHESIS`, the polish loop) and the same `RansacResult`; its
     `hypothesis` field holds the chosen slot.

Steps 1 to 5 are integer or boolean functions of singly rounded fp32 operations: host and device agree in them exactly, with
no guard.  Limits, refused with a `ValueError` before a kernel of this module launches: C_i <=
`CONSENSUS_MAX_CORRESPONDENCES` = 16 384 (a row of n_sj fits LDS as 16-bit counts), and the bit matrices of the batch
together within `GRAPH_BUDGET_BYTES` = 1 GiB (a pair of C = 10 000 needs 12.6 MB).

The device functions raise `NativeLibraryError` on CPU clouds and launch on the current stream (csrc/consensus.hip):
`hfl_consensus_graph` (the hot path: 512 rows in the registers of a workgroup against all the pair's correspondences streaming
through LDS, 32 decisions packed into a word, the degree by popcount), two stable sorts of torch for the seeds as in
`prune_correspondences`, and `hfl_consensus_poses` (one workgroup per seed: AND + popcount of two bit rows per partner, a
repeated arg-max, one Kabsch solve).  No host read between the launches, no float atomics; two runs give the same bits.

The host twins keep a dense boolean B and take n from one matrix product (in float32, exact: the counts stay below 2^24).
"""

import importlib

import numpy as np
import torch

from . import registration as reg
from .overlap import _host_d2_32
from .spectral import _split

# the package binds the function `global_registration` under the module's name
GR = importlib.import_module('hotformerloc_amd.global_registration')

CONSENSUS_MAX_CORRESPONDENCES = 16384  # HFL_CONSENSUS_MAX_CORRESPONDENCES (`ops.CONSENSUS_MAX_CORRESPONDENCES`)
CONSENSUS_MAX_SIZE = 64                # HFL_CONSENSUS_MAX_SIZE
GRAPH_BUDGET_BYTES = 1 << 30           # the bit matrices of one call


# ----------------------------------------------------------------------------------------------------------------- arguments
def _options(distance_threshold, seeds, consensus_size, what):
    d = float(distance_threshold)
    if not (d > 0.0 and np.isfinite(d)) or not (np.float32(d) > 0.0 and np.isfinite(np.float32(d))):
        raise ValueError('%s: distance_threshold must be a finite float32 > 0' % what)
    if int(seeds) != seeds or seeds < 1:
        raise ValueError('%s: seeds must be an integer >= 1' % what)
    if int(consensus_size) != consensus_size or not 3 <= consensus_size <= CONSENSUS_MAX_SIZE:
        raise ValueError('%s: consensus_size must be an integer in 3 .. %d' % (what, CONSENSUS_MAX_SIZE))
    return np.float32(d), int(seeds), int(consensus_size)


def _graph_words(c_off, what):
    """((P + 1,) int64 word offsets of the pairs' bit matrices, their total) after the two limits of the module docstring"""
    from . import ops
    lengths = np.diff(c_off)
    if (lengths > CONSENSUS_MAX_CORRESPONDENCES).any():
        raise ValueError('%s: a pair has %d correspondences; at most %d are supported (prune them first)'
                         % (what, int(lengths.max()), CONSENSUS_MAX_CORRESPONDENCES))
    word_off, _ = ops.consensus_words(lengths)
    if 4 * int(word_off[-1]) > GRAPH_BUDGET_BYTES:
        raise ValueError('%s: the compatibility graphs of the batch need %d bytes; at most %d are supported (split the batch)'
                         % (what, 4 * int(word_off[-1]), GRAPH_BUDGET_BYTES))
    return word_off, int(word_off[-1])


# -------------------------------------------------------------------------------------------------------------- device route
def _device_seeds(degree, b, n_seeds):
    """(P, S) int64 seeds of step 3 from the (C,) int32 degrees of a `_Batch`: two stable sorts, no host read"""
    dev, n = b.device, int(degree.shape[0])
    lengths = torch.from_numpy(np.diff(b.c_off)).to(dev)
    pair = torch.repeat_interleave(torch.arange(b.pairs, device=dev), lengths)
    by_degree = torch.sort(degree, descending=True, stable=True).indices
    order = by_degree[torch.sort(pair[by_degree], stable=True).indices]            # by (pair, -degree, index)
    slot = torch.arange(n_seeds, device=dev)[None, :]
    first = b.c_dev[:-1, None]
    at = (first + slot).clamp(max=max(n - 1, 0))
    local = torch.cat([order, order.new_zeros(1)])[at] - first                     # the extra entry: a batch without a row
    return torch.where(slot < lengths[:, None], local, torch.full_like(local, -1))


def _device_hypotheses(b, d32, n_seeds, k1, what):
    """steps 1 to 6 on a `_Batch`, whose device is current -> (poses (P, S, 12) fp32, valid (P, S) uint8, seeds (P, S) int64,
    members (P, S, k1) int32, support (P, S) int32, degree (C,) int32)"""
    from . import ops
    word_off, n_words = _graph_words(b.c_off, what)
    tiles, _ = ops.consensus_tiles(np.diff(b.c_off))
    tiles, word_off = torch.from_numpy(tiles).to(b.device), torch.from_numpy(word_off).to(b.device)
    bits, degree = ops.consensus_graph(b.corr, b.c_dev, tiles, word_off, n_words, float(d32))
    seeds = _device_seeds(degree, b, n_seeds)
    poses, valid, members, support = ops.consensus_poses(b.corr, b.c_dev, bits, word_off, n_words,
                                                         seeds.to(torch.int32).contiguous(), k1)
    return poses, valid, seeds, members, support, degree


def consensus_hypotheses(source, target, correspondences, *, distance_threshold=0.4, seeds=64, consensus_size=10,
                         return_details=False):
    """S candidate poses for each of P pairs, as the module's docstring defines them, on the device -> `(poses (P, S, 3, 4)
    float32, valid (P, S) bool, seeds (P, S) int64)`, device tensors; an invalid or unused slot has a pose of NaNs.  With
    `return_details` also `members (P, S, consensus_size) int64` (ascending, padded with -1), `support (P, S) int64` and
    `degree`, int32 in the layout of the correspondences.  The arguments and their refusals are those of
    `ransac_registration`."""
    what = 'consensus_hypotheses'
    d32, n_seeds, k1 = _options(distance_threshold, seeds, consensus_size, what)
    b = GR._Batch(source, target, correspondences, what)
    with torch.cuda.device(b.device):
        poses, valid, seed_rows, members, support, degree = _device_hypotheses(b, d32, n_seeds, k1, what)
        out = (poses.view(b.pairs, n_seeds, 3, 4), valid.to(torch.bool), seed_rows)
        if not return_details:
            return out
        return out + (members.to(torch.int64), support.to(torch.int64),
                      _split(degree, b.c_off, isinstance(correspondences, list)))


def consensus_registration(source, target, correspondences, *, distance_threshold=0.4, seeds=64, consensus_size=10,
                           max_correspondence_distance=0.8, refine_iterations=3, min_correspondences=3):
    """Registration of P pairs from the consensus hypotheses of their correspondences, as the module's docstring defines it
    -> `RansacResult` (`hypothesis`: the chosen seed slot).  Everything is enqueued on the current stream without a host
    read; the results are read once at the end."""
    what = 'consensus_registration'
    d32, n_seeds, k1 = _options(distance_threshold, seeds, consensus_size, what)
    dist, iters, min_corr = GR._polish_options(max_correspondence_distance, refine_iterations, min_correspondences, what)
    d2_max = float(GR.inlier_d2(dist))
    b = GR._Batch(source, target, correspondences, what)
    with torch.cuda.device(b.device):
        poses, valid = _device_hypotheses(b, d32, n_seeds, k1, what)[:2]
        return GR._select_and_polish(b, poses, valid, d2_max, iters, min_corr)


# ---------------------------------------------------------------------------------------------------------------- host route
def _host_graph(p, q, d32):
    """(C, C) bool B of one pair, the diagonal False"""
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.sqrt(_host_d2_32(p, p)) - np.sqrt(_host_d2_32(q, q))    # float32 throughout; numpy's root is correctly rounded
        graph = np.abs(e) <= d32
    np.fill_diagonal(graph, False)
    return graph


def _host_member_sums(p, q, members, sizes):
    """(n, 17) float64 sums of n sets: members (n, k1) int64 rows of (p, q), the first sizes[i] of row i; one accumulator per
    sum, in member order"""
    sums = np.zeros((members.shape[0], reg.N_SUMS), np.float64)
    sums[:, 0] = sizes
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    for u in range(members.shape[1]):
        live = sizes > u
        pu, qu = p64[members[live, u]], q64[members[live, u]]
        sums[live, 1:4] += pu
        sums[live, 4:7] += qu
        sums[live, 7:16] += (pu[:, :, None] * qu[:, None, :]).reshape(-1, 9)       # products of two fp32 values: exact
    return sums


def _host_hypotheses_one(p, q, d32, n_seeds, k1):
    """steps 1 to 6 on one pair -> (poses (S, 12) float32, valid (S,) bool, seeds (S,), members (S, k1), support (S,), all
    int64, degree (C,) int32, rank ratios (S,) float64: NaN where nothing was solved)"""
    n_corr = p.shape[0]
    poses, valid = np.full((n_seeds, 12), np.nan, np.float32), np.zeros(n_seeds, bool)
    seeds, members = np.full(n_seeds, -1, np.int64), np.full((n_seeds, k1), -1, np.int64)
    support, ratios = np.zeros(n_seeds, np.int64), np.full(n_seeds, np.nan, np.float64)
    if n_corr == 0:
        return poses, valid, seeds, members, support, np.zeros(0, np.int32), ratios
    graph = _host_graph(p, q, d32)
    degree = graph.sum(1, dtype=np.int32)
    used = min(n_seeds, n_corr)
    seeds[:used] = np.argsort(-degree.astype(np.int64), kind='stable')[:used]      # the lower index of equal degrees
    rows = graph[seeds[:used]]
    second = (rows.astype(np.float32) @ graph.astype(np.float32)).astype(np.int64) * rows      # n_sj; exact below 2^24
    sets, sizes, weakest = np.zeros((used, k1), np.int64), np.zeros(used, np.int64), np.zeros(used, np.int64)
    for h in range(used):
        cand = np.nonzero(second[h] >= 1)[0]                                       # ascending: the lower j of equal n first
        taken = cand[np.argsort(-second[h, cand], kind='stable')][:k1 - 1]
        sizes[h] = taken.shape[0] + 1
        sets[h, :sizes[h]] = np.sort(np.append(taken, seeds[h]))
        weakest[h] = second[h, taken].min() if taken.shape[0] else 0
    big = np.nonzero(sizes >= 3)[0]
    r, t, solved, ratio = reg._host_kabsch_many(_host_member_sums(p, q, sets[big], sizes[big]), want_ratio=True)
    ratios[big] = ratio
    good = big[solved]
    valid[good] = True
    poses[good] = np.concatenate([r[solved], t[solved][:, :, None]], 2).reshape(-1, 12).astype(np.float32)
    support[good] = weakest[good]
    for h in good:
        members[h, :sizes[h]] = sets[h, :sizes[h]]
    return poses, valid, seeds, members, support, degree, ratios


def _host_hypotheses(source, target, correspondences, distance_threshold, seeds, consensus_size, what):
    d32, n_seeds, k1 = _options(distance_threshold, seeds, consensus_size, what)
    b = GR._HostBatch(source, target, correspondences, what)
    _graph_words(b.c_off, what)
    return b, [_host_hypotheses_one(b.p[i], b.q[i], d32, n_seeds, k1) for i in range(b.pairs)]


def consensus_hypotheses_host(source, target, correspondences, *, distance_threshold=0.4, seeds=64, consensus_size=10,
                              return_details=False):
    """`consensus_hypotheses` on the CPU: the module's definition in numpy, pair by pair, the graph in memory (for tests and
    small sets of correspondences) -> the same tuple of numpy arrays.  With `return_details` there is one entry more, `rank
    ratios (P, S) float64`: second over largest singular value as the host Kabsch solver saw it, NaN where a set has fewer
    than three members -- the tests' rule for which poses to compare closely."""
    b, parts = _host_hypotheses(source, target, correspondences, distance_threshold, seeds, consensus_size,
                                'consensus_hypotheses')
    out = (np.stack([x[0] for x in parts]).reshape(b.pairs, -1, 3, 4), np.stack([x[1] for x in parts]),
           np.stack([x[2] for x in parts]))
    if not return_details:
        return out
    degree = [x[5] for x in parts]
    return out + (np.stack([x[3] for x in parts]), np.stack([x[4] for x in parts]),
                  degree if isinstance(correspondences, list) else np.concatenate(degree), np.stack([x[6] for x in parts]))


def consensus_registration_host(source, target, correspondences, *, distance_threshold=0.4, seeds=64, consensus_size=10,
                                max_correspondence_distance=0.8, refine_iterations=3, min_correspondences=3):
    """`consensus_registration` on the CPU: the module's definition in numpy, pair by pair -> `RansacResult`."""
    what = 'consensus_registration'
    dist, iters, min_corr = GR._polish_options(max_correspondence_distance, refine_iterations, min_correspondences, what)
    b, parts = _host_hypotheses(source, target, correspondences, distance_threshold, seeds, consensus_size, what)
    return GR._host_select_and_polish(b, lambda i: parts[i][:2], GR.inlier_d2(dist), iters, min_corr)
