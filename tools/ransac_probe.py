"""Time the RANSAC of `hotformerloc_amd/global_registration.py` against two yardsticks measured in the same run.

  score     `hfl_ransac_score` alone on `--pairs` pairs (and on one pair) x `--hypotheses` candidate poses x C correspondences
            for every C of `--correspondences`, `--launches` launches back to back between two HIP events; tests per second
            (one test = one correspondence under one pose) and their share of an fp32 VALU peak of 256 CUs x 4 SIMDs x 32
            lanes x 2.4 GHz / 17 instructions per test (nine fmaf, three subtractions, three for d2, a compare, an add).
  torch     the same counts in eager torch on the same device: a batched move (`torch.matmul`), the squared differences, a
            compare and a sum, `--torch-chunk` hypotheses of one pair at a time to bound the memory.  The counts are compared
            (they may differ where a d2 is within rounding of the threshold: the products are not fused there).
  nn_dist   `hfl_nn_dist` on as many point pairs: `--hypotheses` queries against C targets per pair.
  call      the whole `ransac_registration` (gather, draw, score, select, `--refine` polish iterations, one read), wall
            clock with a device synchronisation on both sides.

No time is fixed in advance.  Median / min / max of `--repeats` measurements after `--warmup`.  One JSON line.  Run it under
`timeout`."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import ops, ransac_registration                                                             # noqa: E402
from normals_probe import events, wall                                                                            # noqa: E402

GR = importlib.import_module('hotformerloc_amd.global_registration')
VALU_PER_TEST = 17
VALU_PEAK = 256 * 4 * 32 * 2.4e9       # fp32 lane-instructions per second


def random_poses(rng, n):
    """(n, 12) float32 rigid poses: a random rotation (QR of a normal matrix, det +1) and a shift of a few metres"""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return np.concatenate([q, rng.uniform(-5.0, 5.0, (n, 3, 1))], 2).reshape(n, 12).astype(np.float32)


def make(rng, pairs, n_corr, n_hyp, device, wrong=0.7):
    """corr (P C, 6), offsets, rows and clouds of `pairs` pairs whose true pose is candidate 0"""
    poses = random_poses(rng, pairs * n_hyp).reshape(pairs, n_hyp, 12)
    src = rng.uniform(-30.0, 30.0, (pairs, n_corr, 3)).astype(np.float32)
    m = poses[:, 0].reshape(pairs, 3, 4).astype(np.float64)
    dst = (np.einsum('pab,pcb->pca', m[:, :, :3], src.astype(np.float64)) + m[:, None, :, 3]).astype(np.float32)
    rows = np.tile(np.arange(n_corr, dtype=np.int64)[None, :, None], (pairs, 1, 2))
    bad = rng.random((pairs, n_corr)) < wrong
    rows[:, :, 1] = np.where(bad, rng.integers(0, n_corr, (pairs, n_corr)), rows[:, :, 1])
    corr = np.concatenate([src, np.take_along_axis(dst, rows[:, :, 1:2].repeat(3, 2), 1)], 2).reshape(-1, 6)
    off = torch.arange(pairs + 1, dtype=torch.int64, device=device) * n_corr
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)                       # noqa: E731
    return up(corr), off, up(poses), up(src.reshape(-1, 3)), up(dst.reshape(-1, 3)), up(rows.reshape(-1, 2))


def torch_counts(corr, poses, n_corr, d2_max, chunk):
    pairs, n_hyp = poses.shape[0], poses.shape[1]
    out = torch.empty((pairs, n_hyp), dtype=torch.int32, device=corr.device)
    pq = corr.view(pairs, n_corr, 6)
    for p in range(pairs):
        src, dst = pq[p, :, :3], pq[p, :, 3:]
        for h0 in range(0, n_hyp, chunk):
            m = poses[p, h0:h0 + chunk].view(-1, 3, 4)
            moved = torch.matmul(src, m[:, :, :3].transpose(1, 2)) + m[:, None, :, 3]          # (h, C, 3)
            out[p, h0:h0 + chunk] = (((moved - dst) ** 2).sum(2) <= d2_max).sum(1)
    return out


def probe(args, pairs, n_corr, rng, device):
    n_hyp, tau = args.hypotheses, args.distance
    d2_max = float(GR.inlier_d2(tau))
    corr, off, poses, src, dst, rows = make(rng, pairs, n_corr, n_hyp, device)
    valid = torch.ones((pairs, n_hyp), dtype=torch.uint8, device=device)
    tiles = torch.from_numpy(ops.ransac_tiles(np.full(pairs, n_corr))[0]).to(device)
    tests = pairs * n_hyp * n_corr
    res = {'pairs': pairs, 'hypotheses': n_hyp, 'correspondences': n_corr, 'tests': tests,
           'workgroups': int(tiles.shape[0]) * -(-n_hyp // ops.RANSAC_ROWS)}
    counts = ops.ransac_score(corr, off, tiles, poses, valid, d2_max)
    res['hfl_ransac_score'] = events(lambda: ops.ransac_score(corr, off, tiles, poses, valid, d2_max), args.repeats,
                                     args.warmup, args.launches)
    rate = tests / (res['hfl_ransac_score']['median_ms'] * 1e-3)
    res['hfl_ransac_score']['tests_per_s'] = round(rate, 0)
    res['hfl_ransac_score']['share_of_valu_peak'] = round(rate * VALU_PER_TEST / VALU_PEAK, 4)
    eager = torch_counts(corr, poses, n_corr, d2_max, args.torch_chunk)
    res['counts_differ'] = int((eager != counts).sum())
    res['best_is_candidate_0'] = bool((counts.argmax(1) == 0).all())
    res['torch_eager'] = events(lambda: torch_counts(corr, poses, n_corr, d2_max, args.torch_chunk),
                                max(args.repeats // 2, 1), 1)
    res['torch_over_hfl'] = round(res['torch_eager']['median_ms'] / res['hfl_ransac_score']['median_ms'], 3)
    q = torch.from_numpy(rng.uniform(-30.0, 30.0, (pairs * n_hyp, 3)).astype(np.float32)).to(device)
    q_off = torch.arange(pairs + 1, dtype=torch.int64, device=device) * n_hyp
    nn_tiles = torch.from_numpy(ops.overlap_tiles(np.full(pairs, n_hyp))).to(device)
    res['hfl_nn_dist'] = events(lambda: ops.nn_dist(q, q_off, dst, off, nn_tiles), args.repeats, args.warmup, args.launches)
    res['hfl_nn_dist']['tests_per_s'] = round(tests / (res['hfl_nn_dist']['median_ms'] * 1e-3), 0)
    res['score_over_nn_dist'] = round(res['hfl_ransac_score']['median_ms'] / res['hfl_nn_dist']['median_ms'], 3)
    res['ransac_registration_call'] = wall(
        lambda: ransac_registration((src, off), (dst, off), (rows, off), max_correspondence_distance=tau, hypotheses=n_hyp,
                                    refine_iterations=args.refine), max(args.repeats // 2, 1), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, nargs='+', default=[64, 1])
    ap.add_argument('--hypotheses', type=int, default=4096)
    ap.add_argument('--correspondences', type=int, nargs='+', default=[10000, 30000])
    ap.add_argument('--distance', type=float, default=0.8)
    ap.add_argument('--refine', type=int, default=3)
    ap.add_argument('--torch-chunk', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ransac_probe needs a GPU: nothing is timed without one')
    rng = np.random.default_rng(9)
    device = torch.device('cuda', torch.cuda.current_device())
    res = [probe(args, pairs, n_corr, rng, device) for pairs in args.pairs for n_corr in args.correspondences]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
