"""Time the consensus estimator of `hotformerloc_amd/consensus.py` beside two yardsticks measured in the same run.

  graph     `hfl_consensus_graph` alone on `--pairs` pairs x C correspondences for every C of `--correspondences` and every
            share of wrong rows of `--wrong`, `--launches` launches back to back between two HIP events; entries per second
            (one entry = one B_ij).
  poses     `hfl_consensus_poses` alone on the graph and the seeds of that batch (`--seeds` slots of `--size` members).
  matvec    one step of `hfl_spectral_matvec` on the same batch: the same two roots per entry, no bit output.
  calls     the whole `consensus_registration` and the whole `ransac_registration(hypotheses=--hypotheses)` on the same
            batch (gather, hypotheses, score, select, `--refine` polish iterations, one read), wall clock with a device
            synchronisation on both sides; how many pairs each ends within 1 degree and 0.1 m of the truth (with rows
            redirected at random a wrong row now and then lies within `--tau` of its image and shifts the polish by
            millimetres: the count says who found the pose, not who refined it).

No time is fixed in advance.  Median / min / max of `--repeats` measurements after `--warmup`.  One JSON line.  Run it under
`timeout`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import consensus_hypotheses, consensus_registration, ops, ransac_registration             # noqa: E402
from normals_probe import events, wall                                                                            # noqa: E402
from ransac_probe import random_poses                                                                             # noqa: E402


def make(rng, pairs, n_corr, wrong, device):
    """corr (P C, 6), offsets, clouds, rows and the true (P, 3, 4) poses of `pairs` pairs: random points in a 60 m cube, the
    share `wrong` of the rows redirected to a random target row"""
    truth = random_poses(rng, pairs).reshape(pairs, 3, 4).astype(np.float64)
    src = rng.uniform(-30.0, 30.0, (pairs, n_corr, 3)).astype(np.float32)
    dst = (np.einsum('pab,pcb->pca', truth[:, :, :3], src.astype(np.float64)) + truth[:, None, :, 3]).astype(np.float32)
    rows = np.tile(np.arange(n_corr, dtype=np.int64)[None, :, None], (pairs, 1, 2))
    bad = rng.random((pairs, n_corr)) < wrong
    rows[:, :, 1] = np.where(bad, rng.integers(0, n_corr, (pairs, n_corr)), rows[:, :, 1])
    corr = np.concatenate([src, np.take_along_axis(dst, rows[:, :, 1:2].repeat(3, 2), 1)], 2).reshape(-1, 6)
    off = torch.arange(pairs + 1, dtype=torch.int64, device=device) * n_corr
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)                       # noqa: E731
    return up(corr), off, up(src.reshape(-1, 3)), up(dst.reshape(-1, 3)), up(rows.reshape(-1, 2)), truth


def recovered(result, truth):
    """the pairs whose pose lies within 1 degree and 0.1 m of the truth"""
    dr = np.einsum('pab,pcb->pac', result.transforms[:, :3, :3], truth[:, :, :3])
    # from the skew part: the truth went through fp32 and is orthonormal to 1e-7 only, which acos of the trace would magnify
    skew = 0.5 * np.stack([dr[:, 2, 1] - dr[:, 1, 2], dr[:, 0, 2] - dr[:, 2, 0], dr[:, 1, 0] - dr[:, 0, 1]], 1)
    angle = np.degrees(np.arctan2(np.linalg.norm(skew, axis=1), (np.trace(dr, axis1=1, axis2=2) - 1.0) / 2.0))
    shift = np.linalg.norm(result.transforms[:, :3, 3] - truth[:, :, 3], axis=1)
    return int(((angle < 1.0) & (shift < 0.1)).sum())


def probe(args, n_corr, wrong, rng, device):
    pairs = args.pairs
    corr, off, src, dst, rows, truth = make(rng, pairs, n_corr, wrong, device)
    lengths = np.full(pairs, n_corr)
    tiles = torch.from_numpy(ops.consensus_tiles(lengths)[0]).to(device)
    word_off, _ = ops.consensus_words(lengths)
    n_words, word_off = int(word_off[-1]), torch.from_numpy(word_off).to(device)
    entries = pairs * n_corr * n_corr
    res = {'pairs': pairs, 'correspondences': n_corr, 'wrong': wrong, 'entries': entries, 'graph_bytes': 4 * n_words}
    graph = lambda: ops.consensus_graph(corr, off, tiles, word_off, n_words, args.distance)   # noqa: E731
    bits, degree = graph()
    res['mean_degree'] = round(float(degree.double().mean()), 1)
    res['hfl_consensus_graph'] = events(graph, args.repeats, args.warmup, args.launches)
    res['hfl_consensus_graph']['entries_per_s'] = round(entries / (res['hfl_consensus_graph']['median_ms'] * 1e-3), 0)
    clouds = ((src, off), (dst, off), (rows, off))
    _, valid, seeds = consensus_hypotheses(*clouds, distance_threshold=args.distance, seeds=args.seeds, consensus_size=args.size)
    res['valid_share'] = round(float(valid.double().mean()), 4)
    seeds = seeds.to(torch.int32).contiguous()
    res['hfl_consensus_poses'] = events(lambda: ops.consensus_poses(corr, off, bits, word_off, n_words, seeds, args.size),
                                        args.repeats, args.warmup, args.launches)
    s_tiles, s_tile_off = ops.spectral_tiles(lengths)
    s_tiles, s_tile_off = torch.from_numpy(s_tiles).to(device), torch.from_numpy(s_tile_off).to(device)
    inv_s2 = float(np.float32(1.0 / args.distance ** 2))
    res['hfl_spectral_matvec'] = events(lambda: ops.spectral_matvec(corr, off, s_tiles, s_tile_off, inv_s2), args.repeats,
                                        args.warmup, args.launches)
    res['graph_over_matvec'] = round(res['hfl_consensus_graph']['median_ms'] / res['hfl_spectral_matvec']['median_ms'], 3)
    res['poses_over_graph'] = round(res['hfl_consensus_poses']['median_ms'] / res['hfl_consensus_graph']['median_ms'], 3)
    del bits
    consensus = lambda: consensus_registration(*clouds, distance_threshold=args.distance, seeds=args.seeds,      # noqa: E731
                                               consensus_size=args.size, max_correspondence_distance=args.tau,
                                               refine_iterations=args.refine)
    ransac = lambda: ransac_registration(*clouds, max_correspondence_distance=args.tau, hypotheses=args.hypotheses,  # noqa: E731
                                         refine_iterations=args.refine)
    res['consensus_recovered'], res['ransac_recovered'] = recovered(consensus(), truth), recovered(ransac(), truth)
    res['consensus_registration_call'] = wall(consensus, max(args.repeats // 2, 1), 1)
    res['ransac_registration_call'] = wall(ransac, max(args.repeats // 2, 1), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--correspondences', type=int, nargs='+', default=[2000, 10000])
    ap.add_argument('--wrong', type=float, nargs='+', default=[0.3, 0.97])
    ap.add_argument('--distance', type=float, default=0.4, help='the compatibility threshold d')
    ap.add_argument('--tau', type=float, default=0.8, help='the inlier distance of the score and the polish')
    ap.add_argument('--seeds', type=int, default=64)
    ap.add_argument('--size', type=int, default=10)
    ap.add_argument('--hypotheses', type=int, default=4096)
    ap.add_argument('--refine', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('consensus_probe needs a GPU: nothing is timed without one')
    rng = np.random.default_rng(9)
    device = torch.device('cuda', torch.cuda.current_device())
    res = [probe(args, n_corr, wrong, rng, device) for n_corr in args.correspondences for wrong in args.wrong]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
