"""Time the spectral verification of `hotformerloc_amd/spectral.py` against two yardsticks measured in the same run.

  matvec    `hfl_spectral_matvec` alone (a later step: it normalises the previous one as it loads v) on `--pairs` pairs x C
            correspondences for every C of `--correspondences`, `--launches` launches back to back between two HIP events;
            tests per second, one test = one matrix entry times one v_j (C^2 per pair).
  score     `hfl_ransac_score` on as many tests: C candidate poses against the pair's C correspondences.
  torch     the same product from a dense eager-torch M (broadcast differences on both sides, the formula, `torch.bmm`), on
            `--dense-pairs` pairs so that M and its temporaries fit: once with M built every time (what an eager route pays
            per call, M being too large to keep for a batch) and once with M resident.  The products are compared.
  rerank    the whole `rerank_candidates` call for `--queries` queries x `--candidates` candidates of `--points` points
            (`synthetic.raw_submap`), wall clock with a device synchronisation on both sides.

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
from hotformerloc_amd import ops, rerank_candidates                                                               # noqa: E402
from hotformerloc_amd import synthetic as syn                                                                     # noqa: E402
from normals_probe import events, wall                                                                            # noqa: E402
from ransac_probe import make                                                                                     # noqa: E402


def lengths(x):
    """(P, C, C) pairwise distances of (P, C, 3) points, a coordinate at a time.  Not `torch.cdist`: in its exact mode it
    returned wrong values at 8 x 2000^2 entries on ROCm (right at 4 x 700^2), which made the comparison below meaningless"""
    d2 = None
    for c in range(3):
        d = x[:, :, None, c] - x[:, None, :, c]
        d2 = d * d if d2 is None else d2 + d * d
    return torch.sqrt(d2)


def dense_product(corr, v, pairs, n_corr, inv_s2, m=None):
    """(w (P, C), M): the matrix of every pair in memory"""
    if m is None:
        pq = corr.view(pairs, n_corr, 6)
        e = lengths(pq[:, :, :3]) - lengths(pq[:, :, 3:])
        m = torch.clamp_min(1.0 - e * e * inv_s2, 0.0)
        m.diagonal(dim1=1, dim2=2).zero_()
    return torch.bmm(m, v.view(pairs, n_corr, 1)).view(pairs, n_corr), m


def probe(args, pairs, n_corr, rng, device):
    inv_s2 = float(np.float32(1.0 / args.distance ** 2))
    corr, off, poses, _, _, _ = make(rng, pairs, n_corr, n_corr, device)
    tiles, tile_off = ops.spectral_tiles(np.full(pairs, n_corr))
    tiles, tile_off = torch.from_numpy(tiles).to(device), torch.from_numpy(tile_off).to(device)
    tests = pairs * n_corr * n_corr
    res = {'pairs': pairs, 'correspondences': n_corr, 'tests': tests, 'workgroups': int(tiles.shape[0])}
    w0, p0 = ops.spectral_matvec(corr, off, tiles, tile_off, inv_s2)
    w1, p1 = ops.spectral_matvec(corr, off, tiles, tile_off, inv_s2, w0, p0)
    res['hfl_spectral_matvec'] = events(lambda: ops.spectral_matvec(corr, off, tiles, tile_off, inv_s2, w0, p0, w1, p1),
                                        args.repeats, args.warmup, args.launches)
    res['hfl_spectral_matvec']['tests_per_s'] = round(tests / (res['hfl_spectral_matvec']['median_ms'] * 1e-3), 0)
    valid = torch.ones((pairs, n_corr), dtype=torch.uint8, device=device)
    r_tiles = torch.from_numpy(ops.ransac_tiles(np.full(pairs, n_corr))[0]).to(device)
    res['hfl_ransac_score'] = events(lambda: ops.ransac_score(corr, off, r_tiles, poses, valid, 0.64), args.repeats, args.warmup,
                                     args.launches)
    res['hfl_ransac_score']['tests_per_s'] = round(tests / (res['hfl_ransac_score']['median_ms'] * 1e-3), 0)
    res['matvec_over_score'] = round(res['hfl_spectral_matvec']['median_ms'] / res['hfl_ransac_score']['median_ms'], 3)
    dp = min(pairs, args.dense_pairs)
    d_corr = corr[:dp * n_corr]
    norm = torch.sqrt((w0.view(pairs, n_corr)[:dp].double() ** 2).sum(1)).float()
    v = (w0.view(pairs, n_corr)[:dp] / norm[:, None]).contiguous()
    want, m = dense_product(d_corr, v, dp, n_corr, inv_s2)
    got = w1.view(pairs, n_corr)[:dp]
    res['dense_pairs'] = dp
    res['product_max_relative_difference'] = float(((got - want).abs().max(1).values / want.abs().max(1).values).max())
    res['torch_dense_build_and_product'] = events(lambda: dense_product(d_corr, v, dp, n_corr, inv_s2),
                                                  max(args.repeats // 2, 1), 1)
    res['torch_dense_product_only'] = events(lambda: dense_product(d_corr, v, dp, n_corr, inv_s2, m), max(args.repeats // 2, 1), 1)
    per_pair = res['hfl_spectral_matvec']['median_ms'] / pairs
    res['torch_build_and_product_over_hfl'] = round(res['torch_dense_build_and_product']['median_ms'] / dp / per_pair, 3)
    res['torch_product_only_over_hfl'] = round(res['torch_dense_product_only']['median_ms'] / dp / per_pair, 3)
    return res


def probe_rerank(args, rng, device):
    n_db = max(args.candidates * 2, 2)
    queries = [torch.from_numpy(syn.raw_submap(900 + i, args.points, extent=args.extent)).to(device) for i in range(args.queries)]
    database = [torch.from_numpy(syn.raw_submap(1900 + i, args.points, extent=args.extent)).to(device) for i in range(n_db)]
    cand = np.stack([rng.permutation(n_db)[:args.candidates] for _ in range(args.queries)])
    res = {'queries': args.queries, 'candidates': args.candidates, 'points': args.points,
           'distinct_clouds': args.queries + int(np.unique(cand).shape[0])}
    res['rerank_candidates_call'] = wall(lambda: rerank_candidates(queries, database, cand), max(args.repeats // 2, 1), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--correspondences', type=int, nargs='+', default=[2000, 10000])
    ap.add_argument('--dense-pairs', type=int, default=8)
    ap.add_argument('--distance', type=float, default=0.4)
    ap.add_argument('--queries', type=int, default=8)
    ap.add_argument('--candidates', type=int, default=25)
    ap.add_argument('--points', type=int, default=4096)
    ap.add_argument('--extent', type=float, default=86.0)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('spectral_probe needs a GPU: nothing is timed without one')
    rng = np.random.default_rng(9)
    device = torch.device('cuda', torch.cuda.current_device())
    res = {'matvec': [probe(args, args.pairs, n_corr, rng, device) for n_corr in args.correspondences],
           'rerank': probe_rerank(args, rng, device)}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
