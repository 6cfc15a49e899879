"""Cost of the batch-hard triplet and contrastive losses at B = 256 (the reference's `batch_size_limit` default) and B = 2048
(the shipped SmoothAP batch), D = 256.  A call is `loss, stats = loss_fn(emb, pos, neg); loss.backward()`: forward, the
statistics' host reads, backward to d emb.

    fused      BatchHardTripletLossWithMasks / BatchHardContrastiveLossWithMasks: hfl_batch_hard_mine, _terms, _grad
    baseline   the same loss assembled from `euclidean_affinity` (hfl_pairwise_dist and its backward) and the torch masking /
               max / min / gather ops of the reference's miner and of pytorch-metric-learning's two losses, with the host reads
               the reference makes for its statistics

The two routes alternate window by window inside one process.  A window is `reps` calls between two device events, `reps`
chosen after the warm-up so that a window lasts about 0.3 s; the figure is the median window over `--windows`, per call.  Host
synchronisations per call are counted where they are made (baseline) or known (fused: the one read of the statistics).  The
three launches are also timed alone, 20 back-to-back between two events.  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch                                                                    # noqa: E402
import loss_cases as lc                                                         # noqa: E402
from hotformerloc_amd import losses, ops                                        # noqa: E402

SIZES = ((41, 256, 256, 4, 3), (42, 2048, 256, 4, 3))          # `make_case` arguments
MARGINS = (0.0, 0.81, 0.82)                                   # near the medians of make_case's loose clusters: about half active


class Baseline:
    """The reference's route on the parent's kernels; `syncs` counts the host synchronisations of the last call."""
    def __init__(self, kind):
        self.kind = kind
        self.syncs = 0

    def item(self, t):
        self.syncs += 1
        return t.item()

    def __call__(self, emb, pos, neg):
        self.syncs = 0
        d = -losses.euclidean_affinity(emb)
        with torch.no_grad():
            dd = d.detach()
            mp = dd.clone()
            mp[~pos] = 0
            hp_d, hp_i = mp.max(dim=1)
            mn = dd.clone()
            mn[~neg] = float('inf')
            hn_d, hn_i = mn.min(dim=1)
            a = torch.where(pos.any(dim=1) & neg.any(dim=1))[0]
            self.syncs += 1
            p, n = hp_i[a], hn_i[a]
            stats = {'max_pos_pair_dist': self.item(hp_d[a].max()), 'max_neg_pair_dist': self.item(hn_d[a].max()),
                     'mean_pos_pair_dist': self.item(hp_d[a].mean()), 'mean_neg_pair_dist': self.item(hn_d[a].mean()),
                     'min_pos_pair_dist': self.item(hp_d[a].min()), 'min_neg_pair_dist': self.item(hn_d[a].min())}
        d_ap, d_an = d[a, p], d[a, n]
        if self.kind == 'triplet':
            v = torch.relu(d_ap - torch.min(d_an, d[p, n]) + MARGINS[0])
            nz = v > 0
            stats['num_non_zero_triplets'] = self.item(nz.sum())
            loss = v[nz].sum() / max(stats['num_non_zero_triplets'], 1)
            stats['num_triplets'] = len(a)
        else:
            pt, nt = torch.relu(d_ap - MARGINS[1]), torch.relu(MARGINS[2] - d_an)
            stats['pos_pairs_above_threshold'] = self.item((pt > 0).sum())
            stats['neg_pairs_above_threshold'] = self.item((nt > 0).sum())
            pos_loss = pt.sum() / max(stats['pos_pairs_above_threshold'], 1)
            neg_loss = nt.sum() / max(stats['neg_pairs_above_threshold'], 1)
            stats['pos_loss'], stats['neg_loss'] = self.item(pos_loss), self.item(neg_loss)
            loss = pos_loss + neg_loss
            stats['num_pairs'] = 2 * len(a)
        stats['loss'] = self.item(loss)
        stats['avg_embedding_norm'] = self.item(emb.detach().norm(dim=1).mean())
        return loss, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-seconds', type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('batch_hard_probe needs a GPU: a CPU run says nothing about these times')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {'dim': 256, 'windows': args.windows, 'sizes': {}}
    for case in SIZES:
        e, pos, neg = lc.make_case(*case)
        batch = e.shape[0]
        emb0, pos, neg = torch.from_numpy(e).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
        entry = {}
        for kind in ('triplet', 'contrastive'):
            fused = (losses.BatchHardTripletLossWithMasks(MARGINS[0]) if kind == 'triplet'
                     else losses.BatchHardContrastiveLossWithMasks(MARGINS[1], MARGINS[2]))
            routes = {'fused': fused, 'baseline': Baseline(kind)}

            def window(name, reps):
                fn = routes[name]
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    emb = emb0.clone().requires_grad_()
                    loss, stats = fn(emb, pos, neg)
                    loss.backward()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps, stats, emb.grad

            reps, last = {}, {}
            for name in routes:                                       # warm-up of this shape, and the window length
                window(name, 3)
                ms, _, _ = window(name, 5)
                reps[name] = max(5, int(math.ceil(args.window_seconds * 1e3 / ms)))
            ms = {name: [] for name in routes}
            for _ in range(args.windows):
                for name in routes:
                    t, stats, grad = window(name, reps[name])
                    ms[name].append(t)
                    last[name] = (stats, grad)
            med = {name: statistics.median(v) for name, v in ms.items()}
            gref = last['baseline'][1]
            entry[kind] = {
                'call_ms': {name: {'median': round(med[name], 4), 'min': round(min(v), 4), 'max': round(max(v), 4),
                                   'calls_per_window': reps[name]} for name, v in ms.items()},
                'baseline_over_fused': round(med['baseline'] / med['fused'], 2),
                'host_syncs_per_call': {'fused': 1, 'baseline': routes['baseline'].syncs},
                'loss': {name: last[name][0]['loss'] for name in routes},
                'grad_diff_over_max': float('%.3g' % ((last['fused'][1] - gref).abs().max() / gref.abs().max()).item())}
        pos8, neg8 = pos.view(torch.uint8), neg.view(torch.uint8)
        p, d_ap, n, d_an = ops.batch_hard_mine(emb0, pos8, neg8)
        _, scale, d_pn, flags = ops.batch_hard_terms(emb0, p, d_ap, n, d_an, ops.BATCH_HARD_TRIPLET, MARGINS[0])
        kernels = {'hfl_batch_hard_mine': lambda: ops.batch_hard_mine(emb0, pos8, neg8),
                   'hfl_batch_hard_terms': lambda: ops.batch_hard_terms(emb0, p, d_ap, n, d_an, ops.BATCH_HARD_TRIPLET, MARGINS[0]),
                   'hfl_batch_hard_grad': lambda: ops.batch_hard_grad(emb0, p, n, d_ap, d_an, d_pn, flags, scale,
                                                                      ops.BATCH_HARD_TRIPLET)}
        entry['kernel_us'] = {}
        for name, fn in kernels.items():
            for _ in range(3):
                fn()
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            entry['kernel_us'][name] = round(e0.elapsed_time(e1) / 20 * 1e3, 1)
        entry['kernel_how'] = '20 back-to-back launches between two HIP events (mine: both of its launches; triplet mode)'
        out['sizes']['B%d' % batch] = entry
    print(json.dumps(out))


if __name__ == '__main__':
    main()
