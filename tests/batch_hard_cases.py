"""Shared by the tests of the batch-hard triplet and contrastive losses: the case table and a float64 torch-autograd
restatement of the reference's two classes (`models/losses/loss.py:27-135` with pytorch-metric-learning 1.1.2's
LpDistance(p = 2, power = 1, normalize_embeddings=False), TripletMarginLoss(swap=True), ContrastiveLoss, AvgNonZeroReducer).

The restatement: d = plain Euclidean distance from the differences themselves; per row the positive with the largest and the
negative with the smallest distance, lowest column on ties, the search restricted to positives; rows with both are kept;
triplet v = d_ap - min(d_an, d_pn) + margin (the anchor-negative pair on an exact tie), mean of the positive v; contrastive
mean of the positive (d_ap - pos_margin) plus mean of the positive (neg_margin - d_an); an empty set gives 0; pairs at
distance 0 receive no gradient; without a kept row the loss is 0, the counts 0 and the distance statistics nan.

Margins are per case: `make_case` clusters are loose, so the margins that split the triplets into active and inactive sit
near 0.  `conditions(case)` computes what tests/test_batch_hard_host.py asserts of every case, so that no device test can
hide a failure behind a flipped selection."""
import numpy as np
import torch

from loss_cases import direct_dist, make_case

# name -> (generator, generator arguments, triplet margin, pos_margin, neg_margin)
CASES = {
    'b8_g2': ('make_case', (18, 8, 32, 2, 0), -0.08, 0.82, 0.82),
    'b20': ('make_case', (14, 20, 64, 4, 0), -0.03, 0.82, 0.81),
    'b65_d70': ('make_case', (15, 65, 70, 5, 0), -0.05, 0.81, 0.76),            # a one-row tile tail, scalar loads
    'b48_few_pos': ('make_case', (12, 48, 256, 3, 5), 0.04, 0.8, 0.84),       # five rows without positives
    'b96': ('make_case', (13, 96, 128, 6, 2), -0.03, 0.83, 0.8),
    'b300': ('make_case', (16, 300, 256, 4, 3), 0.0, 0.81, 0.821),             # five row tiles
    'b520': ('make_case', (17, 520, 40, 4, 3), -0.2, 0.84, 0.63),              # nine column tiles: above the eight column splits
    'dup24': ('dup_case', (19, 24, 32, 3), -0.26, 0.83, 0.73),                  # coincident rows: zero distances, index ties
    'tight64': ('tight_case', (23, 64, 128, 4), 0.4, 0.2, 0.65),            # tight clusters at the reference's default margins
}
EMPTY_CASES = {'b1': (31, 1, 16, 4, 0), 'b2': (32, 2, 16, 4, 0)}            # `make_case` arguments: no row has a negative


def dup_case(seed, batch, dim, group):
    """`make_case` with coincident rows: rows 0 and 1 (one group) are equal; row 12 is row 0 moved by 1e-3 along the first
    axis, so its two hardest negatives tie exactly (index tie, lowest column 0); row 15 equals row 7 (another group: a
    negative pair at distance 0); rows 18, 19, 20 (a whole group) are equal (positive pairs at distance 0, tied)."""
    e, pos, neg = make_case(seed, batch, dim, group, 0)
    e = e.copy()
    e[1] = e[0]
    e[12] = e[0]
    e[12, 0] += np.float32(1e-3)
    e[15] = e[7]
    e[19] = e[18]
    e[20] = e[18]
    return e, pos, neg


def tight_case(seed, batch, dim, group):
    """Cluster centres in pairs 0.4 to 0.9 apart with members 0.05 to 0.35 from their centre: hardest positives around 0.2 and
    hardest negatives around 0.65, so that the reference's default margins 0.4 / 0.2 / 0.65 split the terms."""
    from hotformerloc_amd import synthetic as syn
    lab = np.arange(batch) // group
    groups = 2 * (batch // (2 * group) + 1)
    c = syn.hash_uniform(seed, groups * dim).reshape(-1, dim)                      # float64 in (-1, 1)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    sep = 0.65 + 0.25 * syn.hash_uniform(seed + 3, groups)
    c[1::2] = c[0::2] + sep[1::2, None] * c[1::2]                    # centres in pairs 0.4 to 0.9 apart: the close negatives
    noise = syn.hash_uniform(seed + 1, batch * dim).reshape(batch, dim)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    amp = (0.14 + 0.1 * syn.hash_uniform(seed + 2, groups))[lab] * (1.0 + 0.4 * syn.hash_uniform(seed + 4, batch))
    e = (c[lab] + amp[:, None] * noise).astype(np.float32)
    pos = (lab[:, None] == lab[None, :]) & ~np.eye(batch, dtype=bool)
    neg = lab[:, None] != lab[None, :]
    return e, pos, neg


_GENERATORS = {'make_case': make_case, 'dup_case': dup_case, 'tight_case': tight_case}
_INPUTS = {}


def inputs(name):
    """(e float32 (B, D), pos, neg bool (B, B)) of a case; computed once, read-only."""
    if name not in _INPUTS:
        if name in EMPTY_CASES:
            out = make_case(*EMPTY_CASES[name])
        else:
            out = _GENERATORS[CASES[name][0]](*CASES[name][1])
        for t in out:
            t.setflags(write=False)
        _INPUTS[name] = out
    return _INPUTS[name]


def margins(name):
    return (0.4, 0.2, 0.65) if name in EMPTY_CASES else CASES[name][2:]


def dist64(e):
    """float64 distances from the differences, zero gradient between coincident rows; torch's own direct-difference kernel
    where the (B, B, D) tensor of `direct_dist` would be large (tests/test_loss_euclid_host.py holds the two together)."""
    if e.shape[0] * e.shape[0] * e.shape[1] > (1 << 24):
        return torch.cdist(e, e, p=2, compute_mode='donot_use_mm_for_euclid_dist')
    return direct_dist(e)


def mine64(d, pos, neg):
    """(a, p, n) from a (B, B) numpy distance matrix: first arg-max over the positives, first arg-min over the negatives."""
    p = np.argmax(np.where(pos, d, -1.0), axis=1)
    n = np.argmin(np.where(neg, d, np.inf), axis=1)
    a = np.nonzero(pos.any(1) & neg.any(1))[0]
    return a, p[a], n[a]


def _mean_positive(x):
    keep = x.detach() > 0
    return (x[keep].mean() if bool(keep.any()) else x.sum() * 0.0), int(keep.sum())


def _common_stats(emb, d_ap, d_an):
    nan = float('nan')
    stats = {'avg_embedding_norm': emb.detach().norm(dim=1).mean().item()}
    for key, v in (('pos', d_ap.detach()), ('neg', d_an.detach())):
        some = v.numel() > 0
        stats['mean_%s_pair_dist' % key] = v.mean().item() if some else nan
        stats['max_%s_pair_dist' % key] = v.max().item() if some else nan
        stats['min_%s_pair_dist' % key] = v.min().item() if some else nan
    return stats


def _mined(emb, pos, neg):
    d = dist64(emb)
    a, p, n = (torch.from_numpy(v) for v in mine64(d.detach().numpy(), np.asarray(pos), np.asarray(neg)))
    return d, a, p, n


def triplet64(emb, pos, neg, margin):
    """(loss, stats, details) of BatchHardTripletLossWithMasks(margin) in the dtype of `emb` (a float64 leaf for the yardstick)."""
    d, a, p, n = _mined(emb, pos, neg)
    d_ap, d_an, d_pn = d[a, p], d[a, n], d[p, n]
    swapped = d_pn.detach() < d_an.detach()
    v = d_ap - torch.where(swapped, d_pn, d_an) + margin
    loss, active = _mean_positive(v)
    stats = {'loss': loss.item(), 'num_non_zero_triplets': active, 'num_triplets': len(a)}
    stats.update(_common_stats(emb, d_ap, d_an))
    details = {'a': a.numpy(), 'p': p.numpy(), 'n': n.numpy(), 'd_ap': d_ap.detach().numpy(), 'd_an': d_an.detach().numpy(),
               'd_pn': d_pn.detach().numpy(), 'v': v.detach().numpy(), 'swapped': swapped.numpy()}
    return loss, stats, details


def contrastive64(emb, pos, neg, pos_margin, neg_margin):
    """(loss, stats, details) of BatchHardContrastiveLossWithMasks(pos_margin, neg_margin), as `triplet64`."""
    d, a, p, n = _mined(emb, pos, neg)
    d_ap, d_an = d[a, p], d[a, n]
    pos_t, neg_t = d_ap - pos_margin, neg_margin - d_an
    pos_loss, n_pos = _mean_positive(pos_t)
    neg_loss, n_neg = _mean_positive(neg_t)
    loss = pos_loss + neg_loss
    stats = {'loss': loss.item(), 'pos_pairs_above_threshold': n_pos, 'neg_pairs_above_threshold': n_neg,
             'pos_loss': pos_loss.item(), 'neg_loss': neg_loss.item(), 'num_pairs': 2 * len(a)}
    stats.update(_common_stats(emb, d_ap, d_an))
    details = {'a': a.numpy(), 'p': p.numpy(), 'n': n.numpy(), 'd_ap': d_ap.detach().numpy(), 'd_an': d_an.detach().numpy(),
               'pos_t': pos_t.detach().numpy(), 'neg_t': neg_t.detach().numpy()}
    return loss, stats, details


_YARDSTICKS = {}


def yardstick(name, kind):
    """The float64 restatement on a case, computed once per process: (loss, grad, stats, details); read-only.
    kind: 'triplet' or 'contrastive'."""
    if (name, kind) not in _YARDSTICKS:
        e, pos, neg = inputs(name)
        m, pm, nm = margins(name)
        emb = torch.from_numpy(e.astype(np.float64)).requires_grad_()
        if kind == 'triplet':
            loss, stats, details = triplet64(emb, pos, neg, m)
        else:
            loss, stats, details = contrastive64(emb, pos, neg, pm, nm)
        loss.backward()
        grad = emb.grad.numpy()
        grad.setflags(write=False)
        _YARDSTICKS[(name, kind)] = (loss.item(), grad, stats, details)
    return _YARDSTICKS[(name, kind)]


def conditions(name):
    """What the case table must satisfy, as numbers (tests/test_batch_hard_host.py asserts them)."""
    from hotformerloc_amd.losses import batch_hard_mine_host
    e, pos, neg = inputs(name)
    _, pm, nm = margins(name)
    _, _, _, t = yardstick(name, 'triplet')
    a32, p32, n32, _, _ = batch_hard_mine_host(e, pos, neg, np.float32)
    active = t['v'] > 0
    c = {'triplets': len(t['a']), 'active': int(active.sum()), 'swapped_active': int((active & t['swapped']).sum()),
         'same_mining': bool(np.array_equal(a32, t['a']) and np.array_equal(p32, t['p']) and np.array_equal(n32, t['n'])),
         'closest_v': float(np.abs(t['v']).min()),
         'closest_swap': float(np.abs(t['d_pn'] - t['d_an'])[active].min()) if active.any() else float('inf'),
         'pos_above': int((t['d_ap'] > pm).sum()), 'neg_above': int((t['d_an'] < nm).sum()),
         'closest_margin': float(min(np.abs(t['d_ap'] - pm).min(), np.abs(t['d_an'] - nm).min()))}
    return c


def stat_keys(kind):
    common = ['loss', 'avg_embedding_norm'] + ['%s_%s_pair_dist' % (f, s) for f in ('mean', 'max', 'min') for s in ('pos', 'neg')]
    if kind == 'triplet':
        return common, ['num_triplets', 'num_non_zero_triplets']
    return common + ['pos_loss', 'neg_loss'], ['num_pairs', 'pos_pairs_above_threshold', 'neg_pairs_above_threshold']
