"""Shared by the tests of the Euclidean TruncatedSmoothAP: the golden cases of `tests/golden/loss_smoothap_euclid.npz`
and a float64 torch-autograd restatement of the reference's loss with `similarity='euclidean'`
(`models/losses/truncated_smoothap.py:22-99` on `-torch.cdist(E, E)`, `models/losses/loss_utils.py:55-60`).

The restatement forms the distances from the differences themselves and gives coincident rows (the diagonal among them) a
zero gradient, which is `torch.cdist`'s convention.  `tests/test_loss_euclid_host.py` pins it to the golden values of the
reference's own class; it is then the live yardstick at sizes that have no golden."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import loss_ref                       # noqa: E402
from oracle.gen_golden_loss import make_case      # noqa: E402,F401  (re-exported)

GOLDEN_NAME = 'loss_smoothap_euclid.npz'
SETTINGS_NAME = 'training_loss_settings.json'
# name -> (seed, batch, dim, group, drop_rows, positives_per_query): `make_case` inputs plus the loss's P
CASES = {'b20': (14, 20, 64, 4, 0, 2),            # below the 25 rows at which torch.cdist switches to the matrix-product form
         'b64': (11, 64, 256, 4, 0, 4),
         'b48_few_pos': (12, 48, 256, 3, 5, 4),
         'b96_p2': (13, 96, 128, 6, 2, 2),
         'b65_d72': (15, 65, 72, 5, 0, 4)}        # a one-row tile tail, D no multiple of 64
TAU1 = 0.01


class _DirectDist(torch.autograd.Function):
    """||e_i - e_j|| from the differences; d e_i = sum_j (g_ij + g_ji) (e_i - e_j) / d_ij with 0 where d_ij == 0."""
    @staticmethod
    def forward(ctx, e):
        diff = e[:, None, :] - e[None, :, :]
        d = diff.pow(2).sum(2).sqrt()
        ctx.save_for_backward(diff, d)
        return d

    @staticmethod
    def backward(ctx, g):
        diff, d = ctx.saved_tensors
        w = torch.where(d > 0, (g + g.t()) / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
        return (w[:, :, None] * diff).sum(1)


def direct_dist(e: torch.Tensor) -> torch.Tensor:
    return _DirectDist.apply(e)


def truncated_smooth_ap_euclid(embeddings, positives_mask, negatives_mask, tau1: float = TAU1, positives_per_query: int = 4):
    """(loss, stats) of the reference's class with similarity='euclidean', in the dtype of `embeddings` (float64 for a
    yardstick).  Everything after the affinity is `oracle.loss_ref.truncated_smooth_ap` line for line."""
    s = -direct_dist(embeddings)
    sp = s.detach().clone()
    sp.masked_fill_(~positives_mask, float('-inf'))
    idx = torch.topk(sp, k=positives_per_query, dim=1, largest=True, sorted=True)[1]
    n_pos = positives_mask.sum(1)
    s_diff = s.unsqueeze(1) - s.gather(1, idx).unsqueeze(2)
    sg = loss_ref.temperature_sigmoid(s_diff, tau1)
    pos = sg * positives_mask.unsqueeze(1)
    pos = pos * torch.ones_like(pos).scatter(2, idx.unsqueeze(2), 0.)
    r_p = pos.sum(2) + 1.0
    r_omega = r_p + (sg * negatives_mask.unsqueeze(1)).sum(2)
    r = r_p / r_omega
    hard = torch.logical_and((s_diff.detach() > 0)[:, 0], negatives_mask).sum(1)
    valid = torch.gather(positives_mask, 1, idx)
    n_valid = valid.sum(1)
    q = n_valid > 0
    ap = ((r * valid)[q].sum(1) / n_valid[q]).mean()
    loss = 1.0 - ap
    stats = {'positives_per_query': n_pos.float().mean().item(),
             'best_positive_ranking': hard.float().mean().item(),
             'recall': {1: (hard <= 1).float().mean().item()},
             'loss': loss.item(), 'ap': ap.item(),
             'avg_embedding_norm': embeddings.norm(dim=1).mean().item()}
    return loss, stats


def stats_vector(stats):
    return [stats['positives_per_query'], stats['best_positive_ranking'], stats['recall'][1], stats['ap'],
            stats['avg_embedding_norm']]


def load_golden(golden_dir):
    return np.load(os.path.join(golden_dir, GOLDEN_NAME))


_YARDSTICKS = {}


def yardstick(seed, batch, dim, group, drop, ppq):
    """float64 restatement on one `make_case`, computed once per process: (e, pos, neg, loss, grad, stats); read-only."""
    key = (seed, batch, dim, group, drop, ppq)
    if key not in _YARDSTICKS:
        e, pos, neg = make_case(seed, batch, dim, group, drop)
        emb = torch.from_numpy(e).double().requires_grad_()
        if batch > 256:                  # the (B, B, D) difference tensor in float64 would take gigabytes
            loss, stats = _big_yardstick(emb, torch.from_numpy(pos), torch.from_numpy(neg), ppq)
        else:
            loss, stats = truncated_smooth_ap_euclid(emb, torch.from_numpy(pos), torch.from_numpy(neg), TAU1, ppq)
        loss.backward()
        grad = emb.grad.numpy()
        grad.setflags(write=False)
        _YARDSTICKS[key] = (e, pos, neg, loss.item(), grad, stats)
    return _YARDSTICKS[key]


def _cdist_direct(e):
    """`direct_dist` at batch sizes where the (B, B, D) tensor does not fit: torch's own direct-difference kernel, which has
    the same zero-distance convention (tests/test_loss_euclid_host.py holds the two together)."""
    return torch.cdist(e, e, p=2, compute_mode='donot_use_mm_for_euclid_dist')


def _big_yardstick(emb, pos, neg, ppq):
    """`truncated_smooth_ap_euclid` without its (B, B, D) and (B, P, B) tensors: one positive at a time."""
    s = -_cdist_direct(emb)
    sp = s.detach().clone()
    sp.masked_fill_(~pos, float('-inf'))
    idx = torch.topk(sp, k=ppq, dim=1, largest=True, sorted=True)[1]
    valid = torch.gather(pos, 1, idx)
    n_valid = valid.sum(1)
    rs = []
    for j in range(ppq):
        sg = loss_ref.temperature_sigmoid(s - s.gather(1, idx[:, j:j + 1]), TAU1)
        not_self = torch.ones_like(sg).scatter(1, idx[:, j:j + 1], 0.)
        r_p = (sg * pos * not_self).sum(1) + 1.0
        rs.append(r_p / (r_p + (sg * neg).sum(1)))
    r = torch.stack(rs, 1)
    q = n_valid > 0
    ap = ((r * valid)[q].sum(1) / n_valid[q]).mean()
    loss = 1.0 - ap
    hard = torch.logical_and(s.detach() > s.detach().gather(1, idx[:, :1]), neg).sum(1)
    stats = {'positives_per_query': pos.sum(1).float().mean().item(),
             'best_positive_ranking': hard.float().mean().item(),
             'recall': {1: (hard <= 1).float().mean().item()},
             'loss': loss.item(), 'ap': ap.item(),
             'avg_embedding_norm': emb.norm(dim=1).mean().item()}
    return loss, stats
