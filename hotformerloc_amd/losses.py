"""Listwise loss of the reference's training step on the GPU: `TruncatedSmoothAP`
(`models/losses/truncated_smoothap.py:10-99`, built by `models/losses/loss.py:17-19` from
`tau1`, `similarity`, `positives_per_query` of the training config).  Same constructor, same call
signature `(embeddings, positives_mask, negatives_mask) -> (loss, stats)`, same `stats` keys.

The (B, P, B) ranking algebra and its gradient run in one HIP kernel per call (`hfl_smoothap_rows`).
`similarity='euclidean'` is what every shipped training config resolves to (none sets the key and `TrainingParams` defaults
it, `misc/utils.py:204`): the affinity is `-cdist(E, E)` (`loss_utils.py:55-60`), here `euclidean_affinity`, two HIP kernels
that sum the differences themselves (`hfl_pairwise_dist`, `hfl_pairwise_dist_bwd`).  `similarity='cosine'`, the class's
own default, keeps the affinity E E^T and dE = (dS + dS^T) E as dense torch ops.  The top-k selection of positives is a
torch op in both.  `make_losses(params)` is the reference's factory (`models/losses/loss.py:10-24`).

`kdloss` is the distillation term of the reference's MESA step (`models/losses/loss.py:138-147`): KL rows and their gradient in
one HIP launch (`hfl_kd_rows`)."""

import numpy as np
import torch

from . import _native
from . import ops


class _SmoothAPRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sim, pos_u8, neg_u8, idx, tau):
        ap, dap = ops.smoothap_rows(sim, pos_u8, neg_u8, idx, tau)
        ctx.save_for_backward(dap)
        return ap

    @staticmethod
    def backward(ctx, grad_ap):
        (dap,) = ctx.saved_tensors
        return dap * grad_ap[:, None], None, None, None, None


class _EuclideanAffinity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb):
        dist = ops.pairwise_dist(emb)
        ctx.save_for_backward(dist, emb)
        return -dist

    @staticmethod
    def backward(ctx, grad_aff):
        dist, emb = ctx.saved_tensors
        return ops.pairwise_dist_bwd(-grad_aff, dist, emb)


def euclidean_affinity(emb):
    """`compute_aff(emb, similarity='euclidean')` of the reference (`loss_utils.py:55-60`): -||e_i - e_j|| as a (B, B) matrix,
    differentiable for an arbitrary (B, B) gradient.  emb: (B, D) fp32 rows on the GPU.  Rows at distance 0 (the diagonal
    among them) receive no gradient from each other, as in `torch.cdist`."""
    if emb.device.type != 'cuda':
        raise _native.NativeLibraryError('euclidean_affinity runs on the GPU only (no CPU fallback)')
    return _EuclideanAffinity.apply(emb.float().contiguous())


class TruncatedSmoothAP:
    def __init__(self, tau1: float = 0.01, similarity: str = 'cosine', positives_per_query: int = 4):
        if similarity not in ('cosine', 'euclidean'):
            raise NotImplementedError('Incorrect similarity measure: %s' % (similarity,))       # loss_utils.py:62
        self.tau1 = tau1
        self.similarity = similarity
        self.positives_per_query = positives_per_query

    def __call__(self, embeddings, positives_mask, negatives_mask):
        device = embeddings.device
        if device.type != 'cuda':
            raise _native.NativeLibraryError('TruncatedSmoothAP runs on the GPU only (no CPU fallback)')
        positives_mask = positives_mask.to(device)
        negatives_mask = negatives_mask.to(device)
        emb = embeddings.float()
        if self.similarity == 'cosine':
            s_qz = emb @ emb.t()                                                   # compute_aff, cosine
        else:
            s_qz = euclidean_affinity(emb)                                         # compute_aff, euclidean
        s_pos = s_qz.detach().clone()
        s_pos.masked_fill_(torch.logical_not(positives_mask), -np.inf)
        idx = torch.topk(s_pos, k=self.positives_per_query, dim=1, largest=True, sorted=True)[1]
        n_positives = positives_mask.sum(dim=1)
        valid = torch.gather(positives_mask, 1, idx)
        n_valid = valid.sum(dim=1)
        valid_q = n_valid > 0
        ap_rows = _SmoothAPRows.apply(s_qz.contiguous(), positives_mask.to(torch.uint8).contiguous(),
                                      negatives_mask.to(torch.uint8).contiguous(), idx.contiguous(), self.tau1)
        ap = ap_rows[valid_q].mean()
        loss = 1. - ap
        with torch.no_grad():                                                      # truncated_smoothap.py:71-80
            best = s_qz.detach().gather(1, idx[:, :1])
            hard_ranking = torch.logical_and(s_qz.detach() > best, negatives_mask).sum(dim=1)
            stats = {'positives_per_query': n_positives.float().mean(dim=0).item(),
                     'best_positive_ranking': hard_ranking.float().mean(dim=0).item(),
                     'recall': {1: (hard_ranking <= 1).float().mean(dim=0).item()},
                     'loss': loss.item(), 'ap': ap.item(),
                     'avg_embedding_norm': embeddings.norm(dim=1).mean().item()}
        return loss, stats


def make_losses(params):
    """The reference's loss factory (`models/losses/loss.py:10-24`).  `params`: any object with `.loss` and, for
    'truncatedsmoothap', `.tau1`, `.similarity` and `.positives_per_query` (what `TrainingParams` resolves from a training
    config).  The two batch-hard losses, which no shipped config selects, are not built."""
    if params.loss in ('batchhardtripletmarginloss', 'batchhardcontrastiveloss'):
        raise NotImplementedError('loss %r is not built: every shipped training config selects TruncatedSmoothAP' % params.loss)
    if params.loss == 'truncatedsmoothap':
        return TruncatedSmoothAP(tau1=params.tau1, similarity=params.similarity,
                                 positives_per_query=params.positives_per_query)
    raise NotImplementedError('Unknown loss: {}'.format(params.loss))


class _KdRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, teacher, temperature):
        kl, dkl = ops.kd_rows(y, teacher, temperature)
        ctx.save_for_backward(dkl)
        return kl

    @staticmethod
    def backward(ctx, grad_kl):
        (dkl,) = ctx.saved_tensors
        return dkl * grad_kl[:, None], None, None


def kdloss(y, teacher_scores, T: float = 3.0, weight: float = 50.0):
    """`weight * KLDivLoss(reduction='batchmean')(log_softmax(y / T), softmax(teacher_scores / T))`: the reference's
    `kdloss(y, teacher_scores)` with its constants T = 3 and 50 as defaults.  y, teacher_scores: (B, D) fp32 rows on the GPU,
    D a multiple of 64 up to 1024.  The gradient flows to `y` only; a teacher that requires grad is an error (detach it)."""
    if teacher_scores.requires_grad:
        raise ValueError('kdloss: the teacher rows must not require grad (the teacher receives no gradient); detach them')
    if y.device.type != 'cuda':
        raise _native.NativeLibraryError('kdloss runs on the GPU only (no CPU fallback)')
    rows = _KdRows.apply(y.float().contiguous(), teacher_scores.float().contiguous(), float(T))
    return weight * rows.sum() / y.shape[0]
