"""Listwise loss of the reference's training step on the GPU: `TruncatedSmoothAP`
(`models/losses/truncated_smoothap.py:10-99`, built by `models/losses/loss.py:17-19` from
`tau1`, `similarity`, `positives_per_query` of the training config).  Same constructor, same call
signature `(embeddings, positives_mask, negatives_mask) -> (loss, stats)`, same `stats` keys.

The (B, P, B) ranking algebra and its gradient run in one HIP kernel per call (`hfl_smoothap_rows`).
`similarity='euclidean'` is what every shipped training config resolves to (none sets the key and `TrainingParams` defaults
it, `misc/utils.py:204`): the affinity is `-cdist(E, E)` (`loss_utils.py:55-60`), here `euclidean_affinity`, two HIP kernels
that sum the differences themselves (`hfl_pairwise_dist`, `hfl_pairwise_dist_bwd`).  `similarity='cosine'`, the class's
own default, keeps the affinity E E^T and dE = (dS + dS^T) E as dense torch ops.  The top-k selection of positives is a
torch op in both.  `make_losses(params)` is the reference's factory (`models/losses/loss.py:10-24`) for that loss.

`BatchHardTripletLossWithMasks` and `BatchHardContrastiveLossWithMasks` (`models/losses/loss.py:27-135`) mine, evaluate and
differentiate in HIP (`hfl_batch_hard_mine`, `hfl_batch_hard_terms`, `hfl_batch_hard_grad`); their definition is written out
under "Batch-hard losses" below, with numpy twins in fp32 (the kernels' arithmetic) and float64.  `make_loss_fn(params)` is
the complete factory: it builds all three losses.

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
    config).  The two batch-hard losses, which no shipped config selects, are not built here: `make_loss_fn` builds them."""
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


# ---- Batch-hard losses --------------------------------------------------------------------------------------------------------
# Definition (the reference's `HardTripletMinerWithMasks` with pytorch-metric-learning 1.1.2's LpDistance(p = 2, power = 1,
# normalize_embeddings=False), TripletMarginLoss(swap=True), ContrastiveLoss and AvgNonZeroReducer):
#   d[i, j] = ||e_i - e_j||, not squared (the reference's comment says "squared", its code does not square).
#   Mining, no gradient: p(a) = the positive of row a with the largest d[a, .], n(a) = the negative with the smallest, the lowest
#   column on ties; row a is kept iff it has a positive and a negative; T = number of kept rows.
#   Triplet: v = d_ap - min(d_an, d_pn) + margin with d_pn = d[p, n] (the swap; on an exact tie the anchor-negative pair is the
#   one differentiated); a triplet is active iff v > 0; loss = mean of the active v, or 0 with a zero gradient when none is.
#   Contrastive: loss = mean of the positive (d_ap - pos_margin) + mean of the positive (neg_margin - d_an), an empty set giving 0.
#   Gradient: a pair at distance exactly 0 contributes nothing (torch.cdist's convention).
#   T == 0 (the reference crashes in torch.max of an empty tensor): loss 0, zero gradient, counts 0, distance statistics nan.
# One deliberate departure: the reference takes the row maximum of a matrix whose non-positives are set to 0, so that when every
# positive of a row coincides with the anchor its index may point at a non-positive; here the search is restricted to positives.

_TRIPLET, _CONTRASTIVE = ops.BATCH_HARD_TRIPLET, ops.BATCH_HARD_CONTRASTIVE


def _batch_hard_stats(vec, mode):
    """the reference's `stats` dictionary from the 16 numbers of `hfl_batch_hard_terms`"""
    stats = {'loss': vec[12], 'avg_embedding_norm': vec[11]}
    if mode == _TRIPLET:
        stats.update({'num_non_zero_triplets': int(vec[1]), 'num_triplets': int(vec[0])})
    else:
        stats.update({'pos_pairs_above_threshold': int(vec[1]), 'neg_pairs_above_threshold': int(vec[2]),
                      'pos_loss': vec[13], 'neg_loss': vec[14], 'num_pairs': 2 * int(vec[0])})
    stats.update({'mean_pos_pair_dist': vec[5], 'mean_neg_pair_dist': vec[8], 'max_pos_pair_dist': vec[6],
                  'max_neg_pair_dist': vec[9], 'min_pos_pair_dist': vec[7], 'min_neg_pair_dist': vec[10]})
    return stats


def _mask_u8(mask, device):
    mask = mask.to(device)
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)               # the same bytes: no launch
    return (mask != 0).contiguous().view(torch.uint8)


class _BatchHard(torch.autograd.Function):
    """(loss, the 16 statistics) of one call; backward scales the unit-gradient dE as `_SmoothAPRows` scales `dap`."""
    @staticmethod
    def forward(ctx, emb, pos_u8, neg_u8, mode, margin0, margin1):
        p, d_ap, n, d_an = ops.batch_hard_mine(emb, pos_u8, neg_u8)
        vec, scale, d_pn, flags = ops.batch_hard_terms(emb, p, d_ap, n, d_an, mode, margin0, margin1)
        ctx.save_for_backward(emb, p, n, d_ap, d_an, d_pn, flags, scale)
        ctx.mode = mode
        ctx.mark_non_differentiable(vec)
        return scale[2:3].clone().reshape(()), vec

    @staticmethod
    def backward(ctx, grad_loss, _grad_vec):
        emb, p, n, d_ap, d_an, d_pn, flags, scale = ctx.saved_tensors
        return ops.batch_hard_grad(emb, p, n, d_ap, d_an, d_pn, flags, scale, ctx.mode) * grad_loss, None, None, None, None, None


def _batch_hard_call(name, embeddings, positives_mask, negatives_mask, mode, margin0, margin1):
    device = embeddings.device
    if device.type != 'cuda':
        raise _native.NativeLibraryError('%s runs on the GPU only (no CPU fallback)' % name)
    loss, vec = _BatchHard.apply(embeddings.float().contiguous(), _mask_u8(positives_mask, device),
                                 _mask_u8(negatives_mask, device), mode, float(margin0), float(margin1))
    return loss, _batch_hard_stats(vec.tolist(), mode)           # the call's one host read


class BatchHardTripletLossWithMasks:
    """The reference's class (`models/losses/loss.py:78-103`): `(embeddings, positives_mask, negatives_mask) -> (loss, stats)`
    with its `stats` keys, on the GPU only.  Three HIP kernels and one host read per call; the definition, and the one
    departure from the reference's miner (the search is restricted to positives), stand above."""
    def __init__(self, margin: float):
        self.margin = margin

    def __call__(self, embeddings, positives_mask, negatives_mask):
        return _batch_hard_call('BatchHardTripletLossWithMasks', embeddings, positives_mask, negatives_mask, _TRIPLET,
                                self.margin, 0.0)


class BatchHardContrastiveLossWithMasks:
    """The reference's class (`models/losses/loss.py:106-135`), as `BatchHardTripletLossWithMasks`."""
    def __init__(self, pos_margin: float, neg_margin: float):
        self.pos_margin = pos_margin
        self.neg_margin = neg_margin

    def __call__(self, embeddings, positives_mask, negatives_mask):
        return _batch_hard_call('BatchHardContrastiveLossWithMasks', embeddings, positives_mask, negatives_mask, _CONTRASTIVE,
                                self.pos_margin, self.neg_margin)


def batch_hard_mine(emb, pos, neg):
    """The reference's miner on the GPU: (a, p, n, d_ap, d_an) with a the kept rows (int64, ascending), p and n their hardest
    positive and negative (int64) and the two distances (fp32), the bits `ops.pairwise_dist(emb)` holds for those entries.
    emb: (B, D) fp32 on the GPU; pos, neg: (B, B) masks.  Compacting to the kept rows costs a host synchronisation, which the
    loss classes do not pay."""
    if emb.device.type != 'cuda':
        raise _native.NativeLibraryError('batch_hard_mine runs on the GPU only (no CPU fallback)')
    p, d_ap, n, d_an = ops.batch_hard_mine(emb.detach().float().contiguous(), _mask_u8(pos, emb.device), _mask_u8(neg, emb.device))
    a = torch.nonzero((p >= 0) & (n >= 0)).flatten()
    return a, p[a].long(), n[a].long(), d_ap[a], d_an[a]


def make_loss_fn(params):
    """The reference's complete loss factory (`models/losses/loss.py:10-24`): 'batchhardtripletmarginloss' with `.margin`
    (default 0.4), 'batchhardcontrastiveloss' with `.pos_margin` and `.neg_margin` (defaults 0.2 and 0.65, as `TrainingParams`
    resolves them, `misc/utils.py:190-195`), and whatever `make_losses` builds.  There are two factories because
    `make_losses` is pinned by its tests to refuse the two batch-hard names, which it did while they were not built; this
    one is the one to call."""
    def margin(name, default):
        value = getattr(params, name, None)
        return default if value is None else value

    if params.loss == 'batchhardtripletmarginloss':
        return BatchHardTripletLossWithMasks(margin('margin', 0.4))
    if params.loss == 'batchhardcontrastiveloss':
        return BatchHardContrastiveLossWithMasks(margin('pos_margin', 0.2), margin('neg_margin', 0.65))
    return make_losses(params)


def _fmaf32(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64; the float64 sum is rounded to odd (its error term
    comes from the two-sum), after which the rounding to float32 is the single rounding of the exact result."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    prod, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        s = prod + c
        t = s - prod
        err = (prod - (s - t)) + (c - t)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _host_dist(e, dtype):
    """(B, B) distances.  float32: the chain of `hfl_pairwise_dist` (fmaf(diff, diff, acc), k ascending, then sqrt), hence
    its bits; float64: the same sum in float64."""
    b, d = e.shape
    acc = np.zeros((b, b), dtype)
    for k in range(d):
        diff = e[:, None, k] - e[None, :, k]
        acc = _fmaf32(diff, diff, acc) if dtype == np.float32 else acc + diff * diff
    return np.sqrt(acc)


def _host_mine_rows(e, pos, neg, dtype):
    dm = _host_dist(e, dtype)
    pos, neg = np.asarray(pos) != 0, np.asarray(neg) != 0
    p = np.where(pos.any(1), np.argmax(np.where(pos, dm, -1), axis=1), -1)           # first arg-max / arg-min
    n = np.where(neg.any(1), np.argmin(np.where(neg, dm, np.inf), axis=1), -1)
    rows = np.arange(e.shape[0])
    return dm, p, n, np.where(p >= 0, dm[rows, p], 0).astype(dtype), np.where(n >= 0, dm[rows, n], 0).astype(dtype)


def batch_hard_mine_host(emb, pos, neg, dtype=np.float32):
    """`batch_hard_mine` in numpy: (a, p, n, d_ap, d_an).  dtype float32 reproduces the kernels' chain, float64 is the yardstick."""
    dtype = np.dtype(dtype).type
    e = np.ascontiguousarray(np.asarray(emb, np.float32)).astype(dtype)
    _, p, n, d_ap, d_an = _host_mine_rows(e, pos, neg, dtype)
    a = np.nonzero((p >= 0) & (n >= 0))[0]
    return a, p[a], n[a], d_ap[a], d_an[a]


def _batch_hard_host(emb, pos, neg, mode, margin0, margin1, dtype):
    dtype = np.dtype(dtype).type
    f32 = dtype == np.float32
    e = np.ascontiguousarray(np.asarray(emb, np.float32)).astype(dtype)
    b, d = e.shape
    dm, p, n, d_ap, d_an = _host_mine_rows(e, pos, neg, dtype)
    kept = (p >= 0) & (n >= 0)
    a = np.nonzero(kept)[0]
    ap, an = d_ap[a].astype(np.float64), d_an[a].astype(np.float64)
    vec = [0.0] * 16
    vec[0] = float(len(a))
    if len(a):
        vec[5:11] = [ap.mean(), ap.max(), ap.min(), an.mean(), an.max(), an.min()]
    else:
        vec[5:11] = [float('nan')] * 6
    if f32:
        sq = np.zeros(b, np.float32)
        for k in range(d):
            sq = _fmaf32(e[:, k], e[:, k], sq)
        vec[11] = float(np.sqrt(sq).astype(np.float64).mean())
    else:
        vec[11] = float(np.sqrt((e * e).sum(1)).mean())
    pairs = []                                            # (anchor, x, y, sign, set, distance): the pairs that carry gradient
    if mode == _TRIPLET:
        d_pn = dm[p[a], n[a]]
        swapped = d_pn < d_an[a]
        v = (ap - np.where(swapped, d_pn, d_an[a]).astype(np.float64)) + margin0
        active = v > 0
        vec[1], vec[2], vec[3] = float(active.sum()), float((active & swapped).sum()), float(v[active].sum())
        vec[12] = vec[3] / vec[1] if vec[1] else 0.0
        for t in np.nonzero(active)[0]:
            pairs.append((a[t], a[t], p[a[t]], 1, 0, d_ap[a[t]]))
            pairs.append((a[t], p[a[t]], n[a[t]], -1, 0, d_pn[t]) if swapped[t] else (a[t], a[t], n[a[t]], -1, 0, d_an[a[t]]))
        extra = {'d_pn': d_pn, 'active': active, 'swapped': swapped, 'v': v}
    else:
        pt, nt = ap - margin0, margin1 - an
        vec[1], vec[2], vec[3], vec[4] = float((pt > 0).sum()), float((nt > 0).sum()), float(pt[pt > 0].sum()), float(nt[nt > 0].sum())
        vec[13] = vec[3] / vec[1] if vec[1] else 0.0
        vec[14] = vec[4] / vec[2] if vec[2] else 0.0
        vec[12] = vec[13] + vec[14]
        for t in range(len(a)):
            if pt[t] > 0:
                pairs.append((a[t], a[t], p[a[t]], 1, 0, d_ap[a[t]]))
            if nt[t] > 0:
                pairs.append((a[t], a[t], n[a[t]], -1, 1, d_an[a[t]]))
        extra = {'pos_t': pt, 'neg_t': nt}
    scale = [dtype(1.0 / vec[1]) if vec[1] else dtype(0), dtype(1.0 / vec[2]) if vec[2] and mode == _CONTRASTIVE else dtype(0)]
    grad = np.zeros((b, d), dtype)
    for _, x, y, sign, which, dist in pairs:              # anchors ascending, the positive pair first: the kernel's order per row
        if not dist > 0:
            continue
        w = dtype(sign * scale[which]) / dtype(dist)
        for i, o in ((x, y), (y, x)):
            grad[i] = _fmaf32(w, e[i] - e[o], grad[i]) if f32 else grad[i] + w * (e[i] - e[o])
    extra.update({'a': a, 'p': p[a], 'n': n[a], 'd_ap': d_ap[a], 'd_an': d_an[a]})
    return vec[12], grad, _batch_hard_stats(vec, mode), extra


def batch_hard_triplet_host(emb, pos, neg, margin, dtype=np.float32, details=False):
    """`BatchHardTripletLossWithMasks(margin)` in numpy: (loss, gradient, stats).  dtype float32 follows the kernels operation
    for operation (the distances' fmaf chain, the float64 terms of float32 distances, the gradient's fmaf order); float64 is the
    yardstick.  `details=True` appends a dict with the mined triples (a, p, n, d_ap, d_an), d_pn, v, active and swapped."""
    out = _batch_hard_host(emb, pos, neg, _TRIPLET, float(margin), 0.0, dtype)
    return out if details else out[:3]


def batch_hard_contrastive_host(emb, pos, neg, pos_margin, neg_margin, dtype=np.float32, details=False):
    """`BatchHardContrastiveLossWithMasks(pos_margin, neg_margin)` in numpy, as `batch_hard_triplet_host`; the details hold
    the mined triples and the two term vectors pos_t and neg_t."""
    out = _batch_hard_host(emb, pos, neg, _CONTRASTIVE, float(pos_margin), float(neg_margin), dtype)
    return out if details else out[:3]
