"""Retrieval metric of the reference's evaluation (`eval/pnv_evaluate.py:199-315`) on the GPU: exact flat-L2
top-25 search of every query descriptor in a database set -- one (Q, D) x (D, N) GEMM plus a top-k instead of a
FAISS index / sklearn KDTree -- then recall@1..25, top-1 % recall and mean reciprocal rank, with the reference's
`get_recall` signature and return value.

The whole evaluation loop of `eval/pnv_evaluate.py:76-225` sits beside it: `encode_clouds` (every set through the model in
`val_batch_size` batches), `FlatL2Index` (the FAISS `GpuIndexFlatL2` role: a streamed HIP search, `hfl_flat_l2_topk`, that
never stores the (Q, N) distance matrix, followed by an f64 re-ranking of its 32 candidates), `recall_from_indices` (the
metric of `get_recall` from a CSR ground truth instead of a dense (Q, N) mask) and `evaluate_embeddings` /
`evaluate_dataset` (the average over the (database set, query set) pairs)."""

import numpy as np
import torch

from . import ops
from ._native import NativeLibraryError


def flat_l2_topk(database: torch.Tensor, queries: torch.Tensor, k: int):
    """(N, D), (Q, D) on the GPU -> squared-L2 distances and indices (Q, k), nearest first (ties: lower index)."""
    if database.device.type != 'cuda' or queries.device.type != 'cuda':
        raise NativeLibraryError('flat_l2_topk runs on the GPU only (no CPU fallback)')
    db, q = database.double(), queries.double()           # (Q, N) of a few thousand: f64 keeps the ranking exact
    d2 = (q * q).sum(1, keepdim=True) + (db * db).sum(1)[None, :] - 2.0 * (q @ db.t())
    order = torch.argsort(d2, dim=1, stable=True)[:, :k]
    return d2.gather(1, order), order


def get_recall(m, n, database_vectors, query_vectors, query_sets, database_sets=None, log=False,
               model_name: str = 'model', device='cuda'):
    """`eval/pnv_evaluate.py:226-315` (the per-query false-positive logging of `log=True` is not reproduced)."""
    if log:
        raise NotImplementedError('log=True writes the reference\'s debug text files; not part of the metric')
    db = torch.as_tensor(np.asarray(database_vectors[m]), dtype=torch.float32, device=device)
    qs = torch.as_tensor(np.asarray(query_vectors[n]), dtype=torch.float32, device=device)
    num_neighbors = 25
    k = min(num_neighbors, db.shape[0])
    _, idx = flat_l2_topk(db, qs, k)
    n_q, n_db = qs.shape[0], db.shape[0]
    truth = torch.zeros((n_q, n_db), dtype=torch.bool)
    has_truth = torch.zeros(n_q, dtype=torch.bool)
    for i in range(n_q):
        tn = query_sets[n][i][m]
        if len(tn) > 0:
            truth[i, torch.as_tensor(list(tn), dtype=torch.long)] = True
            has_truth[i] = True
    truth, has_truth = truth.to(device), has_truth.to(device)
    hits = truth.gather(1, idx) & has_truth[:, None]                       # (Q, k): is the j-th result a true neighbour
    evaluated = int(has_truth.sum().item())
    any_hit = hits.any(1)
    first = torch.where(any_hit, hits.float().argmax(1), torch.full((n_q,), -1, device=device, dtype=torch.long))
    recall = torch.zeros(num_neighbors, dtype=torch.float64, device=device)
    recall.index_add_(0, first[any_hit], torch.ones(int(any_hit.sum().item()), dtype=torch.float64, device=device))
    threshold = max(int(round(n_db / 100.0)), 1)
    one_percent = int(hits[:, :min(threshold, k)].any(1).sum().item())
    recall = (torch.cumsum(recall, 0) / float(evaluated) * 100).cpu().numpy()
    one_percent_recall = (one_percent / float(evaluated)) * 100
    mrr = float((1.0 / (first[any_hit].double() + 1.0)).mean().item() * 100)
    return recall, one_percent_recall, mrr


# ------------------------------------------------------------------------------------------------ streamed search
MAX_K = 32                       # entries of the kernel's running list: the candidates the f64 refinement re-ranks
REFINE_SCRATCH_BYTES = 32 << 20


def _check_descriptors(what: str, shape):
    if len(shape) != 2:
        raise ValueError('%s: a (rows, D) matrix expected, got %s' % (what, tuple(shape)))
    if shape[1] % 4 != 0 or shape[1] < 4 or shape[1] > 1024:
        raise ValueError('%s: D must be a multiple of 4 in 4..1024, got %d' % (what, shape[1]))


def _device_f32(x, device):
    """numpy / torch, any float dtype, any device -> fp32 contiguous on `device`"""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    return x.to(device=device, dtype=torch.float32).contiguous()


class FlatL2Index:
    """Exact flat-L2 index of one database set: an fp32 copy of the (N, D) descriptors on the GPU and their squared row
    norms.  `search` streams the database past the queries in one HIP launch (`ops.flat_l2_topk`); nothing of size (Q, N)
    is ever allocated."""

    def __init__(self, database, device='cuda'):
        _check_descriptors('FlatL2Index database', tuple(database.shape))
        if database.shape[0] < 1:
            raise ValueError('FlatL2Index: the database is empty')
        if torch.device(device).type != 'cuda':
            raise NativeLibraryError('FlatL2Index runs on the GPU only (no CPU fallback)')
        self.database = _device_f32(database, device)
        self.sq_norms = ops.row_sq_norms(self.database)

    def __len__(self):
        return self.database.shape[0]

    @property
    def dim(self):
        return self.database.shape[1]

    def search(self, queries, k: int = 25, refine: bool = True):
        """queries (Q, D) -> (squared distances, indices), both (Q, min(k, N)), nearest first, equal distances by lower index,
        on the GPU.  refine=False: the kernel's own fp32 distances and int32 indices.  refine=True: the kernel's min(32, N)
        candidates re-ranked by their f64 distance ((q - d)^2).sum() -- f64 distances, int64 indices; this is the exact f64
        ranking whenever the f64 top-k lie inside the fp32 top-32, i.e. when the k-th and the 33rd smallest distance differ
        by more than 2^-22 (D + 4) (|q|^2 + |d|^2).  Non-finite descriptors: undefined order."""
        k = int(k)
        if k < 1 or k > MAX_K:
            raise ValueError('FlatL2Index.search: 1 <= k <= %d expected, got %d' % (MAX_K, k))
        _check_descriptors('FlatL2Index.search queries', tuple(queries.shape))
        if queries.shape[1] != self.dim:
            raise ValueError('FlatL2Index.search: queries have D = %d, the index D = %d' % (queries.shape[1], self.dim))
        q = _device_f32(queries, self.database.device)
        n = len(self)
        kk, kp = min(k, n), min(MAX_K, n)
        with torch.cuda.device(self.database.device):
            if not refine:
                return ops.flat_l2_topk(q, self.database, kk, self.sq_norms)
            _, cand = ops.flat_l2_topk(q, self.database, kp, self.sq_norms)
            cand = torch.sort(cand.long(), dim=1).values          # by index, so that the stable sort below breaks ties by it
            d2 = torch.empty((q.shape[0], kp), dtype=torch.float64, device=q.device)
            # per query the gathered fp32 rows, their f64 copy and one more f64 temporary: 20 bytes an element
            chunk = max(1, REFINE_SCRATCH_BYTES // (kp * self.dim * 20))
            for s in range(0, q.shape[0], chunk):
                diff = self.database[cand[s:s + chunk]].double()
                diff -= q[s:s + chunk].double()[:, None, :]
                diff *= diff
                torch.sum(diff, dim=2, out=d2[s:s + chunk])
            order = torch.argsort(d2, dim=1, stable=True)[:, :kk]
            return d2.gather(1, order), cand.gather(1, order)


# ------------------------------------------------------------------------------------------------ metric from a CSR truth
def truth_csr(query_sets, n: int, m: int):
    """Ground truth of query set n against database set m, `query_sets[n][i][m]`, as CSR: (offsets (Q + 1,), indices)
    int64 CPU tensors; query i's true neighbours are indices[offsets[i]:offsets[i + 1]]."""
    qs = query_sets[n]
    offsets = np.zeros(len(qs) + 1, dtype=np.int64)
    rows = []
    for i in range(len(qs)):
        tn = np.asarray(list(qs[i][m]), dtype=np.int64).reshape(-1)
        rows.append(tn)
        offsets[i + 1] = offsets[i] + tn.shape[0]
    indices = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(offsets), torch.from_numpy(indices.astype(np.int64, copy=False))


def recall_from_indices(idx, truth_offsets, truth_indices, n_database: int, num_neighbors: int = 25):
    """The metric of `get_recall` from the (Q, k) search result `idx` and a CSR ground truth: (recall@1..num_neighbors,
    top-1 % recall, mean reciprocal rank).  Runs on idx's device; membership of a result in its query's truth list is a
    binary search over the sorted keys q * n_database + index -- no (Q, N) mask."""
    idx = torch.as_tensor(idx)
    device = idx.device
    idx = idx.long()[:, :num_neighbors]
    n_q, k = idx.shape
    offsets = torch.as_tensor(truth_offsets).to(device=device, dtype=torch.long)
    indices = torch.as_tensor(truth_indices).to(device=device, dtype=torch.long)
    if offsets.shape[0] != n_q + 1:
        raise ValueError('recall_from_indices: %d queries but %d truth offsets' % (n_q, offsets.shape[0]))
    counts = offsets[1:] - offsets[:-1]
    rows = torch.repeat_interleave(torch.arange(n_q, device=device), counts)
    keys = torch.sort(rows * n_database + indices).values
    wanted = torch.arange(n_q, device=device)[:, None] * n_database + idx
    if keys.numel() > 0:
        at = torch.searchsorted(keys, wanted).clamp_(max=keys.numel() - 1)
        hits = keys[at] == wanted                                          # (Q, k): is the j-th result a true neighbour
    else:
        hits = torch.zeros((n_q, k), dtype=torch.bool, device=device)
    evaluated = int((counts > 0).sum().item())                             # queries without true neighbours are skipped
    any_hit = hits.any(1)
    first = torch.where(any_hit, hits.float().argmax(1), torch.full((n_q,), -1, device=device, dtype=torch.long))
    recall = torch.zeros(num_neighbors, dtype=torch.float64, device=device)
    recall.index_add_(0, first[any_hit], torch.ones(int(any_hit.sum().item()), dtype=torch.float64, device=device))
    threshold = max(int(round(n_database / 100.0)), 1)
    one_percent = int(hits[:, :min(threshold, k)].any(1).sum().item())
    recall = (torch.cumsum(recall, 0) / float(evaluated) * 100).cpu().numpy()
    one_percent_recall = (one_percent / float(evaluated)) * 100
    mrr = float((1.0 / (first[any_hit].double() + 1.0)).mean().item() * 100)
    return recall, one_percent_recall, mrr


# ------------------------------------------------------------------------------------------------ whole-dataset evaluation
def encode_clouds(model, clouds, batch_size: int, *, coordinates: str = 'cartesian', normalize: bool = True,
                  octree_depth: int = 7, full_depth: int = 2, device='cuda', voxel_size=None,
                  normalise_submaps: bool = False, downsample_target=None, downsample_type: str = 'pnvlad',
                  remove_ground: bool = False, ground_params=None, radius_max=None, remove_outliers: bool = False,
                  outlier_params=None, **prepare_kwargs):
    """`get_latent_vectors` (`eval/pnv_evaluate.py:129-187`) without the file loading: raw (n, 3) clouds (a sequence or any
    iterable) -> (len, output_dim) fp32 descriptors on the GPU, `batch_size` clouds per forward (the last batch may be
    short).  Puts the model in eval mode; `prepare_kwargs` go to `prepare_clouds`.  With `voxel_size` and / or
    `normalise_submaps` the clouds are raw submaps in a metric frame: every batch first goes through the CS-Wild-Places
    submap post-processing on the device (`voxel.submap_chain`, as `voxel.prepare_submaps` runs it: voxel-grid downsample at
    `voxel_size`, then the PointNetVLAD normalisation); with the defaults nothing changes and the clouds go to
    `prepare_clouds` as they are.  With `downsample_target` = N the raw submaps become fixed-size clouds of N points
    instead (the Oxford / CS-Campus3D format, `voxel.prepare_submaps_fixed`: the `downsample_type` 'pnvlad' or 'random'
    downsampler, then, when `normalise_submaps`, the normalisation with padding);
    it cannot be combined with `voxel_size`.  With `remove_ground` every batch of raw submaps first goes through the cloth
    filter on the device (`ground.remove_ground(**ground_params)`), before whichever of the steps above is asked for.
    With `radius_max` and / or `remove_outliers` every batch is cleaned before everything else (the radius trim, then the
    statistical outlier filter with `outlier_params`)."""
    from .octree import build_batch_octree
    from .preprocess import prepare_clouds
    from . import voxel
    if batch_size < 1:
        raise ValueError('encode_clouds: batch_size >= 1 expected, got %d' % batch_size)
    if downsample_target is not None and voxel_size is not None:
        raise ValueError('encode_clouds: downsample_target (fixed-size clouds) and voxel_size (one voxel grid) exclude '
                         'each other')
    model.eval()
    out, batch = [], []

    def flush():
        src = voxel.submap_chain(batch, device, radius_max=radius_max, remove_outliers=remove_outliers,
                                 outlier_params=outlier_params, remove_ground=remove_ground, ground_params=ground_params,
                                 voxel_size=voxel_size, target=downsample_target, downsample=downsample_type,
                                 normalise=normalise_submaps)
        pts = prepare_clouds(src, coordinates=coordinates, normalize=normalize, device=device, **prepare_kwargs)
        octree = build_batch_octree(pts, octree_depth, full_depth, device)
        out.append(model({'octree': octree})['global'].float())
        batch.clear()

    with torch.inference_mode():
        for cloud in clouds:
            batch.append(cloud)
            if len(batch) >= batch_size:
                flush()
        if batch:
            flush()
    if not out:
        return None
    return torch.cat(out, 0)


def _index_search(index, queries, k):
    return index.search(queries, k=k, refine=True)[1]


def evaluate_embeddings(database_embeddings, query_embeddings, query_sets, skip_same_run: bool = True, only_database=None,
                        num_neighbors: int = 25, build_index=FlatL2Index, search=_index_search):
    """The pair loop of the reference's `evaluate_dataset` (`eval/pnv_evaluate.py:96-119`): every database set i against
    every query set j -- without i == j when `skip_same_run`, without sets whose embeddings are None, and with
    `only_database` = 1 database set 1 alone (the CSCampus3D rule) -> {'ave_one_percent_recall', 'ave_recall', 'ave_mrr'}.
    One index per database set serves all query sets.  `build_index(embeddings)` and `search(index, queries, k)` ->
    (Q, k) indices are the seams the host tests replace."""
    recall = np.zeros(num_neighbors)
    count = 0
    one_percent_recall, mrr = [], []
    for i in range(len(database_embeddings)):
        if database_embeddings[i] is None or (only_database is not None and i != only_database):
            continue
        index = None
        for j in range(len(query_embeddings)):
            if (i == j and skip_same_run) or query_embeddings[j] is None:
                continue
            if index is None:
                index = build_index(database_embeddings[i])
            n_db = int(database_embeddings[i].shape[0])
            idx = search(index, query_embeddings[j], min(num_neighbors, n_db))
            offsets, indices = truth_csr(query_sets, j, i)
            pair_recall, pair_opr, pair_mrr = recall_from_indices(idx, offsets, indices, n_db, num_neighbors)
            recall += np.asarray(pair_recall)
            count += 1
            one_percent_recall.append(pair_opr)
            mrr.append(pair_mrr)
    return {'ave_one_percent_recall': np.mean(one_percent_recall), 'ave_recall': recall / count, 'ave_mrr': np.mean(mrr)}


def evaluate_dataset(model, database_clouds, query_clouds, query_sets, batch_size: int, skip_same_run: bool = True,
                     only_database=None, **encode_kwargs):
    """`evaluate_dataset` of the reference (`eval/pnv_evaluate.py:76-119`) on raw clouds: `database_clouds` / `query_clouds` are
    lists of sets, a set a sequence of (n, 3) arrays or None; `encode_kwargs` go to `encode_clouds`."""
    def encode(sets):
        return [None if s is None else encode_clouds(model, s, batch_size, **encode_kwargs) for s in sets]
    return evaluate_embeddings(encode(database_clouds), encode(query_clouds), query_sets, skip_same_run=skip_same_run,
                               only_database=only_database)
