"""Retrieval metric of the reference's evaluation (`eval/pnv_evaluate.py:199-315`) on the GPU: exact flat-L2
top-25 search of every query descriptor in a database set -- one (Q, D) x (D, N) GEMM plus a top-k instead of a
FAISS index / sklearn KDTree -- then recall@1..25, top-1 % recall and mean reciprocal rank, with the reference's
`get_recall` signature and return value.

The whole evaluation loop of `eval/pnv_evaluate.py:76-225` sits beside it: `encode_clouds` (every set through the model in
`val_batch_size` batches), `FlatL2Index` (the FAISS `GpuIndexFlatL2` role: a streamed HIP search, `hfl_flat_l2_topk`, that
never stores the (Q, N) distance matrix, followed by an f64 re-ranking of its 32 candidates), `recall_from_indices` (the
metric of `get_recall` from a CSR ground truth instead of a dense (Q, N) mask) and `evaluate_embeddings` /
`evaluate_dataset` (the average over the (database set, query set) pairs).

The intra-sequence (loop-closure) protocol of Wild-Places, for which the reference only writes the per-run pickles, is at the
end: `causal_limits`, `FlatL2Index.search(limits=)` (every scan searched among the scans recorded at least `time_thresh`
earlier, `hfl_flat_l2_topk_prefix`), `evaluate_intra_sequence` / `evaluate_intra_sequence_host`, `intra_sequence_arrays`
and `evaluate_intra_dataset`."""

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

    def search(self, queries, k: int = 25, refine: bool = True, limits=None):
        """queries (Q, D) -> (squared distances, indices), both (Q, min(k, N)), nearest first, equal distances by lower index,
        on the GPU.  refine=False: the kernel's own fp32 distances and int32 indices.  refine=True: the kernel's min(32, N)
        candidates re-ranked by their f64 distance ((q - d)^2).sum() -- f64 distances, int64 indices; this is the exact f64
        ranking whenever the f64 top-k lie inside the fp32 top-32, i.e. when the k-th and the 33rd smallest distance differ
        by more than 2^-22 (D + 4) (|q|^2 + |d|^2).  Non-finite descriptors: undefined order.

        limits (Q,) integers in [0, N]: query q sees the database rows [0, limits[q]) only (`ops.flat_l2_topk_prefix`), the
        33rd smallest distance above being that of its prefix.  Both results are then (Q, k) whatever N: the slots past
        min(k, limits[q]) hold distance +inf and index -1."""
        k = int(k)
        if k < 1 or k > MAX_K:
            raise ValueError('FlatL2Index.search: 1 <= k <= %d expected, got %d' % (MAX_K, k))
        _check_descriptors('FlatL2Index.search queries', tuple(queries.shape))
        if queries.shape[1] != self.dim:
            raise ValueError('FlatL2Index.search: queries have D = %d, the index D = %d' % (queries.shape[1], self.dim))
        q = _device_f32(queries, self.database.device)
        n = len(self)
        if limits is None:
            kk, kp = min(k, n), min(MAX_K, n)

            def topk(width):
                return ops.flat_l2_topk(q, self.database, width, self.sq_norms)
        else:
            kk, kp = k, MAX_K

            def topk(width):
                return ops.flat_l2_topk_prefix(q, self.database, limits, width, self.sq_norms)
        with torch.cuda.device(self.database.device):
            if not refine:
                return topk(kk)
            _, cand = topk(kp)
            cand = torch.sort(cand.long(), dim=1).values          # by index, so that the stable sort below breaks ties by it
            # a prefix's unused slots (index -1, in front after the sort) are gathered as row 0 and sort last at +inf
            rows = cand if limits is None else cand.clamp_min(0)
            d2 = torch.empty((q.shape[0], kp), dtype=torch.float64, device=q.device)
            # per query the gathered fp32 rows, their f64 copy and one more f64 temporary: 20 bytes an element
            chunk = max(1, REFINE_SCRATCH_BYTES // (kp * self.dim * 20))
            for s in range(0, q.shape[0], chunk):
                diff = self.database[rows[s:s + chunk]].double()
                diff -= q[s:s + chunk].double()[:, None, :]
                diff *= diff
                torch.sum(diff, dim=2, out=d2[s:s + chunk])
            if limits is not None:
                d2.masked_fill_(cand < 0, float('inf'))
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


# ------------------------------------------------------------------------------------------------ intra-sequence evaluation
# The second Wild-Places protocol (loop closure inside one run): a scan may only be matched against scans of the same run
# recorded at least `time_thresh` seconds earlier.  The reference writes the per-run pickles for it
# (`datasets/WildPlaces/generate_test_sets.py:60-62`) and never reads them, so the protocol is defined here:
# `evaluate_intra_sequence_host` is the definition in numpy float64, `evaluate_intra_sequence` the device route.
_HOST_CHUNK_BYTES = 64 << 20


def causal_limits(timestamps, time_thresh):
    """(N,) int64: limits[i] = the number of j with t_j <= t_i - time_thresh, for non-decreasing timestamps -- scan i may be
    matched against scans [0, limits[i]).  float64 throughout (epoch seconds have an fp32 ulp of minutes).  A tensor gives
    a tensor on its device, anything else a numpy array.  time_thresh > 0, so that limits[i] <= i: no scan sees itself."""
    if not float(time_thresh) > 0:
        raise ValueError('causal_limits: time_thresh > 0 expected, got %r' % (time_thresh,))
    if isinstance(timestamps, torch.Tensor):
        t = timestamps.detach().to(torch.float64).contiguous()
        if t.dim() != 1:
            raise ValueError('causal_limits: (N,) timestamps expected, got %s' % (tuple(t.shape),))
        if t.numel() > 1 and not bool((t[1:] >= t[:-1]).all().item()):
            raise ValueError('causal_limits: timestamps must be non-decreasing (sort the run by time first)')
        return torch.searchsorted(t, t - float(time_thresh), right=True)
    t = np.ascontiguousarray(np.asarray(timestamps, dtype=np.float64))
    if t.ndim != 1:
        raise ValueError('causal_limits: (N,) timestamps expected, got %s' % (t.shape,))
    if t.shape[0] > 1 and not bool((t[1:] >= t[:-1]).all()):
        raise ValueError('causal_limits: timestamps must be non-decreasing (sort the run by time first)')
    return np.searchsorted(t, t - np.float64(time_thresh), side='right').astype(np.int64)


def intra_sequence_arrays(run_set):
    """The reference's per-run dict {i: {'query', 'northing', 'easting', 'pose', 'timestamp'}} (one `<run>.pickle` of
    `generate_test_sets.py`) -> (order (N,) int64, positions (N, 2) float64 as (easting, northing), timestamps (N,)
    float64), positions and timestamps in time order: `order` is the stable sort of the ascending keys by timestamp, so
    scan r of the ordered run is `run_set[order[r]]`."""
    keys = np.asarray(sorted(run_set.keys()), dtype=np.int64)
    t = np.asarray([run_set[int(i)]['timestamp'] for i in keys], dtype=np.float64)
    by_time = np.argsort(t, kind='stable')
    order = keys[by_time]
    positions = np.asarray([[run_set[int(i)]['easting'], run_set[int(i)]['northing']] for i in order],
                           dtype=np.float64).reshape(-1, 2)
    return order, positions, t[by_time]


def _intra_arguments(embeddings, positions, timestamps, num_neighbors):
    n = int(embeddings.shape[0])
    if tuple(positions.shape) != (n, 2) or tuple(timestamps.shape) != (n,):
        raise ValueError('intra-sequence evaluation: %d embeddings, positions %s, timestamps %s'
                         % (n, tuple(positions.shape), tuple(timestamps.shape)))
    if n < 1:
        raise ValueError('intra-sequence evaluation: the run is empty')
    num_neighbors = int(num_neighbors)
    if num_neighbors < 1 or num_neighbors > MAX_K:
        raise ValueError('intra-sequence evaluation: 1 <= num_neighbors <= %d expected, got %d' % (MAX_K, num_neighbors))
    return num_neighbors


def _host_f64(x):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def _device_f64(x, device):
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.array(x, dtype=np.float64))
    return x.detach().to(device=device, dtype=torch.float64).contiguous()


def evaluate_intra_sequence(embeddings, positions, timestamps, time_thresh: float = 600.0, world_thresh: float = 3.0,
                            num_neighbors: int = 25, thresholds=None) -> dict:
    """Intra-sequence (loop-closure) evaluation of one run in time order on the GPU: `embeddings` (N, D), `positions`
    (N, 2) easting / northing, `timestamps` (N,) non-decreasing.

    limits = `causal_limits(timestamps, time_thresh)`; the evaluated scans E are those with limits[i] >= 1; "within
    `world_thresh`" is dx*dx + dy*dy <= r*r in float64; the revisits R are the scans of E with some j < limits[i] within
    `world_thresh` (`radius_lists`, whose lists ascend: the first listed index decides).  Every scan is searched in its own
    prefix (`FlatL2Index.search(limits=)`, refined); hit[i, r]: the r-th result is valid and within `world_thresh` of i.

    Returns numpy arrays and Python numbers:
      'recall' (num_neighbors,) percent, recall[r] = 100 |{i in R: any hit[i, :r + 1]}| / |R|; 'mrr' = 100 mean(1 /
      (first hit + 1)) over the i in R that have one; 'num_evaluated' |E|, 'num_revisits' |R|;
      the sweep over cuts tau of the top-1 embedding distance s_i (square root of the f64 squared distance, i in E), with
      predicted = s_i <= tau, TP = predicted and hit[i, 0], FP = predicted and not hit[i, 0], FN = not predicted and i in R,
      TN the rest: 'thresholds', 'tp', 'fp', 'fn', 'tn' (int64), 'precision' = TP / (TP + FP) or 1, 'recall_curve' =
      TP / (TP + FN) or 0, 'f1' = 2 P R / (P + R) or 0; 'f1_max' and 'f1_max_threshold', the smallest cut attaining it
      (0 and NaN without cuts).  `thresholds=None`: the sorted distinct s_i, the exact curve.
    Without revisits 'recall' and 'mrr' are NaN and 'f1_max' is 0.  After the search: one sort and cumulative sums on the
    device."""
    from . import tuples
    if not torch.cuda.is_available():
        raise NativeLibraryError('evaluate_intra_sequence runs on the GPU (evaluate_intra_sequence_host is the CPU route)')
    index = FlatL2Index(embeddings)
    dev = index.database.device
    pos, ts = _device_f64(positions, dev), _device_f64(timestamps, dev)
    k = _intra_arguments(index.database, pos, ts, num_neighbors)
    limits = causal_limits(ts, time_thresh)
    r2 = float(np.float64(world_thresh) * np.float64(world_thresh))
    with torch.cuda.device(dev):
        evaluated = limits >= 1
        off, ids = tuples.radius_lists(pos, None, world_thresh)
        count = off[1:] - off[:-1]
        first_near = ids[off[:-1].clamp(max=ids.shape[0] - 1)].long()
        revisit = evaluated & (count > 0) & (first_near < limits)
        d2, idx = index.search(index.database, k=k, refine=True, limits=limits)
        valid = idx >= 0
        delta = pos[idx.clamp_min(0)] - pos[:, None, :]
        dx, dy = delta[..., 0], delta[..., 1]
        hit = valid & (dx * dx + dy * dy <= r2)

        n_rev = int(revisit.sum().item())
        n_eval = int(evaluated.sum().item())
        hit_r = hit & revisit[:, None]
        any_hit = hit_r.any(1)
        first = hit_r.to(torch.uint8).argmax(1)[any_hit]
        found = torch.zeros(k, dtype=torch.float64, device=dev)
        found.index_add_(0, first, torch.ones(first.shape[0], dtype=torch.float64, device=dev))
        nan = float('nan')
        recall = (torch.cumsum(found, 0) / float(n_rev) * 100).cpu().numpy() if n_rev else np.full(k, nan)
        mrr = float((1.0 / (first.double() + 1.0)).mean().item() * 100) if first.shape[0] else nan

        s = torch.sqrt(d2[:, 0][evaluated])
        hit0, in_r = hit[:, 0][evaluated], revisit[evaluated]
        s, by_s = torch.sort(s)
        zero = torch.zeros(1, dtype=torch.long, device=dev)
        cum_hit = torch.cat([zero, torch.cumsum(hit0[by_s].long(), 0)])
        cum_r = torch.cat([zero, torch.cumsum(in_r[by_s].long(), 0)])
        cuts = torch.unique(s) if thresholds is None else _device_f64(thresholds, dev).reshape(-1)
        predicted = torch.searchsorted(s, cuts, right=True)               # how many s_i <= tau
        tp = cum_hit[predicted]
        fp = predicted - tp
        fn = n_rev - cum_r[predicted]
        tn = n_eval - tp - fp - fn
        out = _sweep_curves(cuts, tp, fp, fn, tn)
    out = {key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in out.items()}
    out.update(recall=recall, mrr=mrr, num_evaluated=n_eval, num_revisits=n_rev)
    return out


def _sweep_curves(cuts, tp, fp, fn, tn):
    """Precision, recall, F1 and the best cut from the four counts of every cut, on the counts' device."""
    tpf, pred, pos = tp.double(), tp + fp, tp + fn
    one, zero = torch.ones_like(tpf), torch.zeros_like(tpf)
    precision = torch.where(pred > 0, tpf / pred.clamp_min(1).double(), one)
    recall = torch.where(pos > 0, tpf / pos.clamp_min(1).double(), zero)
    denom = precision + recall
    f1 = torch.where(denom > 0, 2.0 * precision * recall / torch.where(denom > 0, denom, one), zero)
    best = (float(f1.max()), float(cuts[f1 == f1.max()].min())) if f1.shape[0] else (0.0, float('nan'))
    return {'thresholds': cuts, 'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn, 'precision': precision, 'recall_curve': recall,
            'f1': f1, 'f1_max': best[0], 'f1_max_threshold': best[1]}


def _sweep_curves_host(cuts, tp, fp, fn, tn):
    """`_sweep_curves` in numpy: the same float64 operations in the same order."""
    tpf, pred, pos = tp.astype(np.float64), tp + fp, tp + fn
    one, zero = np.ones_like(tpf), np.zeros_like(tpf)
    precision = np.where(pred > 0, tpf / np.maximum(pred, 1).astype(np.float64), one)
    recall = np.where(pos > 0, tpf / np.maximum(pos, 1).astype(np.float64), zero)
    denom = precision + recall
    f1 = np.where(denom > 0, 2.0 * precision * recall / np.where(denom > 0, denom, one), zero)
    best = (float(f1.max()), float(cuts[f1 == f1.max()].min())) if f1.shape[0] else (0.0, float('nan'))
    return {'thresholds': cuts, 'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn, 'precision': precision, 'recall_curve': recall,
            'f1': f1, 'f1_max': best[0], 'f1_max_threshold': best[1]}


def evaluate_intra_sequence_host(embeddings, positions, timestamps, time_thresh: float = 600.0, world_thresh: float = 3.0,
                                 num_neighbors: int = 25, thresholds=None) -> dict:
    """`evaluate_intra_sequence` in numpy float64 on the CPU, the definition of the protocol: dense squared distances summed
    over the differences of the fp32 descriptors (chunked over query rows), columns >= limits[i] masked, a stable argsort
    (equal distances by lower index).  The same arguments, the same keys."""
    emb = embeddings.detach().cpu().numpy() if isinstance(embeddings, torch.Tensor) else np.asarray(embeddings)
    _check_descriptors('evaluate_intra_sequence_host embeddings', emb.shape)
    emb = emb.astype(np.float32).astype(np.float64)
    pos, ts = _host_f64(positions), _host_f64(timestamps)
    k = _intra_arguments(emb, pos, ts, num_neighbors)
    n, dim = emb.shape
    limits = causal_limits(ts, time_thresh)
    r2 = np.float64(world_thresh) * np.float64(world_thresh)
    cols = np.arange(n)
    d2 = np.full((n, k), np.inf)
    idx = np.full((n, k), -1, dtype=np.int64)
    near_before = np.zeros(n, dtype=bool)
    rows = max(1, _HOST_CHUNK_BYTES // (n * dim * 8))
    for r0 in range(0, n, rows):
        diff = emb[r0:r0 + rows, None, :] - emb[None, :, :]
        dist = (diff * diff).sum(-1)
        allowed = cols[None, :] < limits[r0:r0 + rows, None]
        dist[~allowed] = np.inf
        order = np.argsort(dist, axis=1, kind='stable')[:, :k]
        got = np.take_along_axis(dist, order, 1)
        ok = np.arange(order.shape[1])[None, :] < limits[r0:r0 + rows, None]
        d2[r0:r0 + rows, :order.shape[1]] = np.where(ok, got, np.inf)
        idx[r0:r0 + rows, :order.shape[1]] = np.where(ok, order, -1)
        dx = pos[r0:r0 + rows, None, 0] - pos[None, :, 0]
        dy = pos[r0:r0 + rows, None, 1] - pos[None, :, 1]
        near_before[r0:r0 + rows] = ((dx * dx + dy * dy <= r2) & allowed).any(1)
    evaluated = limits >= 1
    revisit = evaluated & near_before
    valid = idx >= 0
    delta = pos[np.maximum(idx, 0)] - pos[:, None, :]
    dx, dy = delta[..., 0], delta[..., 1]
    hit = valid & (dx * dx + dy * dy <= r2)

    n_rev, n_eval = int(revisit.sum()), int(evaluated.sum())
    hit_r = hit & revisit[:, None]
    any_hit = hit_r.any(1)
    first = hit_r.argmax(1)[any_hit]
    found = np.bincount(first, minlength=k).astype(np.float64)
    nan = float('nan')
    recall = np.cumsum(found) / float(n_rev) * 100 if n_rev else np.full(k, nan)
    mrr = float((1.0 / (first.astype(np.float64) + 1.0)).mean() * 100) if first.shape[0] else nan

    s = np.sqrt(d2[evaluated, 0])
    hit0, in_r = hit[evaluated, 0], revisit[evaluated]
    cuts = np.unique(s) if thresholds is None else np.asarray(thresholds, dtype=np.float64).reshape(-1)
    predicted = s[None, :] <= cuts[:, None]                                 # (cuts, |E|)
    tp = (predicted & hit0[None, :]).sum(1).astype(np.int64)
    fp = (predicted & ~hit0[None, :]).sum(1).astype(np.int64)
    fn = (~predicted & in_r[None, :]).sum(1).astype(np.int64)
    tn = n_eval - tp - fp - fn
    out = _sweep_curves_host(cuts, tp, fp, fn, tn)
    out.update(recall=recall, mrr=mrr, num_evaluated=n_eval, num_revisits=n_rev)
    return out


def evaluate_intra_dataset(model, clouds, run_set, batch_size: int, *, time_thresh: float = 600.0, world_thresh: float = 3.0,
                           num_neighbors: int = 25, thresholds=None, **encode_kwargs) -> dict:
    """Intra-sequence evaluation of one run from raw clouds: `run_set` the reference's per-run dict, `clouds[i]` the (n, 3)
    cloud of `run_set[i]`; the clouds go through `encode_clouds` in time order (`intra_sequence_arrays`), `encode_kwargs`
    to it, then `evaluate_intra_sequence`."""
    order, positions, timestamps = intra_sequence_arrays(run_set)
    emb = encode_clouds(model, (clouds[int(i)] for i in order), batch_size, **encode_kwargs)
    return evaluate_intra_sequence(emb, positions, timestamps, time_thresh=time_thresh, world_thresh=world_thresh,
                                   num_neighbors=num_neighbors, thresholds=thresholds)
