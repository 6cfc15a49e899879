"""Training tuples and evaluation ground truth straight from scan positions, on the GPU.

The reference derives both offline (`datasets/pointnetvlad/generate_training_tuples_*.py`, `generate_test_sets.py`, the
WildPlaces pair, `datasets/CSWildPlaces/generate_train_test_tuples.py:92-212`): a `sklearn.neighbors.KDTree` over the N
positions, `query_radius` at `pos_thresh` and `neg_thresh`, a Python loop of `np.setdiff1d` / `np.sort` per anchor, one
`query_radius` per query and database for the evaluation truth, and a pickle for each.  Here the whole step is a
fixed-radius join in two dimensions (`hfl_radius_lists`, csrc/radius.hip): a count launch, one `torch.cumsum`, a fill
launch, and the lists are CSR on the device -- what `TupleIndex.from_csr` and `retrieval.recall_from_indices` take.

Membership is exactly `dx*dx + dy*dy <= r*r` with every operation rounded to float64: what `KDTree.query_radius` evaluates
for the Euclidean metric (the reduced distance against `r*r`).  With two terms the sum does not depend on the column
order, so `[easting, northing]` and `[northing, easting]` callers agree.  float64 is not optional: a UTM northing is about
6.9e6, where one float32 ulp is half a metre.  Every list is strictly ascending, as `np.sort` / `np.setdiff1d` leave it.
`radius_lists_host` / `radius_counts_host` restate the same expression in numpy: the route without a GPU and the yardstick
of the tests, equal to the kernel bit for bit.
"""

import numpy as np
import torch

from . import _native
from .batch_masks import TupleIndex

_HOST_CHUNK_PAIRS = 1 << 22            # pairs of one host chunk: (rows, N) float64 temporaries of 32 MiB


def _positions(x, what: str):
    """(rows, 2) float64, contiguous, as the array or tensor kind that came in; ValueError for anything else."""
    if isinstance(x, torch.Tensor):
        if x.dim() != 2 or x.shape[1] != 2:
            raise ValueError('%s: (rows, 2) positions expected, got shape %s (only D = 2 is supported)' % (what, tuple(x.shape)))
        if x.shape[0] < 1:
            raise ValueError('%s: no positions' % what)
        if x.dtype == torch.bool or x.is_complex():
            raise ValueError('%s: real positions expected, got %s' % (what, x.dtype))
        return x.detach().to(torch.float64).contiguous()
    a = np.asarray(x)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError('%s: (rows, 2) positions expected, got shape %s (only D = 2 is supported)' % (what, a.shape))
    if a.shape[0] < 1:
        raise ValueError('%s: no positions' % what)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError('%s: real positions expected, got %s' % (what, a.dtype))
    return np.ascontiguousarray(a, dtype=np.float64)


def _arguments(queries, database, r_a, r_b, exclude_self):
    same = database is None or database is queries
    if exclude_self and not same:
        raise ValueError('exclude_self is meaningful only when queries and database are the same array '
                         '(pass the same object, or database=None)')
    q = _positions(queries, 'queries')
    d = q if same else _positions(database, 'database')
    if d.shape[0] >= 2 ** 31:
        raise ValueError('%d database positions: ids must fit int32' % d.shape[0])
    r_a = float(r_a)
    r_b = r_a if r_b is None else float(r_b)
    for name, r in (('r_a', r_a), ('r_b', r_b)):
        if not r >= 0.0:
            raise ValueError('%s = %r: a radius is a number >= 0' % (name, r))
    if r_a > r_b:
        raise ValueError('r_a = %r exceeds r_b = %r: list A must be the subset' % (r_a, r_b))
    return q, d, r_a, r_b


def _to_host(x) -> np.ndarray:
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _to_device(x, device) -> torch.Tensor:
    return x.to(device) if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(device)


def _pick_device(q, d):
    """Where the device route runs: the device of a position tensor that is already on a GPU, else the current one."""
    for x in (q, d):
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise _native.NativeLibraryError('radius_lists runs on the GPU (radius_lists_host is the CPU route)')
    return torch.device('cuda', torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------------ device route
def radius_lists(queries, database, r_a, r_b=None, *, exclude_self: bool = False):
    """`(off_a, idx_a)` or, with `r_b`, `(off_a, idx_a, off_b, idx_b)` on the device: list A of query i is
    `idx_a[off_a[i]:off_a[i + 1]]`, the database ids j with `dx*dx + dy*dy <= r_a*r_a` in float64, strictly ascending; list
    B the same at `r_b >= r_a` from the same distance evaluation.  Offsets (Q + 1,) int64, ids int32.

    `queries` (Q, 2), `database` (N, 2): numpy arrays or tensors on either device, Q, N >= 1, N < 2**31; `database=None` or
    the same object as `queries` is the self join.  float32 (and integer) positions are widened to float64 first -- exact,
    but the half-metre float32 grid at UTM magnitudes is then already in the data.  `exclude_self` drops j == i from list A
    only (the reference's `positives` exclude the anchor, its `non_negatives` keep it) and needs the self join.  A NaN
    coordinate is in no list.  A family without a single entry keeps a (1,) id tensor holding 0 (kernels take no null
    pointer); `off[-1]` is always the number of entries.  Two launches on the current stream and one device-to-host read
    of the totals.  No CPU fallback: NativeLibraryError without a GPU (`radius_lists_host` is the CPU route)."""
    from . import ops
    q, d, ra, rb = _arguments(queries, database, r_a, r_b, exclude_self)
    device = _pick_device(q, d)
    dq = _to_device(q, device)
    dd = dq if d is q else _to_device(d, device)
    with torch.cuda.device(device):
        out = ops.radius_lists(dq, dd, ra, rb, exclude_self, want_b=r_b is not None)
    return out if r_b is not None else out[:2]


def radius_counts(queries, database, r):
    """(Q,) int32 on the device: how many database positions lie within `r` of each query (`query_radius(...,
    count_only=True)`: the buffer-zone test of `check_in_test_set`, `filter_query_elements`).  One launch."""
    from . import ops
    q, d, r, _ = _arguments(queries, database, r, None, False)
    device = _pick_device(q, d)
    dq = _to_device(q, device)
    dd = dq if d is q else _to_device(d, device)
    with torch.cuda.device(device):
        return ops.radius_counts(dq, dd, r, r)[:, 0].contiguous()


# -------------------------------------------------------------------------------------------------------------- host route
def _host_chunks(q: np.ndarray, d: np.ndarray):
    """(row0, d2 (rows, N)) over chunks of query rows: the kernel's expression, one rounding per numpy operation."""
    rows = max(1, _HOST_CHUNK_PAIRS // d.shape[0])
    for r0 in range(0, q.shape[0], rows):
        c = q[r0:r0 + rows]
        dx = c[:, None, 0] - d[None, :, 0]
        dy = c[:, None, 1] - d[None, :, 1]
        yield r0, dx * dx + dy * dy


def radius_lists_host(queries, database, r_a, r_b=None, *, exclude_self: bool = False):
    """`radius_lists` in numpy float64 on the CPU, chunked over query rows: the same arguments, the same lists as numpy
    arrays (int64 offsets, int32 ids; an empty family is a (0,) array)."""
    q, d, ra, rb = _arguments(queries, database, r_a, r_b, exclude_self)
    q, d = _to_host(q), _to_host(d)
    ra2, rb2 = np.float64(ra) * np.float64(ra), np.float64(rb) * np.float64(rb)
    counts = np.zeros((2, q.shape[0]), np.int64)
    parts = ([], [])
    for r0, d2 in _host_chunks(q, d):
        masks = [d2 <= ra2] + ([d2 <= rb2] if r_b is not None else [])
        if exclude_self:
            k = np.arange(d2.shape[0])
            masks[0][k, r0 + k] = False
        for f, m in enumerate(masks):
            counts[f, r0:r0 + m.shape[0]] = m.sum(1)
            parts[f].append(np.nonzero(m)[1].astype(np.int32))          # row-major: ascending within every row
    out = []
    for f in range(2 if r_b is not None else 1):
        off = np.zeros(q.shape[0] + 1, np.int64)
        np.cumsum(counts[f], out=off[1:])
        out += [off, np.concatenate(parts[f])]
    return tuple(out)


def radius_counts_host(queries, database, r):
    """`radius_counts` in numpy float64 on the CPU: (Q,) int32."""
    q, d, r, _ = _arguments(queries, database, r, None, False)
    q, d = _to_host(q), _to_host(d)
    r2 = np.float64(r) * np.float64(r)
    out = np.zeros(q.shape[0], np.int32)
    for r0, d2 in _host_chunks(q, d):
        out[r0:r0 + d2.shape[0]] = (d2 <= r2).sum(1)
    return out


# ------------------------------------------------------------------------------------------------- what the pipeline takes
def tuple_index_from_poses(positions, pos_thresh, neg_thresh, device='cuda') -> TupleIndex:
    """The `TupleIndex` of a training set from its (N, 2) scan positions alone, through `TupleIndex.from_csr`:
    positives[i] = the scans within `pos_thresh` of scan i without i itself, non_negatives[i] = the scans within
    `neg_thresh` (i included), both ascending -- the `TrainingTuple` lists of the reference's
    `construct_training_query_dict` (the `generate_training_tuples*` scripts compute the same two lists).  `device='cuda'`
    (or a device tensor) joins on the GPU, `device='cpu'` takes the host route and builds a host-only index.

    Out of scope: the CS-Wild-Places generator's `test_set`, `--ground_aerial_positives_only` and
    `--query_requires_ground` variants (the first two union every same-source scan into each element's non_negatives:
    O(N^2) ids as explicit lists; the README's shipped command uses none of them for the training file), and the polygon
    split of scans into train, test and buffer (it needs shapely and is not the hot part; `radius_counts` is its
    buffer-zone test).  Pass the positions of the training scans only."""
    dev = torch.device(device)
    if dev.type == 'cpu':
        lists = radius_lists_host(positions, None, pos_thresh, neg_thresh, exclude_self=True)
    elif dev.type == 'cuda':
        if dev.index is not None or (isinstance(positions, torch.Tensor) and not positions.is_cuda):
            positions = torch.as_tensor(positions).to(dev)             # an explicit device decides where the join runs
        lists = radius_lists(positions, None, pos_thresh, neg_thresh, exclude_self=True)
        lists = [x.cpu().numpy() for x in lists]
    else:
        raise ValueError("device must be 'cuda' or 'cpu'")
    off_a, idx_a, off_b, idx_b = lists
    return TupleIndex.from_csr(off_a, idx_a[:off_a[-1]], off_b, idx_b[:off_b[-1]], device=device)


def truth_from_poses(query_positions, database_positions, eval_thresh):
    """Evaluation ground truth `(offsets (Q + 1,), indices)` as int64 tensors, query i's true neighbours being the database
    scans within `eval_thresh` of it, ascending: what `retrieval.truth_csr` returns for the reference's
    `construct_query_and_database_sets` dicts, ready for `retrieval.recall_from_indices`.  It runs where the positions
    are: on the GPU, returning tensors there, when a position tensor is on one; otherwise on the host route, returning CPU
    tensors as `truth_csr` does."""
    if any(isinstance(x, torch.Tensor) and x.is_cuda for x in (query_positions, database_positions)):
        off, idx = radius_lists(query_positions, database_positions, eval_thresh)
        return off, idx[:int(off[-1])].long()
    off, idx = radius_lists_host(query_positions, database_positions, eval_thresh)
    return torch.from_numpy(off), torch.from_numpy(idx.astype(np.int64))
