"""Cases and float64 references for the octree convolution kernels (csrc/dwconv.hip, csrc/tapconv.hip and the gather pair of
csrc/window_misc.hip).  CPU only: no GPU code and no oracle is imported here; tests/test_octree_conv_cases_host.py proves the
generators and references, tests/test_gpu_octree_conv_shapes.py runs the kernels against them.

Two kinds of operands:

* integer data (`int_operands`): small integers stored as f32, every product and every partial sum in any order exact in
  fp32 (the generator proves |sum| < 2^24 from the table), so a kernel must EQUAL the float64 reference bit for bit;
* real data (`real_operands`): standard normals; the per-element bound is `(T + 2) u S`, u = 2^-24, T the number of terms of
  the element's sum and S their absolute sum in float64 -- the textbook bound gamma_T S of a T-term fp32 sum in any order,
  plus one rounding for a bias or addend and one for the final store.
"""
import numpy as np
import torch

U = 2.0 ** -24
EDGE_COUNTS = (0, 1, 8, 9, 10, 16, 17, 18, 19, 24, 25, 26, 27)
DEAD_RUN = 16


# ------------------------------------------------------------------------------------------------ tables
def edge_counts(K):
    """live-tap counts the first rows of an 'edges' table carry: the gather-batch edges (B = 9 and B = 8) up to K, and K"""
    return sorted({c for c in EDGE_COUNTS if c <= K} | {K})


def edges_min_rows(K):
    return len(edge_counts(K)) + DEAD_RUN + 2


def make_table(n_out, n_src, K, live, seed, dtype=torch.int32):
    """(n_out, K) gather table into n_src source rows, -1 = no neighbour, injective per column (every column is a random
    injection of output rows into source rows; `inverse_neigh_kernel` is only defined for such tables).  `live`:
    'dense' all entries live, 'sparse' about 20 %, 'edges' the rows described in `edge_counts` first, then DEAD_RUN all-dead
    rows, a row whose only live tap is the last one, a row whose only live tap is tap 0, and 'sparse'-like rows after them.
    A table that cannot hold the promised rows is refused (ValueError), never silently reduced."""
    rng = np.random.default_rng(seed)
    m = min(n_out, n_src)
    t = np.full((n_out, K), -1, dtype=np.int64)
    for k in range(K):
        t[rng.permutation(n_out)[:m], k] = rng.permutation(n_src)[:m]
    if live == 'dense':
        if n_src < n_out:
            raise ValueError('a dense table needs n_src >= n_out')
    elif live == 'sparse':
        t[rng.random((n_out, K)) >= 0.2] = -1
    elif live == 'edges':
        counts = edge_counts(K)
        need = edges_min_rows(K)
        if n_out < need or n_src < n_out:
            raise ValueError("an 'edges' table of K = %d needs %d <= n_out <= n_src (got %d, %d)" % (K, need, n_out, n_src))
        keep = rng.random((n_out, K)) < 0.5
        r = 0
        for c in counts:
            keep[r] = False
            keep[r, rng.permutation(K)[:c]] = True
            r += 1
        keep[r:r + DEAD_RUN] = False
        r += DEAD_RUN
        keep[r] = False
        keep[r, K - 1] = True
        keep[r + 1] = False
        keep[r + 1, 0] = True
        t[~keep] = -1
        check_edges(t, K)
    else:
        raise ValueError(live)
    return torch.from_numpy(t).to(dtype)


def check_edges(t, K):
    """every promised row of an 'edges' table is there"""
    t = np.asarray(t)
    n_live = (t >= 0).sum(1)
    counts = edge_counts(K)
    assert n_live[:len(counts)].tolist() == counts, (n_live[:len(counts)].tolist(), counts)
    r = len(counts)
    assert (n_live[r:r + DEAD_RUN] == 0).all()
    r += DEAD_RUN
    assert n_live[r] == 1 and t[r, K - 1] >= 0
    assert n_live[r + 1] == 1 and t[r + 1, 0] >= 0


def zero_live_rows(table):
    return (np.asarray(table) >= 0).sum(1) == 0


def is_injective(table):
    t = np.asarray(table)
    for k in range(t.shape[1]):
        col = t[:, k][t[:, k] >= 0]
        if np.unique(col).size != col.size:
            return False
    return True


def single_reader(table, src_row=0, seed=0):
    """A copy of `table` in which source row `src_row` is read by exactly one live (row, tap) pair, and that pair: every
    reference to it is killed, then one dead entry is revived (the column holds no other reference, so it stays injective)."""
    t = table.numpy().astype(np.int64)
    t[t == src_row] = -1
    dead = np.argwhere(t < 0)
    # a row that keeps other live taps: the poisoned element's own sum has finite terms too
    n_live = (t >= 0).sum(1)
    dead = dead[n_live[dead[:, 0]] > 0]
    h, k = dead[np.random.default_rng(seed).integers(len(dead))]
    t[h, k] = src_row
    assert (t == src_row).sum() == 1 and is_injective(t)
    return torch.from_numpy(t).to(table.dtype), int(h), int(k)


# ------------------------------------------------------------------------------------------------ operands
def _ints(rng, shape, lim):
    return torch.from_numpy(rng.integers(-lim, lim + 1, size=shape).astype(np.float32))


def int_operands(table, n_src, C, seed, lim=3, rows_sum=False):
    """(data (n_src, C), weight (K, 1, C), grad (n_out, C), bound): integers of magnitude <= lim stored as f32.  `bound` is the
    worst |sum| any kernel of the family can form from them over this table -- per output row lim^2 * live taps (+ lim for an
    addend or bias), or with `rows_sum` (the weight gradients, lim = 1) lim^2 * the live rows of a tap -- and is asserted to
    stay below 2^24: every partial sum in any order is then exact in fp32."""
    t = np.asarray(table)
    rng = np.random.default_rng(seed)
    n_out, K = t.shape
    data, weight, grad = _ints(rng, (n_src, C), lim), _ints(rng, (K, 1, C), lim), _ints(rng, (n_out, C), lim)
    live = t >= 0
    per_row = int(live.sum(1).max()) if n_out else 0
    bound = lim * lim * per_row + lim
    if rows_sum:
        bound = max(bound, lim * lim * int(live.sum(0).max()))
    assert bound < 2 ** 24, bound
    return data, weight, grad, bound


def real_operands(table, n_src, C, seed):
    """(data, weight, grad): standard normals"""
    g = torch.Generator().manual_seed(seed)
    n_out, K = table.shape
    return torch.randn(n_src, C, generator=g), torch.randn(K, 1, C, generator=g), torch.randn(n_out, C, generator=g)


def norm_params(C, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        return (torch.randint(-3, 4, (C,), generator=g).float(), torch.randint(-3, 4, (C,), generator=g).float())
    return 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def bound(T, S):
    """per-element error bound (T + 2) u S; T broadcasts against S"""
    return (torch.as_tensor(T, dtype=torch.float64) + 2) * U * S


# ------------------------------------------------------------------------------------------------ float64 references
def _taps(table):
    t = torch.as_tensor(np.asarray(table)).long()
    return t, t >= 0


def dwconv_ref(data, weight, table, add=None):
    """out[h, c] = sum_k [t[h, k] >= 0] w[k, c] data[t[h, k], c] [+ add[h, c]]  ->  (out, S, T): the float64 sum, the absolute
    sum of its terms and the number of live taps of the row (n_out, 1)"""
    t, live = _taps(table)
    d, w = data.double(), weight.double().reshape(t.shape[1], -1)
    out = torch.zeros(t.shape[0], d.shape[1], dtype=torch.float64)
    S = torch.zeros_like(out)
    for k in range(t.shape[1]):
        term = d[t[:, k].clamp_min(0)] * w[k]
        term = torch.where(live[:, k:k + 1], term, torch.zeros_like(term))
        out += term
        S += term.abs()
    if add is not None:
        out += add.double()
        S += add.double().abs()
    return out, S, live.sum(1, keepdim=True)


def dwconv_transpose_ref(grad, weight, table, n_src):
    """d/d data of dwconv: ddata[n, c] = sum over (h, k) with t[h, k] = n of w[k, c] grad[h, c]  ->  (ddata, S, T (n_src, 1))"""
    t, live = _taps(table)
    g, w = grad.double(), weight.double().reshape(t.shape[1], -1)
    out = torch.zeros(n_src, g.shape[1], dtype=torch.float64)
    S = torch.zeros_like(out)
    T = torch.zeros(n_src, 1, dtype=torch.int64)
    for k in range(t.shape[1]):
        rows = live[:, k].nonzero().flatten()
        term = g[rows] * w[k]
        out.index_add_(0, t[rows, k], term)
        S.index_add_(0, t[rows, k], term.abs())
        T.index_add_(0, t[rows, k], torch.ones(rows.numel(), 1, dtype=torch.int64))
    return out, S, T


def wgrad_ref(grad, data, table):
    """gW[k, 0, c] = sum_h [t[h, k] >= 0] data[t[h, k], c] grad[h, c]  ->  (gW (K, 1, C), S, live rows per tap (K, 1, 1))"""
    t, live = _taps(table)
    d, g = data.double(), grad.double()
    K = t.shape[1]
    out = torch.zeros(K, 1, d.shape[1], dtype=torch.float64)
    S = torch.zeros_like(out)
    for k in range(K):
        rows = live[:, k].nonzero().flatten()
        term = d[t[rows, k]] * g[rows]
        out[k, 0] = term.sum(0)
        S[k, 0] = term.abs().sum(0)
    return out, S, live.sum(0).reshape(K, 1, 1)


def wgrad_slabs(n_rows, C, K, cus):
    """partial slabs the depth-wise weight gradient adds per element (launch_wgrad / wgrad_blocks of csrc/dwconv.hip): one per
    workgroup, whole groups of eight; the scalar kernel has none"""
    if C % 4 != 0 or C > 1024 or K > 27:
        return 0
    rpb = max(1, min(16, 256 // (C // 4)))
    b = max(1, min(-(-n_rows // (8 * rpb)), 3 * cus))
    return (b + 7) // 8 * 8


def inverse_ref(table, n_src):
    """inv[t[h, k], k] = h, -1 elsewhere, (n_src, K), in the table's dtype"""
    t, live = _taps(table)
    inv = torch.full((n_src, t.shape[1]), -1, dtype=torch.int64)
    h, k = live.nonzero(as_tuple=True)
    inv[t[h, k], k] = h
    return inv.to(table.dtype)


def cpe_ref(x, weight, gamma, beta, table, residual, eps=1e-5):
    """[x +] LayerNorm(dwconv(x)) * gamma + beta over the channel axis (biased variance)  ->  (out, conv, S, T)"""
    conv, S, T = dwconv_ref(x, weight, table)
    mean = conv.mean(1, keepdim=True)
    var = ((conv - mean) ** 2).mean(1, keepdim=True)
    out = (conv - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    if residual:
        out = out + x.double()
    return out, conv, S, T


def slot_sum_ref(part, slot, bias=None):
    """out[h] = sum of part[slot[h, k]] over the live slots [+ bias]  ->  (out, S, T)"""
    K = slot.shape[1]
    out, S, T = dwconv_ref(part, torch.ones(K, 1, part.shape[1]), slot)
    if bias is not None:
        out = out + bias.double()
        S = S + bias.double().abs()
    return out, S, T


def gather_ref(data, table):
    """octree2col: col[m, k * C + c] = data[t[m, k], c], zero where there is no neighbour; in data's dtype (a copy: exact)"""
    t, live = _taps(table)
    col = data[t.clamp_min(0)]
    return torch.where(live.unsqueeze(-1), col, torch.zeros_like(col)).reshape(t.shape[0], -1)


def gather_transpose_ref(dcol, table, n_src):
    """ddata[n, c] = sum over (m, k) with t[m, k] = n of dcol[m, k * C + c], float64"""
    t, live = _taps(table)
    K = t.shape[1]
    d = dcol.double().reshape(t.shape[0], K, -1)
    out = torch.zeros(n_src, d.shape[2], dtype=torch.float64)
    for k in range(K):
        rows = live[:, k].nonzero().flatten()
        out.index_add_(0, t[rows, k], d[rows, k])
    return out


# ------------------------------------------------------------------------------------------------ tap_wgrad
TAP_PAIR_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4100)
# an empty tap first, last and between two full (2048-pair, one whole chunk) ones; 27 taps hold every count of the list
TAP_COUNTS = {
    8: (0, 2048, 0, 2048, 65, 2049, 4100, 0),
    27: (0, 1, 15, 16, 17, 63, 64, 65, 2047, 2048, 0, 2048, 2049, 4100, 1, 0, 15, 17, 65, 63, 16, 64, 2047, 1, 17, 65, 0),
}
TAP_CHUNK = 2048


def tap_tables(counts):
    """(edges (taps + 1) int64, chunks (n, 3) int32 {tap, begin, end}, tap_chunk_off (taps + 1) int32) for per-tap pair
    counts, cut by the product's own `_split_ranges` (the layout `Octree.sparse_taps_bwd` documents and the kernel reads)"""
    from hotformerloc_amd.octree import _split_ranges
    assert set(counts) <= set(TAP_PAIR_COUNTS)
    e = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    tap, a, rows = _split_ranges(e, TAP_CHUNK)
    chunks = np.stack([tap, a, a + rows], 1).astype(np.int32).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum((np.diff(e) + TAP_CHUNK - 1) // TAP_CHUNK)]).astype(np.int32)
    assert (rows >= 1).all() and (rows <= TAP_CHUNK).all() and off[-1] == len(chunks)
    return e, torch.from_numpy(chunks), torch.from_numpy(off)


def tap_wgrad_ref(g, dpart, edges):
    """dW[k] (cin, cout) = g_k^T dpart_k over the pairs [edges[k], edges[k + 1]) of pair-major g (P, cin), dpart (P, cout)
    ->  (dW, S); inf and NaN propagate as IEEE arithmetic has them (numpy warnings silenced)"""
    taps = len(edges) - 1
    dw = torch.zeros(taps, g.shape[1], dpart.shape[1], dtype=torch.float64)
    S = torch.zeros_like(dw)
    for k in range(taps):
        a, b = g[edges[k]:edges[k + 1]].double(), dpart[edges[k]:edges[k + 1]].double()
        if a.shape[0]:
            dw[k] = torch.einsum('pi,pj->ij', a, b)
            S[k] = torch.einsum('pi,pj->ij', a.abs(), b.abs())
    return dw, S


def tap_terms(counts):
    """T of the bound per tap: its pairs plus its chunks, (taps, 1, 1)"""
    c = np.asarray(counts, dtype=np.int64)
    return torch.from_numpy(c + (c + TAP_CHUNK - 1) // TAP_CHUNK).reshape(-1, 1, 1)


def seq32(terms):
    """the same sum evaluated sequentially in fp32 on the CPU: terms (T, ...) f32 -> their running sum in storage order"""
    acc = torch.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc
