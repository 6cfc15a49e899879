"""`hfl_pairwise_dist` / `hfl_pairwise_dist_bwd` (hotformerloc_amd/csrc/pairwise.hip) against float64 `torch.cdist` in its
direct-difference mode and float64 autograd through it, at every tile shape the kernels distinguish: one row, less than a
tile, exact tiles, a one-row tile tail, several tiles, a D that is no multiple of 4 (scalar loads), B and D tails together."""
import numpy as np
import pytest
import torch

import loss_cases as lc
from hotformerloc_amd import ops
from hotformerloc_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (20, 64), (64, 256), (65, 72), (96, 128), (130, 7), (257, 256)]
KINDS = ['unit', 'scaled', 'duplicate']
U = 2.0 ** -24
_CACHE = {}


def rows(batch, dim, kind):
    """`make_case` rows (unit norm, clustered in groups of 4); 'scaled': every row times a factor in 1..50; 'duplicate':
    row 9 is a copy of row 3."""
    e = lc.make_case(100 + batch, batch, dim, 4, 0)[0].copy()
    if kind == 'scaled':
        e *= (1.0 + 49.0 * syn.hash_uniform(7 + batch, batch)).astype(np.float32)[:, None]
    if kind == 'duplicate':
        e[9] = e[3]
    return e


def reference(batch, dim, kind):
    """(e, g, d64, dE64, bound sum) once per case: float64 cdist without the matrix product, autograd through it for a
    random non-symmetric g, and sum_j |g_ij + g_ji| |e_ik - e_jk| / d_ij for the backward's bound."""
    key = (batch, dim, kind)
    if key not in _CACHE:
        e = rows(batch, dim, kind)
        g = (syn.hash_uniform(900 + batch, batch * batch).reshape(batch, batch) - 0.5).astype(np.float32)
        x = torch.from_numpy(e).double().requires_grad_()
        d = torch.cdist(x, x, p=2, compute_mode='donot_use_mm_for_euclid_dist')
        g64 = torch.from_numpy(g).double()
        d.backward(g64)
        d = d.detach()
        w = torch.where(d > 0, (g64 + g64.t()).abs() / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
        xd = x.detach()
        mag = torch.cat([(w[i:i + 32, :, None] * (xd[i:i + 32, None, :] - xd[None, :, :]).abs()).sum(1)
                         for i in range(0, batch, 32)], 0)
        _CACHE[key] = (e, g, d.numpy(), x.grad.numpy(), mag.numpy())
    return _CACHE[key]


def cases():
    return [pytest.param(b, d, k, id='b%d_d%d_%s' % (b, d, k)) for b, d in SHAPES for k in KINDS
            if not (k == 'duplicate' and b < 10)]


@pytest.mark.parametrize('batch,dim,kind', cases())
def test_pairwise_dist_forward(batch, dim, kind):
    e, _, d64, _, _ = reference(batch, dim, kind)
    dist = ops.pairwise_dist(torch.from_numpy(e).cuda())
    assert dist.shape == (batch, batch) and dist.dtype == torch.float32
    got = dist.cpu().numpy()
    # a sum of D non-negative terms, each the square of a rounded difference, under a square root
    excess = np.abs(got.astype(np.float64) - d64) - (dim / 2 + 2) * U * d64
    print('forward worst |d - d64| / d64 in units of 2^-24:',
          (np.abs(got - d64)[d64 > 0] / d64[d64 > 0]).max() / U if (d64 > 0).any() else 0.0, 'allowed', dim / 2 + 2)
    assert excess.max() <= 0.0
    assert (np.diagonal(got) == 0.0).all()
    assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32))               # bitwise symmetric
    if kind == 'duplicate':
        assert got[3, 9] == 0.0 and got[9, 3] == 0.0


@pytest.mark.parametrize('batch,dim,kind', cases())
def test_pairwise_dist_backward(batch, dim, kind):
    e, g, _, de64, mag = reference(batch, dim, kind)
    emb, grad = torch.from_numpy(e).cuda(), torch.from_numpy(g).cuda()
    dist = ops.pairwise_dist(emb)
    de = ops.pairwise_dist_bwd(grad, dist, emb)
    again = ops.pairwise_dist_bwd(grad, dist, emb)
    assert de.shape == (batch, dim) and de.dtype == torch.float32
    got = de.cpu().numpy()
    assert np.isfinite(got).all()
    # B accumulations, the distance's own (D/2 + 2), the sum g_ij + g_ji, the division, the difference, the product
    bound = (batch + dim / 2 + 8) * U * mag
    err = np.abs(got.astype(np.float64) - de64)
    print('backward worst error / bound:', (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
    assert (err <= bound).all()
    assert torch.equal(de, again) and np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))
    if kind == 'duplicate':
        # the coincident pair contributes nothing: the same rows with grad_dist[3, 9] and [9, 3] changed give the same bits
        grad2 = grad.clone()
        grad2[3, 9] += 5.0
        grad2[9, 3] -= 3.0
        assert torch.equal(ops.pairwise_dist_bwd(grad2, dist, emb), de)


def test_pairwise_wrappers_reject_bad_arguments():
    from hotformerloc_amd._native import NativeLibraryError
    with pytest.raises(NativeLibraryError):
        ops.pairwise_dist(torch.zeros(4, 8))
    with pytest.raises(NativeLibraryError):
        ops.pairwise_dist_bwd(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 8))
    emb = torch.zeros(4, 8, device='cuda')
    with pytest.raises(ValueError):
        ops.pairwise_dist(torch.zeros(4, device='cuda'))
    with pytest.raises(ValueError):
        ops.pairwise_dist(torch.zeros(0, 8, device='cuda'))
    with pytest.raises(ValueError):
        ops.pairwise_dist_bwd(torch.zeros(4, 5, device='cuda'), torch.zeros(4, 4, device='cuda'), emb)
    with pytest.raises(ValueError):
        ops.pairwise_dist_bwd(torch.zeros(4, 4, device='cuda'), torch.zeros(5, 5, device='cuda'), emb)
    with pytest.raises(TypeError):
        ops.pairwise_dist(emb.double())


def test_pairwise_launchers_return_einval_on_non_positive_sizes():
    from hotformerloc_amd import _native
    lib, buf = _native.load(), torch.zeros(64, device='cuda')
    p = buf.data_ptr()
    for b, d in [(0, 8), (-1, 8), (4, 0), (4, -3)]:
        assert lib.hfl_pairwise_dist(p, p, b, d, ops._stream()) == -1
        assert lib.hfl_pairwise_dist_bwd(p, p, p, p, b, d, ops._stream()) == -1
    torch.cuda.synchronize()
    assert (buf == 0).all()
