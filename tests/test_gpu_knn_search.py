"""The one grid k-NN search of `csrc/knn_common.h` under its three consumers -- the mean neighbour distance
(`ops.knn_mean_dist`), the normals (`ops.knn_normals`) and the FPFH radius (`ops.fpfh_radius`): on the same sorted batch they
make the same decisions.  The pending counters and the sets of pending points are equal, the block proves exactly the points
that are not pending, the normals' neighbourhood is { d2 <= r2 } of the FPFH radius, and r2 does not depend on the grid.

The batch: `plane_and_far` (its isolated point is alone in its 3 x 3 x 3 block, so its k-th distance there is +inf for every
k >= 2 and at least one point is pending at any cell size), a noisy plane of 257 points, and a cloud of 5 points, fewer than
any nb here.  nb 8 and 9 lie on the two sides of a list length of the kernels, 32 is the largest.  At a cell of 1 mm no
block holds a point's neighbours and every point goes to the whole-cloud scan."""
import functools

import pytest
import torch

from hotformerloc_amd import normals, ops, outliers, ragged
from tests import normals_cases as nc

pytestmark = pytest.mark.gpu

NBS = (8, 9, 32)
SMALL_CELL = 1e-3


@functools.lru_cache(maxsize=None)
def clouds():
    plane = nc.noisy_plane(257, 357)
    return (nc.plane_and_far(), plane, plane[:5].copy())


def pending_set(ws, counter):
    return torch.sort(ws.pending[:int(counter.item())]).values


@functools.lru_cache(maxsize=None)
def search(nb, cell):
    """the three consumers on one sorted batch, run once per (nb, cell) and shared; nothing in it is changed afterwards"""
    with ragged.intake(list(clouds()), 'cuda') as packed:
        table, spts, skeys, perm = outliers.sorted_batch(packed, nb, cell)
        n, dev = int(spts.shape[0]), spts.device
        ws_avg, ws_nrm = ops.KnnWorkspace(n, table.cells, dev), ops.KnnWorkspace(n, table.cells, dev)
        ws = ops.FpfhWorkspace(n, table.cells, dev)
        _, c_avg = ops.knn_mean_dist(spts, skeys, perm, packed.off, table, workspace=ws_avg)
        _, _, counts, c_nrm = ops.knn_normals(spts, skeys, perm, packed.off, table, workspace=ws_nrm)
        c_rad = ops.fpfh_radius(ws, spts, skeys, packed.off, table)
        r2 = torch.empty_like(ws.r2)
        r2[perm] = ws.r2                                         # back to input order
        return dict(n=n, pts=packed.pts.clone(), off=packed.off_host.tolist(), counts=counts, r2=r2,
                    proven=int(ws.proven.sum().item()),
                    counters=[int(c.item()) for c in (c_avg, c_nrm, c_rad)],
                    pending=[pending_set(w, c) for w, c in ((ws_avg, c_avg), (ws_nrm, c_nrm), (ws, c_rad))])


@pytest.mark.parametrize('cell', (None, SMALL_CELL))
@pytest.mark.parametrize('nb', NBS)
def test_pending_counters_and_lists_agree(nb, cell):
    s = search(nb, cell)
    print('nb=%d cell=%s: pending %s of %d, proven %d' % (nb, cell, s['counters'], s['n'], s['proven']))
    assert s['counters'][0] == s['counters'][1] == s['counters'][2]
    if cell is None:
        assert s['counters'][0] >= 1
    else:
        assert s['counters'][0] == s['n']
    assert s['proven'] == s['n'] - s['counters'][0]
    assert torch.equal(s['pending'][0], s['pending'][1]) and torch.equal(s['pending'][0], s['pending'][2])


@pytest.mark.parametrize('cell', (None, SMALL_CELL))
@pytest.mark.parametrize('nb', NBS)
def test_normals_counts_are_the_points_within_r2(nb, cell):
    s = search(nb, cell)
    want = torch.empty_like(s['counts'])
    for b in range(len(s['off']) - 1):
        p = s['pts'][s['off'][b]:s['off'][b + 1]]
        d = p[:, None, :] - p[None, :, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz                       # eager fp32: every operation rounded once
        want[s['off'][b]:s['off'][b + 1]] = (d2 <= s['r2'][s['off'][b]:s['off'][b + 1], None]).sum(1).to(torch.int32)
    assert torch.equal(s['counts'], want)
    by_module = normals.estimate_normals(list(clouds()), nb, cell_size=cell, return_counts=True)[1]
    assert torch.equal(torch.cat(by_module), s['counts'])


@pytest.mark.parametrize('nb', NBS)
def test_r2_does_not_depend_on_the_cell_size(nb):
    assert torch.equal(search(nb, None)['r2'], search(nb, SMALL_CELL)['r2'])
