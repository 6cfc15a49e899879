"""Normal estimation on the device (`csrc/normals.hip`, `hotformerloc_amd/normals.py`) against the numpy route of the same
module.

Comparison rule.  counts: EQUAL, and the set of zero normals EQUAL -- the neighbourhood is a pure function of the input.
Where the host's eigenvalues have (l1 - l0) / l2 > 1e-6: normals within 2e-7 absolute per component (two fp32 ulps at 1) and
curvature within 1e-6 relative + 1e-12; the float64 sums are taken in another order, a difference of about 1e-15 that such
a gap amplifies by at most 1e6, far below one fp32 ulp.  The points that gap rule leaves out are at most 1 % of a case,
which is asserted; on the clouds used here it leaves out none."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import _native, normals
from tests import normals_cases as nc

pytestmark = pytest.mark.gpu

CLOUDS = {
    'plane1500': lambda: nc.noisy_plane(1500, 1),
    'plane_offset': lambda: nc.noisy_plane(900, 2, offset=(100.0, -80.0, 30.0)),
    'sphere': nc.sphere_shell,
    'forest': nc.forest,
    'tie_lattice': nc.tie_lattice,
    'duplicated': nc.duplicated,
    'plane_and_far': nc.plane_and_far,
    'collinear': nc.collinear,
}


@functools.lru_cache(maxsize=None)
def cloud_of(key):
    return nc.noisy_plane(key, 100 + key) if isinstance(key, int) else CLOUDS[key]()


@functools.lru_cache(maxsize=None)
def host(key, nb=30, view=None):
    """the numpy route, computed once per (cloud, nb, viewpoint) and shared: (normals, curvature, counts, eigenvalues)"""
    out = normals.estimate_normals_host([cloud_of(key)], nb, viewpoint=None if view is None else np.array(view),
                                        return_curvature=True, return_counts=True, return_eigenvalues=True)
    return tuple(o[0] for o in out)


def check(device_out, keys, nb=30, views=None):
    nrm, curv, counts = device_out[:3]
    for i, key in enumerate(keys):
        h_nrm, h_curv, h_counts, h_lam = host(key, nb, None if views is None else tuple(views[i]))
        assert nrm[i].dtype == torch.float32 and curv[i].dtype == torch.float32 and counts[i].dtype == torch.int32
        d_nrm, d_curv, d_counts = nrm[i].cpu().numpy(), curv[i].cpu().numpy(), counts[i].cpu().numpy()
        assert d_nrm.shape == h_nrm.shape and d_curv.shape == h_curv.shape
        assert np.array_equal(d_counts, h_counts), key
        assert np.array_equal((d_nrm != 0).any(1), (h_nrm != 0).any(1)), key
        assert not d_curv[~(h_nrm != 0).any(1)].any(), key
        share, sure = nc.undetermined_share(h_nrm, h_lam)
        assert share <= nc.MAX_SHARE, (key, share)
        if sure.any():
            err_n = np.abs(d_nrm[sure].astype(np.float64) - h_nrm[sure]).max()
            err_c = (np.abs(d_curv[sure].astype(np.float64) - h_curv[sure]) - 1e-6 * np.abs(h_curv[sure])).max()
            print('%s nb=%d: normals %.3g, curvature excess %.3g, compared %d of %d' % (key, nb, err_n, err_c, sure.sum(),
                                                                                       len(sure)))
            assert err_n <= 2e-7, key
            assert err_c <= 1e-12, key


def run(keys, nb=30, **kw):
    return normals.estimate_normals([cloud_of(k) for k in keys], nb, return_curvature=True, return_counts=True, **kw)


@pytest.mark.parametrize('n', [255, 256, 257, 1, 2, 3, 5])
def test_sizes_at_the_launch_boundaries_and_below_k(n):
    check(run([n]), [n])


@pytest.mark.parametrize('nb', [3, 8, 9, 16, 17, 30, 32])
def test_every_template_bucket_and_its_edges(nb):
    check(run(['plane1500'], nb), ['plane1500'], nb)


def test_ragged_batch_in_one_call():
    keys = [1, 'sphere', 5, 'forest', 257, 'collinear', 2]
    check(run(keys), keys)


def test_cell_size_extremes_agree():
    keys = ['forest', 'plane_offset']
    total = sum(len(cloud_of(k)) for k in keys)
    one_cell = run(keys, cell_size=1e4, return_pending=True)             # brute force in the query kernel
    all_pending = run(keys, cell_size=1e-3, return_pending=True)         # the whole-cloud scan does everything
    default = run(keys, return_pending=True)
    assert one_cell[3] == 0 and all_pending[3] == total and 0 <= default[3] < total
    for out in (one_cell, all_pending, default):
        check(out, keys)
    for i in range(len(keys)):
        assert torch.equal(one_cell[2][i], all_pending[2][i]) and torch.equal(one_cell[2][i], default[2][i])


@pytest.mark.parametrize('key', ['tie_lattice', 'duplicated'])
def test_ties_and_duplicates(key):
    out = run([key])
    check(out, [key])
    counts = out[2][0].cpu().numpy()
    assert (counts > 30).any()
    if key == 'duplicated':                                              # 41 coincident copies: no normal there
        assert not out[0][0][0].any() and not out[0][0][-50:-10].any()


def test_isolated_far_point_is_finished_by_the_whole_cloud_scan():
    out = run(['plane_and_far'], return_pending=True)
    assert out[3] >= 1
    check(out, ['plane_and_far'])
    assert out[0][0][-1].any()                                           # its 30 neighbours lie on the plane: a normal


def test_viewpoints_per_cloud_and_one_for_all():
    keys = ['sphere', 'plane1500']
    views = [(3.0, -2.0, 1.0), (0.0, 0.0, -40.0)]                        # the sphere's centre: inward normals; below the plane
    out = run(keys, viewpoint=np.array(views))
    check(out, keys, views=views)
    assert (out[0][1][:, 2] < 0).all()
    one = run(keys, viewpoint=torch.tensor(views[0], dtype=torch.float64))
    check(one, keys, views=[views[0], views[0]])


def test_two_runs_give_the_same_bits():
    keys = ['forest', 'duplicated', 'plane_and_far']
    first, second = run(keys), run(keys)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_device_tensors_go_in_and_cpu_device_is_refused():
    cloud = cloud_of(257)
    with pytest.raises(_native.NativeLibraryError):
        normals.estimate_normals([cloud], device='cpu')
    with pytest.raises(_native.NativeLibraryError):
        normals.estimate_normals([torch.from_numpy(cloud)], device='cpu')
    on_device = normals.estimate_normals([torch.from_numpy(cloud).cuda()], return_curvature=True, return_counts=True)
    check(on_device, [257])
    assert normals.estimate_normals([]) == [] and normals.estimate_normals([], return_counts=True) == ([], [])
