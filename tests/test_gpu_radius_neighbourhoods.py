"""Radius and hybrid neighbourhoods on the device (`hfl_knn_normals_radius`, `hfl_fpfh_radius_capped`, `hfl_knn_radius_count`,
`hfl_count_mask`) against the numpy routes of `normals.py`, `fpfh.py` and `outliers.py` with the same `radius=`.

Comparison rules: those of `tests/test_gpu_normals.py` and `tests/test_gpu_fpfh.py`, unchanged.  counts, the set of zero
normals, hist, pairs, the radius counts and the masks: EQUAL.  Normals within 2e-7 absolute per component and curvature
within 1e-6 relative + 1e-12 where the host's eigenvalues have (l1 - l0) / l2 > 1e-6, which leaves out at most 1 % of a
case (asserted).  FPFH within one fp32 ulp."""
import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native, fpfh, normals, outliers
from hotformerloc_amd import registration as reg
from tests import fpfh_cases as fc
from tests import normals_cases as nc
from tests import radius_cases as rc

pytestmark = pytest.mark.gpu

VIEW = np.array(fc.VIEW)
# `global_registration_host(nb_neighbors=None, normal_radius=1.7, feature_radius=1.7)` on the density case's first seeds ends
# 0.0932 degrees and 0.00687 m from the truth (the two clouds are independent samples with 0.02 m of noise); the device may
# take twice that, the rule of `tests/test_gpu_global_registration.py`
CHAIN_BOUNDS = (2 * 0.0932, 2 * 0.00687)


def within_one_ulp(device, host):
    d, h = device.astype(np.float64), host.astype(np.float64)
    return bool(np.all(np.abs(d - h) <= np.spacing(np.maximum(np.abs(device), np.abs(host)))))


def run_normals(keys, mode, nb=30, radius=None, **kw):
    r = rc.radius_of(keys[0]) if radius is None else radius
    return normals.estimate_normals([rc.cloud_of(k) for k in keys], rc.nb_of(mode, nb), radius=r, viewpoint=VIEW,
                                    return_curvature=True, return_counts=True, **kw)


def check_normals(out, keys, mode, nb=30, radius=None):
    nrm, curv, counts = out[:3]
    for i, key in enumerate(keys):
        h_nrm, h_curv, h_counts, h_lam = rc.host_normals(key, mode, nb, radius)
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
            print('%s %s nb=%d: normals %.3g, curvature excess %.3g, compared %d of %d' % (key, mode, nb, err_n, err_c,
                                                                                          sure.sum(), len(sure)))
            assert err_n <= 2e-7, key
            assert err_c <= 1e-12, key


def run_fpfh(keys, mode, nb=30, radius=None, **kw):
    r = rc.radius_of(keys[0]) if radius is None else radius
    out = fpfh.compute_fpfh([rc.cloud_of(k) for k in keys], [rc.host_normals(k, mode, nb, radius)[0] for k in keys],
                            rc.nb_of(mode, nb), radius=r, return_histograms=True, return_pending=True, **kw)
    return [[t.cpu().numpy() for t in part] for part in out[:3]] + [out[3]]


def check_fpfh(out, keys, mode, nb=30, radius=None):
    feat, hist, pairs, _ = out
    for i, key in enumerate(keys):
        h_feat, h_hist, h_pairs = rc.host_fpfh(key, mode, nb, radius)
        assert feat[i].dtype == np.float32 and hist[i].dtype == np.int32 and pairs[i].dtype == np.int32
        assert feat[i].shape == h_feat.shape
        assert np.array_equal(hist[i], h_hist), key
        assert np.array_equal(pairs[i], h_pairs), key
        assert within_one_ulp(feat[i], h_feat), key


def check_counts(keys, radius, nb_points=4, **kw):
    clouds = [rc.cloud_of(k) for k in keys]
    counts, pending = outliers.radius_neighbour_counts(clouds, radius, return_pending=True, **kw)
    kept, masks = outliers.remove_radius_outliers(clouds, nb_points, radius, return_mask=True, **kw)
    h_counts = outliers.radius_neighbour_counts_host(clouds, radius)
    h_kept, h_masks = outliers.remove_radius_outliers_host(clouds, nb_points, radius, return_mask=True)
    for i, key in enumerate(keys):
        assert counts[i].dtype == torch.int32 and masks[i].dtype == torch.bool and kept[i].dtype == torch.float32
        assert np.array_equal(counts[i].cpu().numpy(), h_counts[i]), key
        assert np.array_equal(masks[i].cpu().numpy(), h_masks[i]), key
        assert np.array_equal(kept[i].cpu().numpy().view(np.int32), h_kept[i].view(np.int32)), key
    return pending, [c.cpu().numpy() for c in counts]


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('n', [255, 256, 257, 1, 2, 3, 5])
def test_sizes_at_the_launch_boundaries_and_below_k(n, mode):
    check_normals(run_normals([n], mode), [n], mode)
    check_fpfh(run_fpfh([n], mode), [n], mode)
    if mode == 'radius_only':
        check_counts([n], rc.radius_of(n))


# ------------------------------------------------------------------------------------------------ list lengths
@pytest.mark.parametrize('nb', [3, 8, 9, 16, 17, 32])
def test_every_list_length_with_points_capped_by_k_and_points_capped_by_the_radius(nb):
    keys = ['planes700']
    out = run_normals(keys, 'hybrid', nb)
    check_normals(out, keys, 'hybrid', nb)
    check_fpfh(run_fpfh(keys, 'hybrid', nb), keys, 'hybrid', nb)
    ball = outliers.radius_neighbour_counts([rc.cloud_of('planes700')], rc.radius_of('planes700'))[0].cpu().numpy()
    counts = out[2][0].cpu().numpy()
    by_k, by_radius = ball > nb, ball < nb                            # the k-th neighbour inside the ball; the ball short of k
    assert by_k.any() and by_radius.any()
    assert (counts[by_k] >= nb).all() and (counts[by_k] < ball[by_k]).all() and np.array_equal(counts[by_radius], ball[by_radius])


# ------------------------------------------------------------------------------------------------ one ragged call
@pytest.mark.parametrize('mode', rc.MODES)
def test_ragged_batch_in_one_call(mode):
    keys, radius = [1, 'planes', 5, 'planes700', 257, 'collinear', 2, 'duplicated'], 2.0
    check_normals(run_normals(keys, mode, radius=radius), keys, mode, radius=radius)
    check_fpfh(run_fpfh(keys, mode, radius=radius), keys, mode, radius=radius)
    if mode == 'radius_only':
        check_counts(keys, radius)


# ------------------------------------------------------------------------------------------------ the grid decides nothing
@pytest.mark.parametrize('mode', rc.MODES)
def test_cell_size_extremes_agree(mode):
    keys, radius = ['planes', 'planes700'], 2.0
    quarter = run_normals(keys, mode, radius=radius, cell_size=radius / 4, return_pending=True)
    one_cell = run_normals(keys, mode, radius=radius, cell_size=1e4, return_pending=True)
    default = run_normals(keys, mode, radius=radius, return_pending=True)
    assert quarter[3] > 0 and one_cell[3] == 0
    if mode == 'radius_only':
        assert default[3] == 0
    for out in (quarter, one_cell, default):
        check_normals(out, keys, mode, radius=radius)
    f_quarter = run_fpfh(keys, mode, radius=radius, cell_size=radius / 4)
    f_one_cell = run_fpfh(keys, mode, radius=radius, cell_size=1e4)
    f_default = run_fpfh(keys, mode, radius=radius)
    assert f_quarter[3] > 0 and f_one_cell[3] == 0
    if mode == 'radius_only':
        assert f_default[3] == 0
    for out in (f_quarter, f_one_cell, f_default):
        check_fpfh(out, keys, mode, radius=radius)
    for a, b, c in zip(f_quarter[0], f_one_cell[0], f_default[0]):
        assert within_one_ulp(a, b) and within_one_ulp(a, c)
    if mode == 'radius_only':
        assert check_counts(keys, radius, cell_size=radius / 4)[0] > 0
        assert check_counts(keys, radius, cell_size=1e4)[0] == 0
        assert check_counts(keys, radius)[0] == 0


def test_default_cell_leaves_no_point_pending_for_radius_only():
    """what `outliers.radius_cell` promises, on clouds of every shape here and radii from a tenth of the spacing to the
    cloud's size, the budget doubling included ('planes700' spans 800 m)"""
    keys = ['plane37', 'planes', 'planes700', 'duplicated', 'collinear', 257, 1]
    for radius in (0.03, 0.35, 1.7, 8.0):
        assert check_counts(keys, radius)[0] == 0
        assert run_normals(keys, 'radius_only', radius=radius, return_pending=True)[3] == 0
        nrms = [np.tile(np.float32([0, 0, 1]), (len(rc.cloud_of(k)), 1)) for k in keys]
        assert fpfh.compute_fpfh([rc.cloud_of(k) for k in keys], nrms, None, radius=radius, return_pending=True)[1] == 0


def test_far_points_by_the_block_scan_and_by_the_whole_cloud_scan():
    """The cloud spans 800 m, so the cell-table budget doubles a cell of 0.25 m to 4 m.  Alone in a block of 4 m cells a far
    point is still proven complete within 2 m -- the cap at work: the faces of its block are 4 m to 6 m away -- so the radius
    here is 6.5 m: then no block proves a ball complete, and the whole-cloud scan finishes every point of the radius-only
    search and, of the hybrid one, the far points (a plane point's 30th neighbour lies well inside its block).  The radius
    cell of 6.5 m fits the budget as it is."""
    keys, radius = ['planes700'], 6.5
    for mode in rc.MODES:
        for cell in (None, 0.25):
            out = run_normals(keys, mode, radius=radius, cell_size=cell, return_pending=True)
            if cell is not None:
                assert out[3] == (20 if mode == 'hybrid' else 700)
            elif mode == 'radius_only':
                assert out[3] == 0
            check_normals(out, keys, mode, radius=radius)
            assert (out[2][0][-20:] == 1).all() and not out[0][0][-20:].any()
            f_out = run_fpfh(keys, mode, radius=radius, cell_size=cell)
            assert f_out[3] == out[3]
            check_fpfh(f_out, keys, mode, radius=radius)
            assert not f_out[2][0][-20:].any() and not f_out[0][0][-20:].any()
    for cell in (None, 0.25):
        pending, counts = check_counts(keys, radius, nb_points=1, cell_size=cell)
        assert (counts[0][-20:] == 1).all() and pending == (700 if cell else 0)
    assert outliers.remove_radius_outliers([rc.cloud_of('planes700')], 1, radius)[0].shape[0] == 680


# ------------------------------------------------------------------------------------------------ ties and duplicates
@pytest.mark.parametrize('radius, interior', zip(rc.LATTICE_RADII, rc.LATTICE_INTERIOR))
def test_lattice_boundary_is_inclusive(radius, interior):
    cloud, nrm = fc.lattice()
    want = rc.lattice_counts(radius)
    assert want[62] == interior
    for cell in (None, 0.75):
        counts = outliers.radius_neighbour_counts([cloud], radius, cell_size=cell)[0].cpu().numpy()
        assert np.array_equal(counts, want)
        for nb in (None, 9):
            n_out = normals.estimate_normals([cloud], nb, radius=radius, cell_size=cell, return_counts=True)
            h_out = normals.estimate_normals_host([cloud], nb, radius=radius, return_counts=True)
            assert np.array_equal(n_out[1][0].cpu().numpy(), h_out[1][0])
            assert np.array_equal((n_out[0][0].cpu().numpy() != 0).any(1), (h_out[0][0] != 0).any(1))
            feat, hist, pairs = fpfh.compute_fpfh([cloud], [nrm], nb, radius=radius, cell_size=cell, return_histograms=True)
            h_feat, h_hist, h_pairs = fpfh.compute_fpfh_host([cloud], [nrm], nb, radius=radius, return_histograms=True)
            assert np.array_equal(hist[0].cpu().numpy(), h_hist[0]) and np.array_equal(pairs[0].cpu().numpy(), h_pairs[0])
            assert within_one_ulp(feat[0].cpu().numpy(), h_feat[0])
        assert np.array_equal(normals.estimate_normals([cloud], None, radius=radius, cell_size=cell,
                                                       return_counts=True)[1][0].cpu().numpy(), want)


@pytest.mark.parametrize('mode', rc.MODES)
def test_duplicates(mode):
    keys = ['duplicated']
    out = run_normals(keys, mode)
    check_normals(out, keys, mode)
    check_fpfh(run_fpfh(keys, mode), keys, mode)
    assert (out[2][0][-20:-8] >= 13).all()                            # the 13 coincident copies see one another
    pending, counts = check_counts(keys, 1e-3, nb_points=12)          # nothing but the copies within a millimetre
    assert sorted(np.unique(counts[0]).tolist()) == [1, 3, 13]


# ------------------------------------------------------------------------------------------------ unchanged bits
def test_hybrid_with_a_huge_radius_is_the_k_nearest_call_bit_for_bit():
    keys = ['planes700', 'duplicated', 257, 2]
    clouds = [rc.cloud_of(k) for k in keys]
    for nb, cell in ((30, None), (8, 0.25), (16, None)):
        kw = dict(viewpoint=VIEW, cell_size=cell, return_curvature=True, return_counts=True, return_pending=True)
        plain, capped = normals.estimate_normals(clouds, nb, **kw), normals.estimate_normals(clouds, nb, radius=1e30, **kw)
        assert plain[3] == capped[3]
        for a, b in zip(plain[:3], capped[:3]):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        kw = dict(cell_size=cell, return_histograms=True, return_pending=True)
        f_plain = fpfh.compute_fpfh(clouds, plain[0], nb, **kw)
        f_capped = fpfh.compute_fpfh(clouds, plain[0], nb, radius=1e30, **kw)
        assert f_plain[3] == f_capped[3]
        for a, b in zip(f_plain[:3], f_capped[:3]):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize('mode', rc.MODES)
def test_two_runs_give_the_same_bits(mode):
    keys, radius = ['planes700', 'duplicated', 'collinear'], 2.0
    for cell in (None, 0.5):
        first, second = (run_normals(keys, mode, radius=radius, cell_size=cell) for _ in range(2))
        for a, b in zip(first, second):
            for x, y in zip(a, b):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        first, second = (run_fpfh(keys, mode, radius=radius, cell_size=cell) for _ in range(2))
        for a, b in zip(first[:3], second[:3]):
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.int32), y.view(np.int32))
        assert first[3] == second[3]


# ------------------------------------------------------------------------------------------------ refusals
def test_device_tensors_go_in_and_cpu_device_is_refused():
    cloud, nrm = rc.cloud_of(257), rc.host_normals(257, 'radius_only')[0]
    for call in (lambda c: normals.estimate_normals([c], None, radius=1.5, device='cpu'),
                 lambda c: fpfh.compute_fpfh([c], [nrm], None, radius=1.5, device='cpu'),
                 lambda c: outliers.radius_neighbour_counts([c], 1.5, device='cpu'),
                 lambda c: outliers.remove_radius_outliers([c], 2, 1.5, device='cpu')):
        with pytest.raises(_native.NativeLibraryError):
            call(cloud)
        with pytest.raises(_native.NativeLibraryError):
            call(torch.from_numpy(np.array(cloud)))
    on_device = torch.from_numpy(np.array(cloud)).cuda()
    out = normals.estimate_normals([on_device], None, radius=1.5, viewpoint=VIEW, return_curvature=True, return_counts=True)
    check_normals(out, [257], 'radius_only')
    counts = outliers.radius_neighbour_counts([on_device], 1.5)[0]
    assert counts.is_cuda and torch.equal(counts, out[2][0])
    assert outliers.radius_neighbour_counts([], 1.0) == []
    assert outliers.remove_radius_outliers([], 2, 1.0, return_mask=True) == ([], [])
    assert outliers.radius_neighbour_counts([], 1.0, return_pending=True) == ([], 0)


# ------------------------------------------------------------------------------------------------ the chain
def test_chain_on_the_density_case():
    src, dst, truth = rc.density_pair(rc.DENSITY_SEEDS[0])
    on = [torch.from_numpy(np.array(src)).cuda()], [torch.from_numpy(np.array(dst)).cuda()]
    coarse, fine = hfl.global_registration(*on, nb_neighbors=None, normal_radius=rc.DENSITY_RADIUS,
                                           feature_radius=rc.DENSITY_RADIUS)
    angle, shift = rc.density_errors(fine.transforms[0], truth)
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m'
          % (rc.density_errors(coarse.transforms[0], truth) + (angle, shift)))
    assert fine.status.tolist() == [reg.CONVERGED]
    assert angle <= CHAIN_BOUNDS[0] and shift <= CHAIN_BOUNDS[1]
