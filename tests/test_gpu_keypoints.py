"""ISS keypoints on the device (`hfl_iss_saliency`, `hfl_iss_select`) against the numpy routes of `keypoints.py`.

Comparison rules.  `iss_select`: the mask EQUALS `iss_select_host` on the same fp32 saliency, for any grid.  `iss_saliency`:
counts EQUAL; the zero pattern EQUAL, after `keypoint_cases.guard_gamma` has asserted on the host eigenvalues that no row
lies within 1e-9 relative of a gamma threshold (no row is left out); values within one fp32 spacing of the host value +
1e-12 x the host's l2 (the float64 sums run in another order, a Jacobi's error is about 1e-15 l2).  `iss_keypoints`: EQUAL to
`iss_select_host` of the device's own saliency, always; EQUAL to the full numpy route after `keypoint_cases.guard_ties`."""
import importlib

import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native
from tests import fpfh_cases as fc
from tests import global_registration_cases as gc
from tests import keypoint_cases as kc
from tests import spectral_cases as sc

pytestmark = pytest.mark.gpu

GR = importlib.import_module('hotformerloc_amd.global_registration')
RS, RN = kc.RADII[0]


def clouds_of(keys):
    return [kc.cloud_of(k) for k in keys]


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def check_saliency(out, keys, rs):
    """counts, zero pattern and values of a device saliency against the numpy route, the guard first"""
    sal, counts = out[:2]
    for i, key in enumerate(keys):
        h_sal, h_counts, _ = kc.host_saliency(key, rs)
        assert sal[i].dtype == torch.float32 and counts[i].dtype == torch.int32 and sal[i].is_cuda
        d_sal = sal[i].cpu().numpy()
        assert np.array_equal(counts[i].cpu().numpy(), h_counts), key
        if key not in kc.GUARDED:
            continue
        kc.guard_gamma(key, rs)
        assert np.array_equal(d_sal > 0, h_sal > 0), key
        excess = np.abs(d_sal.astype(np.float64) - h_sal.astype(np.float64)) - kc.value_bound(key, rs)
        if len(excess):
            print('%s at %g: largest |device - host| - bound = %.3g' % (key, rs, excess.max()))
        assert (excess <= 0).all(), key


def check_select(keys, saliencies, rn, **kw):
    """the device mask and index lists against `iss_select_host` on the same saliency -> the pending counter"""
    clouds = clouds_of(keys)
    masks, pending = hfl.iss_select(clouds, saliencies, rn, return_mask=True, return_pending=True, **kw)
    lists = hfl.iss_select(clouds, saliencies, rn, **kw)
    h_masks = hfl.iss_select_host(clouds, saliencies, rn, return_mask=True, min_neighbors=kw.get('min_neighbors', 5))
    for i, key in enumerate(keys):
        assert masks[i].dtype == torch.bool and lists[i].dtype == torch.int64 and lists[i].is_cuda
        assert np.array_equal(masks[i].cpu().numpy(), h_masks[i]), key
        assert np.array_equal(lists[i].cpu().numpy(), np.nonzero(h_masks[i])[0]), key
    return pending


def check_keypoints(keys, rs, rn, **kw):
    """`iss_keypoints` against `iss_select_host` of its own saliency, and against the numpy route under the guards"""
    clouds = clouds_of(keys)
    lists, sal, pending = hfl.iss_keypoints(clouds, rs, rn, return_saliency=True, return_pending=True, **kw)
    own = hfl.iss_select_host(clouds, host(sal), rn)
    for i, key in enumerate(keys):
        assert lists[i].dtype == torch.int64 and lists[i].is_cuda
        assert np.array_equal(lists[i].cpu().numpy(), own[i]), key
        if key in kc.GUARDED:
            kc.guard_gamma(key, rs)
            kc.guard_ties(key, rs, rn)
            assert np.array_equal(lists[i].cpu().numpy(), kc.host_keypoints(key, rs, rn)), key
    return lists, sal, pending


# ------------------------------------------------------------------------------------------------ sizes and named clouds
@pytest.mark.parametrize('key', kc.SIZES + kc.NAMED)
def test_every_size_and_named_cloud(key):
    check_saliency(hfl.iss_saliency([kc.cloud_of(key)], RS, return_counts=True), [key], RS)
    lists, sal, pending = check_keypoints([key], RS, RN)
    assert pending == 0                                               # the default cell leaves no point to the fallback
    if isinstance(key, int) and key < 5:
        assert lists[0].shape == (0,) and not sal[0].any()
    check_select([key], [kc.integer_saliency(key)], RN)


@pytest.mark.parametrize('radii', kc.RADII)
def test_ragged_batch_in_one_call(radii):
    keys = list(kc.RAGGED)
    check_saliency(hfl.iss_saliency(clouds_of(keys), radii[0], return_counts=True), keys, radii[0])
    lists, _, _ = check_keypoints(keys, *radii)
    assert lists[3].shape[0] == kc.PLANES_KEYPOINTS[radii]
    check_select(keys, [kc.integer_saliency(k) for k in keys], radii[1])


# ------------------------------------------------------------------------------------------------ the selection to the bit
@pytest.mark.parametrize('rn', [0.7, 1.0, 2.5])
def test_integer_saliency_the_index_rule_decides(rn):
    """ties everywhere; `non_max_radius` below and above the salient radius of the other tests; the fallback forced"""
    keys = ['planes', 'duplicated', 'collinear', 257, 'planes700', 2]
    sal = [kc.integer_saliency(k) for k in keys]
    assert check_select(keys, sal, rn) == 0
    assert check_select(keys, sal, rn, cell_size=rn / 4) > 0          # the whole-cloud scan has run, the mask is the same
    assert check_select(keys, sal, rn, cell_size=1e4) == 0
    assert check_select(keys, sal, rn, min_neighbors=1) == 0
    on_device = [torch.from_numpy(np.array(s)).cuda() for s in sal]
    assert check_select(keys, on_device, rn) == 0


def test_lattice_boundary_is_inclusive():
    cloud, _ = fc.lattice()
    sal = np.random.default_rng(5).integers(0, 4, 125).astype(np.float32)
    for cell in (None, 0.75):
        at = hfl.iss_select([cloud], [sal], kc.LATTICE_RADIUS, cell_size=cell)[0].cpu().numpy()
        below = hfl.iss_select([cloud], [sal], kc.LATTICE_RADIUS_BELOW, cell_size=cell)[0].cpu().numpy()
        assert np.array_equal(at, kc.lattice_select_exact(sal, 5)) and np.array_equal(below, kc.lattice_select_exact(sal, 4))


def test_a_nan_saliency_is_no_candidate_and_beats_nobody():
    sal = np.full(37, np.nan, np.float32)
    sal[7], sal[11] = 1.0, -1.0
    for cell in (None, 0.5):
        assert hfl.iss_select([kc.cloud_of('plane37')], [sal], 1e4, cell_size=cell)[0].tolist() == [7]


# ------------------------------------------------------------------------------------------------ the grid decides nothing
def test_cell_sizes_and_the_forced_fallback_agree():
    keys = ['planes', 'planes700', 257]
    outs = {}
    for cell in (None, RS / 4, 1e4):
        out = hfl.iss_saliency(clouds_of(keys), RS, return_counts=True, return_pending=True, cell_size=cell)
        check_saliency(out, keys, RS)
        outs[cell] = out
        _, _, pending = check_keypoints(keys, RS, RN, cell_size=cell)
        assert (pending > 0) == (cell == RS / 4)
    assert outs[None][2] == 0 and outs[1e4][2] == 0 and outs[RS / 4][2] > 0
    for a, b, c in zip(outs[None][0], outs[RS / 4][0], outs[1e4][0]):
        assert torch.equal(a > 0, b > 0) and torch.equal(a > 0, c > 0)


def test_far_points_and_a_non_max_radius_above_the_salient_one():
    """'planes700' spans 800 m: the 20 far points stand alone (count 1, saliency 0), and the one sorted batch is laid out for
    the larger radius, here the non-maximum one"""
    key = 'planes700'
    clouds = clouds_of([key])
    for rs, rn in ((1.0, 1.5), (1.5, 6.5)):
        check_saliency(hfl.iss_saliency(clouds, rs, return_counts=True), [key], rs)
        lists, sal, pending = hfl.iss_keypoints(clouds, rs, rn, return_saliency=True, return_pending=True)
        assert np.array_equal(lists[0].cpu().numpy(), hfl.iss_select_host(clouds, host(sal), rn)[0])
        assert pending == 0 and not sal[0][-20:].any() and (lists[0] < 680).all() and lists[0].shape[0] > 0


# ------------------------------------------------------------------------------------------------ determinism
def test_two_runs_give_the_same_bits():
    keys = ['planes700', 'duplicated', 'collinear', 257]
    for cell in (None, 0.5):
        first, second = (hfl.iss_keypoints(clouds_of(keys), RS, RN, return_saliency=True, cell_size=cell) for _ in range(2))
        for a, b in zip(first[0] + first[1], second[0] + second[1]):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
        sal = [kc.integer_saliency(k) for k in keys]
        one, two = (hfl.iss_select(clouds_of(keys), sal, RN, return_mask=True, cell_size=cell) for _ in range(2))
        assert all(torch.equal(a, b) for a, b in zip(one, two))


# ------------------------------------------------------------------------------------------------ refusals
def test_device_tensors_go_in_and_cpu_device_is_refused():
    cloud = kc.cloud_of(257)
    sal = kc.integer_saliency(257)
    for call in (lambda c: hfl.iss_saliency([c], RS, device='cpu'), lambda c: hfl.iss_select([c], [sal], RN, device='cpu'),
                 lambda c: hfl.iss_keypoints([c], RS, RN, device='cpu')):
        with pytest.raises(_native.NativeLibraryError):
            call(cloud)
    on_device = torch.from_numpy(np.array(cloud)).cuda()
    assert np.array_equal(hfl.iss_keypoints([on_device], RS, RN)[0].cpu().numpy(), kc.host_keypoints(257, RS, RN))
    assert hfl.iss_keypoints([], RS, RN) == [] and hfl.iss_saliency([], RS, return_pending=True) == ([], 0)
    assert hfl.iss_select([], [], RN) == []
    with pytest.raises(ValueError):
        hfl.iss_select([cloud], [sal[:-1]], RN)
    with pytest.raises(TypeError):
        hfl.iss_select([cloud], [sal.astype(np.float64)], RN)
    with pytest.raises(ValueError):
        hfl.iss_keypoints([cloud], RS, 0.0)
    with pytest.raises(ValueError):
        hfl.iss_keypoints([np.array([[0, 0, np.nan]], np.float32)], RS, RN)


# ------------------------------------------------------------------------------------------------ the purpose
def on_gpu(cloud):
    return torch.from_numpy(np.array(cloud)).cuda()


def test_global_registration_on_keypoints():
    src, dst = gc.clouds()
    for key in ('planes', 'planes_moved'):
        assert np.array_equal(hfl.iss_keypoints([kc.cloud_of(key)], RS, RN)[0].cpu().numpy(), kc.host_keypoints(key, RS, RN))
    coarse, fine = hfl.global_registration([on_gpu(src)], [on_gpu(dst)], salient_radius=RS, non_max_radius=RN)
    angle, shift = gc.pose_error(fine.transforms[0])
    print('%.3g degrees, %.3g m, %d inliers of the coarse pose' % (angle, shift, coarse.inliers[0]))
    assert angle <= gc.ANGLE_TOL_DEG and shift <= gc.SHIFT_TOL


def test_a_cloud_without_a_keypoint_ends_no_hypothesis():
    flat, (src, dst) = kc.cloud_of('plane37'), gc.clouds()
    coarse, fine = hfl.global_registration([on_gpu(flat), on_gpu(src)], [on_gpu(flat), on_gpu(dst)], salient_radius=RS,
                                           non_max_radius=RN)
    assert coarse.status.tolist()[0] == GR.NO_HYPOTHESIS and np.array_equal(coarse.transforms[0], np.eye(4))
    assert gc.pose_error(fine.transforms[1])[0] <= gc.ANGLE_TOL_DEG


def test_rerank_on_keypoints_equals_the_host_order():
    queries, database, cand = sc.rerank_inputs()
    want = hfl.rerank_candidates_host(queries, database, cand, salient_radius=RS, non_max_radius=RN)
    assert sc.DATABASE[want.indices[0, 0]] == 'planes'                # confirmed on the host route first
    got = hfl.rerank_candidates([on_gpu(c) for c in queries], [on_gpu(c) for c in database], cand, salient_radius=RS,
                                non_max_radius=RN)
    assert np.array_equal(got.indices.cpu().numpy(), want.indices) and np.array_equal(got.order.cpu().numpy(), want.order)
    assert sc.DATABASE[int(got.indices[0, 0])] == 'planes'


def test_wiring_refusals():
    src, dst = (on_gpu(c) for c in gc.clouds())
    queries, database, cand = sc.rerank_inputs()
    queries, database = [on_gpu(c) for c in queries], [on_gpu(c) for c in database]
    for kw in (dict(salient_radius=1.5), dict(non_max_radius=1.0), dict(salient_radius=-1.0, non_max_radius=1.0),
               dict(salient_radius=1.5, non_max_radius=float('inf'))):
        with pytest.raises(ValueError):
            hfl.global_registration([src], [dst], **kw)
        with pytest.raises(ValueError):
            hfl.rerank_candidates(queries, database, cand, **kw)
