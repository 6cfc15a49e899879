"""The cloth filter on the device (`csrc/ground.hip`, `hotformerloc_amd/ground.py`) against the numpy route of the same
module.  There is no tolerance: both routes follow one definition in fp32, every operation rounded once, so the terrain
values, the cloth heights, the movable flags, the number of steps and the masks are equal and the returned rows are the
input's rows bit for bit.

About the stop-flag case.  A cloth that hangs over a pit comes to rest geometrically, so its largest move always passes
through the stop window 0 < m < 0.005: over a 9 x 9-cell pit the run ends after 4 steps (measured with the numpy route,
rigidness 2; 5 and 3 steps for rigidness 1 and 3), and no such scene runs all 500 steps under the definition.  What does
run them all is a cloth whose hanging particle is pulled back to an exact fp32 fixed point within a step (m == 0 with a
movable particle left): a one-cell pit in ground that does not lie at height 0, where the floats are too dense for that.
`stop_flag_batch` therefore holds the 9 x 9 pit (4 steps), a one-cell pit (500 steps) and a flat lattice (1 step) in one
batch, and the test asserts these counts."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import ground, load_config, model_factory, retrieval, voxel
from hotformerloc_amd import synthetic as syn
from tests import ground_cases as gc

pytestmark = pytest.mark.gpu
F = np.float32


def _small_forest(seed=0):
    return gc.forest(seed, size=20.0, trunks_per_m2=10 / 400.0, blobs_per_m2=2 / 400.0)[0]


def _rough(nx, ny, seed):
    """a lattice, one point per cell, jittered by less than 0.3 of a cell, on a gentle rough surface with a few posts"""
    rng = np.random.default_rng(seed)
    pts = gc.lattice(nx, ny, 0.0)
    pts[:, 2] = (0.8 * np.sin(pts[:, 0] / 9.0) + 0.05 * pts[:, 1] + rng.uniform(-0.05, 0.05, len(pts))).astype(F)
    pts[rng.choice(len(pts), max(len(pts) // 40, 1), replace=False), 2] += F(5.0)
    pts[:, :2] += rng.uniform(-0.3, 0.3, (len(pts), 2)).astype(F)
    pts[0, :2], pts[-1, :2] = (0, 0), (nx - 1, ny - 1)                     # the bounds, and so the cloth size, stay put
    return pts


CASES = {
    'one_point': lambda: ([np.array([[5.25, -1.5, 2.0]], F)], {}),
    'two_points_in_one_cell': lambda: ([np.array([[0.0, 0.0, 1.0], [0.3, 0.2, 1.4]], F)], {}),
    'flat_lattice': lambda: ([gc.lattice()], {}),
    'lattice_with_elevated': lambda: ([gc.lattice_with_elevated()], {}),
    'cloth_5_by_37': lambda: ([_rough(2, 34, 1)], {}),                     # ragged tails in every parity class
    'cloth_near_the_limit': lambda: ([_rough(99, 97, 2)], {}),             # 102 x 100 = 10 200 of 10 240 particles
    'small_forest': lambda: ([_small_forest()], {}),
    'stop_flag_batch': lambda: ([gc.block_scene(ground=3.0), gc.block_scene(size=1, ground=3.0), gc.lattice(30, 30, 3.0)], {}),
    'rigidness_1': lambda: ([_small_forest()], {'rigidness': 1}),
    'rigidness_3': lambda: ([_small_forest()], {'rigidness': 3}),
    'no_slope_smoothing': lambda: ([_small_forest()], {'slope_smooth': False}),
    'resolution_half_metre': lambda: ([_small_forest()], {'cloth_resolution': 0.5}),
}
CLOTH_SIZES = {'one_point': (4, 4), 'two_points_in_one_cell': (4, 4), 'cloth_5_by_37': (5, 37),
               'cloth_near_the_limit': (102, 100), 'resolution_half_metre': None}


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(clouds, params, kept rows, masks, cloths) by the numpy route, computed once and shared"""
    clouds, params = CASES[name]()
    out, masks, cloths = ground.remove_ground_host(clouds, return_mask=True, return_cloth=True, **params)
    return clouds, params, out, masks, cloths


def assert_same(got, want, what):
    """the device's (rows, masks, cloths) equal the host's to the bit"""
    for i, (rows, mask, cloth) in enumerate(zip(*got)):
        w_rows, w_mask, (u, movable, t, steps) = want[0][i], want[1][i], want[2][i]
        assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == w_rows.shape, (what, i)
        np.testing.assert_array_equal(cloth[2].cpu().numpy(), t, err_msg='%s cloud %d: t' % (what, i))
        assert cloth[3] == steps, '%s cloud %d: %d steps, host %d' % (what, i, cloth[3], steps)
        np.testing.assert_array_equal(cloth[1].cpu().numpy(), movable, err_msg='%s cloud %d: movable' % (what, i))
        np.testing.assert_array_equal(cloth[0].cpu().numpy().view(np.uint32), u.view(np.uint32), err_msg='%s cloud %d: u' % (what, i))
        np.testing.assert_array_equal(mask.cpu().numpy(), w_mask, err_msg='%s cloud %d: mask' % (what, i))
        np.testing.assert_array_equal(rows.cpu().numpy().view(np.uint32), w_rows.view(np.uint32))


@pytest.mark.parametrize('name', list(CASES))
def test_device_equals_host(name):
    clouds, params, out, masks, cloths = host_case(name)
    got = ground.remove_ground(clouds, return_mask=True, return_cloth=True, **params)
    print(name, [(tuple(c[0].shape), c[3], int(c[1].sum())) for c in cloths], [o.shape[0] for o in out])
    assert_same(got, (out, masks, cloths), name)
    if CLOTH_SIZES.get(name):
        assert tuple(cloths[0][0].shape) == CLOTH_SIZES[name][::-1]
    surf = ground.cloth_surface(clouds, **params)                          # the seam alone returns the same cloth
    for a, b in zip(surf, got[2]):
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_cases_cover_what_they_claim():
    steps = [c[3] for c in host_case('stop_flag_batch')[4]]
    assert steps == [4, 500, 1], steps                                     # see the module docstring
    assert host_case('stop_flag_batch')[4][1][1].sum() == 1                # one particle hangs, movable, to the end
    cloths = host_case('small_forest')[4]
    assert 0 < cloths[0][1].sum() < cloths[0][1].size and 1 < cloths[0][3] < 500
    assert len(host_case('small_forest')[0][0]) in range(3500, 4600)
    smooth, rough = host_case('small_forest')[4][0], host_case('no_slope_smoothing')[4][0]
    assert smooth[1].sum() < rough[1].sum()                                # the smoothing took particles
    assert host_case('resolution_half_metre')[4][0][0].shape[0] > 40
    assert 0 < host_case('cloth_near_the_limit')[2][0].shape[0] < 99 * 97


# ---------------------------------------------------------------------------------------------- batching
@functools.lru_cache(maxsize=None)
def ragged_batch():
    clouds = [np.array([[5.25, -1.5, 2.0]], F), _rough(2, 34, 1), gc.lattice_with_elevated(), _small_forest(1)[:1501],
              gc.block_scene(12, 4, 3, 6.0)]
    starts = np.cumsum([0] + [len(c) for c in clouds[:-1]]) * 12
    assert any(s % 16 for s in starts)                                     # a cloud that starts off a 16-byte boundary
    return clouds, ground.remove_ground_host(clouds, return_mask=True, return_cloth=True)


def test_ragged_batch_equals_each_cloud_alone():
    clouds, want = ragged_batch()
    got = ground.remove_ground(clouds, return_mask=True, return_cloth=True)
    assert_same(got, want, 'batch')
    for i, c in enumerate(clouds):
        rows, mask, cloth = ground.remove_ground([c], return_mask=True, return_cloth=True)
        assert torch.equal(rows[0], got[0][i]) and torch.equal(mask[0], got[1][i])
        assert all(torch.equal(x, y) for x, y in zip(cloth[0][:3], got[2][i][:3])) and cloth[0][3] == got[2][i][3]
    again = ground.remove_ground(clouds, return_mask=True, return_cloth=True)
    for i in range(len(clouds)):                                           # two runs give the same bits
        assert torch.equal(again[0][i], got[0][i]) and torch.equal(again[2][i][0], got[2][i][0])


def test_inputs_may_live_anywhere():
    clouds, want = ragged_batch()
    want_rows = want[0]
    for make in (lambda c: c, lambda c: torch.from_numpy(c), lambda c: torch.from_numpy(c).cuda(), lambda c: c.tolist()):
        got = ground.remove_ground([make(c) for c in clouds])
        for g, w in zip(got, want_rows):
            np.testing.assert_array_equal(g.cpu().numpy(), w)
    mixed = ground.remove_ground([torch.from_numpy(c).cuda() if i % 2 else c for i, c in enumerate(clouds)])
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(mixed, want_rows))
    assert ground.remove_ground([]) == []


def test_cloth_over_the_limit_is_refused_by_name():
    wide = np.array([[0, 0, 0], [200, 200, 1]], F)
    with pytest.raises(ValueError, match='cloud 1 needs a cloth of 204 x 204'):
        ground.remove_ground([gc.lattice(), wide])


# ---------------------------------------------------------------------------------------------- the chain
@functools.lru_cache(maxsize=None)
def raw_submaps():
    return [gc.forest(3, size=30.0)[0], gc.forest(4, size=24.0)[0], gc.forest(5, size=30.0)[0][:9001]]


def test_prepare_submaps_with_ground_removal_equals_the_chain():
    raw = raw_submaps()
    filtered = ground.remove_ground(raw)
    assert all(0 < f.shape[0] < len(r) for f, r in zip(filtered, raw))
    chained = voxel.normalise_submaps(voxel.voxel_downsample(filtered, 0.8))
    fused = voxel.prepare_submaps(raw, 0.8, remove_ground=True)
    assert all(torch.equal(a, b) for a, b in zip(fused, chained))
    only = voxel.prepare_submaps(raw, 0.8, normalise=False, remove_ground=True, ground_params={'rigidness': 3})
    want = voxel.voxel_downsample(ground.remove_ground(raw, rigidness=3), 0.8)
    assert all(torch.equal(a, b) for a, b in zip(only, want))


@pytest.mark.parametrize('downsample', ['pnvlad', 'random'])
def test_prepare_submaps_fixed_with_ground_removal_equals_the_chain(downsample):
    raw = raw_submaps()
    filtered = ground.remove_ground(raw)
    target = 512
    assert all(f.shape[0] > target for f in filtered)
    chained = voxel.prepare_submaps_fixed(filtered, target, downsample=downsample)      # the filtered cloud is the raw one
    fused = voxel.prepare_submaps_fixed(raw, target, downsample=downsample, remove_ground=True)
    assert all(tuple(a.shape) == (target, 3) and torch.equal(a, b) for a, b in zip(fused, chained))


def test_ground_removal_that_leaves_too_little_is_refused_by_name():
    clouds = [gc.lattice_with_elevated(), gc.lattice()]
    with pytest.raises(ValueError, match='cloud 1 has no point left after ground removal'):
        voxel.prepare_submaps(clouds, 0.8, remove_ground=True)
    with pytest.raises(ValueError, match='cloud 0 has 3 points left after ground removal, fewer than target = 4'):
        voxel.prepare_submaps_fixed(clouds, 4, downsample='random', remove_ground=True)


def test_encode_clouds_from_raw_submaps_with_ground():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    raw = raw_submaps()
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 2, remove_ground=True, voxel_size=0.8, normalise_submaps=True, **kw)
    filtered = ground.remove_ground(raw)
    want = retrieval.encode_clouds(model, filtered, 2, voxel_size=0.8, normalise_submaps=True, **kw)
    assert tuple(got.shape) == (3, 256) and bool(torch.isfinite(got).all())
    assert torch.allclose(got.norm(dim=1), torch.ones(3, device=got.device), atol=1e-5)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- nothing else changes
def test_without_the_keyword_nothing_changes():
    raw = raw_submaps()
    a = voxel.prepare_submaps(raw, 0.8)
    b = voxel.normalise_submaps(voxel.voxel_downsample(raw, 0.8))
    c = voxel.prepare_submaps(raw, 0.8, remove_ground=False, ground_params={'rigidness': 3})
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    fixed = voxel.prepare_submaps_fixed(raw, 512)
    want = voxel.normalise_submaps_padded(voxel.pnvlad_downsample(raw, 512), raw, 512)
    assert all(torch.equal(x, y) for x, y in zip(fixed, want))
    with pytest.raises(TypeError):
        voxel.prepare_submaps(raw, 0.8, True, 'cuda', True)               # the keyword cannot be passed by position
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 2, voxel_size=0.8, normalise_submaps=True, **kw)
    want = retrieval.encode_clouds(model, a, 2, **kw)
    assert torch.equal(got, want)
