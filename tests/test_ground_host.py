"""The cloth filter's numpy route (`hotformerloc_amd/ground.py`) against answers known in closed form, values worked out by
hand from the definition in that module's docstring, serial re-statements of single rules, and a synthetic forest whose
truth is known by construction.  No GPU."""
import numpy as np
import pytest

from hotformerloc_amd import ground
from hotformerloc_amd import remove_ground_host
from tests import ground_cases as gc

F = np.float32


# ---------------------------------------------------------------------------------------------- closed form
def test_flat_lattice_is_all_ground():
    cloud = gc.lattice()
    out, cloth = remove_ground_host([cloud], return_cloth=True)
    u, movable, t, steps = cloth[0]
    assert out[0].shape == (0, 3) and out[0].dtype == np.float32
    assert u.shape == (11, 11) and u.dtype == np.float32
    assert np.all(u == F(-3)) and np.all(t == F(-3))
    assert not movable.any()
    assert steps < 500


def test_elevated_points_come_back_from_half_a_metre_on():
    cloud = gc.lattice_with_elevated()
    out, mask = remove_ground_host([cloud], return_mask=True)
    want = cloud[64:][np.array(gc.ELEVATED_HEIGHTS) >= 0.5]              # strict <: the point at exactly 0.5 is not ground
    assert want.shape == (3, 3)
    np.testing.assert_array_equal(out[0], want)
    assert mask[0].tolist() == [False] * 64 + [False, True, True, True]


# ---------------------------------------------------------------------------------------------- grid, raster, fill by hand
def test_single_point_gives_a_four_by_four_cloth():
    W, H, ox, oy, u0, t, rastered = ground.raster_host(np.array([[5.25, -1.5, 2.0]], F), 1.0)
    assert (W, H) == (4, 4) and (ox, oy) == (F(3.25), F(-3.5)) and u0 == F(-2.0) + F(0.05)
    assert np.argwhere(rastered).tolist() == [[2, 2]]
    np.testing.assert_array_equal(t, np.full((4, 4), -2.0, F))


@pytest.mark.parametrize('swap', [False, True])
def test_raster_tie_goes_to_the_lowest_index(swap):
    # x spans [0, 2], y = 0: ox = oy = -2, W = 6, H = 4; the last two points both map to particle (3, 2) at x = 1, each
    # 0.25 away (exact in fp32), so the one that comes first in the cloud wins
    tie = [[1.25, 0.0, 7.0], [0.75, 0.0, 8.0]]
    cloud = np.array([[0.0, 0.0, 5.0], [2.0, 0.0, 6.0]] + (tie[::-1] if swap else tie), F)
    W, H, ox, oy, _, t, rastered = ground.raster_host(cloud, 1.0)
    assert (W, H, ox, oy) == (6, 4, F(-2), F(-2))
    assert np.argwhere(rastered).tolist() == [[2, 2], [2, 3], [2, 4]]
    won = -8.0 if swap else -7.0
    # row 2: particles 0, 1 find particle 2 scanning towards larger i, particle 5 finds particle 4 towards smaller i; the
    # other rows are empty: columns 2..4 take their column's value, columns 0, 1, 5 the nearest rastered particle
    row = [-5.0, -5.0, -5.0, won, -6.0, -6.0]
    np.testing.assert_array_equal(t, np.array([row] * 4, F))


def test_fill_of_an_empty_row():
    cloud = np.array([[0, 0, 1], [1, 0, 2], [0, 2, 3], [1, 2, 4]], F)
    W, H, _, _, _, t, rastered = ground.raster_host(cloud, 1.0)
    assert (W, H) == (5, 6)
    assert np.argwhere(rastered).tolist() == [[2, 2], [2, 3], [4, 2], [4, 3]]
    low, high = [-1, -1, -1, -2, -2], [-3, -3, -3, -4, -4]
    # row 3 is empty: its particles look down their column first (towards smaller j), and (1, 3), at index distance 2 from
    # both (2, 2) and (2, 4), takes the one with the lowest j
    np.testing.assert_array_equal(t, np.array([low, low, low, low, high, high], F))


def test_fill_of_an_empty_row_and_column_at_a_corner():
    cloud = np.array([[0, 0, 1], [1, 1, 2]], F)
    W, H, _, _, _, t, rastered = ground.raster_host(cloud, 1.0)
    assert (W, H) == (5, 5)
    assert np.argwhere(rastered).tolist() == [[2, 2], [3, 3]]
    # A = (2, 2) -> -1, B = (3, 3) -> -2.  (4, 0): A at 4 + 4 beats B at 1 + 9; (4, 1) and (1, 4): A and B tie at 5, the
    # lowest j wins; (4, 4): B at 2
    want = np.array([[-1, -1, -1, -2, -1],
                     [-1, -1, -1, -2, -1],
                     [-1, -1, -1, -1, -1],
                     [-2, -2, -2, -2, -2],
                     [-1, -1, -1, -2, -2]], F)
    np.testing.assert_array_equal(t, want)


# ---------------------------------------------------------------------------------------------- pair rule, parity classes
@pytest.mark.parametrize('rigidness', [1, 2, 3])
def test_one_sweep_on_a_displaced_particle(rigidness):
    # only the centre of a 5 x 5 cloth is movable, and it alone is displaced: every offset has two pairs that hold it, once
    # as p and once as q, so one sweep moves it sixteen times by f1 d towards its partner at 0
    u = np.zeros((5, 5), F)
    u[2, 2] = 1
    movable = np.zeros((5, 5), bool)
    movable[2, 2] = True
    f1 = F(1.0 - 0.7 ** rigidness)
    assert f1 == F({1: 0.3, 2: 0.51, 3: 0.657}[rigidness])
    x = F(1)
    for _ in range(16):
        x = F(x + F(f1 * F(F(0) - x)))
    want = np.zeros((5, 5), F)
    want[2, 2] = x
    got = ground.constraint_sweep_host(u, movable, rigidness)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(u[2, 2], F(1))                          # the input is not changed


@pytest.mark.parametrize('rigidness', [1, 2, 3])
def test_one_sweep_equals_the_pairs_taken_one_by_one(rigidness):
    rng = np.random.default_rng(rigidness)
    u = rng.uniform(-1, 1, (5, 5)).astype(F)
    movable = rng.uniform(size=(5, 5)) < 0.7
    f1, f2 = F(1.0 - 0.7 ** rigidness), F(0.5 * (1.0 - 0.4 ** rigidness))
    assert f2 == F({1: 0.3, 2: 0.42, 3: 0.468}[rigidness])
    want = u.copy()
    for dx, dy in [(1, 0), (0, 1), (1, 1), (1, -1), (2, 0), (0, 2), (2, 2), (2, -2)]:
        for cls in (0, 1):
            for j in range(5):
                for i in range(5):
                    sel = i // max(abs(dx), 1) if dx else j // abs(dy)
                    if sel % 2 != cls or not (i + dx < 5 and 0 <= j + dy < 5):
                        continue
                    a, b = want[j, i], want[j + dy, i + dx]
                    d = F(b - a)
                    if movable[j, i] and movable[j + dy, i + dx]:
                        want[j, i], want[j + dy, i + dx] = F(a + F(f2 * d)), F(b - F(f2 * d))
                    elif movable[j, i]:
                        want[j, i] = F(a + F(f1 * d))
                    elif movable[j + dy, i + dx]:
                        want[j + dy, i + dx] = F(b - F(f1 * d))
    np.testing.assert_array_equal(ground.constraint_sweep_host(u, movable, rigidness), want)


def test_no_sub_pass_touches_a_particle_twice():
    for W in range(4, 10):
        for H in range(4, 10):
            passes = ground.constraint_passes(W, H)
            assert len(passes) == 16
            pairs = set()
            for k, (p, q) in enumerate(passes):
                both = np.concatenate([p, q])
                assert both.size == np.unique(both).size, (W, H, k)
                dx, dy = ground.OFFSETS[k // 2]
                assert np.all(q - p == dy * W + dx) and np.all(p % W + dx < W) and np.all((q >= 0) & (q < W * H))
                pairs |= set(zip(p.tolist(), q.tolist()))
            # and together the sub-passes hold every pair of every offset once
            want = sum((W - dx) * (H - abs(dy)) for dx, dy in ground.OFFSETS)
            assert len(pairs) == want == sum(p.size for p, _ in passes), (W, H)


# ---------------------------------------------------------------------------------------------- slope smoothing
def _smooth_naive(u, t, movable, reverse):
    u, movable = u.copy(), movable.copy()
    H, W = u.shape
    order = [(j, i) for j in range(H) for i in range(W)]
    if reverse:
        order.reverse()
    changed = True
    while changed:
        changed = False
        for j, i in order:
            if not movable[j, i] or not abs(F(u[j, i] - t[j, i])) < F(0.3):
                continue
            for b, a in ((j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i)):
                if 0 <= a < W and 0 <= b < H and not movable[b, a] and abs(F(t[j, i] - t[b, a])) < F(0.3):
                    u[j, i], movable[j, i], changed = t[j, i], False, True
                    break
    return u, movable


def test_slope_smoothing_is_the_closure_whatever_the_order():
    rng = np.random.default_rng(5)
    t = rng.uniform(0, 0.6, (12, 12)).astype(F)
    u = (t + rng.uniform(0, 0.5, (12, 12))).astype(F)
    movable = rng.uniform(size=(12, 12)) < 0.8
    got_u, got_m = ground.slope_smooth_host(u, t, movable)
    taken = int(movable.sum() - got_m.sum())
    assert 10 < taken < movable.sum(), taken                               # the state exercises the rule, and its limits
    for reverse in (False, True):
        want_u, want_m = _smooth_naive(u, t, movable, reverse)
        np.testing.assert_array_equal(got_m, want_m)
        np.testing.assert_array_equal(got_u, want_u)


# ---------------------------------------------------------------------------------------------- synthetic forest
FOREST_GROUND_SHARE = 0.99921875       # recorded from this route; the floors are these minus 0.01
FOREST_OBJECT_SHARE = 1.0


def test_synthetic_forest():
    pts, is_ground, is_object = gc.forest(0)
    assert (is_ground | is_object).mean() >= 0.90                          # a condition on the scene
    out, mask = remove_ground_host([pts], return_mask=True)
    ground_share, object_share = gc.forest_shares(mask[0], is_ground, is_object)
    print('forest: %d points, ground share %.6f, object share %.6f' % (len(pts), ground_share, object_share))
    assert ground_share >= FOREST_GROUND_SHARE - 0.01
    assert object_share >= FOREST_OBJECT_SHARE - 0.01
    np.testing.assert_array_equal(out[0], pts[mask[0]])


# ---------------------------------------------------------------------------------------------- errors before any work
@pytest.mark.parametrize('params', [{'rigidness': 0}, {'rigidness': 4}, {'cloth_resolution': 0.0}, {'cloth_resolution': -1.0},
                                    {'class_threshold': 0.0}, {'class_threshold': -0.5}, {'cloth_resolution': float('nan')}])
def test_bad_parameters(params, monkeypatch):
    monkeypatch.setattr(ground, 'simulate_host', lambda *a, **k: pytest.fail('work was done'))
    with pytest.raises(ValueError):
        remove_ground_host([gc.lattice()], **params)
    with pytest.raises(ValueError):
        ground.remove_ground([gc.lattice()], **params)                     # the device route checks them first, too


def test_empty_cloud_and_cloth_over_the_limit(monkeypatch):
    monkeypatch.setattr(ground, 'simulate_host', lambda *a, **k: pytest.fail('work was done'))
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        remove_ground_host([gc.lattice(), np.zeros((0, 3), F)])
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        ground.remove_ground([gc.lattice(), np.zeros((0, 3), F)])
    wide = np.array([[0, 0, 0], [200, 200, 1]], F)                         # a cloth of 204 x 204
    with pytest.raises(ValueError, match='cloud 1 needs a cloth of 204 x 204'):
        remove_ground_host([gc.lattice(), wide])
    assert ground.cloth_grid([0, 0, 0, 96, 96, 1], 1.0)[:2] == (100, 100)  # 100 x 100 fits
    with pytest.raises(ValueError, match='cloud 3 needs a cloth'):
        ground.cloth_grid([0, 0, 0, 99, 99, 1], 1.0, 3)
