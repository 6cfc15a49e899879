"""Host side of the training augmentation (`hotformerloc_amd.augment`): the Philox generator against its published
known-answer vectors, `augment_clouds_host` against goldens produced by the reference's own classes
(`tools/gen_golden_augment.py`), `draw_params`, and the bookkeeping of `training.make_training_minibatches`.  No GPU."""

import numpy as np
import pytest
import torch

from augment_cases import CASE_NAMES, cases, compare
from hotformerloc_amd import augment as A
from hotformerloc_amd import training


@pytest.mark.parametrize('counter, key, want', [
    ([0, 0, 0, 0], (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, want):
    got = A.philox4x32_10(np.array(counter, dtype=np.uint32), key)
    assert ' '.join('%08x' % w for w in got) == want
    # vectorised: the same words at every row of a batch of counters
    many = A.philox4x32_10(np.tile(np.array(counter, dtype=np.uint32), (5, 1)), key)
    assert (many == got[None, :]).all()


def test_per_point_numbers_depend_on_seed_cloud_and_point_only():
    a = A.jitter_normals(100, 7, 3)
    assert np.array_equal(A.jitter_normals(40, 7, 3), a[:40])             # not on the cloud's size
    assert not np.array_equal(A.jitter_normals(100, 7, 4), a) and not np.array_equal(A.jitter_normals(100, 8, 3), a)
    assert np.isfinite(a).all()
    n = A.jitter_normals(200000, 1, 0)
    assert np.abs(n.mean(0)).max() < 0.01 and np.abs(n.std(0) - 1.0).max() < 0.01
    k = A.philox_selection_keys(100, 7, 3)
    assert k.dtype == np.uint32 and np.array_equal(A.philox_selection_keys(10, 7, 3), k[:10])
    assert not np.array_equal(k, A.jitter_normals(100, 7, 3)[:, 0].view(np.uint32))


def test_select_removed_tie_rule():
    assert A.select_removed(np.zeros(9, np.uint32), 5).tolist() == [0, 1, 2, 3, 4]
    keys = (np.arange(1025) % 4).astype(np.uint32)
    assert A.select_removed(keys, 257).tolist() == list(range(0, 1025, 4))         # all of class 0
    assert A.select_removed(keys, 258).tolist() == sorted(list(range(0, 1025, 4)) + [1])
    assert A.select_removed(keys, 256).tolist() == list(range(0, 1024, 4))
    assert A.select_removed(keys, 0).tolist() == []


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_chain_against_the_reference(name):
    c = cases()[name]
    pts, idx = A.augment_clouds_host(c.raws, c.cfg, seed=c.seed, params=c.params, cylindrical='none', return_index=True)
    for i, raw in enumerate(c.raws):
        assert len(c.near[i]) == c.near_count[i]
        compare(c.pts[i], c.idx[i], pts[i].numpy(), idx[i].numpy(), c.near[i], len(raw), '%s cloud %d' % (name, i))


def test_goldens_cover_what_they_must():
    cs = cases()
    modes = {(c.cfg.aug_mode, c.cfg.set_aug_mode) for c in cs.values()}
    assert {(1, 1), (1, 2), (2, 1), (2, 2)} <= modes
    assert any(not c.cfg.normalize_points for c in cs.values())
    assert any(c.cfg.coordinates == 'cylindrical' for c in cs.values())
    assert {c.params.flip_axis for c in cs.values()} >= {0, 1, -1}
    coins = np.concatenate([c.params.block for c in cs.values()])
    assert (coins == 1).any() and (coins == 0).any()
    assert {len(r) for c in cs.values() for r in c.raws} >= {3, 65} and max(len(r) for r in cs['a1_s1'].raws) >= 4000


def test_cylindrical_host_stage_follows_the_cartesian_one():
    from hotformerloc_amd import synthetic as syn
    c = cases()['cyl_a2_s1']
    cart = A.augment_clouds_host(c.raws, c.cfg, seed=c.seed, params=c.params, cylindrical='none')
    cyl = A.augment_clouds_host(c.raws, c.cfg, seed=c.seed, params=c.params)
    for a, b in zip(cart, cyl):
        assert a.shape == b.shape and float(b.abs().max()) <= 1.0
        inside = (a.abs() <= 1.0).all(dim=1).numpy()                  # where the batch-wide rotation kept |c| <= 1
        assert np.array_equal(syn.cylindrical(a.numpy()[inside]), b.numpy()[inside])


def test_draw_params_ranges_and_reproducibility():
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cartesian')
    sizes = [1, 3, 65, 4000, 20000] * 40
    p = A.draw_params(sizes, cfg, torch.Generator().manual_seed(5))
    n = np.asarray(sizes)
    assert len(p) == len(sizes)
    assert (p.remove_k >= 0).all() and (p.remove_k <= 0.1 * n).all() and (p.remove_k[n == 20000] > 0).any()
    assert np.array_equal(p.remove_k, [int(m * r) for m, r in zip(sizes, p.remove_r)])
    assert (np.abs(p.theta) <= np.pi).all() and np.abs(p.theta).max() > 1.0 and abs(p.set_theta) <= np.pi
    assert np.allclose(p.rot_cos, np.cos(p.theta), atol=1e-7) and np.allclose(p.rot_sin, np.sin(p.theta), atol=1e-7)
    assert p.rot_cos.dtype == np.float32 and p.trans.dtype == np.float32
    assert set(np.unique(p.block)) == {0, 1} and np.array_equal(p.block == 1, p.block_coin < 0.4)
    assert 0.25 < p.block.mean() < 0.55
    u = p.block_u
    assert (u[:, 0] >= 0.02).all() and (u[:, 0] <= 0.33).all() and (u[:, 1] >= 0.3).all() and (u[:, 1] <= 3.3).all()
    assert (u[:, 2:] >= 0).all() and (u[:, 2:] < 1).all()
    assert np.array_equal(p.trans, (0.01 * p.trans_n).astype(np.float32))
    assert p.flip_axis in (-1, 0, 1)
    # the flip classes are exhaustive and ordered as RandomFlip orders them
    assert [A.flip_axis_of(d) for d in (0.0, 0.25, 0.2500001, 0.5, 0.5000001, 0.99)] == [0, 0, 1, 1, -1, -1]
    # reproducible from the generator state, and consuming it
    g = torch.Generator().manual_seed(5)
    q = A.draw_params(sizes, cfg, g)
    assert all(np.array_equal(getattr(p, f), getattr(q, f)) for f in A.AugmentParams._ARRAYS)
    assert (p.set_theta, p.flip_draw, p.flip_axis) == (q.set_theta, q.flip_draw, q.flip_axis)
    r = A.draw_params(sizes, cfg, g)
    assert not np.array_equal(r.remove_r, q.remove_r)
    # aug_mode 1: no rotation; set_aug_mode 2: no batch-wide rotation
    p1 = A.draw_params(sizes, A.AugmentConfig.from_training_params(1, 2, 180.0, True, 'cartesian'),
                       torch.Generator().manual_seed(5))
    assert (p1.theta == 0).all() and (p1.rot_cos == 1).all() and p1.set_theta == 0.0 and p1.set_cos == 1.0


def test_draw_params_draws_nothing_without_augmentation():
    cfg = A.AugmentConfig.from_training_params(0, 0, 180.0, True, 'cartesian')
    g = torch.Generator().manual_seed(9)
    before = g.get_state().clone()
    p = A.draw_params([5, 7], cfg, g)
    assert torch.equal(g.get_state(), before)
    assert (p.remove_k == 0).all() and (p.block == 0).all() and (p.trans == 0).all() and p.flip_axis == -1
    assert p.rows().shape == (2, 12) and p.rows().dtype == np.uint32


def test_config_rejects_what_prepare_clouds_rejects():
    with pytest.raises(NotImplementedError):
        A.AugmentConfig.from_training_params(1, 1, 5.0, True, 'cartesian', unit_sphere_norm=True)
    with pytest.raises(NotImplementedError):
        A.AugmentConfig.from_training_params(1, 1, 5.0, True, 'cartesian', scale_factor=30.0)
    with pytest.raises(NotImplementedError):
        A.AugmentConfig.from_training_params(3, 1, 5.0, True, 'cartesian')
    cfg = A.AugmentConfig.from_training_params(1, 1, 5.0, True, 'cartesian')
    with pytest.raises(ValueError):
        A.augment_clouds_host([np.zeros((0, 3), np.float32)], cfg, seed=1)
    far = np.full((4, 3), 5.0, np.float32)                                 # not normalised: every point outside the cube
    with pytest.raises(ValueError):
        A.augment_clouds_host([far], A.AugmentConfig.from_training_params(1, 1, 5.0, False, 'cartesian'), seed=1)


def test_minibatch_bookkeeping(monkeypatch):
    """One scalar draw for the whole batch, sliced per minibatch; cloud_base = index of the minibatch's first cloud."""
    calls = []

    def fake_augment(clouds, cfg, *, seed, params, cloud_base, cylindrical, device):
        calls.append(dict(n=len(clouds), seed=seed, params=params, cloud_base=cloud_base))
        return ['aug%d' % (cloud_base + i) for i in range(len(clouds))]

    monkeypatch.setattr(A, 'augment_clouds', fake_augment)
    from hotformerloc_amd import octree
    monkeypatch.setattr(octree, 'build_batch_octree', lambda pts, depth, full_depth, device: (tuple(pts), depth, full_depth))
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cartesian')
    clouds = [np.zeros((n, 3), np.float32) for n in (10, 20, 30, 40, 50)]
    g = torch.Generator().manual_seed(3)
    mb = training.make_training_minibatches(clouds, 2, cfg, 7, 2, seed=99, generator=g)
    whole = A.draw_params([10, 20, 30, 40, 50], cfg, torch.Generator().manual_seed(3))
    assert [c['cloud_base'] for c in calls] == [0, 2, 4] and [c['n'] for c in calls] == [2, 2, 1]
    assert all(c['seed'] == 99 for c in calls)
    for c in calls:
        s = c['cloud_base']
        assert np.array_equal(c['params'].remove_r, whole.remove_r[s:s + c['n']])
        assert np.array_equal(c['params'].trans, whole.trans[s:s + c['n']])
        assert (c['params'].set_theta, c['params'].flip_draw) == (whole.set_theta, whole.flip_draw)
    assert [m['octree'] for m in mb] == [(('aug0', 'aug1'), 7, 2), (('aug2', 'aug3'), 7, 2), (('aug4',), 7, 2)]
    # the generator moved on by exactly one batch's draws
    assert torch.equal(g.get_state(), _state_after(cfg, [10, 20, 30, 40, 50], 3))
    calls.clear()
    mb = training.make_training_minibatches(clouds, None, cfg, 7, 2, seed=99, params=whole)
    assert [c['cloud_base'] for c in calls] == [0] and calls[0]['n'] == 5 and len(mb) == 1
    with pytest.raises(ValueError):
        training.make_training_minibatches(clouds[:3], 2, cfg, 7, 2, seed=1, params=whole)
    assert training.make_training_minibatches([], 2, cfg, 7, 2, seed=1) == []


def _state_after(cfg, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    A.draw_params(sizes, cfg, g)
    return g.get_state()
