"""Build container only: golden vectors of the reference's training augmentation -> tests/golden/augment.npz.

Runs the reference's OWN classes from `datasets/augmentation.py` in the order of `TrainTransform`
(`datasets/CSWildPlaces/CSWildPlaces_train.py:19-57`), the masks of `datasets/base_datasets.py:77-83` and the batch-wide
`TrainSetTransform` of `datasets/dataset_utils.py:111-116`.  The list is composed here (the dataset modules are not
imported); torchvision, absent from the image, is stood in for as in `oracle/gen_golden_coords.py`.  The reference's random
sources -- `random.random`, `random.uniform`, `np.random.rand`, `np.random.randn`, `np.random.choice`, `torch.randn_like` --
are patched to hand out this project's draws (`hotformerloc_amd.augment`: the scalar table of `draw_params`, the Philox
normals and the Philox selection) in the order the reference asks for them; a draw asked for out of order aborts.

Per case `<c>` the file holds `<c>.cfg` (JSON: the configuration, the Philox seed and the clouds' (seed, n, kind, extent,
offset) for `oracle.gen_golden_coords.raw_cloud`), the scalar table `<c>.p.*` (`AugmentParams.to_arrays`) and per cloud i
  <c>.<i>.pts    the reference's points after the batch-wide transform, in front of the cylindrical transform, float32
  <c>.<i>.idx    their indices in the input cloud, int32
  <c>.<i>.near   indices of input points of which a coordinate that feeds a decision (|c| = 1, |xy| = 1, a block edge) lies
                 within 1e-6 of that decision's boundary in the reference's run: only these may be left out of a comparison
and `<c>.near_count` (per cloud).  The generator asserts that `near` stays within 0.5 % of every cloud.

Usage:  python tools/gen_golden_augment.py"""
import collections
import importlib.util
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hotformerloc_amd import augment as A                      # noqa: E402
from oracle.gen_golden_coords import REF, _reference_classes, raw_cloud    # noqa: E402

NEAR = 1.0e-6
CAP = 0.005

FOREST = ('forest', (45.0, 45.0, 25.0), (-3.0, 7.0, 1.0))
BALL_M = ('ball', (35.0, 20.0, 8.0), (250.0, -120.0, 12.0))
READY = ('ball', (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))


def _clouds(seed, kind):
    return [(seed, 3) + kind, (seed + 1, 65) + kind, (seed + 2, 4001) + kind]


# case -> (aug_mode, set_aug_mode, random_rot_theta, normalize, coordinates, philox seed, generator seed, clouds,
#          block coins forced per cloud, flip draw forced)
CASES = {
    'a1_s1': (1, 1, 180.0, True, 'cartesian', 0x1234567, 11, _clouds(700, FOREST), (1, 0, 1), 0.10),
    'a1_s2': (1, 2, 180.0, True, 'cartesian', 0x9E3779B97F4A7C15, 12, _clouds(710, BALL_M), (0, 1, 1), 0.40),
    'a2_s1': (2, 1, 180.0, True, 'cartesian', 77, 13, _clouds(720, BALL_M), (1, 1, 0), 0.90),
    'a2_s2': (2, 2, 5.0, True, 'cartesian', 2 ** 63 + 5, 14, _clouds(730, FOREST), (0, 0, 1), 0.20),
    'raw_a2_s1': (2, 1, 180.0, False, 'cartesian', 31337, 15, _clouds(740, READY), (1, 0, 1), 0.45),
    'cyl_a2_s1': (2, 1, 180.0, True, 'cylindrical', 424242, 16, _clouds(750, FOREST), (0, 1, 1), 0.05),
}


class Draws:
    """The queue of this project's draws in the order the reference asks for them."""

    def __init__(self):
        self.q = collections.deque()

    def push(self, kind, value):
        self.q.append((kind, value))

    def pop(self, kind):
        got, value = self.q.popleft()
        assert got == kind, 'the reference asked for %s, the next draw is %s' % (kind, got)
        return value

    # stand-ins
    def random(self):
        return self.pop('random')

    def uniform(self, a, b):
        (lo, hi), v = self.pop('uniform')
        assert (a, b) == (lo, hi), ((a, b), (lo, hi))
        return v

    def rand(self, *shape):
        assert shape == (1,), shape
        return np.array([self.pop('rand')])

    def randn(self, *shape):
        assert shape == (1, 3), shape
        return self.pop('randn').reshape(1, 3)

    def choice(self, a, size=None, replace=True):
        n, idx = self.pop('choice')
        assert len(a) == n and size == len(idx) and replace is False, (len(a), n, size, len(idx))
        return idx

    def randn_like(self, e):
        v = self.pop('randn_like')
        assert tuple(e.shape) == tuple(v.shape)
        return torch.from_numpy(v)


def theta_uniform(theta, max_theta):
    """The uniform that `RandomRotation.__call__` turns into (nearly) theta, and the theta it really gives."""
    u = theta / ((np.pi * max_theta / 180.) * 2.) + 0.5
    return u, float((np.pi * max_theta / 180.) * 2. * (u - 0.5))


def main():
    _reference_classes()                                 # installs the torchvision stand-in
    spec = importlib.util.spec_from_file_location('ref_augmentation', os.path.join(REF, 'datasets', 'augmentation.py'))
    aug = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aug)
    out = {}
    for name, (aug_mode, set_mode, max_theta, normalize, coords, seed, gseed, clouds, coins, flip_draw) in CASES.items():
        cfg = A.AugmentConfig.from_training_params(aug_mode, set_mode, max_theta, normalize, coords)
        raws = [raw_cloud(*c) for c in clouds]
        sizes = [len(r) for r in raws]
        p = A.draw_params(sizes, cfg, torch.Generator().manual_seed(gseed))
        # forced coverage: the block coin per cloud and the flip class per case; thetas made exactly reproducible
        for i, coin in enumerate(coins):
            p.block[i] = coin
            p.block_coin[i] = 0.2 if coin else 0.7
        p.flip_draw = flip_draw
        p.flip_axis = A.flip_axis_of(flip_draw, cfg.flip_p)
        rot_u = [0.5] * len(sizes)
        if aug_mode == 2:
            for i in range(len(sizes)):
                rot_u[i], p.theta[i] = theta_uniform(p.theta[i], max_theta)
                p.rot_cos[i], p.rot_sin[i] = A._cos_sin32(p.theta[i])
        set_u = 0.5
        if set_mode == 1:
            set_u, p.set_theta = theta_uniform(p.set_theta, max_theta)
            p.set_cos, p.set_sin = A._cos_sin32(p.set_theta)

        d = Draws()
        fake_random = mock.Mock()
        fake_random.random = d.random
        fake_random.uniform = d.uniform
        results, nears = [], []
        with mock.patch.object(aug, 'random', fake_random), mock.patch.object(np.random, 'rand', d.rand), \
                mock.patch.object(np.random, 'randn', d.randn), mock.patch.object(np.random, 'choice', d.choice), \
                mock.patch.object(torch, 'randn_like', d.randn_like):
            kept = []
            for i, raw in enumerate(raws):
                n = len(raw)
                # ---- the queue of cloud i
                d.push('randn_like', A.jitter_normals(n, seed, i))
                d.push('uniform', (cfg.remove_ratio, float(p.remove_r[i])))
                d.push('choice', (n, A.select_removed(A.philox_selection_keys(n, seed, i), int(p.remove_k[i]))))
                if aug_mode == 2:
                    d.push('rand', rot_u[i])
                d.push('randn', p.trans_n[i])
                d.push('random', float(p.block_coin[i]))
                if p.block[i]:
                    d.push('uniform', (cfg.block_scale, float(p.block_u[i, 0])))
                    d.push('uniform', (cfg.block_ratio, float(p.block_u[i, 1])))
                    d.push('uniform', ((0, 1), float(p.block_u[i, 2])))
                    d.push('uniform', ((0, 1), float(p.block_u[i, 3])))
                # ---- TrainTransform, composed as CSWildPlaces_train.py:32-45 composes it
                t = []
                if normalize:
                    t.append(aug.Normalize(scale_factor=None, unit_sphere_norm=False, zero_mean=True))
                t.extend([aug.JitterPoints(sigma=0.001, clip=0.002), aug.RemoveRandomPoints(r=(0.0, 0.1))])
                if aug_mode == 2:
                    t.append(aug.RandomRotation(max_theta=max_theta, axis=np.array([0, 0, 1])))
                block = aug.RemoveRandomBlock(p=0.4)
                rect = {}
                inner = block.get_params

                def spy(coords, inner=inner, rect=rect):
                    rect['pre'] = coords.clone()
                    rect['xywh'] = inner(coords)
                    return rect['xywh']
                block.get_params = spy
                t.extend([aug.RandomTranslation(max_delta=0.01), block])
                data = torch.tensor(raw, dtype=torch.float)
                for f in t:
                    data = f(data)
                assert int(n * p.remove_r[i]) == int(p.remove_k[i])
                assert isinstance(data, torch.Tensor) and data.dtype == torch.float32
                # ---- base_datasets.py:77-83, with the indices carried along
                pre = data.clone()
                idx = torch.arange(n)
                mask = torch.all(abs(data) <= 1.0, dim=1)
                data, idx = data[mask], idx[mask]
                if coords == 'cylindrical':
                    data_norm = torch.linalg.norm(data[:, :2], dim=1)[:, None]
                    mask = torch.all(data_norm <= 1.0, dim=1)
                    data, idx = data[mask], idx[mask]
                kept.append((data, idx))
                # ---- points whose decisions sit within NEAR of a boundary in this run
                pn = pre.double().numpy()
                near = (np.abs(np.abs(pn) - 1.0) <= NEAR).any(axis=1)
                if coords == 'cylindrical':
                    near |= np.abs(np.hypot(pn[:, 0], pn[:, 1]) - 1.0) <= NEAR
                if p.block[i]:
                    x, y, w, h = rect['xywh']
                    x0, x1, y0, y1 = float(x), float(x + w), float(y), float(y + h)
                    q = rect['pre'].double().numpy()
                    in_x = (q[:, 0] >= x0 - NEAR) & (q[:, 0] <= x1 + NEAR)
                    in_y = (q[:, 1] >= y0 - NEAR) & (q[:, 1] <= y1 + NEAR)
                    near |= ((np.abs(q[:, 0] - x0) <= NEAR) | (np.abs(q[:, 0] - x1) <= NEAR)) & in_y
                    near |= ((np.abs(q[:, 1] - y0) <= NEAR) | (np.abs(q[:, 1] - y1) <= NEAR)) & in_x
                    mine = A.block_rectangle(rect['pre'].numpy(), p.block_u[i])
                    print('   block', i, 'reference', (x0, x1, y0, y1), 'restated', tuple(float(v) for v in mine))
                nears.append(np.nonzero(near)[0].astype(np.int32))
                assert len(nears[-1]) <= CAP * n, (name, i, len(nears[-1]), n)
            # ---- dataset_utils.py:111-116: one TrainSetTransform on the concatenation
            if set_mode == 1:
                d.push('rand', set_u)
            if set_mode != 0:
                d.push('random', p.flip_draw)
            t = []
            if set_mode == 1:
                t.append(aug.RandomRotation(max_theta=max_theta, axis=np.array([0, 0, 1])))
            t.append(aug.RandomFlip([0.25, 0.25, 0.]))
            lens = [len(k[0]) for k in kept]
            merged = torch.cat([k[0] for k in kept], dim=0)
            for f in t:
                merged = f(merged)
            results = merged.split(lens)
            assert not d.q, 'draws left over: %r' % [k for k, _ in d.q]
        out[name + '.cfg'] = np.array(json.dumps(dict(
            aug_mode=aug_mode, set_aug_mode=set_mode, random_rot_theta=max_theta, normalize_points=normalize,
            coordinates=coords, seed=seed, clouds=[list(c[:3]) + [list(c[3]), list(c[4])] for c in clouds])))
        out.update(p.to_arrays(name + '.p.'))
        for i, (r, (_, idx)) in enumerate(zip(results, kept)):
            out['%s.%d.pts' % (name, i)] = r.numpy().astype(np.float32)
            out['%s.%d.idx' % (name, i)] = idx.numpy().astype(np.int32)
            out['%s.%d.near' % (name, i)] = nears[i]
        out[name + '.near_count'] = np.array([len(x) for x in nears], dtype=np.int32)
        # how the repository's own restatement fares against the reference on this case (the tests assert it)
        mine, mine_idx = A.augment_clouds_host(raws, cfg, seed=seed, params=p, cylindrical='none', return_index=True)
        for i in range(len(raws)):
            gi, hi = out['%s.%d.idx' % (name, i)], mine_idx[i].numpy()
            common, ga, ha = np.intersect1d(gi, hi, return_indices=True)
            err = np.abs(out['%s.%d.pts' % (name, i)][ga].astype(np.float64) - mine[i].numpy()[ha]).max() if len(common) else 0.0
            print('%-10s cloud %d: n %5d kept %5d (restated %5d, differing %d) near %d k %d block %d flip %d  max |diff| %.3g'
                  % (name, i, sizes[i], len(gi), len(hi), len(np.setxor1d(gi, hi)), len(nears[i]), p.remove_k[i], p.block[i],
                     p.flip_axis, err))
    path = os.path.join(ROOT, 'tests', 'golden', 'augment.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
