"""What the augmentation tests share: the golden cases of tests/golden/augment.npz (`tools/gen_golden_augment.py`) and the
comparison rule of both test files.

The rule.  Coordinates are compared at 1e-6 absolute in the cartesian stages: between the input and a decision there are at
most 8 float32 roundings of quantities below 1.5 in magnitude (the jitter add, a 3-term dot product whose summation order and
FMA use torch's CPU matmul does not fix, the translation add, the batch-wide rotation), 8 * 2^-23 = 9.5e-7.  A point may be
left out only if the golden lists it as `near`: in the reference's run a coordinate that feeds a decision lay within 1e-6 of
that decision's boundary.  The generator capped `near` at 0.5 % of every cloud."""
import functools
import json
import os

import numpy as np

from hotformerloc_amd import augment as A
from oracle.gen_golden_coords import raw_cloud

TOL = 1.0e-6
CAP = 0.005
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment.npz')
CASE_NAMES = ('a1_s1', 'a1_s2', 'a2_s1', 'a2_s2', 'raw_a2_s1', 'cyl_a2_s1')


class Case:
    def __init__(self, g, name):
        c = json.loads(str(g[name + '.cfg']))
        self.name = name
        self.cfg = A.AugmentConfig.from_training_params(c['aug_mode'], c['set_aug_mode'], c['random_rot_theta'],
                                                        c['normalize_points'], c['coordinates'])
        self.seed = int(c['seed'])
        self.raws = [raw_cloud(s, n, kind, tuple(ext), tuple(off)) for s, n, kind, ext, off in c['clouds']]
        self.params = A.AugmentParams.from_arrays(g, name + '.p.')
        self.pts = [g['%s.%d.pts' % (name, i)] for i in range(len(self.raws))]
        self.idx = [g['%s.%d.idx' % (name, i)] for i in range(len(self.raws))]
        self.near = [g['%s.%d.near' % (name, i)] for i in range(len(self.raws))]
        self.near_count = g[name + '.near_count']


@functools.lru_cache(maxsize=None)
def cases():
    g = np.load(GOLDEN)
    return {n: Case(g, n) for n in CASE_NAMES}


def compare(want_pts, want_idx, got_pts, got_idx, near, n, what, tol=TOL):
    """Kept sets equal and coordinates within `tol`, leaving out at most the points of `near` (and never more than CAP * n)."""
    want_idx, got_idx = np.asarray(want_idx), np.asarray(got_idx)
    near = np.asarray(near)
    assert len(near) <= CAP * n, (what, len(near), n)
    differ = np.setxor1d(want_idx, got_idx)
    assert np.isin(differ, near).all(), (what, 'kept sets differ away from every boundary', differ[:8])
    common, wa, ga = np.intersect1d(want_idx, got_idx, return_indices=True)
    take = ~np.isin(common, near)
    err = np.abs(np.asarray(want_pts, dtype=np.float64)[wa][take] - np.asarray(got_pts, dtype=np.float64)[ga][take])
    worst = float(err.max()) if err.size else 0.0
    print('%s: kept %d / %d, left out %d, max |diff| %.3g' % (what, len(got_idx), n, int((~take).sum()) + len(differ), worst))
    assert worst <= tol, (what, worst)
