"""Shared inputs of the voxel tests (tests/test_voxel_host.py, tests/test_gpu_voxel.py): seeded raw clouds from the package's
counter-based hash (`synthetic.hash_uniform`), at the smallest shapes at which each path of csrc/voxel.hip can go wrong."""
import numpy as np

from hotformerloc_amd import synthetic as syn


def box_cloud(seed, n, extent=(20.0, 20.0, 20.0), offset=(0.0, 0.0, 0.0)):
    """n points uniform in a box of `extent` metres centred on `offset`, (n, 3) float32 (sum in float64, rounded once)"""
    u = syn.hash_uniform(seed, 3 * n).reshape(n, 3)
    return (u * (0.5 * np.asarray(extent, np.float64)) + np.asarray(offset, np.float64)).astype(np.float32)


def five_in_one_cell():
    """five points inside one cell of v = 1: origin = min - 0.5, every coordinate in [min, min + 0.3]"""
    return [np.array([[0.1, 0.2, 0.3], [0.4, 0.2, 0.3], [0.1, 0.5, 0.35], [0.25, 0.25, 0.6], [0.3, 0.3, 0.3]], np.float32)], 1.0


def single_point():
    return [np.array([[3.5, -2.25, 7.0]], np.float32)], 0.8


def ragged():
    """1, 257 and 4 099 points: chunk and workgroup tails, and the second cloud starts 12 bytes into a 16-byte line"""
    return [box_cloud(11, 1), box_cloud(12, 257), box_cloud(13, 4099)], 0.8


def quarter_grid(n=3000):
    """coordinates that are multiples of 0.25 in [-10, 10] with v = 0.5: every quotient (p - origin) / v is an exact integer
    or half-integer, so many points lie exactly on cell faces"""
    u = syn.hash_uniform(21, 3 * n).reshape(n, 3)
    return [(np.round(u * 40.0) * 0.25).astype(np.float32)], 0.5


def utm_offset(n=5000):
    """a 60 m forest submap moved by (3e5, 6e6, 50): fp32 spacing 0.03 m in x and 0.5 m in y"""
    return [syn.raw_submap(31, n, extent=60.0, offset=(3.0e5, 6.0e6, 50.0))], 0.8


def long_segment():
    """300 copies of one point plus 3 others"""
    p = np.array([[1.5, 2.5, -0.5]], np.float32).repeat(300, 0)
    others = np.array([[4.0, 2.5, -0.5], [1.5, 9.0, -0.5], [-3.0, -3.0, -3.0]], np.float32)
    return [np.concatenate([p[:100], others[:1], p[100:250], others[1:], p[250:]])], 0.8


SEGMENT_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 129, 200)


def threshold_segments():
    """cells with 1, 31, 32, 33, 63, 64, 65, 129 and 200 distinct members (v = 1): both sides of the length at which the
    reduction hands a segment to the whole wave, and of the wave size.  Cell k is centred on x = 10 k, members within
    +-0.2 of the centre, interleaved so that no cell's members are contiguous in the input."""
    pts, owner = [], []
    for k, ln in enumerate(SEGMENT_LENGTHS):
        j = syn.hash_uniform(40 + k, 3 * ln).reshape(ln, 3) * 0.2
        j[:, 0] += 10.0 * k
        pts.append(j)
        owner.append(np.full(ln, k))
    pts, owner = np.concatenate(pts), np.concatenate(owner)
    order = np.argsort(syn.hash_uniform(50, len(pts)), kind='stable')
    return [pts[order].astype(np.float32)], 1.0


def big_cloud(n=200000):
    """200 000 points in a 100 x 100 x 20 m box at v = 0.8: many workgroups for the bounds, a scan over ~100 blocks, and
    about 1.5e5 segments"""
    return [box_cloud(61, n, extent=(100.0, 100.0, 20.0))], 0.8


def with_outliers():
    """three clouds whose normalisation drops points: a 20 m box plus a few returns 150-250 m away"""
    out = []
    for i, (n, far) in enumerate(((900, 4), (2500, 7), (333, 1))):
        core = box_cloud(70 + i, n)
        tail = box_cloud(80 + i, far, extent=(100.0, 100.0, 20.0), offset=(200.0, -150.0, 5.0))
        out.append(np.concatenate([core[:n // 2], tail, core[n // 2:]]))
    return out, 0.8


def overflow_batch(v=0.8):
    """cloud 1 spans 70 001 cells along x (two points at 0 and 70 000 v); clouds 0 and 2 are ordinary"""
    wide = np.array([[0.0, 0.0, 0.0], [70000.0 * v, 0.0, 0.0]], np.float32)
    return [box_cloud(91, 50), wide, box_cloud(92, 70)], v


DOWNSAMPLE_CASES = {
    'five_in_one_cell': five_in_one_cell,
    'single_point': single_point,
    'ragged_1_257_4099': ragged,
    'quarter_grid_faces': quarter_grid,
    'utm_offset': utm_offset,
    'long_segment_300': long_segment,
    'threshold_segments': threshold_segments,
    'with_outliers': with_outliers,
    'big_200k': big_cloud,
}

# raw batches whose downsampled clouds the normalisation is tested on (a single point cannot be normalised)
NORMALISE_CASES = ('ragged_257_4099', 'quarter_grid_faces', 'with_outliers', 'big_200k')


def normalise_case(name):
    if name == 'ragged_257_4099':
        clouds, v = ragged()
        return clouds[1:], v
    return DOWNSAMPLE_CASES[name]()
