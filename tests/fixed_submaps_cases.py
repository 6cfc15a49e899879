"""Shared inputs of the fixed-size submap tests (tests/test_fixed_submaps_host.py, tests/test_gpu_fixed_submaps.py): seeded
raw clouds from the package's counter-based hash (`synthetic.hash_uniform`).  Lidar-like scenes: points on a ground plane
and two walls, a few clusters and a sparse halo, tens of metres across, so that the PointNetVLAD search crosses its target
at a voxel well below 3.001 m."""
import numpy as np

from hotformerloc_amd import synthetic as syn


def scene(seed, n, extent=40.0, offset=(0.0, 0.0, 0.0)):
    """(n, 3) float32: 50 % ground (z within 2 cm of 0), 20 % two walls, 25 % eight clusters of 1 m, 5 % halo; the sum with
    `offset` is formed in float64 and rounded once"""
    u = syn.hash_uniform(seed, 3 * n).reshape(n, 3)                               # in [-1, 1)
    half = 0.5 * extent
    p = np.empty((n, 3), np.float64)
    a, b, c = n // 2, n // 2 + n // 5, n - n // 20
    p[:a] = u[:a] * (half, half, 0.02)
    wall = u[a:b]
    p[a:b] = np.where((np.arange(b - a) % 2 == 0)[:, None],
                      np.stack([wall[:, 0] * half, np.full(b - a, 0.3 * half) + 0.01 * wall[:, 1], (wall[:, 2] + 1) * 0.1 * extent], 1),
                      np.stack([np.full(b - a, -0.4 * half) + 0.01 * wall[:, 0], wall[:, 1] * half, (wall[:, 2] + 1) * 0.08 * extent], 1))
    centres = syn.hash_uniform(seed + 1000, 24).reshape(8, 3) * (0.8 * half, 0.8 * half, 0.1 * extent) + (0, 0, 0.12 * extent)
    p[b:c] = centres[np.arange(c - b) % 8] + u[b:c]
    p[c:] = u[c:] * (half, half, 0.125 * extent) + (0, 0, 0.125 * extent)
    order = np.argsort(syn.hash_uniform(seed + 2000, n), kind='stable')           # no part contiguous in the input
    return (p[order] + np.asarray(offset, np.float64)).astype(np.float32)


def lattice(per_axis=4, members=6, spacing=3 * 3.001):
    """per_axis^3 groups of `members` points within 0.3 m, the groups 3 cells of v = 3.001 apart: exactly per_axis^3 cells
    are occupied at the first candidate of the search"""
    g = np.stack(np.meshgrid(*[np.arange(per_axis)] * 3, indexing='ij'), -1).reshape(-1, 3) * spacing
    j = (syn.hash_uniform(77, 3 * members * len(g)).reshape(len(g), members, 3) + 1.0) * 0.15
    j[0, 0] = 0.0                                                                 # the minimum sits on the first node
    return (g[:, None, :] + j).reshape(-1, 3).astype(np.float32)


def quarter_grid(n=3000):
    """coordinates that are multiples of 0.25 in [-10, 10]: at v = 0.5, 1 and 2 every quotient (p - origin) / v is an exact
    multiple of 1 / 8 (the origin is min - 0.5 v), so many points lie exactly on cell faces"""
    u = syn.hash_uniform(21, 3 * n).reshape(n, 3)
    return (np.round(u * 40.0) * 0.25).astype(np.float32)


FACE_SIZES = (0.5, 1.0, 2.0)

# (cloud id, sizes): 3.001 .. 1.0 fit the LDS bitmap (8 192 words = 262 144 cells), 0.25 and 0.11 of a 40 m scene do not
OCCUPANCY_SIZES = (3.001, 2.3409999999999998, 1.0, 0.5, 0.25, 0.11)


def occupancy_batch():
    """five ragged clouds: the second starts 4 bytes into a 16-byte line, the 20 000-point one takes three workgroups per
    candidate, one is UTM-sized, one is the lattice"""
    return [scene(1, 301, extent=30.0), scene(2, 20000), scene(3, 4099, extent=60.0, offset=(5.0e5, 6.9e6, 120.0)),
            lattice(), scene(4, 1025, extent=25.0)]


def general_1024():
    """target 1024 on 30 - 40 m scenes: phase one takes well over 64 steps (several rounds of the device search)"""
    return [scene(11, 6000, extent=30.0), scene(11, 20000, extent=40.0)], 1024


def general_256():
    return [scene(11, 2000, extent=20.0), scene(11, 777, extent=25.0), scene(13, 3001, extent=30.0)], 256


def utm_256():
    """the float64 cell arithmetic: x near 5e5 (fp32 spacing 0.03 m), y near 6.9e6 (0.5 m)"""
    return [scene(16, 5000, extent=20.0, offset=(5.0e5, 6.9e6, 80.0))], 256


def over_at_start_64():
    """a 30 m scene occupies more than 64 cells at v = 3.001: phase one takes no step, phase two hundreds"""
    return [scene(17, 1500, extent=30.0)], 64


def lattice_exact_64():
    """exactly 64 occupied cells at v = 3.001: no step in either phase, and nothing to pad"""
    return [lattice()], 64


EXACT_HIT_SEED = 101


def exact_hit_64():
    """a scene whose phase one ends on exactly 64 occupied cells after several steps (seed found by a CPU search)"""
    return [scene(EXACT_HIT_SEED, 400, extent=12.0)], 64


def mixed_rounds_64():
    """the lattice finishes in the first round of the device search, the 30 m scene needs many"""
    return [lattice(), scene(18, 3000, extent=30.0), scene(19, 333, extent=20.0)], 64


PNVLAD_CASES = {
    'general_1024': general_1024,
    'general_256': general_256,
    'utm_256': utm_256,
    'over_at_start_64': over_at_start_64,
    'lattice_exact_64': lattice_exact_64,
    'exact_hit_64': exact_hit_64,
    'mixed_rounds_64': mixed_rounds_64,
}
GENERAL_CASES = ('general_1024', 'general_256', 'utm_256')


def with_outliers(target=256):
    """raw clouds with returns 150 - 250 m away: the normalisation drops rows of the downsampled cloud and the padding loop
    draws some rows that it has to reject, so it runs more than once"""
    out = []
    for i, n in enumerate((2000, 900, 5000)):
        core = scene(30 + i, n, extent=30.0)
        k = n // 6
        far = (syn.hash_uniform(40 + i, 3 * k).reshape(k, 3) * (50.0, 50.0, 10.0) + (200.0, -150.0, 5.0)).astype(np.float32)
        out.append(np.concatenate([core[:n // 2], far, core[n // 2:]]))
    return out, target
