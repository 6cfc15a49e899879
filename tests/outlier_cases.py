"""Clouds for the outlier-filter tests (`tests/test_outliers_host.py`, `tests/test_gpu_outliers.py`).  Everything is seeded
and float32."""
import numpy as np

from tests import ground_cases as gc

N_STRAYS = 40


def gauss(n: int, offset=(0.0, 0.0, 0.0), seed: int = 0) -> np.ndarray:
    """n Gaussian points, 8 m wide and 2 m high (one sigma), round `offset`"""
    return (np.random.default_rng(seed).standard_normal((n, 3)) * [8.0, 8.0, 2.0] + np.asarray(offset, np.float64)).astype(
        np.float32)


def forest_with_strays(seed: int = 0, size: float = 20.0):
    """the sparse forest of the cloth tests (4 300 points at 20 m) plus `N_STRAYS` uniform points 15 to 40 m above its floor,
    shuffled -> (points (n, 3) float32, is_stray (n,) bool)"""
    trees = gc.forest(seed, size=size, trunks_per_m2=10 / 400.0, blobs_per_m2=2 / 400.0)[0]
    rng = np.random.default_rng(seed + 1000)
    x, y = rng.uniform(0, size, N_STRAYS), rng.uniform(0, size, N_STRAYS)
    strays = np.stack([x, y, gc.surface(x, y) + rng.uniform(15.0, 40.0, N_STRAYS)], 1).astype(np.float32)
    pts = np.concatenate([trees, strays])
    is_stray = np.arange(pts.shape[0]) >= trees.shape[0]
    order = rng.permutation(pts.shape[0])
    return pts[order], is_stray[order]


def _lattice3() -> np.ndarray:
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(4), indexing='ij'), -1).reshape(-1, 3)
    return g.astype(np.float32)


def lattice_ties() -> np.ndarray:
    """a 12 x 12 x 4 unit lattice and one point at (30, 30, 30): many exactly equal distances at the k-th place"""
    return np.concatenate([_lattice3(), np.array([[30.0, 30.0, 30.0]], np.float32)])


def duplicates() -> np.ndarray:
    """the lattice and 25 more copies of each of its first three points: 78 points whose 20 nearest are all coincident
    (avg == 0)"""
    lat = _lattice3()
    return np.concatenate([lat, np.repeat(lat[:3], 25, axis=0)])


def flat(n: int = 700, seed: int = 3) -> np.ndarray:
    """points of one height: the search grid is one cell thick"""
    pts = gauss(n, seed=seed)
    pts[:, 2] = np.float32(1.5)
    return pts


def clump_and_far(seed: int = 5) -> np.ndarray:
    """500 points within a quarter of a metre and one point 50 m away, which no 3 x 3 x 3 block of a fine grid resolves"""
    rng = np.random.default_rng(seed)
    clump = rng.uniform(0.0, 0.25, (500, 3))
    return np.concatenate([clump, [[50.0, 0.1, 0.1]]]).astype(np.float32)


def trim_boundary_cloud():
    """rows exactly at r = 30 (coordinates exact in fp32), one fp32 ulp inside and outside it, and far on either side"""
    f = np.float32
    up, down = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(0)))
    rows = [(18, 24, 1), (-24, 18, -2), (30, 0, 5), (0, -30, 0),                      # at the radius: kept
            (down(30), 0, 1), (18, down(24), 2), (-down(18), -24, 3),                 # one ulp inside: kept
            (up(30), 0, 1), (18, up(24), 2), (-up(18), 24, 3), (0, -up(30), 9),       # one ulp outside: cut
            (0, 0, 100), (1, 2, 3), (40, 0, 0), (-25, -25, 0)]
    keep = [True] * 7 + [False] * 4 + [True, True, False, False]
    return np.array(rows, dtype=np.float32), np.array(keep)
