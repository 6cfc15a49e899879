"""Scenes for the cloth-filter tests (`tests/test_ground_host.py`, `tests/test_gpu_ground.py`): small clouds whose answer is
known by hand, and a synthetic forest whose truth is known by construction.  Everything is seeded and float32."""
import numpy as np


def lattice(nx: int = 8, ny: int = 8, z: float = 3.0, step: float = 1.0) -> np.ndarray:
    """points on the lattice x in {0..nx-1} step, y in {0..ny-1} step at height z"""
    xs, ys = np.meshgrid(np.arange(nx, dtype=np.float32) * np.float32(step), np.arange(ny, dtype=np.float32) * np.float32(step))
    return np.stack([xs.ravel(), ys.ravel(), np.full(nx * ny, z, np.float32)], 1).astype(np.float32)


ELEVATED_HEIGHTS = (0.25, 0.5, 0.75, 4.0)


def lattice_with_elevated() -> np.ndarray:
    """the 8 x 8 lattice at z = 3 and, after it, four points off the lattice at `ELEVATED_HEIGHTS` above it (all values are
    exact in fp32, and so are the cloth heights: the cloth lies at u = -3 everywhere)"""
    xy = np.array([[2.5, 3.5], [4.5, 1.5], [5.5, 5.5], [1.5, 6.5]], np.float32)
    z = np.float32(3.0) + np.array(ELEVATED_HEIGHTS, np.float32)
    return np.concatenate([lattice(), np.concatenate([xy, z[:, None]], 1)]).astype(np.float32)


def block_scene(n: int = 30, lo: int = 10, size: int = 9, height: float = 20.0, ground: float = 0.0) -> np.ndarray:
    """an n x n lattice at z = `ground` with a size x size block of cells raised by `height`: under the inverted cloth the
    block is a pit the cloth hangs over"""
    pts = lattice(n, n, ground)
    inside = (pts[:, 0] >= lo) & (pts[:, 0] < lo + size) & (pts[:, 1] >= lo) & (pts[:, 1] < lo + size)
    pts[inside, 2] += np.float32(height)
    return pts


def surface(x, y):
    """the forest floor"""
    return 0.04 * x + 1.5 * np.sin(x / 12.0) * np.cos(y / 17.0)


def forest(seed: int = 0, size: float = 40.0, density: float = 8.0, trunks_per_m2: float = 60 / 1600.0,
           blobs_per_m2: float = 24 / 1600.0):
    """A seeded size x size metre scene -> (points (n, 3) float32, shuffled; is_ground (n,) bool: generated on the surface;
    is_object (n,) bool: at least 1.5 m above the surface).  The points in neither set (the lowest 1.5 m of the trunks)
    are not judged.  Surface: `surface` at `density` points per square metre with noise of at most +-0.03; trunks of radius
    0.25 m and height 6 m; canopy blobs of radius 2 m at 8 m above the floor."""
    rng = np.random.default_rng(seed)
    n_floor = int(round(size * size * density))
    fx, fy = rng.uniform(0, size, n_floor), rng.uniform(0, size, n_floor)
    floor = np.stack([fx, fy, surface(fx, fy) + rng.uniform(-0.03, 0.03, n_floor)], 1)
    parts, height = [floor], [np.zeros(n_floor)]
    for _ in range(int(round(size * size * trunks_per_m2))):
        cx, cy = rng.uniform(1, size - 1, 2)
        ang, h = rng.uniform(0, 2 * np.pi, 80), rng.uniform(0, 6, 80)
        x, y = cx + 0.25 * np.cos(ang), cy + 0.25 * np.sin(ang)
        parts.append(np.stack([x, y, surface(cx, cy) + h], 1))
        height.append(parts[-1][:, 2] - surface(x, y))
    for _ in range(int(round(size * size * blobs_per_m2))):
        cx, cy = rng.uniform(2, size - 2, 2)
        d = rng.normal(size=(150, 3))
        d *= (2.0 * rng.uniform(0, 1, 150) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        x, y = cx + d[:, 0], cy + d[:, 1]
        parts.append(np.stack([x, y, surface(cx, cy) + 8.0 + d[:, 2]], 1))
        height.append(parts[-1][:, 2] - surface(x, y))
    pts, height = np.concatenate(parts), np.concatenate(height)
    is_ground = np.arange(pts.shape[0]) < n_floor
    order = rng.permutation(pts.shape[0])
    pts, height, is_ground = pts[order].astype(np.float32), height[order], is_ground[order]
    return pts, is_ground, (~is_ground) & (height >= 1.5)


def forest_shares(keep_mask, is_ground, is_object):
    """(share of the judged surface points called ground, share of the judged object points kept)"""
    keep_mask = np.asarray(keep_mask, dtype=bool)
    return float((~keep_mask)[is_ground].mean()), float(keep_mask[is_object].mean())
