"""Shared inputs of the registration tests (tests/test_registration_host.py, tests/test_gpu_registration.py).

Targets are jittered cubic lattices: 1 m spacing, uniform jitter of +-0.2 m per coordinate, rows shuffled, centred on the
origin; 13^3 = 2197 or 17^3 = 4913 points, cut (or, past 4913, drawn from a larger lattice) to the wanted row count.  Two
lattice points are at least 0.6 m apart, so a source point within 0.3 m of its true target has that target as its nearest.
A source cloud is a subset of the target moved by the inverse of a known rigid G (a rotation about the axis (0.3, -0.5, 0.81)
and a shift), so ICP from the identity must find G.  Two families:

    exact   1 degree, 0.05 m, no noise, max_correspondence_distance 0.5: one update lands on G
    noisy   6 degrees, 0.3 m, Gaussian noise of sigma 0.02 m, max_correspondence_distance 1.0: several updates

`trace` replays `icp_refine_host` from the public single-step functions and ASSERTS at every iteration what lets a float32
route and a float64 route, or the device and the host, be compared for equality rather than approximately:
  * every nearest / second-nearest gap exceeds GAP (1e-5 m): the routes' coordinates differ by a few float32 ulps (4e-6 m at
    16 m), which cannot reorder candidates that far apart;
  * every distance is more than DIST_RTOL (1e-6) x max_correspondence_distance away from it: no inlier flag can flip;
  * the rmse change that the CONVERGED rule compares with 1e-6 is outside [0.5e-6, 2e-6]: the routes' rmse differ by far less
    than 5e-7 (the same float32 coordinates, float64 sums in another order), so they stop at the same iteration.
Under these guards no comparison is skipped."""
import numpy as np

from hotformerloc_amd import icp_correspondences_host, kabsch_update_host
from hotformerloc_amd import registration as reg

AXIS = np.array([0.3, -0.5, 0.81])
SHIFT_DIR = np.array([0.6, -0.64, 0.48])                               # a unit vector
GAP = 1e-5                             # metres between the nearest and the second-nearest target
DIST_RTOL = 1e-6                       # as tests/overlap_cases.py
EXACT = dict(deg=1.0, shift=0.05, noise=0.0, max_dist=0.5)
NOISY = dict(deg=6.0, shift=0.3, noise=0.02, max_dist=1.0)


def lattice(side, seed, jitter=0.2):
    """side^3 float32 points of a jittered unit lattice centred on the origin, rows shuffled"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    g = g - (side - 1) / 2 + rng.uniform(-jitter, jitter, g.shape)
    rng.shuffle(g)
    return g.astype(np.float32)


def target(rows, seed=1):
    """`rows` lattice points: the first rows of the 13^3 lattice, of the 17^3 one, or of the smallest larger one"""
    side = 13 if rows <= 13 ** 3 else 17
    while side ** 3 < rows:
        side += 4
    return np.ascontiguousarray(lattice(side, seed)[:rows])


def rigid(deg, shift):
    """4 x 4 float64: a rotation by `deg` degrees about AXIS (Rodrigues) and a translation of `shift` metres along SHIFT_DIR"""
    k = AXIS / np.linalg.norm(AXIS)
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.radians(deg)
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(a) * kx + (1.0 - np.cos(a)) * (kx @ kx)
    m[:3, 3] = shift * SHIFT_DIR
    return m


def source_of(dst, rows, g, seed, noise=0.0):
    """`rows` points of `dst` (a seeded subset, with repetition only where rows > len(dst)) moved by inv(g), plus noise"""
    rng = np.random.default_rng(seed)
    sel = rng.permutation(len(dst))[:rows] if rows <= len(dst) else rng.integers(0, len(dst), rows)
    gi = np.linalg.inv(g)
    moved = dst[sel].astype(np.float64) @ gi[:3, :3].T + gi[:3, 3]
    if noise:
        moved = moved + rng.normal(0.0, noise, moved.shape)
    return moved.astype(np.float32)


def pair(family, rows_s=1025, rows_t=2197, seed=2):
    """(source, target, G, max_correspondence_distance) of one family"""
    dst = target(rows_t)
    g = rigid(family['deg'], family['shift'])
    return source_of(dst, rows_s, g, seed, family['noise']), dst, g, family['max_dist']


def far_points(count, seed):
    """points some 40 m off the lattice: outliers at any distance the tests use"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, (count, 3)) * 3.0 + 40.0).astype(np.float32)


def two_nearest(moved, dst):
    """float64 (nearest, second nearest) distances of every row of `moved` in `dst` (second = +inf for a single target)"""
    d = np.sqrt(((moved.astype(np.float64)[:, None, :] - dst.astype(np.float64)[None, :, :]) ** 2).sum(-1))
    if d.shape[1] < 2:
        return d[:, 0], np.full(d.shape[0], np.inf)
    part = np.partition(d, 1, axis=1)
    return part[:, 0], part[:, 1]


def trace(src, dst, max_dist, init=None, max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, min_correspondences=3):
    """`icp_refine_host` of one pair replayed from `icp_correspondences_host` and `kabsch_update_host`, with the guards of the
    module's docstring asserted at every iteration.  Returns dict(transform, fitness, rmse, iterations, status, history), the
    history holding (fitness, rmse, idx, inlier) of every evaluation."""
    pose = np.eye(4) if init is None else np.array(init, np.float64)
    history, prev, status = [], None, reg.RUNNING
    for k in range(max_iterations + 1):
        dist, idx, inl, sums = icp_correspondences_host([src], [dst], pose[None], max_dist)
        if len(src) and len(dst):
            moved = reg._host_move(src, pose[:3])
            first, second = two_nearest(moved, dst)
            assert (second - first > GAP).all(), 'iteration %d: a nearest / second-nearest gap of %.3g m' % (k, (second - first).min())
            assert (np.abs(first - max_dist) > DIST_RTOL * max_dist).all(), 'iteration %d: a distance at the threshold' % k
            assert (np.abs(dist.astype(np.float64) - first) <= 1e-6 * first + 1e-12).all()
        n = sums[0, 0]
        fitness = n / len(src) if len(src) else float('nan')
        rmse = float(np.sqrt(sums[0, 16] / n)) if n >= max(min_correspondences, 1) else float('nan')
        history.append((fitness, rmse, idx, inl))
        if n < min_correspondences:
            status = reg.TOO_FEW
            break
        if k >= 1 and abs(fitness - prev[0]) < relative_fitness:
            step = abs(rmse - prev[1])
            assert not 0.5 * relative_rmse <= step <= 2.0 * relative_rmse, 'iteration %d: rmse step %.3g at the threshold' % (k, step)
            if step < relative_rmse:
                status = reg.CONVERGED
                break
        if k == max_iterations:
            status = reg.MAX_ITERATIONS
            break
        r, t, solved = kabsch_update_host(sums, min_correspondences)
        if solved[0] != reg.RUNNING:
            status = int(solved[0])
            break
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = r[0], t[0]
        pose = step @ pose
        prev = (fitness, rmse)
    return dict(transform=pose, fitness=fitness, rmse=rmse, iterations=k, status=status, history=history)


def sums_of(p, q):
    """the 17 sums of given correspondences p -> q, (n, 3) float64 each"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    d2 = ((p - q) ** 2).sum()
    return np.concatenate([[p.shape[0]], p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).reshape(9), [d2]])


def kabsch_by_svd(s):
    """the update of one pair's sums by `numpy.linalg.svd`: (R, t)"""
    n = s[0]
    sp, sq = s[1:4], s[4:7]
    h = s[7:16].reshape(3, 3) - np.outer(sp, sq) / n
    u, _, vt = np.linalg.svd(h)
    r = vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ u.T))]) @ u.T
    return r, sq / n - r @ (sp / n)


def kabsch_cases(seed=11):
    """(sums (K, 17), kind (K,) of str): 'rigid' random clouds under a random rigid motion plus noise; 'mirror' a cloud and
    its mirror image (the unconstrained optimum is a reflection); 'planar' the same within the plane z = 0, where H has rank 2
    and a proper rotation still fits exactly; 'line' collinear points (DEGENERATE); 'few' two points (TOO_FEW)."""
    rng = np.random.default_rng(seed)
    rows, kinds = [], []
    for i in range(6):
        p = rng.normal(0.0, 4.0, (40 + 7 * i, 3)) + rng.uniform(-5.0, 5.0, 3)
        g = rigid(rng.uniform(-170.0, 170.0), rng.uniform(0.0, 3.0))
        rows.append(sums_of(p, p @ g[:3, :3].T + g[:3, 3] + rng.normal(0.0, 0.05, p.shape)))
        kinds.append('rigid')
    p = rng.normal(0.0, 3.0, (60, 3)) * [1.0, 0.7, 0.4]
    rows.append(sums_of(p, p * [-1.0, 1.0, 1.0] + rng.normal(0.0, 0.01, p.shape)))
    kinds.append('mirror')
    p = rng.normal(0.0, 3.0, (60, 3)) * [1.0, 0.6, 0.0]
    rows.append(sums_of(p, (p + rng.normal(0.0, 0.01, p.shape) * [1.0, 1.0, 0.0]) * [-1.0, 1.0, 1.0]))
    kinds.append('planar')
    s = rng.uniform(-4.0, 4.0, (30, 1))
    p = s * np.array([[1.0, 2.0, -0.5]])
    rows.append(sums_of(p, p))
    kinds.append('line')
    p = rng.normal(0.0, 1.0, (2, 3))
    rows.append(sums_of(p, p))
    kinds.append('few')
    return np.stack(rows), np.array(kinds)
