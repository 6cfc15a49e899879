"""Clouds and helpers of the normal-estimation and point-to-plane tests (`tests/test_normals_host.py`,
`tests/test_gpu_normals.py`, `tests/test_gpu_registration_plane.py`).  Everything is seeded and float32.

The device tests compare a normal only where the host's eigenvalues say it is determined: GAP = 1e-6 <
(l1 - l0) / l2.  `undetermined_share` is the share of a cloud's points that have a normal but miss that; the clouds here
are chosen so that it stays at or below MAX_SHARE = 1 %, which the tests assert."""
import numpy as np

from hotformerloc_amd import synthetic as syn
from tests import registration_cases as rc

GAP = 1e-6
MAX_SHARE = 0.01


def tilted_plane(side=24, a=0.3, b=-0.2, c=1.5, seed=0):
    """side^2 points of the plane z = a x + b y + c on a unit grid jittered by +-0.3, rows shuffled: noise-free but for the
    float32 rounding of z"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 2).astype(np.float64)
    g = (g - (side - 1) / 2 + rng.uniform(-0.3, 0.3, g.shape)).astype(np.float32).astype(np.float64)
    z = a * g[:, 0] + b * g[:, 1] + c
    pts = np.concatenate([g, z[:, None]], 1)
    rng.shuffle(pts)
    return pts.astype(np.float32)


def noisy_plane(n, seed=0, noise=0.02, offset=(0.0, 0.0, 0.0)):
    """n points of a tilted plane, uniform over 10 m x 10 m, with Gaussian noise of sigma `noise` along every axis"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-5.0, 5.0, (n, 2))
    z = 0.25 * xy[:, 0] - 0.4 * xy[:, 1] + 2.0
    return (np.concatenate([xy, z[:, None]], 1) + rng.normal(0.0, noise, (n, 3)) + np.asarray(offset)).astype(np.float32)


def sphere_shell(n=2000, seed=0, radius=6.0, noise=0.01):
    """n points of a sphere of `radius` round (3, -2, 1), radial noise of sigma `noise`"""
    rng = np.random.default_rng(seed)
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (radius + rng.normal(0.0, noise, (n, 1))) + [3.0, -2.0, 1.0]).astype(np.float32)


def forest(n=3000, seed=7):
    """the variable-density 'forest' of `synthetic.forest_cloud` stretched to 40 m"""
    return (syn.forest_cloud(seed, n).astype(np.float64) * 20.0).astype(np.float32)


def tie_lattice():
    """a 10 x 10 x 3 lattice of spacing (1, 1, 0.5) -- every distance exact in fp32, so many are exactly equal at the k-th
    place -- and one point at (30, 30, 30)"""
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(3), indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    return np.concatenate([g * [1.0, 1.0, 0.5], [[30.0, 30.0, 30.0]]]).astype(np.float32)


def duplicated(seed=3):
    """a noisy plane of 600 points, 40 more copies of its first point and 2 more of each of its next five"""
    p = noisy_plane(600, seed)
    return np.concatenate([p, np.repeat(p[:1], 40, axis=0), np.repeat(p[1:6], 2, axis=0)])


def plane_and_far(seed=5):
    """a noisy plane of 500 points and one point 60 m away, which no 3 x 3 x 3 block of the default grid resolves"""
    return np.concatenate([noisy_plane(500, seed), [[60.0, 1.0, 2.0]]]).astype(np.float32)


def collinear(n=40, seed=1):
    t = np.random.default_rng(seed).uniform(-4.0, 4.0, (n, 1))
    return (t * np.array([[1.0, 2.0, -0.5]])).astype(np.float32)


def undetermined_share(normals, eigenvalues):
    """the share of the points with a normal whose host eigenvalues miss (l1 - l0) / l2 > GAP, and the mask of those that
    pass it"""
    has = (normals != 0).any(1)
    with np.errstate(all='ignore'):
        sure = has & ((eigenvalues[:, 1] - eigenvalues[:, 0]) / eigenvalues[:, 2] > GAP)
    return float((has & ~sure).sum()) / max(int(normals.shape[0]), 1), sure


# ------------------------------------------------------------------------------------------ the corner of three planes
def _corner_points(n_per_face, rng, noise):
    """three mutually non-parallel faces (z = 0.1 x, x = 0.15 y, y = -0.1 z) over [0, 8]^2 each, Gaussian noise of sigma
    `noise` along the face's own axis -> (points float64, the faces' unit normals per point)"""
    faces, normals = [], []
    for axis, (slope_axis, slope) in enumerate(((0, 0.1), (1, 0.15), (2, -0.1))):
        height_axis = (2, 0, 1)[axis]
        u = rng.uniform(0.0, 8.0, (n_per_face, 3))
        u[:, height_axis] = slope * u[:, slope_axis] + rng.normal(0.0, noise, n_per_face)
        nrm = np.zeros(3)
        nrm[height_axis], nrm[slope_axis] = 1.0, -slope
        faces.append(u)
        normals.append(np.tile(nrm / np.linalg.norm(nrm), (n_per_face, 1)))
    return np.concatenate(faces), np.concatenate(normals)


def corner_pair(n_source=900, n_target=1500, seed=0, noise=0.01, deg=3.0, shift=0.15):
    """(source, target, G): a target sampled on three noisy planes that meet in a corner, and a source sampled at DIFFERENT
    positions on the same planes and moved by inv(G), G = `registration_cases.rigid(deg, shift)`: registration from the
    identity must find G.  The point spacing (about 0.35 m) is far above the noise, so the nearest target of a source point
    is another place on the surface: the case point-to-plane is made for."""
    rng = np.random.default_rng(seed)
    dst, _ = _corner_points(n_target // 3, rng, noise)
    src, _ = _corner_points(n_source // 3, rng, noise)
    g = rc.rigid(deg, shift)
    gi = np.linalg.inv(g)
    return (src @ gi[:3, :3].T + gi[:3, 3]).astype(np.float32), dst.astype(np.float32), g


def pose_errors(transform, g):
    """(rotation error in degrees, translation error in metres) of a 4 x 4 estimate against the truth"""
    delta = np.asarray(transform, np.float64) @ np.linalg.inv(g)
    cos = np.clip((np.trace(delta[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(cos))), float(np.linalg.norm(delta[:3, 3]))


# ------------------------------------------------------------------------------------------ the 6 x 6 solve
def plane_sums_of(p, q, n):
    """the 29 sums of given correspondences p -> q with the normals n at q, (m, 3) float64 each, by matrix products"""
    p, q, n = (np.asarray(x, np.float64) for x in (p, q, n))
    r = ((p - q) * n).sum(1)
    jac = np.concatenate([np.cross(p, n), n], 1)
    a = jac.T @ jac
    return np.concatenate([[p.shape[0]], [((p - q) ** 2).sum()], jac.T @ r, a[np.triu_indices(6)]])


def system_of(sums):
    """(A (6, 6), g (6,)) of one pair's 29 sums"""
    a = np.zeros((6, 6))
    a[np.triu_indices(6)] = sums[8:]
    return a + np.triu(a, 1).T, np.asarray(sums[2:8], np.float64)


def scaled_cond(a):
    """cond_2 of D A D, D = diag(A)^(-1/2)"""
    d = 1.0 / np.sqrt(np.diag(a))
    return float(np.linalg.cond(a * d[:, None] * d[None, :]))


def rotation_of(x):
    """Rz(gamma) Ry(beta) Rx(alpha) by three matrix products"""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rz = np.array([[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx


def plane_cases(seed=21):
    """(sums (K, 29), kind (K,) of str): 'corner' correspondences on three planes under a small rigid motion plus noise;
    'parallel' all normals parallel (A has rank 3: DEGENERATE); 'few' four correspondences (TOO_FEW at the default 6)."""
    rng = np.random.default_rng(seed)
    rows, kinds = [], []
    for i in range(6):
        q, n = _corner_points(60 + 9 * i, rng, 0.01)
        g = rc.rigid(rng.uniform(-4.0, 4.0), rng.uniform(0.0, 0.2))
        gi = np.linalg.inv(g)
        rows.append(plane_sums_of(q @ gi[:3, :3].T + gi[:3, 3] + rng.normal(0.0, 0.005, q.shape), q, n))
        kinds.append('corner')
    q = rng.uniform(0.0, 8.0, (80, 3)) * [1.0, 1.0, 0.0]
    rows.append(plane_sums_of(q + rng.normal(0.0, 0.01, q.shape), q, np.tile([0.0, 0.0, 1.0], (80, 1))))
    kinds.append('parallel')
    q, n = _corner_points(2, rng, 0.01)
    rows.append(plane_sums_of(q[:4] + 0.01, q[:4], n[:4]))
    kinds.append('few')
    return np.stack(rows), np.array(kinds)
