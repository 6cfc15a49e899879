"""`hotformerloc_amd.augment.augment_clouds` (HIP, one launch per batch) against the repository's host restatement
(`augment_clouds_host`, same Philox streams) and against goldens produced by the reference's own classes
(`tools/gen_golden_augment.py`).  The comparison rule and its 1e-6 bound are in tests/augment_cases.py.

Device against host there is no reference run to say which points sat near a boundary, so `near` is taken from the host
restatement's own coordinates in front of the masks (|c| = 1, |xy| = 1) and in front of the block (its edges), at the same
1e-6 and under the same 0.5 % cap.  The set removed by RemoveRandomPoints is integer work (Philox, radix select): identical."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from augment_cases import CASE_NAMES, TOL, cases, compare
from hotformerloc_amd import _native, build_batch_octree, ops, training
from hotformerloc_amd import augment as A
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.preprocess import prepare_clouds

SIZES = (1, 3, 63, 64, 65, 1023, 1024, 1025, 4096)
ULP = 2.0 ** -23


def _cloud(seed, n):
    return (syn.unit_ball_cloud(seed, n).astype(np.float64) * (30.0, 20.0, 8.0) + (5.0, -3.0, 1.0)).astype(np.float32)


def _host_near(raw, cfg, params, i, seed, cloud_id, keys=None):
    """Host chain of one cloud with its stages, and the points within TOL of one of its decision boundaries."""
    st = {}
    pts, idx = A.augment_cloud_host(raw, cfg, params, i, seed, cloud_id, keys, cylindrical=False, stages=st)
    p = st['pre_mask'].astype(np.float64)
    near = (np.abs(np.abs(p) - 1.0) <= TOL).any(axis=1)
    if cfg.coordinates == 'cylindrical':
        near |= np.abs(np.hypot(p[:, 0], p[:, 1]) - 1.0) <= TOL
    if cfg.aug_mode != 0 and int(params.block[i]):
        # in front of the block a point is where it ends up unless the block zeroed it: rebuild that stage
        only = A.AugmentParams.from_arrays(params.to_arrays())
        only.block = np.zeros_like(params.block)
        st2 = {}
        A.augment_cloud_host(raw, cfg, only, i, seed, cloud_id, keys, cylindrical=False, stages=st2)
        q = st2['pre_mask'].astype(np.float64)
        x0, x1, y0, y1 = (float(v) for v in A.block_rectangle(st2['pre_mask'], params.block_u[i]))
        for lo, hi, a in ((x0, x1, 0), (y0, y1, 1)):
            near |= (np.abs(q[:, a] - lo) <= TOL) | (np.abs(q[:, a] - hi) <= TOL)
    return pts, idx, np.nonzero(near)[0], st


def _removed_on_device(raw, k, seed, cloud_base=0, keys=None):
    """Which points the kernel's RemoveRandomPoints zeroed, and how many points came out.  The cloud is shrunk into
    |c| < 0.36 and taken without normalisation, rotation or block, with a translation that keeps every point inside the cube
    and that no jittered point can equal: the removed points are the output rows that equal the translation exactly."""
    cfg = A.AugmentConfig.from_training_params(1, 0, 0.0, False, 'cartesian')
    p = A.identity_params([len(raw)])
    p.remove_k[0] = k
    p.trans[0] = (0.5, 0.25, 0.125)
    pts, idx = A.augment_clouds([raw * np.float32(0.01)], cfg, seed=seed, params=p, cloud_base=cloud_base, return_index=True,
                                selection_keys=None if keys is None else [keys])
    pts, idx = pts[0].cpu().numpy(), idx[0].cpu().numpy()
    hit = (pts == np.array([0.5, 0.25, 0.125], np.float32)).all(axis=1)
    return np.sort(idx[hit]), len(idx)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_device_against_host_and_golden(name):
    c = cases()[name]
    pts, idx = A.augment_clouds(c.raws, c.cfg, seed=c.seed, params=c.params, cylindrical='none', return_index=True)
    for i, raw in enumerate(c.raws):
        assert pts[i].is_cuda and pts[i].dtype == torch.float32 and idx[i].dtype == torch.int32
        got, gi = pts[i].cpu().numpy(), idx[i].cpu().numpy()
        assert (np.diff(gi) > 0).all()                                            # order-preserving compaction
        compare(c.pts[i], c.idx[i], got, gi, c.near[i], len(raw), 'golden %s cloud %d' % (name, i))
        want, wi, near, _ = _host_near(raw, c.cfg, c.params, i, c.seed, i)
        compare(want, wi, got, gi, near, len(raw), 'host %s cloud %d' % (name, i))


@pytest.mark.parametrize('aug_mode, coords', [(1, 'cartesian'), (2, 'cylindrical')])
def test_device_against_host_at_every_size(aug_mode, coords):
    cfg = A.AugmentConfig.from_training_params(aug_mode, 1, 180.0, True, coords)
    raws = [_cloud(900 + n, n) for n in SIZES]
    params = A.draw_params(SIZES, cfg, torch.Generator().manual_seed(21))
    params.block[:] = [0, 1] * 4 + [1]
    params.remove_k[:] = [0, 0, 6, 1, 3, 102, 51, 7, 409]                         # <= 0.1 n each
    pts, idx = A.augment_clouds(raws, cfg, seed=1234, params=params, cylindrical='none', return_index=True)
    for i, raw in enumerate(raws):
        want, wi, near, _ = _host_near(raw, cfg, params, i, 1234, i)
        compare(want, wi, pts[i].cpu().numpy(), idx[i].cpu().numpy(), near, len(raw), 'n=%d' % len(raw))


@pytest.mark.parametrize('n', SIZES)
def test_removed_set_is_identical(n):
    raw = _cloud(950 + n, n)
    for k in sorted({0, n // 10, n // 3, n}):
        got, kept = _removed_on_device(raw, k, seed=77, cloud_base=5)
        want = A.select_removed(A.philox_selection_keys(n, 77, 5), k)
        assert kept == n and np.array_equal(got, want), (n, k)


def test_aug_mode_0_is_prepare_clouds_bit_for_bit():
    raws = [_cloud(960 + n, n) for n in (3, 65, 1025, 4096)]
    for coords in ('cartesian', 'cylindrical'):
        for normalize in (True, False):
            src = raws if normalize else [syn.unit_ball_cloud(970 + i, len(r)) * np.float32(1.2) for i, r in enumerate(raws)]
            cfg = A.AugmentConfig.from_training_params(0, 0, 180.0, normalize, coords)
            a = A.augment_clouds(src, cfg, seed=3)
            b = prepare_clouds(src, coordinates=coords, normalize=normalize)
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), (coords, normalize)


def test_tie_rule_through_selection_keys():
    raw = _cloud(980, 40)
    got, _ = _removed_on_device(raw, 5, seed=1, keys=np.zeros(40, np.uint32))
    assert got.tolist() == [0, 1, 2, 3, 4]
    got, _ = _removed_on_device(raw, 5, seed=1, keys=np.full(40, 0xFFFFFFFF, np.uint32))
    assert got.tolist() == [0, 1, 2, 3, 4]
    raw = _cloud(981, 1025)
    keys = (np.arange(1025) % 4).astype(np.uint32)                                # classes of 257, 256, 256, 256 points
    for k in (256, 257, 258, 512, 513, 514, 1024):                                # below, on and above a class boundary
        got, _ = _removed_on_device(raw, k, seed=1, keys=keys)
        assert np.array_equal(got, A.select_removed(keys, k)), k
    wide = (keys << np.uint32(24)) | np.uint32(0x00ABCDEF)                        # the classes differ in the first pass only
    got, _ = _removed_on_device(raw, 300, seed=1, keys=wide)
    assert np.array_equal(got, A.select_removed(wide, 300))
    for k in (0, 1025):
        got, kept = _removed_on_device(raw, k, seed=1, keys=keys)
        assert len(got) == k and kept == 1025
    one = _cloud(982, 1)
    for k in (0, 1):
        got, kept = _removed_on_device(one, k, seed=1, keys=np.array([7], np.uint32))
        assert got.tolist() == list(range(k)) and kept == 1


def test_batch_independence_and_determinism():
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cartesian')
    raws = [_cloud(990, 700), _cloud(991, 1500), _cloud(992, 65)]
    params = A.draw_params([700, 1500, 65], cfg, torch.Generator().manual_seed(8))
    params.block[:] = 1
    inputs = [torch.from_numpy(r.copy()) for r in raws]
    batch = A.augment_clouds(inputs, cfg, seed=42, params=params, cloud_base=10)
    assert all(np.array_equal(t.numpy(), r) for t, r in zip(inputs, raws))        # the input is not modified
    for j in range(3):
        alone = A.augment_clouds([raws[j]], cfg, seed=42, params=params.slice(j, j + 1), cloud_base=10 + j)[0]
        assert torch.equal(alone, batch[j]), j
    again = A.augment_clouds(raws, cfg, seed=42, params=params, cloud_base=10)
    assert all(torch.equal(x, y) for x, y in zip(again, batch))
    other = A.augment_clouds(raws, cfg, seed=43, params=params, cloud_base=10)
    assert not any(x.shape == y.shape and torch.equal(x, y) for x, y in zip(other, batch))
    dev_in = torch.from_numpy(raws[1]).cuda()
    keep = dev_in.clone()
    A.augment_clouds([dev_in], cfg, seed=42, params=params.slice(1, 2))
    assert torch.equal(dev_in, keep)


def test_cylindrical_device_against_host_mode():
    c = cases()['cyl_a2_s1']
    dev = A.augment_clouds(c.raws, c.cfg, seed=c.seed, params=c.params, cylindrical='device')
    host = A.augment_clouds(c.raws, c.cfg, seed=c.seed, params=c.params, cylindrical='host')
    for a, b in zip(dev, host):
        assert a.shape == b.shape                                                  # the same counts
        a, b = a.cpu().numpy(), b.cpu().numpy().astype(np.float64)
        d = np.abs(a - b)
        d[:, 1] = np.minimum(d[:, 1], 2.0 - d[:, 1])                               # phi on the circle
        assert np.array_equal(a[:, 2], b[:, 2].astype(np.float32)) and d.max() <= 3 * ULP, d.max()
        assert np.abs(a).max() <= 1.0


def test_feeds_the_octree_build_and_split_size_does_not_matter():
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cylindrical')
    raws = [_cloud(1000 + i, n) for i, n in enumerate((1200, 65, 2000, 700, 1025))]
    params = A.draw_params([len(r) for r in raws], cfg, torch.Generator().manual_seed(4))
    whole = A.augment_clouds(raws, cfg, seed=6, params=params)
    octree = build_batch_octree(whole, 7, 2, 'cuda')
    assert int(octree.nnum_nempty[7]) > 0 and octree.batch_size == 5
    a = training.make_training_minibatches(raws, 2, cfg, 7, 2, seed=6, params=params)
    b = training.make_training_minibatches(raws, 3, cfg, 7, 2, seed=6, params=params)
    assert [m['octree'].batch_size for m in a] == [2, 2, 1] and [m['octree'].batch_size for m in b] == [3, 2]
    pa = [p for m in a for p in m['octree']._clouds]
    pb = [p for m in b for p in m['octree']._clouds]
    assert len(pa) == len(pb) == 5
    assert all(torch.equal(x, y) and torch.equal(x, w) for x, y, w in zip(pa, pb, whole))
    # from the generator: one draw for the batch, whatever the split
    a = training.make_training_minibatches(raws, 2, cfg, 7, 2, seed=6, generator=torch.Generator().manual_seed(4))
    assert all(torch.equal(x, w) for x, w in zip([p for m in a for p in m['octree']._clouds], whole))


def test_errors():
    cfg = A.AugmentConfig.from_training_params(1, 1, 180.0, False, 'cartesian')
    far = np.full((4, 3), 5.0, np.float32)                                          # every point outside the unit cube
    # a generator of its own: with the process-wide one the draw depends on the tests that ran before, and one draw in eight
    # blanks a block of `far` (RemoveRandomBlock puts its points at the origin, inside the cube), so that nothing is raised
    draw = torch.Generator().manual_seed(0)
    assert not A.draw_params([10, 4], cfg, torch.Generator().manual_seed(0)).block.any()
    with pytest.raises(ValueError):
        A.augment_clouds([_cloud(1, 10) * np.float32(0.01), far], cfg, seed=1, generator=draw)
    with pytest.raises(ValueError):
        A.augment_clouds([np.zeros((0, 3), np.float32)], cfg, seed=1)
    with pytest.raises(_native.NativeLibraryError):
        A.augment_clouds([far], cfg, seed=1, device='cpu')
    # the launcher itself: aliased buffers, k > n, a negative size
    lib = _native.load()
    pts = torch.zeros(8, 3, device='cuda')
    out = torch.empty_like(pts)
    counts = torch.empty(1, dtype=torch.int32, device='cuda')
    off_host = np.array([0, 8], dtype=np.int64)
    off = torch.from_numpy(off_host).cuda()
    p = A.identity_params([8])
    ncfg = A.native_config(cfg, p, True)

    def launch(out_t, off_h, params, pts_ptr=None):
        rows = params.rows()
        table = torch.from_numpy(rows.view(np.int32)).cuda()
        return lib.hfl_augment_clouds(out_t.data_ptr(), counts.data_ptr(), None, pts_ptr or pts.data_ptr(), off.data_ptr(),
                                      off_h.ctypes.data, 1, table.data_ptr(), rows.ctypes.data, ctypes.byref(ncfg), 1, 0,
                                      None, ops._stream())
    assert launch(out, off_host, p) == 0
    assert launch(pts, off_host, p) == -1                                           # HFL_EINVAL: out aliases in
    assert launch(out, off_host, p, pts_ptr=counts.data_ptr()) == -1                # counts alias the input
    p.remove_k[0] = 9
    assert launch(out, off_host, p) == -1                                           # k > n
    p.remove_k[0] = -1
    assert launch(out, off_host, p) == -1
    p.remove_k[0] = 0
    assert launch(out, np.array([8, 0], dtype=np.int64), p) == -1                   # a negative size
    torch.cuda.synchronize()
