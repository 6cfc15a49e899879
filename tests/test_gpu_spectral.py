"""Spectral verification on the device (`csrc/spectral.hip`, `hotformerloc_amd/spectral.py`) against the numpy twins of the
same module.

Comparison rule.  Weights: the order of the fp32 chain is defined, so bit equality is expected and its share is printed;
asserted is |dv_i| <= 2^-21 max v, which allows for the double rounding of the host's fmaf-through-float64 emulation and for a
float64 sum that rounds fp32(sqrt(s2)) the other way -- the normalisation does not amplify either.  A weight is zero on the
device exactly where it is zero on the host.  Eigenvalue: within 1e-6 relative (the same float64 sums in another order).
A batch run equals the single runs, and a second run the first, bit for bit.  Shapes: R = ops.SPECTRAL_ROWS rows and T =
ops.SPECTRAL_TILE columns per workgroup and every size around them, K in {1, 2, 10}."""
import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native
from tests import global_registration_cases as gc
from tests import spectral_cases as sc
from tests.test_gpu_global_registration import GLOBAL_BOUNDS

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def on_device(batch):
    return [dev(c) for c in batch[0]], [dev(c) for c in batch[1]], [dev(r) for r in batch[2]]


def assert_result_of_the_host(res, host, label):
    """the rule of the module docstring; -> (largest |dv| / max v, largest relative eigenvalue error)"""
    assert res.eigenvalue.dtype == np.float64 and res.score.dtype == np.float64
    worst_v = worst_e = 0.0
    equal = total = 0
    for i, (w, hw) in enumerate(zip(res.weights, host.weights)):
        w = w.cpu().numpy()
        assert w.dtype == np.float32 and w.shape == hw.shape
        assert np.array_equal(w == 0, hw == 0), 'pair %d: the zero weights differ' % i
        if hw.shape[0] and hw.max() > 0:
            worst_v = max(worst_v, float(np.abs(w.astype(np.float64) - hw).max() / hw.max()))
        equal, total = equal + int((w == hw).sum()), total + w.shape[0]
        if host.eigenvalue[i] == 0.0:
            assert res.eigenvalue[i] == 0.0 and res.score[i] == 0.0
        else:
            worst_e = max(worst_e, abs(res.eigenvalue[i] - host.eigenvalue[i]) / host.eigenvalue[i])
    print('%s: %d of %d weights bit-equal, largest |dv| / max v %.3g (bound %.3g), largest eigenvalue error %.3g'
          % (label, equal, total, worst_v, 2.0 ** -21, worst_e))
    assert worst_v <= 2.0 ** -21 and worst_e <= 1e-6
    assert np.allclose(res.score, host.score, rtol=1e-6, atol=0.0)
    return worst_v, worst_e


@pytest.mark.parametrize('iterations', sc.K_SIZES)
def test_ragged_batch_and_single_pairs(iterations):
    batch = sc.ragged_batch()
    on = on_device(batch)
    res = hfl.spectral_consistency(*on, iterations=iterations)
    again = hfl.spectral_consistency(*on, iterations=iterations)
    host = sc.host_ragged(iterations)
    assert_result_of_the_host(res, host, 'K = %d' % iterations)
    assert np.array_equal(res.eigenvalue, again.eigenvalue) and np.array_equal(res.score, again.score)
    assert all(torch.equal(a, b) for a, b in zip(res.weights, again.weights))      # two runs, the same bits
    assert res.eigenvalue[:2].tolist() == [0.0, 0.0] and (res.eigenvalue[3:] > 0).all()
    for i in range(len(sc.C_SIZES)):                                               # a pair alone: the same bits
        one = hfl.spectral_consistency([on[0][i]], [on[1][i]], [on[2][i]], iterations=iterations)
        assert one.eigenvalue[0] == res.eigenvalue[i] and one.score[0] == res.score[i], sc.C_SIZES[i]
        assert torch.equal(one.weights[0], res.weights[i]), sc.C_SIZES[i]


def test_packed_layout_and_threshold():
    batch = sc.ragged_batch()
    on = on_device(batch)
    lists = hfl.spectral_consistency(*on, distance_threshold=sc.SIGMA, iterations=3)
    off = np.cumsum([0] + [r.shape[0] for r in batch[2]])
    cat = lambda parts: (torch.cat(parts, 0), np.cumsum([0] + [int(p.shape[0]) for p in parts]))       # noqa: E731
    packed = hfl.spectral_consistency(cat(on[0]), cat(on[1]), (torch.cat(on[2], 0), off), distance_threshold=sc.SIGMA,
                                      iterations=3)
    assert torch.equal(packed.weights, torch.cat(lists.weights)) and np.array_equal(packed.eigenvalue, lists.eigenvalue)
    host = hfl.spectral_consistency_host(*batch, distance_threshold=sc.SIGMA, iterations=3)
    assert_result_of_the_host(lists, host, 'sigma = %.1f, K = 3' % sc.SIGMA)


@pytest.mark.parametrize('frac', (0.6, 0.9))
def test_purpose_cases_against_the_host(frac):
    src, dst, rows = gc.corrupted(frac)
    res = hfl.spectral_consistency([dev(src)], [dev(dst)], [dev(rows)], distance_threshold=sc.SIGMA, iterations=sc.ITERATIONS)
    assert_result_of_the_host(res, sc.host_corrupted(frac), 'frac = %.1f' % frac)
    true = gc.true_rows(frac)
    kept = hfl.prune_correspondences([dev(rows)], res.weights, int(true.sum()))
    assert kept[0].is_cuda and np.array_equal(kept[0].cpu().numpy(), rows[true])
    # the device's pruning equals the host's on the device's weights
    host_kept = hfl.prune_correspondences_host([rows], [res.weights[0].cpu().numpy()], 100)
    assert np.array_equal(hfl.prune_correspondences([dev(rows)], res.weights, 100)[0].cpu().numpy(), host_kept[0])


@pytest.mark.parametrize('n_true,n_corr', ((16, 40), (64, 600)))
def test_exact_case(n_true, n_corr):
    src, dst, rows, true = sc.exact_case(n_true, n_corr)
    res = hfl.spectral_consistency([dev(src)], [dev(dst)], [dev(rows)])
    w = res.weights[0].cpu().numpy()
    assert not w[~true].any() and np.array_equal(w[~true].view(np.uint32), np.zeros(int((~true).sum()), np.uint32))
    assert (w[true] == np.float32(1.0 / np.sqrt(n_true))).all()
    assert abs(res.eigenvalue[0] - (n_true - 1)) <= 1e-12 * (n_true - 1) and res.score[0] == res.eigenvalue[0] / n_corr
    host = hfl.spectral_consistency_host([src], [dst], [rows])
    assert np.array_equal(w, host.weights[0]) and res.eigenvalue[0] == host.eigenvalue[0]


def test_prune_on_the_device_equals_the_host():
    batch = sc.ragged_batch()
    on = on_device(batch)
    res = hfl.spectral_consistency(*on)
    host_w = [w.cpu().numpy() for w in res.weights]
    for keep in (0, 1, 300):
        got = hfl.prune_correspondences(on[2], res.weights, keep)
        want = hfl.prune_correspondences_host(batch[2], host_w, keep)
        assert all(g.is_cuda and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), keep
    off = np.cumsum([0] + [r.shape[0] for r in batch[2]])
    rows, new_off = hfl.prune_correspondences((torch.cat(on[2], 0), off), torch.cat(res.weights), 300)
    want = hfl.prune_correspondences_host(batch[2], host_w, 300)
    assert np.array_equal(rows.cpu().numpy(), np.concatenate(want)) and new_off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()


def test_rerank_on_the_device():
    queries, database, cand = sc.rerank_inputs()
    res = hfl.rerank_candidates([dev(c) for c in queries], [dev(c) for c in database], dev(cand))
    host = sc.host_rerank()
    print('device scores', res.scores[0].cpu().numpy(), 'host scores', host.scores[0])
    assert res.indices.is_cuda and res.indices.dtype == torch.int64 and res.scores.dtype == torch.float64
    assert np.array_equal(res.indices.cpu().numpy(), host.indices) and np.array_equal(res.order.cpu().numpy(), host.order)
    assert np.abs(res.scores.cpu().numpy() - host.scores).max() <= 1e-5
    assert [sc.DATABASE[i] for i in res.indices[0, :5].tolist()] == list(sc.EXPECTED_ORDER)


def test_rerank_with_registration_on_the_device():
    queries, database, cand = sc.rerank_inputs()
    ranked, coarse, fine = hfl.rerank_candidates([dev(c) for c in queries], [dev(c) for c in database], dev(cand), register=True)
    assert np.array_equal(ranked.indices.cpu().numpy(), sc.host_rerank().indices)
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0], sc.rerank_truth()) + (angle, shift)))
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]
    # the pruned route ends there too
    _, _, pruned = hfl.rerank_candidates([dev(c) for c in queries], [dev(c) for c in database], dev(cand), register=True,
                                         keep=300)
    angle, shift = gc.pose_error(pruned.transforms[0], sc.rerank_truth())
    print('keep = 300: fine %.3g degrees %.3g m' % (angle, shift))
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]


def test_cpu_tensors_are_refused():
    src, dst, rows = gc.corrupted(0.6)
    with pytest.raises(_native.NativeLibraryError):
        hfl.spectral_consistency([torch.from_numpy(src.copy())], [torch.from_numpy(dst.copy())], [dev(rows)])
    queries, database, cand = sc.rerank_inputs()
    with pytest.raises(_native.NativeLibraryError):
        hfl.rerank_candidates([torch.from_numpy(c.copy()) for c in queries], [dev(c) for c in database], cand)
    with pytest.raises(_native.NativeLibraryError):
        hfl.rerank_candidates([dev(c) for c in queries], [torch.from_numpy(c.copy()) for c in database], cand)
