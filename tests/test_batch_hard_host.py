"""Host side of the batch-hard triplet and contrastive losses: what the case table of tests/batch_hard_cases.py must satisfy,
the numpy twins of hotformerloc_amd/losses.py against the float64 restatement, hand-computed examples, the loss factory
`make_loss_fn` and the two helpers of the dynamic batch sizing."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import batch_hard_cases as bc
from hotformerloc_amd import losses
from hotformerloc_amd.training import expand_batch_size, should_expand_batch

ALL_CASES = sorted(bc.CASES) + sorted(bc.EMPTY_CASES)


@pytest.mark.parametrize('case', sorted(bc.CASES))
def test_case_table_conditions(case):
    """1. float64 and fp32 mining pick the same triples; 2. 25 % to 75 % of the triplets are active and both swap branches
    occur among them; 3. no |v| < 1e-4 and no active |d_pn - d_an| < 1e-5; 4. both contrastive term sets are 25 % to 75 %
    full and no |d - margin| < 1e-4."""
    c = bc.conditions(case)
    print(case, c)
    assert c['same_mining']
    assert 0.25 * c['triplets'] <= c['active'] <= 0.75 * c['triplets']
    assert 1 <= c['swapped_active'] < c['active']
    assert c['closest_v'] >= 1e-4 and c['closest_swap'] >= 1e-5
    assert 0.25 * c['triplets'] <= c['pos_above'] <= 0.75 * c['triplets']
    assert 0.25 * c['triplets'] <= c['neg_above'] <= 0.75 * c['triplets']
    assert c['closest_margin'] >= 1e-4


def test_case_table_covers_the_launch_shapes():
    shapes = {name: bc.inputs(name)[0].shape for name in ALL_CASES}
    assert shapes['b1'][0] == 1 and shapes['b2'][0] == 2
    assert shapes['b65_d70'] == (65, 70) and shapes['b65_d70'][1] % 4 != 0
    assert shapes['b300'][0] > 4 * 64 and shapes['b520'][0] > 8 * 64          # row tiles of 64; at most eight column splits
    assert int((~bc.inputs('b48_few_pos')[1].any(1)).sum()) == 5
    e = bc.inputs('dup24')[0]
    assert np.array_equal(e[0], e[1]) and np.array_equal(e[7], e[15]) and np.array_equal(e[18], e[20])
    _, _, _, t = bc.yardstick('dup24', 'triplet')
    assert t['d_an'][7] == 0.0 and t['d_ap'][18] == 0.0 and t['p'][18] == 19 and t['n'][12] == 0


def _check_stats(kind, got, want, tol):
    floats, counts = bc.stat_keys(kind)
    assert sorted(got) == sorted(floats + counts)
    for key in counts:
        assert got[key] == want[key], key
    for key in floats:
        assert (math.isnan(got[key]) and math.isnan(want[key])) or abs(got[key] - want[key]) <= tol, (key, got[key], want[key])


@pytest.mark.parametrize('kind', ['triplet', 'contrastive'])
@pytest.mark.parametrize('case', ALL_CASES)
def test_float64_twin_matches_the_restatement(case, kind):
    e, pos, neg = bc.inputs(case)
    m, pm, nm = bc.margins(case)
    want_loss, want_grad, want_stats, want = bc.yardstick(case, kind)
    if kind == 'triplet':
        loss, grad, stats, got = losses.batch_hard_triplet_host(e, pos, neg, m, dtype=np.float64, details=True)
    else:
        loss, grad, stats, got = losses.batch_hard_contrastive_host(e, pos, neg, pm, nm, dtype=np.float64, details=True)
    for key in ('a', 'p', 'n'):
        assert np.array_equal(got[key], want[key]), key
    assert abs(loss - want_loss) <= 1e-12
    _check_stats(kind, stats, want_stats, 1e-12)
    assert grad.dtype == np.float64 and grad.shape == e.shape
    assert np.abs(grad - want_grad).max() <= 1e-12 * max(np.abs(want_grad).max(), 1e-300)
    if case in bc.EMPTY_CASES:
        assert loss == 0.0 and not grad.any() and math.isnan(stats['mean_pos_pair_dist']) and math.isnan(stats['min_neg_pair_dist'])


@pytest.mark.parametrize('kind', ['triplet', 'contrastive'])
@pytest.mark.parametrize('case', sorted(bc.CASES))
def test_fp32_twin_stays_within_the_device_bars_of_float64(case, kind):
    """The fp32 twin is the kernels' arithmetic, so it must meet the bars the device tests use: loss and float stats 2e-6,
    counts equal, gradient 2e-5 max|g| + 1e-7."""
    e, pos, neg = bc.inputs(case)
    m, pm, nm = bc.margins(case)
    want_loss, want_grad, want_stats, _ = bc.yardstick(case, kind)
    if kind == 'triplet':
        loss, grad, stats = losses.batch_hard_triplet_host(e, pos, neg, m)
    else:
        loss, grad, stats = losses.batch_hard_contrastive_host(e, pos, neg, pm, nm)
    assert grad.dtype == np.float32
    assert abs(loss - want_loss) <= 2e-6
    _check_stats(kind, stats, want_stats, 2e-6)
    assert np.abs(grad - want_grad).max() <= 2e-5 * np.abs(want_grad).max() + 1e-7


def test_fmaf_emulation_is_single_rounded():
    """Products whose float64 sum with c lands on a float32 midpoint: rounding twice would go to even, fmaf does not."""
    a = np.float32(1 + 2.0 ** -12)
    b = np.float32(1 + 2.0 ** -12)                     # a b = 1 + 2^-11 + 2^-24: half an ulp above a float32
    c = np.float32(2.0 ** -60)
    assert losses._fmaf32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert losses._fmaf32(a, b, -c) == np.float32(1 + 2.0 ** -11)
    assert (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32) == np.float32(1 + 2.0 ** -11)   # the naive route
    x = np.float32([0.1, 0.3, -0.7])
    assert np.array_equal(losses._fmaf32(x, x, np.float32(0)), (x.astype(np.float64) ** 2).astype(np.float32))


def test_mine_host_returns_first_extrema_of_the_chain_matrix():
    e, pos, neg = bc.inputs('dup24')
    a, p, n, d_ap, d_an = losses.batch_hard_mine_host(e, pos, neg)
    dm = losses._host_dist(e, np.float32)
    assert dm.dtype == np.float32 and np.array_equal(dm, dm.T) and not dm.diagonal().any()
    assert np.array_equal(a, np.arange(24))
    assert np.array_equal(p, np.argmax(np.where(pos, dm, -1), axis=1)) and np.array_equal(d_ap, dm[a, p])
    assert np.array_equal(n, np.argmin(np.where(neg, dm, np.inf), axis=1)) and np.array_equal(d_an, dm[a, n])
    assert n[12] == 0 and dm[12, 0] == dm[12, 1] and p[18] == 19 and d_ap[18] == 0.0 and d_an[7] == 0.0


# ---- hand-computed examples: points on a line or in the plane, distances read off by eye ------------------------------------
def _masks(b, positives, negatives):
    pos, neg = np.zeros((b, b), bool), np.zeros((b, b), bool)
    for i, j in positives:
        pos[i, j] = pos[j, i] = True
    for i, j in negatives:
        neg[i, j] = neg[j, i] = True
    return pos, neg


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_example_pins_the_swap_branch(dtype):
    """Points 0, 2, 3 on a line, 0 ~ 1 positives, 2 negative to both.  Row 0: d_ap = 2, d_an = 3, d_pn = 1: swapped,
    v = 2 - 1 + 0.5.  Row 1: d_ap = 2, d_an = 1, d_pn = 3: not swapped, v = 2 - 1 + 0.5.  Row 2 has no positive."""
    e = np.array([[0., 0.], [2., 0.], [3., 0.]], np.float32)
    pos, neg = _masks(3, [(0, 1)], [(0, 2), (1, 2)])
    loss, grad, stats, d = losses.batch_hard_triplet_host(e, pos, neg, 0.5, dtype=dtype, details=True)
    assert d['a'].tolist() == [0, 1] and d['p'].tolist() == [1, 0] and d['n'].tolist() == [2, 2]
    assert d['swapped'].tolist() == [True, False] and d['v'].tolist() == [1.5, 1.5]
    assert loss == 1.5 and stats['num_triplets'] == 2 and stats['num_non_zero_triplets'] == 2
    # row 0's triplet: +d(0,1) - d(1,2); row 1's: +d(1,0) - d(1,2); each weighted 1/2
    want = 0.5 * np.array([[-1. - 1., 0.], [1. + 1. + 1. + 1., 0.], [-1. - 1., 0.]])
    assert np.array_equal(grad, want.astype(dtype))
    assert stats['mean_pos_pair_dist'] == 2.0 and stats['max_neg_pair_dist'] == 3.0 and stats['min_neg_pair_dist'] == 1.0
    assert abs(stats['avg_embedding_norm'] - 5.0 / 3.0) < 1e-6


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_example_exact_tie_differentiates_the_anchor_negative_pair(dtype):
    """An isosceles triangle: d(0,2) = d(1,2) = 5, d(0,1) = 6.  d_pn == d_an exactly: no swap, the gradient reaches the
    negative through the anchor only."""
    e = np.array([[-3., 0.], [3., 0.], [0., 4.]], np.float32)
    pos, neg = _masks(3, [(0, 1)], [(0, 2)])
    pos[1, 0] = False                                   # row 0 alone is kept
    loss, grad, stats, d = losses.batch_hard_triplet_host(e, pos, neg, 0.25, dtype=dtype, details=True)
    assert d['a'].tolist() == [0] and d['swapped'].tolist() == [False] and loss == 1.25
    want = np.array([[-1. - (-3. / 5.), 0. - (-4. / 5.)], [1., 0.], [-3. / 5., -4. / 5.]])
    assert np.allclose(grad, want, atol=1e-6 if dtype == np.float32 else 1e-15)
    assert grad[1, 1] == 0.0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_example_none_active_is_an_exact_zero(dtype):
    e = np.array([[0., 0.], [1., 0.], [9., 0.], [9., 1.]], np.float32)
    pos, neg = _masks(4, [(0, 1), (2, 3)], [(0, 2), (0, 3), (1, 2), (1, 3)])
    loss, grad, stats = losses.batch_hard_triplet_host(e, pos, neg, 0.4, dtype=dtype)
    assert loss == 0.0 and not grad.any() and stats['num_triplets'] == 4 and stats['num_non_zero_triplets'] == 0
    assert stats['max_pos_pair_dist'] == 1.0 and stats['min_neg_pair_dist'] == 8.0
    loss, grad, stats = losses.batch_hard_contrastive_host(e, pos, neg, 1.5, 0.65, dtype=dtype)
    assert loss == 0.0 and not grad.any() and stats['num_pairs'] == 8
    assert stats['pos_pairs_above_threshold'] == 0 and stats['neg_pairs_above_threshold'] == 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_example_no_kept_row(dtype):
    e = np.array([[0., 0.], [1., 0.], [2., 0.]], np.float32)
    pos, neg = _masks(3, [(0, 1)], [])
    for loss, grad, stats in (losses.batch_hard_triplet_host(e, pos, neg, 0.4, dtype=dtype),
                              losses.batch_hard_contrastive_host(e, pos, neg, 0.2, 0.65, dtype=dtype)):
        assert loss == 0.0 and grad.shape == (3, 2) and not grad.any()
        assert stats.get('num_triplets', stats.get('num_pairs')) == 0
        assert all(math.isnan(stats['%s_%s_pair_dist' % (f, s)]) for f in ('mean', 'max', 'min') for s in ('pos', 'neg'))
        assert stats['avg_embedding_norm'] == 1.0
    a, p, n, d_ap, d_an = losses.batch_hard_mine_host(e, pos, neg, dtype)
    assert len(a) == len(p) == len(n) == len(d_ap) == len(d_an) == 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_example_zero_distance_pairs_receive_no_gradient(dtype):
    """Rows 0 and 1 coincide and are each other's positive; row 2 at distance 2 is their negative, row 3 = row 2 its positive.
    Contrastive with pos_margin -1 makes the pairs at distance 0 active (0 + 1 > 0): they must contribute nothing, not nan."""
    e = np.array([[1., 1.], [1., 1.], [1., 3.], [1., 3.]], np.float32)
    pos, neg = _masks(4, [(0, 1), (2, 3)], [(0, 2), (0, 3), (1, 2), (1, 3)])
    loss, grad, stats, d = losses.batch_hard_contrastive_host(e, pos, neg, -1.0, 2.5, dtype=dtype, details=True)
    assert d['d_ap'].tolist() == [0.0] * 4 and d['d_an'].tolist() == [2.0] * 4 and d['n'].tolist() == [2, 2, 0, 0]
    assert stats['pos_pairs_above_threshold'] == 4 and stats['neg_pairs_above_threshold'] == 4
    assert stats['pos_loss'] == 1.0 and stats['neg_loss'] == 0.5 and loss == 1.5
    # -d(a, n) / 4 for each of the four rows: rows 0 and 2 are named by three pairs each, rows 1 and 3 by one
    assert np.array_equal(grad, np.array([[0., 0.75], [0., 0.25], [0., -0.75], [0., -0.25]], dtype))
    loss, grad, stats = losses.batch_hard_triplet_host(e, pos, neg, 2.5, dtype=dtype)       # v = 0 - 2 + 2.5, d_pn == d_an
    assert loss == 0.5 and np.array_equal(grad, np.array([[0., 0.75], [0., 0.25], [0., -0.75], [0., -0.25]], dtype))


# ---- the factory and the batch-size helpers -----------------------------------------------------------------------------------
def test_make_loss_fn_builds_each_class_with_the_config_margins():
    fn = losses.make_loss_fn(SimpleNamespace(loss='batchhardtripletmarginloss', margin=0.3))
    assert isinstance(fn, losses.BatchHardTripletLossWithMasks) and fn.margin == 0.3
    fn = losses.make_loss_fn(SimpleNamespace(loss='batchhardcontrastiveloss', pos_margin=0.1, neg_margin=0.7))
    assert isinstance(fn, losses.BatchHardContrastiveLossWithMasks) and (fn.pos_margin, fn.neg_margin) == (0.1, 0.7)
    assert losses.make_loss_fn(SimpleNamespace(loss='batchhardtripletmarginloss')).margin == 0.4
    fn = losses.make_loss_fn(SimpleNamespace(loss='batchhardcontrastiveloss'))
    assert (fn.pos_margin, fn.neg_margin) == (0.2, 0.65)
    fn = losses.make_loss_fn(SimpleNamespace(loss='truncatedsmoothap', tau1=0.02, similarity='euclidean', positives_per_query=3))
    assert isinstance(fn, losses.TruncatedSmoothAP) and (fn.tau1, fn.similarity, fn.positives_per_query) == (0.02, 'euclidean', 3)
    with pytest.raises(NotImplementedError, match='Unknown loss: focal'):
        losses.make_loss_fn(SimpleNamespace(loss='focal', tau1=0.01, similarity='euclidean', positives_per_query=4))


def test_new_names_are_exported():
    import hotformerloc_amd as hfl
    for name in ('BatchHardTripletLossWithMasks', 'BatchHardContrastiveLossWithMasks', 'batch_hard_mine', 'batch_hard_mine_host',
                 'batch_hard_triplet_host', 'batch_hard_contrastive_host', 'make_loss_fn', 'expand_batch_size',
                 'should_expand_batch'):
        assert hasattr(hfl, name), name


def test_batch_hard_losses_have_no_cpu_fallback():
    from hotformerloc_amd._native import NativeLibraryError
    e, m = torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.bool)
    with pytest.raises(NativeLibraryError):
        losses.BatchHardTripletLossWithMasks(0.4)(e, m, m)
    with pytest.raises(NativeLibraryError):
        losses.BatchHardContrastiveLossWithMasks(0.2, 0.65)(e, m, m)
    with pytest.raises(NativeLibraryError):
        losses.batch_hard_mine(e, m, m)


def test_batch_size_helpers_follow_the_reference_arithmetic():
    sizes = [64]
    for _ in range(5):
        sizes.append(expand_batch_size(sizes[-1], 1.5, 256))
    assert sizes == [64, 96, 144, 216, 256, 256]
    assert expand_batch_size(10, 1.25, 256) == 12 and expand_batch_size(300, 1.5, 256) == 300
    with pytest.raises(ValueError):
        expand_batch_size(64, 1.0, 256)
    stats = {'num_triplets': 40.0, 'num_non_zero_triplets': 11.0}
    assert should_expand_batch(stats, 0.3) and not should_expand_batch(stats, 0.25) and not should_expand_batch(stats, None)
    assert not should_expand_batch({'num_triplets': 40, 'num_non_zero_triplets': 12}, 0.3)       # 0.3 is not below 0.3
    assert not should_expand_batch({'num_triplets': 0, 'num_non_zero_triplets': 0}, 0.3)
    with pytest.raises(KeyError):
        should_expand_batch({'loss': 1.0}, 0.3)
    with pytest.raises(ValueError):
        should_expand_batch(stats, 1.5)
