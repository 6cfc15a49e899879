"""Intra-sequence evaluation without a GPU: `causal_limits`, `intra_sequence_arrays` and the numpy definition of the
protocol, `evaluate_intra_sequence_host`, against plain Python loops written here."""
import math

import numpy as np
import pytest
import torch

from hotformerloc_amd import ops, retrieval
from hotformerloc_amd._native import NativeLibraryError

import intra_sequence_cases as ic


def limits_by_loop(t, thresh):
    return [sum(1 for j in range(len(t)) if t[j] <= t[i] - thresh) for i in range(len(t))]


@pytest.mark.parametrize('name', ['repeats', 'epoch', 'single'])
def test_causal_limits_equal_the_loop(name):
    if name == 'repeats':
        t, thresh = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 2.5, 4.0, 4.0, 9.0]), 1.0
    elif name == 'epoch':                                 # half a second apart at 1.6e9: fp32 could not tell them apart
        t, thresh = ic.EPOCH + np.arange(64) * 0.5, 3.0
    else:
        t, thresh = np.array([5.0]), 600.0
    want = limits_by_loop(np.asarray(t, dtype=np.float64), np.float64(thresh))
    got = retrieval.causal_limits(t, thresh)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == want
    assert all(lim <= i for i, lim in enumerate(got))                       # no scan sees itself
    as_tensor = retrieval.causal_limits(torch.from_numpy(np.asarray(t)), thresh)
    assert as_tensor.dtype == torch.int64 and as_tensor.tolist() == want
    if name == 'epoch':
        assert got.tolist() == [max(0, i - 5) for i in range(64)]


def test_causal_limits_rejects_unordered_time_and_a_zero_threshold():
    with pytest.raises(ValueError):
        retrieval.causal_limits(np.array([0.0, 2.0, 1.0]), 1.0)
    with pytest.raises(ValueError):
        retrieval.causal_limits(torch.tensor([0.0, 2.0, 1.0]), 1.0)
    for thresh in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            retrieval.causal_limits(np.array([0.0, 1.0]), thresh)


def test_intra_sequence_arrays_on_a_shuffled_dict():
    rng = np.random.RandomState(3)
    pos = ic.UTM + rng.uniform(0, 50, (9, 2))
    ts = ic.EPOCH + np.array([0.0, 1.0, 1.0, 2.0, 3.5, 3.5, 3.5, 7.0, 8.0])
    # equal timestamps keep the order of their keys: give them ascending keys, everything else shuffled
    keys = np.array([7, 2, 5, 0, 1, 3, 8, 6, 4])
    ordered = ic.run_set_from(pos, ts, keys)
    shuffled = {key: ordered[key] for key in [4, 8, 0, 6, 2, 7, 5, 1, 3]}   # another insertion order, the same run
    for run_set in (ordered, shuffled):
        order, got_pos, got_ts = retrieval.intra_sequence_arrays(run_set)
        assert order.dtype == np.int64 and order.tolist() == keys.tolist()
        assert got_pos.dtype == np.float64 and got_pos.shape == (9, 2) and np.array_equal(got_pos, pos)
        assert got_ts.dtype == np.float64 and np.array_equal(got_ts, ts)
        assert [run_set[int(i)]['easting'] for i in order] == got_pos[:, 0].tolist()
        assert [run_set[int(i)]['northing'] for i in order] == got_pos[:, 1].tolist()


def evaluate_by_loops(emb, pos, ts, time_thresh, world_thresh, k, cuts):
    """The protocol as a double loop over (i, j) in Python floats (float64)."""
    emb = emb.astype(np.float64)
    n = len(ts)
    r2 = world_thresh * world_thresh
    near = [[(pos[i, 0] - pos[j, 0]) ** 2 + (pos[i, 1] - pos[j, 1]) ** 2 <= r2 for j in range(n)] for i in range(n)]
    evaluated, revisit, top, hits = [], [], {}, {}
    for i in range(n):
        allowed = [j for j in range(n) if ts[j] <= ts[i] - time_thresh]
        if not allowed:
            continue
        evaluated.append(i)
        if any(near[i][j] for j in allowed):
            revisit.append(i)
        dist = [(float(((emb[i] - emb[j]) ** 2).sum()), j) for j in allowed]
        dist.sort()                                                         # by (distance, index)
        top[i] = dist[:k]
        hits[i] = [near[i][j] for _, j in top[i]]
    out = {'num_evaluated': len(evaluated), 'num_revisits': len(revisit)}
    firsts = [hits[i].index(True) for i in revisit if any(hits[i])]
    out['recall'] = [100.0 * sum(1 for f in firsts if f <= r) / len(revisit) for r in range(k)] if revisit else None
    out['mrr'] = 100.0 * sum(1.0 / (f + 1) for f in firsts) / len(firsts) if firsts else None
    s = {i: math.sqrt(top[i][0][0]) for i in evaluated}
    if cuts is None:
        cuts = sorted(set(s.values()))
    rows = []
    for tau in cuts:
        tp = sum(1 for i in evaluated if s[i] <= tau and hits[i][0])
        fp = sum(1 for i in evaluated if s[i] <= tau and not hits[i][0])
        fn = sum(1 for i in revisit if not s[i] <= tau)
        tn = len(evaluated) - tp - fp - fn
        p = tp / (tp + fp) if tp + fp else 1.0
        r = tp / (tp + fn) if tp + fn else 0.0
        rows.append((tau, tp, fp, fn, tn, p, r, 2 * p * r / (p + r) if p + r else 0.0))
    out['rows'] = rows
    return out


def check_against_loops(got, want, k):
    assert got['num_evaluated'] == want['num_evaluated'] and got['num_revisits'] == want['num_revisits']
    assert got['recall'].shape == (k,)
    if want['recall'] is None:
        assert np.isnan(got['recall']).all() and math.isnan(got['mrr'])
    else:
        np.testing.assert_allclose(got['recall'], want['recall'], rtol=1e-12, atol=0)
        assert abs(got['mrr'] - want['mrr']) <= 1e-12 * want['mrr']
    rows = want['rows']
    assert len(got['thresholds']) == len(rows)
    for key, col in (('tp', 1), ('fp', 2), ('fn', 3), ('tn', 4)):
        assert got[key].dtype == np.int64 and got[key].tolist() == [row[col] for row in rows], key
    for key, col in (('thresholds', 0), ('precision', 5), ('recall_curve', 6), ('f1', 7)):
        np.testing.assert_allclose(got[key], [row[col] for row in rows], rtol=1e-12, atol=0, err_msg=key)
    best = max(row[7] for row in rows) if rows else 0.0
    assert abs(got['f1_max'] - best) <= 1e-12
    if rows and want['recall'] is not None:
        assert got['f1_max_threshold'] == min(g for g, f in zip(got['thresholds'], got['f1']) if f == got['f1_max'])


@pytest.mark.parametrize('cuts', [None, 'grid'])
def test_host_protocol_equals_the_double_loop(cuts):
    """A slice of the perturbed two-lap run that keeps every kind of scan: the first 60 scans of lap one and the 60 of lap
    two that pass the same places, with the time threshold scaled to it."""
    emb, pos, ts = ic.run('perturbed')
    rows = np.concatenate([np.arange(0, 60), np.arange(400, 460)])
    emb, pos, ts = emb[rows], pos[rows], ts[rows]
    grid = None if cuts is None else np.linspace(0.0, 2.0, 41)
    got = retrieval.evaluate_intra_sequence_host(emb, pos, ts, time_thresh=20.0, world_thresh=3.0, num_neighbors=5,
                                                 thresholds=grid)
    want = evaluate_by_loops(emb, pos, ts, 20.0, 3.0, 5, None if grid is None else grid.tolist())
    assert want['num_revisits'] > 0 and any(row[2] > 0 for row in want['rows']) and any(row[3] > 0 for row in want['rows'])
    check_against_loops(got, want, 5)


def test_two_laps_in_closed_form():
    """limits[i] = max(0, i - 99): 700 scans are evaluated.  Lap one revisits nothing until it closes -- its last three
    scans are 3, 2 and 1 m from scan 0, recorded more than 100 s earlier -- and every scan of lap two stands where the scan
    400 s before it stood: 403 revisits, all of them found at rank 1 by the clean embeddings."""
    emb, pos, ts = ic.run('loop')
    limits = retrieval.causal_limits(ts, ic.TIME_THRESH)
    assert limits.tolist() == [max(0, i - 99) for i in range(800)]
    got = ic.host_result('loop')
    assert got['num_evaluated'] == 700 and got['num_revisits'] == 403
    assert got['recall'].shape == (25,) and np.array_equal(got['recall'], np.full(25, 100.0)) and got['mrr'] == 100.0
    assert got['f1_max'] == 1.0
    assert (got['tp'] + got['fp'] + got['fn'] + got['tn'] == 700).all()
    assert (np.diff(got['thresholds']) > 0).all() and got['tp'][-1] + got['fp'][-1] == 700 and got['fn'][-1] == 0
    perturbed = ic.host_result('perturbed')
    assert perturbed['num_evaluated'] == 700 and perturbed['num_revisits'] == 403
    assert perturbed['fp'][-1] > 0 and perturbed['fn'][0] > 0 and perturbed['recall'][0] < 100.0
    assert 0.0 < perturbed['f1_max'] < 1.0


def test_a_run_without_revisits():
    got = ic.host_result('line')
    assert got['num_evaluated'] == 200 and got['num_revisits'] == 0
    assert np.isnan(got['recall']).all() and got['recall'].shape == (25,) and math.isnan(got['mrr'])
    assert got['f1_max'] == 0.0 and (got['tp'] == 0).all() and (got['fn'] == 0).all()
    assert (got['precision'] == 0.0).all() and (got['recall_curve'] == 0.0).all()


def test_argument_checks():
    emb, pos, ts = ic.run('line')
    with pytest.raises(ValueError):
        retrieval.evaluate_intra_sequence_host(emb, pos[:-1], ts)
    with pytest.raises(ValueError):
        retrieval.evaluate_intra_sequence_host(emb, pos, ts, num_neighbors=33)
    with pytest.raises(ValueError):
        retrieval.evaluate_intra_sequence_host(emb, pos, ts[::-1].copy())
    cpu = torch.zeros((4, 16))
    with pytest.raises(NativeLibraryError):
        ops.flat_l2_topk_prefix(cpu, cpu, torch.zeros(4, dtype=torch.int64), 5)     # CPU tensors: no fallback
    if not torch.cuda.is_available():
        with pytest.raises(NativeLibraryError):
            retrieval.evaluate_intra_sequence(emb, pos, ts)
