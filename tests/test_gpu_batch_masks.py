"""`hfl_batch_masks` (hotformerloc_amd/csrc/batch_masks.hip) through `batch_masks.batch_masks` against the numpy route
`batch_masks_host`, bit for bit: batch sizes around a wave, a workgroup's width and the packed store's tail; lists on both
sides of the LDS staging capacity; the shipped batch size; counts, label sources, a side stream, label validation, the loss
and `training.make_training_batch`."""
import numpy as np
import pytest
import torch

import batch_masks_cases as bc
from hotformerloc_amd import TupleIndex, batch_masks, batch_masks_host, ops, training
from hotformerloc_amd import augment as A
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.losses import TruncatedSmoothAP

pytestmark = pytest.mark.gpu

N = 50
_CACHE = {}


def small():
    """(queries, device index) over N = 50 random lists of lengths 0..N, once."""
    if 'small' not in _CACHE:
        q = bc.random_queries(N, 5)
        _CACHE['small'] = (q, TupleIndex(q))
    return _CACHE['small']


def check(index, labels, counts=True):
    want_pos, want_neg = batch_masks_host(index, labels)
    pos, neg, cnt = batch_masks(index, labels, return_counts=True)
    torch.cuda.synchronize()
    b = len(labels)
    assert pos.dtype == torch.bool and neg.dtype == torch.bool and pos.is_contiguous() and neg.is_contiguous()
    assert tuple(pos.shape) == (b, b) and tuple(neg.shape) == (b, b) and pos.device == index.device
    assert set(pos.view(torch.uint8).unique().tolist()) <= {0, 1} and set(neg.view(torch.uint8).unique().tolist()) <= {0, 1}
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(neg.cpu().numpy(), want_neg)
    assert cnt.dtype == torch.int32 and tuple(cnt.shape) == (b, 2)
    assert np.array_equal(cnt.cpu().numpy(), np.stack([want_pos.sum(1), want_neg.sum(1)], 1))
    return pos, neg, cnt


@pytest.mark.parametrize('batch', [1, 4, 5, 63, 64, 65, 257])
def test_batch_sizes(batch):
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, batch, 100 + batch)
    check(index, labels)
    want_pos, want_neg = bc.brute_force(q, labels)                          # the yardstick itself, at these shapes
    host_pos, host_neg = batch_masks_host(index, labels)
    assert np.array_equal(host_pos, want_pos) and np.array_equal(host_neg, want_neg)


def test_repeated_labels():
    q, index = small()
    e = 7
    labels = np.asarray([e, e, 0, N - 1, 0, e, N - 1, 1, 1, e, 2], np.int64)     # own label, repeats, 0 and N - 1
    pos, neg, _ = check(index, labels)
    pos = pos.cpu().numpy()
    assert np.array_equal(pos[0], pos[1]) and np.array_equal(pos[:, 0], pos[:, 5])      # equal labels, equal rows / columns
    # membership alone decides the diagonal
    assert [bool(pos[i, i]) for i in range(len(labels))] == [int(l) in set(q[int(l)].positives.tolist()) for l in labels]


@pytest.mark.parametrize('family', ['positives', 'non_negatives'])
def test_lists_across_the_staging_capacity(family):
    cap = ops.BATCH_MASKS_LDS_ENTRIES
    q, n = bc.long_queries(cap, family)
    assert [len(getattr(q[k], family)) for k in range(6)] == [0, 1, cap - 1, cap, cap + 1, n] and n == cap + 300
    index = TupleIndex(q)
    labels = bc.long_labels(q, n, family)
    assert len(labels) == 65
    pos, neg, cnt = check(index, labels)
    mask = (pos if family == 'positives' else ~neg).cpu().numpy()
    assert not mask[0].any() and mask[5].all() and mask[1].sum() >= 1              # empty list, full list, the one entry


def test_shipped_batch_size():
    n, b = 20000, 2048
    index = TupleIndex.from_csr(*syn.tuple_lists(n, 17, 30, 300))
    rng = np.random.RandomState(2)
    anchors = rng.randint(0, n, b // 2)
    mates = [int(index.get_positives(a)[rng.randint(len(index.get_positives(a)))]) for a in anchors]
    labels = np.stack([anchors, np.asarray(mates)], 1).reshape(-1)                # pairs of positives, as the sampler draws
    pos, neg, cnt = check(index, labels)
    assert int(pos.sum()) >= b and int(neg.sum()) > b * b // 2


def test_counts_are_optional_and_do_not_change_the_masks():
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, 130, 9)
    out = batch_masks(index, labels)
    assert isinstance(out, tuple) and len(out) == 2
    pos, neg, cnt = batch_masks(index, labels, return_counts=True)
    assert torch.equal(out[0], pos) and torch.equal(out[1], neg)
    assert torch.equal(cnt[:, 0].long(), pos.sum(1)) and torch.equal(cnt[:, 1].long(), neg.sum(1))


def test_label_sources():
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, 70, 21)
    base = batch_masks(index, labels.tolist())
    for src in (torch.from_numpy(labels).cuda(), labels.astype(np.int32), torch.from_numpy(labels),
                torch.from_numpy(labels.astype(np.int32)).cuda()):
        got = batch_masks(index, src)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    want = batch_masks_host(q, labels)
    assert np.array_equal(base[0].cpu().numpy(), want[0]) and np.array_equal(base[1].cpu().numpy(), want[1])


def test_side_stream():
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, 257, 33)
    want = batch_masks_host(index, labels)
    dev_labels = torch.from_numpy(labels).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pos, neg, cnt = batch_masks(index, dev_labels, return_counts=True)
    s.synchronize()
    assert np.array_equal(pos.cpu().numpy(), want[0]) and np.array_equal(neg.cpu().numpy(), want[1])
    assert np.array_equal(cnt.cpu().numpy()[:, 0], want[0].sum(1))


def test_labels_out_of_range_raise_before_any_launch(monkeypatch):
    q, index = small()

    def no_launch(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(ops, 'batch_masks', no_launch)
    for bad in ([0, N], [-1, 3]):
        with pytest.raises(ValueError):
            batch_masks(index, bad)
        with pytest.raises(ValueError):
            batch_masks(index, torch.tensor(bad, device='cuda'))
    with pytest.raises(ValueError):
        batch_masks(index, torch.zeros(0, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError):
        batch_masks(index, torch.zeros(3, device='cuda'))


@pytest.mark.parametrize('offsets', [(0, 0), (1, 1), (3, 3), (1, 2), (0, 2)])
@pytest.mark.parametrize('batch', [1, 5, 64, 67])
def test_output_alignment(batch, offsets):
    """Masks whose storage starts at any byte: equal offsets modulo 4 take the packed stores with a shifted head, unequal
    ones the byte stores."""
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, batch, 50 + batch)
    want = batch_masks_host(index, labels)
    bufs = [torch.full((batch * batch + 8,), 7, dtype=torch.uint8, device='cuda') for _ in range(2)]
    outs = [buf[o:o + batch * batch].view(batch, batch) for buf, o in zip(bufs, offsets)]
    pos, neg, _ = ops.batch_masks(torch.from_numpy(labels).cuda(), *index.dev, len(index), out=outs)
    assert pos.data_ptr() == bufs[0].data_ptr() + offsets[0]
    assert np.array_equal(pos.cpu().numpy(), want[0].astype(np.uint8)) and np.array_equal(neg.cpu().numpy(), want[1].astype(np.uint8))
    for buf, o in zip(bufs, offsets):                                          # nothing outside the matrix was touched
        assert (buf[:o] == 7).all() and (buf[o + batch * batch:] == 7).all()


def test_empty_index_lists():
    """Every list empty: the id arrays keep a placeholder element, no positives, everything a negative."""
    index = TupleIndex([bc.Tup([], []) for _ in range(5)])
    pos, neg, cnt = batch_masks(index, [4, 0, 0], return_counts=True)
    assert not pos.any() and neg.all() and cnt.tolist() == [[0, 3]] * 3


@pytest.mark.parametrize('similarity', ['euclidean', 'cosine'])
def test_loss_takes_the_device_masks(similarity):
    b, d = 16, 256
    q, index = small()
    labels = bc.labels_hitting_ends(q, N, b, 71, e=2)
    emb = torch.from_numpy(syn.hash_uniform(5, b * d).reshape(b, d).astype(np.float32) - 0.5).cuda()
    emb = emb / emb.norm(dim=1, keepdim=True)
    loss_fn = TruncatedSmoothAP(tau1=0.01, similarity=similarity, positives_per_query=4)
    host_pos, host_neg = batch_masks_host(index, labels)
    assert host_pos.any()
    results = []
    for pos, neg in (batch_masks(index, labels), (torch.tensor(host_pos).cuda(), torch.tensor(host_neg).cuda())):
        e = emb.clone().requires_grad_(True)
        loss, stats = loss_fn(e, pos, neg)
        loss.backward()
        results.append((loss.detach(), e.grad.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert torch.isfinite(results[0][1]).all() and results[0][1].abs().sum() > 0


def test_make_training_batch():
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cylindrical')
    raws = [(syn.unit_ball_cloud(1000 + i, n).astype(np.float64) * (30.0, 20.0, 8.0)).astype(np.float32)
            for i, n in enumerate((600, 65, 900, 300, 513))]
    params = A.draw_params([len(r) for r in raws], cfg, torch.Generator().manual_seed(4))
    q, index = small()
    labels = [7, 2, 7, 0, N - 1]
    mbs, pos, neg = training.make_training_batch(raws, labels, index, split_size=2, cfg=cfg, depth=7, full_depth=2, seed=6,
                                                 params=params)
    want = training.make_training_minibatches(raws, 2, cfg, 7, 2, seed=6, params=params)
    assert [m['octree'].batch_size for m in mbs] == [2, 2, 1] == [m['octree'].batch_size for m in want]
    for a, w in zip(mbs, want):
        assert len(a['octree']._clouds) == len(w['octree']._clouds)
        assert all(torch.equal(x, y) for x, y in zip(a['octree']._clouds, w['octree']._clouds))
    host = batch_masks_host(index, labels)
    assert pos.dtype == torch.bool and np.array_equal(pos.cpu().numpy(), host[0]) and np.array_equal(neg.cpu().numpy(), host[1])
    with pytest.raises(ValueError):
        training.make_training_batch(raws, labels[:4], index, split_size=2, cfg=cfg, depth=7, seed=6, params=params)
