"""The consumers of `csrc/pair_scan.h` make the same decisions on the same pairs.

`feature_correspondences` on (N, 3) float32 rows runs the chain of `nn_distances`: d0 d0, then two fmaf; the zero column
that pads D = 3 to 4 adds fmaf(0, 0, acc) == acc.  So on the same clouds the indices are equal, the float32 square root of
dist2 (correctly rounded in numpy as on the device) has the bits of dist, on every row, ties included (both keep the lowest
index), and the mutual mask is the one the indices of `nn_distances` in both directions give.  The 4097 targets of the
second batch cross the 2048-point tile of the 3-D scan and the 1536-row tile of `feature_nn_kernel<4>` twice each."""
import numpy as np
import pytest
import torch

import overlap_cases as oc
from hotformerloc_amd import feature_correspondences, nn_distances, ops

pytestmark = pytest.mark.gpu


def dev(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def offsets(clouds):
    return np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)


def test_feature_nn_and_nn_dist_agree_bit_for_bit():
    batches, lowest = oc.pair_scan_batches(ops.OVERLAP_ROWS, ops.OVERLAP_TILE)
    seen = []
    for src, dst in batches:
        dist, idx, _ = nn_distances(dev(src), dev(dst))
        back = nn_distances(dev(dst), dev(src))[1]
        f_idx, f_d2, f_mask = (torch.cat(x) for x in feature_correspondences(dev(src), dev(dst), mutual=True))
        torch.cuda.synchronize()
        seen.append((dist, idx))
        assert f_idx.dtype == torch.int32 and f_d2.dtype == torch.float32 and f_mask.dtype == torch.bool
        assert torch.equal(f_idx, idx)                                   # every row, the pairs without a side included
        assert np.array_equal(bits(np.sqrt(f_d2.cpu().numpy())), bits(dist.cpu().numpy()))
        want = oc.mutual_from_indices(idx.cpu().numpy(), back.cpu().numpy(), offsets(src), offsets(dst))
        assert np.array_equal(f_mask.cpu().numpy(), want) and want.any() and not want.all()
    assert int(idx[0]) == lowest and float(dist[0]) == 0.0               # the tie across a tile edge: the lowest copy
    (a, b), (dist, idx) = batches[0], seen[0]
    off = offsets(a)
    assert len(a[1]) == 0 and len(b[2]) == 0                             # a pair without source, a pair without target
    assert (idx[off[2]:off[3]] == -1).all() and torch.isinf(dist[off[2]:off[3]]).all()
