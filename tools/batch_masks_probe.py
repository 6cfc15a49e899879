"""Time the two (B, B) masks of one training batch by three routes, at the shipped batch size.

B = 2048 labels (pairs of positives, as the reference's sampler draws them) over a synthetic index of 20 000 elements whose
lists are about 30 positives and 300 non-negatives long (`synthetic.tuple_lists`).

  device   `batch_masks.batch_masks` on host labels: the upload of B labels and ONE `hfl_batch_masks` launch.  Also the launch
           alone on device labels, between two HIP events over 50 back-to-back launches, against its algorithmic traffic
           (2 B^2 bytes written; the lists and labels are re-read from cache).
  host     the route without the kernel: `batch_masks_host` (numpy `np.isin` per row) plus the two host-to-device copies.
  python   the reference's style (`datasets/dataset_utils.py:118-123`): a double Python loop of one `np.searchsorted` per
           pair and mask, timed on a slice of `--python-rows` rows and scaled by B / rows, plus the same two copies at the
           host route's measured cost.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; every
route's masks are compared bit for bit before anything is timed.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import TupleIndex, batch_masks, batch_masks_host, ops      # noqa: E402
from hotformerloc_amd import synthetic as syn                                    # noqa: E402

HBM_PEAK_GBS = 8000.0


def in_sorted(e, array):
    pos = np.searchsorted(array, e)
    return pos != len(array) and array[pos] == e


def python_rows(index, labels, rows):
    pos = [[in_sorted(e, index.get_positives(label)) for e in labels] for label in labels[:rows]]
    neg = [[not in_sorted(e, index.get_non_negatives(label)) for e in labels] for label in labels[:rows]]
    return np.asarray(pos, bool), np.asarray(neg, bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--elements', type=int, default=20000)
    ap.add_argument('--python-rows', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--host-repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('batch_masks_probe needs a GPU: nothing is timed without one')
    b, n = args.batch, args.elements
    index = TupleIndex.from_csr(*syn.tuple_lists(n, 17, 30, 300))
    rng = np.random.RandomState(2)
    anchors = rng.randint(0, n, b // 2)
    mates = [int(index.get_positives(a)[rng.randint(len(index.get_positives(a)))]) for a in anchors]
    labels = np.stack([anchors, np.asarray(mates)], 1).reshape(-1)
    label_list = labels.tolist()
    rows = min(args.python_rows, b)
    res = {'batch': b, 'elements': n, 'mean_positives': round(index.pos_idx.size / n, 1),
           'mean_non_negatives': round(index.nn_idx.size / n, 1)}

    # the three routes agree before anything is timed
    dev = batch_masks(index, label_list)
    host = batch_masks_host(index, labels)
    py = python_rows(index, label_list, rows)
    assert np.array_equal(dev[0].cpu().numpy(), host[0]) and np.array_equal(dev[1].cpu().numpy(), host[1])
    assert np.array_equal(py[0], host[0][:rows]) and np.array_equal(py[1], host[1][:rows])

    def timed(fn, repeats, warmup):
        ms = []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}

    res['device_call'] = timed(lambda: batch_masks(index, label_list), args.repeats, args.warmup)
    res['host_isin_and_upload'] = timed(lambda: [torch.from_numpy(m).cuda() for m in batch_masks_host(index, labels)],
                                        args.host_repeats, 1)
    upload = timed(lambda: [torch.from_numpy(m).cuda() for m in host], args.host_repeats, 1)
    loop = timed(lambda: python_rows(index, label_list, rows), 3, 0)
    scale = b / rows
    res['python_loop_scaled'] = {'rows_timed': rows, 'slice_median_ms': loop['median_ms'],
                                 'median_ms': round(loop['median_ms'] * scale + upload['median_ms'], 1),
                                 'min_ms': round(loop['min_ms'] * scale + upload['min_ms'], 1),
                                 'max_ms': round(loop['max_ms'] * scale + upload['max_ms'], 1),
                                 'upload_median_ms': upload['median_ms']}
    # the launch alone
    dev_labels = torch.from_numpy(labels).cuda()
    outs = (torch.empty((b, b), dtype=torch.bool, device='cuda'), torch.empty((b, b), dtype=torch.bool, device='cuda'))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            ops.batch_masks(dev_labels, *index.dev, n, out=outs)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / 50)
    per = per[args.warmup:]
    ms = statistics.median(per)
    nbytes = 2 * b * b
    gbs = nbytes / (ms * 1e-3) / 1e9
    res['launch'] = {'median_ms': round(ms, 4), 'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4),
                     'algorithmic_bytes': nbytes, 'GBps': round(gbs, 1), 'frac_of_8TBps': round(gbs / HBM_PEAK_GBS, 4),
                     'how': '50 back-to-back launches into the same two matrices between two HIP events'}
    res['speedup_vs_host'] = round(res['host_isin_and_upload']['median_ms'] / res['device_call']['median_ms'], 1)
    res['speedup_vs_python'] = round(res['python_loop_scaled']['median_ms'] / res['device_call']['median_ms'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
