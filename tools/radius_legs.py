"""What the `--radius` option of tools/normals_probe.py, tools/fpfh_probe.py and tools/outlier_probe.py shares: the radius at
which a ball holds about k points, and a timing loop that ALTERNATES the routes it compares -- k nearest, hybrid,
radius-only -- so that whatever else the machine does falls on all of them alike.  Whole calls, wall clock with a device
synchronisation on both sides; median / min / max of `repeats` rounds after `warmup`."""
import statistics
import time

import torch

from hotformerloc_amd import outliers


def mean_count(resident, radius, with_pending=False):
    counts, pending = outliers.radius_neighbour_counts(resident, radius, return_pending=True)
    mean = float(sum(int(c.sum()) for c in counts)) / sum(int(c.shape[0]) for c in counts)
    return (mean, pending) if with_pending else mean


def pick_radius(resident, k, low=1e-3, high=100.0, steps=18):
    """the radius, by bisection in log space on `radius_neighbour_counts`, at which the mean |N(i)| of the batch is about k"""
    for _ in range(steps):
        mid = (low * high) ** 0.5
        if mean_count(resident, mid) < k:
            low = mid
        else:
            high = mid
    return high


def alternate(routes, repeats, warmup):
    """{name: {'median_ms', 'min_ms', 'max_ms'}} of the callables of `routes`, run one after the other in every round"""
    ms = {name: [] for name in routes}
    for i in range(warmup + repeats):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {'median_ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)}
            for name, v in ms.items()}


def radius_of(args, resident, k):
    """(the radius of the leg, how it was chosen)"""
    if args.radius > 0.0:
        return float(args.radius), 'given'
    return pick_radius(resident, k), 'mean count about k'


def add_arguments(ap):
    ap.add_argument('--radius', type=float, default=None,
                    help='also time the hybrid and the radius-only neighbourhood against the k nearest, the three routes '
                         'alternating; 0 picks the radius at which a ball holds about k points')
    ap.add_argument('--only-radius', action='store_true', help='the --radius leg alone')
