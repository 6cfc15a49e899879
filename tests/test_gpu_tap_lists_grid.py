"""hfl_tap_lists at the row counts around its block geometry: a wave is 64 rows, a workgroup 256 (one row per thread; rounds
2-6 gave a workgroup four such slices), and the scan walks the per-block counts 64 at a time.  Integer work: bit for bit against a
stable compaction in numpy."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import ops

DEV = 'cuda'
ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)


def _table(rows, taps, density, seed):
    rng = np.random.default_rng(seed)
    table = rng.integers(0, max(rows, 2), size=(rows, taps), dtype=np.int32)
    if density < 1.0:
        table[rng.random((rows, taps)) >= density] = -1
    return table


def _want(table):
    """(src, slot, edges): pairs by tap, rows ascending inside a tap."""
    rows, taps = table.shape
    live_t = (table >= 0).T                                        # (taps, rows): flattening it IS the list order
    counts = live_t.sum(1)
    edges = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    src = table.T[live_t]
    rank = np.cumsum(live_t.reshape(-1)) - 1
    slot = np.where(live_t, rank.reshape(taps, rows), -1).T.astype(np.int32)
    return src, slot, edges


def _check(got, table):
    src, slot, edges = got
    w_src, w_slot, w_edges = _want(table)
    assert np.array_equal(edges.cpu().numpy(), w_edges)
    assert np.array_equal(slot.cpu().numpy(), w_slot)
    assert np.array_equal(src[:int(w_edges[-1])].cpu().numpy().reshape(-1), w_src)


@pytest.mark.parametrize('taps', [8, 9, 27])
@pytest.mark.parametrize('density', [0.0, 0.2, 1.0])
def test_tap_lists_at_every_block_boundary(taps, density):
    """The 8-tap, the generic and the 27-tap path, with no live pair, one in five, and all of them."""
    for rows in ROWS:
        table = _table(rows, taps, density, rows * 100 + taps)
        _check(ops.tap_lists(torch.from_numpy(table).to(DEV)), table)


def test_sixteen_tables_in_one_call_equal_the_single_table_calls():
    """One hfl_tap_lists_multi call over 16 tables of mixed sizes and widths, one of them a single row."""
    shapes = [(5000, 27), (1, 27), (257, 8), (1024, 9), (63, 27), (1025, 8), (256, 27), (3000, 5), (65, 8), (255, 9), (1023, 27),
              (64, 8), (2049, 27), (1, 8), (700, 32), (4097, 8)]
    tables = [_table(r, t, 0.2 if i % 5 else 1.0, 7 * i + 1) for i, (r, t) in enumerate(shapes)]
    dev = [torch.from_numpy(t).to(DEV) for t in tables]
    edges = [torch.empty(t.shape[1] + 1, dtype=torch.int32, device=DEV) for t in dev]
    multi = ops.tap_lists_multi(dev, edges)
    assert len(multi) == 16
    for t, d, (src, slot, e) in zip(tables, dev, multi):
        _check((src, slot, e), t)
        src1, slot1, e1 = ops.tap_lists(d)
        n = int(e1[-1])
        assert torch.equal(e, e1) and torch.equal(slot, slot1) and torch.equal(src[:n], src1[:n])
