"""Stochastic depth and training gradients against the reference itself.

The fixtures tests/golden/train_*.npz (oracle/gen_golden_train.py) hold a train-mode forward and backward of the
reference's own model files with stochastic depth on (drop_path = 0.5, as the configs train): the per-cloud factor of every
drop-path call, keyed by the reference module name, the fp64 descriptors and a sketch of every fp64 parameter gradient
(oracle.testing.grad_sketch), next to the exact error of the reference's own fp32 run.  Here the product replays those
factors through `arm_drop_paths` on the MI355X, in GEMM mode x3, in x6 and on x6's fp32 library route, with and without
gradient checkpointing, and must land on the reference.  Two negative controls (factors shifted by one cloud, attention and
MLP rows swapped) must miss by far, so a wrong row-to-cloud mapping cannot pass."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import build_batch_octree, load_config, model_factory
from hotformerloc_amd import model as M
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.model import OctreeDropPath, set_checkpoint_policy, set_gemm_mode, set_train_x6
from oracle.testing import grad_sketch, load_train_case, sketch_error

REL_TOL = 1e-3            # descriptors, rel-L2 per cloud against the fp64 reference
GRAD_TOL = 1e-3           # every parameter gradient (its sketch) against the fp64 reference
# x6 and its fp32 library route are fp32-grade: per tensor within MATCHED x the reference's own fp32 error (floor 1e-6),
# and never above GRAD_TOL.  Measured on an MI355X: worst ratio 8.5 (x6) and 8.6 (fp32 route), both on Linear weights;
# the two routes differ by little, the rest is the order of the sums outside the GEMMs.  x3 runs at up to 38x.
MATCHED = 12.0
MATCHED_FLOOR = 1e-6
# a negative control must miss the bar by at least this factor (measured: 3300x to 5700x)
NEGATIVE_MARGIN = 10.0

CASES = ['train_wild_places_ragged', 'train_cs_wild_places_ragged', 'train_cs_wild_places_b8_var']
_CASES = {}


def _case(golden_dir, case):
    if case not in _CASES:
        _CASES[case] = load_train_case(golden_dir, case)
    return _CASES[case]


def _kind(name):
    return 'rpe_table' if 'rpe_table' in name else name.split('.')[-1]


def _run(g, mode, checkpoint, monkeypatch, factors=None):
    """Train-mode forward + backward of (y * proj).sum() with the fixture's factors replayed; returns
    (descriptor rel-L2 per cloud, {name: gradient sketch error}, draw log)."""
    params, depth = load_config(g['cfg'])
    assert params.drop_path == 0.5 and depth == g['octree_depth']
    factors = g['factor_dict'] if factors is None else factors
    model = model_factory(params)
    syn.fill_synthetic_weights(model, g['profile'])
    model = model.cuda().train()
    names = {m: n for n, m in model.named_modules()}
    active = {names[m]: m for m in model.modules() if isinstance(m, OctreeDropPath) and m.drop_prob > 0.0}
    assert not set(active) - set(factors), ('product drop paths without recorded factors', set(active) - set(factors))
    assert not set(factors) - set(active), ('recorded drop paths without a product module', set(factors) - set(active))

    def arm(model_, batch_size, device, dtype=torch.float32):
        assert model_ is model and batch_size == len(g['clouds'])
        for n, m in active.items():
            m._factors = torch.from_numpy(np.ascontiguousarray(factors[n])).to(device=device, dtype=dtype)
            m._calls = 0
    monkeypatch.setattr(M, 'arm_drop_paths', arm)

    # every draw, counted as it happens (`_checkpoint_block` resets and restores `_calls`, so its final value says nothing)
    log = []
    draw = OctreeDropPath._draw

    def counted_draw(self, batch_size, dtype, device):
        f = self._factors
        log.append((names.get(self), None if f is None else self._calls % f.shape[0]))
        return draw(self, batch_size, dtype, device)
    monkeypatch.setattr(OctreeDropPath, '_draw', counted_draw)

    B = len(g['clouds'])
    proj = torch.from_numpy(syn.hash_uniform(4242, B * 256).reshape(B, 256).astype(np.float32)).cuda()
    set_gemm_mode('x3' if mode == 'x3' else 'x6')
    set_train_x6(mode != 'x6-fp32')
    prev = set_checkpoint_policy('always' if checkpoint else 'never')
    try:
        octree = build_batch_octree(g['clouds'], depth, 2, 'cuda')
        assert np.array_equal(octree.nnum_nempty.cpu().numpy(), g['nnum_nempty'])
        y = model({'octree': octree})['global']
        (y * proj).sum().backward()
        torch.cuda.synchronize()
    finally:
        set_checkpoint_policy(prev)
        set_train_x6(True)
        set_gemm_mode('x3')

    # the draws: no fresh one, every active module took both armed rows -- once per forward, and a second time in the
    # recomputation under checkpointing
    fresh = [n for n, r in log if r is None]
    assert not fresh, ('drop paths drew fresh factors', sorted(set(map(str, fresh)))[:8])
    counts = {}
    for n, r in log:
        counts[(n, r)] = counts.get((n, r), 0) + 1
    allowed = (1, 2) if checkpoint else (1,)
    for n in active:
        for r in (0, 1):
            assert counts.get((n, r), 0) in allowed, (n, r, counts.get((n, r), 0))
    if checkpoint:
        assert any(c == 2 for c in counts.values()), 'checkpointing on, but no block replayed its draws'

    want = g['desc64']
    got = y.detach().double().cpu().numpy()
    desc = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(grads) == sorted(g['grad_names']), set(grads) ^ set(g['grad_names'])
    errs = {}
    for i, n in enumerate(g['grad_names']):
        assert grads[n] is not None, n
        errs[n] = sketch_error(grad_sketch(grads[n].double().cpu().numpy()), g['grad_norm'][i], g['grad_entries'][i],
                               g['grad_proj'][i], int(g['grad_numel'][i]))
    return desc, errs, counts


def _report(case, mode, checkpoint, g, desc, errs):
    ref32 = dict(zip(g['grad_names'], g['grad_rel32']))
    kinds = {}
    for n, e in errs.items():
        k = kinds.setdefault(_kind(n), [0.0, 0.0, 0.0])
        k[0] = max(k[0], e)
        k[1] = max(k[1], ref32[n])
        k[2] = max(k[2], e / max(ref32[n], MATCHED_FLOOR / MATCHED))     # the x6 bar is MATCHED x this denominator
    d32 = np.linalg.norm(g['desc32'] - g['desc64'], axis=1) / np.linalg.norm(g['desc64'], axis=1)
    print('\n%s %s checkpoint=%s: descriptor rel %.3g (reference fp32 %.3g)' % (case, mode, checkpoint, desc.max(), d32.max()))
    for k, (e, r, q) in sorted(kinds.items()):
        print('  %-10s worst grad error %.3g   reference fp32 worst %.3g   worst ratio %.3g' % (k, e, r, q))


RUNS = [(c, m, ck) for c in CASES for m in ('x3', 'x6', 'x6-fp32') for ck in (True, False)
        if ck or c == 'train_wild_places_ragged']


@pytest.mark.parametrize('case,mode,checkpoint', RUNS)
def test_training_with_stochastic_depth_matches_reference(golden_dir, monkeypatch, case, mode, checkpoint):
    g = _case(golden_dir, case)
    desc, errs, _ = _run(g, mode, checkpoint, monkeypatch)
    _report(case, mode, checkpoint, g, desc, errs)
    assert desc.max() <= REL_TOL, desc
    if mode == 'x3':
        bad = {n: e for n, e in errs.items() if not e <= GRAD_TOL}
    else:
        ref32 = dict(zip(g['grad_names'], g['grad_rel32']))
        bad = {n: (e, ref32[n]) for n, e in errs.items()
               if not e <= min(GRAD_TOL, max(MATCHED * ref32[n], MATCHED_FLOOR))}
    assert not bad, sorted(bad.items(), key=lambda kv: -np.max(kv[1]))[:8]


NEGATIVE = {
    'factors shifted by one cloud': lambda f: {n: np.roll(v, 1, axis=1) for n, v in f.items()},
    'attention and MLP rows swapped': lambda f: {n: v[::-1] for n, v in f.items()},
}


@pytest.mark.parametrize('control', list(NEGATIVE))
@pytest.mark.parametrize('case', ['train_wild_places_ragged', 'train_cs_wild_places_ragged'])
def test_wrong_drop_path_mapping_is_detected(golden_dir, monkeypatch, case, control):
    """Negative control: the same x3 run with the recorded factors mapped wrongly must miss the bars of
    test_training_with_stochastic_depth_matches_reference by at least NEGATIVE_MARGIN."""
    g = _case(golden_dir, case)
    factors = NEGATIVE[control](g['factor_dict'])
    assert any(not np.array_equal(factors[n], v) for n, v in g['factor_dict'].items())
    desc, errs, _ = _run(g, 'x3', False, monkeypatch, factors)
    margin = max(desc.max() / REL_TOL, max(errs.values()) / GRAD_TOL)
    print('\n%s, %s: descriptor rel %.3g, worst grad error %.3g -> %.0fx the bar: detected'
          % (case, control, desc.max(), max(errs.values()), margin))
    assert margin >= NEGATIVE_MARGIN, margin
