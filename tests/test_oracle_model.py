"""Pin `oracle.hotformer_ref` against the reference's own model outputs.

The fixtures tests/golden/model_*.npz were produced by `oracle/gen_golden.py`, which
imports the reference's Python model files in the build container; here only the
oracle runs (no reference needed), so this test also runs on the GPU box."""

import os

import numpy as np
import pytest
import torch

from hotformerloc_amd.params import load_config
from hotformerloc_amd import synthetic as syn
from oracle import hotformer_ref
from oracle.ocnn_ref import Octree, Points, merge_octrees
from oracle.testing import load_case, oracle_octree, synthetic_state_dict

CASES = ['wild_places_b1', 'wild_places_ragged', 'cs_wild_places_b2', 'oxford_b2', 'wild_places_b3', 'cs_campus3d_b2']


@pytest.mark.parametrize('case', CASES)
def test_oracle_matches_reference_golden(golden_dir, case):
    g = load_case(golden_dir, case)
    params, depth = load_config(g['cfg'])
    assert depth == g['octree_depth']
    octree = oracle_octree(g['clouds'], depth)
    assert np.array_equal(octree.nnum_nempty.numpy(), g['nnum_nempty'])
    sd = synthetic_state_dict(params)
    cap = {}
    y = hotformer_ref.forward(sd, params, octree, cap).numpy()
    ref = g['descriptors']
    rel = np.linalg.norm(y - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert rel.max() < 2e-5, rel
    for name, val in (('patch_embed', cap['patch_embed']), ('octf_out', cap['octf_out'])):
        head = g[name + '_head']
        assert np.abs(val[:head.shape[0]].numpy() - head).max() < 1e-4
        s = val.double()
        assert abs(s.sum().item() - g[name + '_sum'][0]) < 1e-3 * max(1.0, abs(g[name + '_sum'][0]))
    for d in cap['plan'].pyramid_depths:
        for kind in ('feat_final', 'rt_final'):
            head = g['%s_%d_head' % (kind, d)]
            val = cap['%s.%d' % (kind, d)]
            assert np.abs(val[:head.shape[0]].numpy() - head).max() < 2e-4


def test_oracle_matches_reference_on_the_bench_workload(golden_dir):
    """The batch `bench.py` times (32 clouds x 4096 points, Wild-Places cfg, 'init' weights): the oracle -- which the bench's
    `parity` block and `cpu_baseline` run -- against the reference's own descriptors for that batch
    (oracle/gen_golden.py::WORKLOAD_CASES)."""
    g = load_case(golden_dir, 'wild_places_b32')
    params, depth = load_config(g['cfg'])
    octree = oracle_octree(g['clouds'], depth)
    assert np.array_equal(octree.nnum_nempty.numpy(), g['nnum_nempty'])
    y = hotformer_ref.forward(synthetic_state_dict(params, g['profile']), params, octree).numpy()
    ref = g['descriptors']
    rel = np.linalg.norm(y - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert rel.max() < 2e-5, rel


def test_oracle_matches_reference_live(golden_dir):
    """The oracle against the reference model on a cs-wild-places batch with 'stress' weights: the reference is rerun where
    its tree is present, elsewhere its stored output for the same batch and weights is the yardstick
    (oracle/gen_golden_live.py -> tests/golden/model_live_cs_wild_places.npz)."""
    from oracle import ref_import
    g = np.load(os.path.join(golden_dir, 'model_live_cs_wild_places.npz'))
    offs = np.concatenate([[0], np.cumsum(g['n_points'])])
    clouds = [g['points'][offs[i]:offs[i + 1]] for i in range(len(g['n_points']))]
    octree = oracle_octree(clouds, 7)
    if ref_import.reference_available():
        model, params = ref_import.reference_model(
            os.path.join(ref_import.REFERENCE_ROOT, 'models', 'hotformerloc_cs-wild-places_cfg.txt'))
        syn.fill_synthetic_weights(model, 'stress')
        with torch.inference_mode():
            ref = model({'octree': octree})['global'].numpy()
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    else:
        params, _ = load_config('cs-wild-places')
        ref = g['descriptors']
        sd = synthetic_state_dict(params, 'stress')
    y = hotformer_ref.forward(sd, params, octree).numpy()
    rel = np.linalg.norm(y - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert rel.max() < 2e-5


@pytest.mark.parametrize('case', ['train_wild_places_ragged', 'train_cs_wild_places_ragged'])
def test_oracle_training_gradients_match_reference_with_stochastic_depth(golden_dir, case):
    """The oracle's train-mode forward AND backward against the reference's own autograd: fp64 on both sides, stochastic
    depth on with the per-cloud draws the reference made (oracle/gen_golden_train.py -> tests/golden/train_*.npz).  Pins
    the row-to-cloud rules of the drop paths (tokens their own cloud, relay rows their window's owner, padding the last
    cloud, the relay-token block by padded row) and every parameter gradient, through its sketch, within 1e-8."""
    from oracle.testing import grad_sketch, load_train_case, sketch_error
    g = load_train_case(golden_dir, case)
    params, depth = load_config(g['cfg'])
    assert depth == g['octree_depth']
    octree = oracle_octree(g['clouds'], depth)
    assert np.array_equal(octree.nnum_nempty.numpy(), g['nnum_nempty'])
    B = len(g['clouds'])
    sd = {k: v.double().requires_grad_() for k, v in synthetic_state_dict(params, g['profile']).items()}
    factors = {k: torch.from_numpy(v) for k, v in g['factor_dict'].items()}
    y = hotformer_ref.forward_with_grad(sd, params, octree, drop_factors=factors)
    proj = torch.from_numpy(syn.hash_uniform(4242, B * 256).reshape(B, 256))
    (y * proj).sum().backward()
    ref = g['desc64']
    rel = np.linalg.norm(y.detach().numpy() - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert rel.max() <= 1e-8, rel
    assert sorted(sd) == sorted(g['grad_names']), set(sd) ^ set(g['grad_names'])
    errs = {}
    for i, name in enumerate(g['grad_names']):
        got = grad_sketch(sd[name].grad.numpy())
        errs[name] = sketch_error(got, g['grad_norm'][i], g['grad_entries'][i], g['grad_proj'][i], int(g['grad_numel'][i]))
    worst = max(errs, key=errs.get)
    print(case, 'descriptor rel', rel.max(), 'worst gradient sketch error', worst, errs[worst])
    assert errs[worst] <= 1e-8, (worst, errs[worst])
