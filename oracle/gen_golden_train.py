"""Generate the stochastic-depth training fixtures tests/golden/train_<case>.npz (BUILD CONTAINER ONLY).

TEST INFRASTRUCTURE (see oracle/__init__.py).  Runs the reference's own Python model files (oracle/ref_import.py) in train
mode with its stochastic depth ON (`OctreeDropPath`, models/layers/octformer_layers.py:213-289) and records what a test
needs to replay the same forward and backward elsewhere:

  * every drop-path call draws its `rand(B, 1)` from one seeded generator here; the per-cloud factor
    floor(u + keep) / keep (0 or 1 / keep) is stored, keyed by the reference module name, row 0 = the attention branch
    (first call), row 1 = the MLP branch (second call).  A call whose clouds all come out the same is re-drawn, so every
    call drops some clouds and keeps others (a fixture, not the reference's distribution);
  * the reference then receives u = 0 (drop) or 1 - keep / 2 (keep), so that it computes exactly the recorded decision in
    its own arithmetic, in fp64 and in fp32 alike;
  * grad checkpointing is off (`grad_checkpoint = False` on octf_stage.0 and hotf_stage): every active module is called
    exactly twice;
  * one octree, built from float32 points as the product does, serves both runs; only the model and the input feature
    are cast to fp64;
  * forward and backward of (y * proj).sum(), proj = hash_uniform(4242, B * 256) as in the other gradient tests, once in
    fp64 (the truth) and once in fp32 (the reference's own fp32 error).

    tests/golden/train_<case>.npz
        cfg, octree_depth, profile     model cfg, octree depth, synthetic weight profile
        points_case                    '' or the model_<case>.npz fixture whose points are used (then no `points`)
        n_points, points               the clouds (after the coordinate transform), float32
        nnum_nempty                    per-depth node counts of the merged octree
        factor_names, factors          (M,) reference module names, (M, 2, B) float64 factors
        desc64, desc32                 (B, 256) descriptors of the fp64 and the fp32 run
        grad_names, grad_numel         (P,) parameter names, element counts
        grad_norm, grad_entries, grad_proj
                                       fp64 gradient sketch (oracle.testing.grad_sketch): L2 norm, 64 strided entries,
                                       16 projections onto hash-seeded +-1 vectors
        grad_rel32                     (P,) exact rel-L2 of the fp32 run's gradient against the fp64 one

Usage:  python -m oracle.gen_golden_train [case ...]
"""

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import                                    # noqa: E402
from oracle.testing import grad_sketch, oracle_octree            # noqa: E402
from hotformerloc_amd import synthetic as syn                     # noqa: E402

FACTOR_SEED = 20261016
PROJ_SEED = 4242

# case -> (cfg, octree depth, weight profile, points: name of a model_<case>.npz fixture or a list of (n, kind, seed))
#
# train_cs_wild_places_b8_var is config 3's 8-cloud workload at full size (76 k points, fp64 forward + backward of the
# reference on the CPU in a few minutes): no reduction in clouds was needed.
CASES = {
    'train_wild_places_ragged': ('wild-places', 7, 'stress', 'wild_places_ragged'),
    'train_cs_wild_places_ragged': ('cs-wild-places', 7, 'stress',
                                    [(6000, 'forest', 3100), (40, 'ball', 3101), (4096, 'ball', 3102)]),
    'train_cs_wild_places_b8_var': ('cs-wild-places', 7, 'init', 'cs_wild_places_b8_var'),
}


def case_clouds(spec, coordinates):
    if isinstance(spec, str):
        z = np.load(os.path.join(ROOT, 'tests', 'golden', 'model_%s.npz' % spec))
        offs = np.concatenate([[0], np.cumsum(z['n_points'])])
        return [z['points'][offs[i]:offs[i + 1]] for i in range(len(z['n_points']))]
    clouds = []
    for n, kind, seed in spec:
        pc = syn.unit_ball_cloud(seed, n) if kind == 'ball' else syn.forest_cloud(seed, n)
        if coordinates == 'cylindrical':
            pc = syn.cylindrical(pc)
        clouds.append(np.ascontiguousarray(pc, dtype=np.float32))
    return clouds


def draw_factors(names_probs, batch, seed):
    """{name: (2, B) float64}: floor(u + keep) / keep per call, re-drawn until a call both drops and keeps."""
    g = np.random.default_rng(seed)
    out = {}
    for name, p in names_probs:
        keep = 1.0 - p
        rows = []
        for _ in range(2):
            while True:
                u = g.random(batch)
                f = np.floor(u + keep) / keep
                if (f == 0).any() and (f != 0).any():
                    break
            rows.append(f)
        out[name] = np.stack(rows)
    return out


def run_reference(cfg_path, profile, octree, factors, proj, dtype):
    """Train-mode forward + backward of the reference with the recorded factors; returns (y, {name: grad}, calls)."""
    import models.layers.octformer_layers as L             # noqa: E402  (reference, importable after reference_model)
    model, _ = ref_import.reference_model(cfg_path)
    syn.fill_synthetic_weights(model, profile)
    model = model.to(dtype).train()
    base = model.backbone.backbone
    base.octf_stage[0].grad_checkpoint = False
    base.hotf_stage.grad_checkpoint = False
    names = {m: n for n, m in model.named_modules()}

    # float32 inputs built inside the reference (input feature, ADaPE window statistics) meet the fp64 weights here
    def to_weight_dtype(mod, args):
        return tuple(a.to(mod.weight.dtype) if torch.is_tensor(a) and a.is_floating_point() else a for a in args)
    hooks = [m.register_forward_pre_hook(to_weight_dtype) for m in model.modules() if isinstance(m, torch.nn.Linear)]
    get_feat = model.get_input_feature
    model.get_input_feature = lambda o: get_feat(o).to(dtype)

    calls = {}
    orig_forward = L.OctreeDropPath.forward
    orig_rand = torch.rand

    def forward(self, data, *a, **k):
        name = names[self]
        i = calls.get(name, 0)
        if self.drop_prob <= 0.0 or not self.training:
            return orig_forward(self, data, *a, **k)
        calls[name] = i + 1
        f = factors[name][i]
        keep = 1.0 - self.drop_prob
        u = np.where(f > 0, 1.0 - keep / 2, 0.0)

        def rand(*shape, dtype=None, device=None, **kw):
            assert tuple(shape) == (len(f), 1), shape
            return torch.from_numpy(u).reshape(-1, 1).to(dtype=dtype or torch.float32, device=device)
        torch.rand = rand
        try:
            return orig_forward(self, data, *a, **k)
        finally:
            torch.rand = orig_rand
    L.OctreeDropPath.forward = forward
    try:
        y = model({'octree': octree})['global']
        (y * proj.to(dtype)).sum().backward()
    finally:
        L.OctreeDropPath.forward = orig_forward
        for h in hooks:
            h.remove()
    grads = {n: p.grad.detach().double().numpy().reshape(-1) for n, p in model.named_parameters() if p.grad is not None}
    return y.detach(), grads, calls


def build_case(case):
    cfg, depth, profile, spec = CASES[case]
    cfg_path = os.path.join(ref_import.REFERENCE_ROOT, 'models', 'hotformerloc_%s_cfg.txt' % cfg)
    model, params = ref_import.reference_model(cfg_path)
    clouds = case_clouds(spec, params.coordinates)
    B = len(clouds)
    import models.layers.octformer_layers as L             # noqa: E402  (reference)
    active = [(n, float(m.drop_prob)) for n, m in model.named_modules()
              if isinstance(m, L.OctreeDropPath) and m.drop_prob > 0.0]
    factors = draw_factors(active, B, FACTOR_SEED + B)
    proj = torch.from_numpy(syn.hash_uniform(PROJ_SEED, B * 256).reshape(B, 256))

    octree = oracle_octree(clouds, depth)
    nne = octree.nnum_nempty.clone()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        t = time.time()
        y, grads, calls = run_reference(cfg_path, profile, octree, factors, proj, dtype)
        assert torch.equal(octree.nnum_nempty, nne)
        assert set(calls) == set(factors) and all(c == 2 for c in calls.values()), calls
        assert torch.isfinite(y).all()
        runs[dtype] = (y, grads)
        print('  %s %s: %.1f s, %d drop-path modules x 2 calls' % (case, dtype, time.time() - t, len(calls)))

    y64, g64 = runs[torch.float64]
    y32, g32 = runs[torch.float32]
    names = sorted(g64)
    sk = [grad_sketch(g64[n]) for n in names]
    rel32 = [np.linalg.norm(g32[n] - g64[n]) / max(np.linalg.norm(g64[n]), 1e-300) for n in names]
    fnames = sorted(factors)
    out = dict(cfg=np.array(cfg), octree_depth=np.array(depth), profile=np.array(profile),
               points_case=np.array(spec if isinstance(spec, str) else ''),
               n_points=np.array([c.shape[0] for c in clouds], dtype=np.int64),
               nnum_nempty=nne.numpy(),
               factor_names=np.array(fnames), factors=np.stack([factors[n] for n in fnames]),
               desc64=y64.numpy(), desc32=y32.numpy().astype(np.float32),
               grad_names=np.array(names), grad_numel=np.array([g64[n].size for n in names], dtype=np.int64),
               grad_norm=np.array([s[0] for s in sk]), grad_entries=np.stack([s[1] for s in sk]),
               grad_proj=np.stack([s[2] for s in sk]), grad_rel32=np.array(rel32))
    if not isinstance(spec, str):
        out['points'] = np.ascontiguousarray(np.concatenate(clouds, 0).astype(np.float32))
    return out


def main():
    dst = os.path.join(ROOT, 'tests', 'golden')
    torch.set_num_threads(os.cpu_count())
    for case in (sys.argv[1:] or list(CASES)):
        out = build_case(case)
        path = os.path.join(dst, '%s.npz' % case)
        np.savez_compressed(path, **out)
        d64, d32 = out['desc64'], out['desc32']
        rel = np.linalg.norm(d32 - d64, axis=1) / np.linalg.norm(d64, axis=1)
        print(case, out['n_points'].tolist(), 'nne', out['nnum_nempty'].tolist(), 'fp32 desc rel', rel.max(),
              'fp32 grad rel-L2 max / median', out['grad_rel32'].max(), np.median(out['grad_rel32']),
              '%.0f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
