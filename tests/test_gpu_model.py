"""End-to-end GPU parity: `model_factory(params)(batch)['global']` on the MI355X path against
(1) the committed golden descriptors produced by the reference's own model files and
(2) the CPU oracle run here on the same inputs, with intermediates compared stage by stage.

Tolerance (BASELINE.json north_star): relative L2 per descriptor <= 1e-3 in fp32."""

import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import (Octree, Points, merge_octrees, build_batch_octree, load_config,
                              model_factory)
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.model import set_gemm_mode
from oracle import hotformer_ref
from oracle.testing import load_case, oracle_octree, synthetic_state_dict

REL_TOL = 1e-3
GRAD_TOL = 1e-3         # parameter gradients: relative L2 per tensor against autograd through the CPU oracle (worst observed 8.5e-4)
CASES = ['wild_places_b1', 'wild_places_b3', 'wild_places_ragged', 'cs_wild_places_b2', 'oxford_b2', 'cs_campus3d_b2']


def _device_model(params, profile='stress'):
    model = model_factory(params)
    syn.fill_synthetic_weights(model, profile)
    return model.cuda().eval()


def _run_with_capture(model, octree):
    cap = {}
    base = model.backbone.backbone
    hooks = [base.patch_embed.register_forward_hook(lambda m, i, o: cap.__setitem__('patch_embed', o)),
             base.downsample[0].register_forward_hook(lambda m, i, o: cap.__setitem__('octf_out', o)),
             base.hotf_stage.register_forward_hook(lambda m, i, o: cap.__setitem__('hotf', o))]
    with torch.inference_mode():
        y = model({'octree': octree})['global']
    for h in hooks:
        h.remove()
    return y, cap


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-12)


def _stage_err(got, want) -> float:
    """Error of an intermediate tensor, every stage held to the same 1e-3 bar as the descriptor: largest
    element difference relative to the largest reference magnitude (the stages are LayerNorm-fed feature maps;
    a per-element relative error would be dominated by values that cancel to ~0)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-12))


@pytest.fixture(params=['x3', 'bf16x3', 'fp32', 'x6'])
def gemm_mode(request):
    """Linear layers on the hand-written split-bf16 GEMM (default), as one hipBLASLt split-bf16 GEMM, as hipBLASLt fp32
    GEMMs, or at matched precision on the hand-written three-plane GEMM (hfl_linear_x6: transformer blocks, stem and
    downsample convolutions)."""
    set_gemm_mode(request.param)
    yield request.param
    set_gemm_mode('x3')


@pytest.mark.parametrize('case', CASES)
def test_descriptors_match_reference_golden(golden_dir, case, gemm_mode):
    g = load_case(golden_dir, case)
    params, depth = load_config(g['cfg'])
    model = _device_model(params)
    # the reference's own call sequence: per-cloud Octree -> merge -> to(device) -> neighbours
    octs = []
    for pc in g['clouds']:
        o = Octree(depth, 2)
        o.build_octree(Points(torch.from_numpy(pc)))
        octs.append(o)
    octree = merge_octrees(octs).to('cuda')
    octree.construct_all_neigh()
    assert np.array_equal(octree.nnum_nempty.numpy(), g['nnum_nempty'])
    y, cap = _run_with_capture(model, octree)
    y = y.cpu().numpy()
    assert y.shape == g['descriptors'].shape and np.isfinite(y).all()
    report = {'descriptor': float(_rel(y, g['descriptors']).max())}
    for name in ('patch_embed', 'octf_out'):
        head = g[name + '_head']
        report[name] = _stage_err(cap[name][:head.shape[0]], head)
        s = cap[name].double()
        # checksum over the whole tensor (the head covers the first rows only): relative to the sum of magnitudes
        report[name + '_sum'] = abs(s.sum().item() - g[name + '_sum'][0]) / max(s.abs().sum().item(), 1e-12)
    feats, rts = cap['hotf']
    for d in feats:
        head = g['feat_final_%d_head' % d]
        report['feat_final_%d' % d] = _stage_err(feats[d][:head.shape[0]], head)
        head = g['rt_final_%d_head' % d]
        nreal = min(head.shape[0], -(-feats[d].shape[0] // params.patch_size))   # skip padding windows
        report['rt_final_%d' % d] = _stage_err(rts[d][:nreal], head[:nreal])
    print(case, gemm_mode, report)
    bad = {k: v for k, v in report.items() if not v <= REL_TOL}
    assert not bad, (bad, report)
    assert np.allclose(np.linalg.norm(y, axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize('case', ['wild_places_b32', 'cs_wild_places_b8_var'])
@pytest.mark.parametrize('mode', ['x3', 'fp32', 'x6'])
def test_full_size_workloads_match_reference_golden(golden_dir, case, mode):
    """BASELINE configs 2 and 3 at their real sizes against the REFERENCE's own output (oracle/gen_golden.py::WORKLOAD_CASES:
    the reference model files run in the build container on the bench's batch -- 32 clouds x 4096 points, Wild-Places cfg,
    the bench's 'init' weights -- and on 8 clouds of config 3's generator, 4.5 k .. 23 k points, CS-Wild-Places cfg):
    descriptors within 1e-3 relative L2 per cloud, in the default split-bf16 mode and with fp32 Linear layers."""
    g = load_case(golden_dir, case)
    params, depth = load_config(g['cfg'])
    set_gemm_mode(mode)
    try:
        model = _device_model(params, g['profile'])
        octs = []
        for pc in g['clouds']:
            o = Octree(depth, 2)
            o.build_octree(Points(torch.from_numpy(pc)))
            octs.append(o)
        octree = merge_octrees(octs).to('cuda')
        octree.construct_all_neigh()
        assert np.array_equal(octree.nnum_nempty.numpy(), g['nnum_nempty'])
        y, cap = _run_with_capture(model, octree)
    finally:
        set_gemm_mode('x3')
    y = y.cpu().numpy()
    assert y.shape == g['descriptors'].shape and np.isfinite(y).all()
    report = {'descriptor': float(_rel(y, g['descriptors']).max())}
    for name in ('patch_embed', 'octf_out'):
        head = g[name + '_head']
        report[name] = _stage_err(cap[name][:head.shape[0]], head)
    feats, rts = cap['hotf']
    for d in feats:
        head = g['feat_final_%d_head' % d]
        report['feat_final_%d' % d] = _stage_err(feats[d][:head.shape[0]], head)
    print(case, mode, report)
    bad = {k: v for k, v in report.items() if not v <= REL_TOL}
    assert not bad, (bad, report)


_ORACLE_CACHE = {}


@pytest.mark.parametrize('cfg,octree_depth,sizes', [('wild-places', 7, [4096, 1500, 4096]),
                                                    ('cs-wild-places', 7, [5500, 4096])])
def test_stage_by_stage_against_oracle(cfg, octree_depth, sizes, gemm_mode):
    """Fresh inputs (not in the fixtures), both weight profiles; oracle run live on the CPU."""
    params, _ = load_config(cfg)
    clouds = syn.make_clouds(77, len(sizes), 4096, params.coordinates)
    clouds = [c[:n] if n <= 4096 else np.concatenate([c, syn.forest_cloud(5, n - 4096)])
              for c, n in zip(clouds, sizes)]
    if params.coordinates == 'cylindrical':
        clouds = [np.clip(c, -0.999, 0.999) for c in clouds]
    for profile in ('stress', 'init'):
        key = (cfg, profile)
        if key not in _ORACLE_CACHE:                 # the CPU oracle dominates the run time: once per case
            sd = synthetic_state_dict(params, profile)
            ocap = {}
            want = hotformer_ref.forward(sd, params, oracle_octree(clouds, octree_depth), ocap).numpy()
            _ORACLE_CACHE[key] = (want, ocap)
        want, ocap = _ORACLE_CACHE[key]
        model = _device_model(params, profile)
        octree = build_batch_octree(clouds, octree_depth, 2, 'cuda')
        y, cap = _run_with_capture(model, octree)
        errs = {'patch_embed': _stage_err(cap['patch_embed'], ocap['patch_embed']),
                'octf_out': _stage_err(cap['octf_out'], ocap['octf_out'])}
        feats, rts = cap['hotf']
        for d in feats:
            errs['feat_final.%d' % d] = _stage_err(feats[d], ocap['feat_final.%d' % d])
            nreal = -(-feats[d].shape[0] // params.patch_size)                  # skip padding windows
            errs['rt_final.%d' % d] = _stage_err(rts[d][:nreal], ocap['rt_final.%d' % d][:nreal])
        errs['descriptor'] = float(_rel(y.cpu().numpy(), want).max())
        print(cfg, profile, gemm_mode, errs)
        bad = {k: v for k, v in errs.items() if not v <= REL_TOL}
        assert not bad, (bad, errs)


def test_batch_composition_semantics():
    """Descriptors depend on the ordered batch (windows straddle clouds): the
    first cloud is batch-invariant, and a contiguous sub-batch evaluated alone equals the
    oracle on that same sub-batch (the multi-GPU sharding contract, section 8e)."""
    params, depth = load_config('wild-places')
    model = _device_model(params)
    clouds = syn.make_clouds(31, 4, 4096, params.coordinates)
    with torch.inference_mode():
        full = model({'octree': build_batch_octree(clouds, depth, 2, 'cuda')})['global'].cpu().numpy()
        solo = model({'octree': build_batch_octree(clouds[:1], depth, 2, 'cuda')})['global'].cpu().numpy()
        sub = model({'octree': build_batch_octree(clouds[2:], depth, 2, 'cuda')})['global'].cpu().numpy()
    assert _rel(solo[0], full[0]) < 1e-4
    sd = synthetic_state_dict(params)
    want = hotformer_ref.forward(sd, params, oracle_octree(clouds[2:], depth)).numpy()
    assert _rel(sub, want).max() <= REL_TOL
    # determinism: same inputs, same bits
    with torch.inference_mode():
        again = model({'octree': build_batch_octree(clouds, depth, 2, 'cuda')})['global'].cpu().numpy()
    assert np.array_equal(full, again)


_ORACLE_GRADS = {}


@pytest.mark.parametrize('cfg,sizes,linear', [('cs-wild-places', [2000, 1400], 'x3'),
                                              ('wild-places', [1300, 800, 1000], 'x3'),
                                              ('wild-places', [1300, 800, 1000], 'fp32'),
                                              ('cs-wild-places', [2000, 1400], 'bf16x3-lt')])
def test_forward_backward_matches_oracle_autograd(cfg, sizes, linear):
    """BASELINE config 3 (fwd+bwd): parameter gradients of the HIP training path against torch
    autograd through the CPU oracle, drop_path = 0.  Stochastic depth is checked against the reference with its recorded
    draws in tests/test_gpu_train_drop_path.py."""
    params, depth = load_config(cfg)
    clouds = [syn.forest_cloud(1400 + i, n) if i % 2 else syn.unit_ball_cloud(1400 + i, n)
              for i, n in enumerate(sizes)]
    if params.coordinates == 'cylindrical':
        clouds = [syn.cylindrical(c) for c in clouds]
    proj = torch.from_numpy(syn.hash_uniform(4242, len(sizes) * 256).reshape(len(sizes), 256).astype(np.float32))
    key = (cfg, tuple(sizes))
    if key not in _ORACLE_GRADS:                 # the CPU oracle's forward + backward is the slow part: once per workload
        sd = {k: v.clone().requires_grad_() for k, v in synthetic_state_dict(params, 'stress').items()}
        y_ref = hotformer_ref.forward_with_grad(sd, params, oracle_octree(clouds, depth))
        (y_ref * proj).sum().backward()
        _ORACLE_GRADS[key] = (y_ref.detach(), {k: v.grad for k, v in sd.items()})
    y_ref, grads_ref = _ORACLE_GRADS[key]
    params.drop_path = 0.0                       # stochastic depth off (its own test replays the reference's draws)
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().train()
    # training-path Linear layers: 'x3' = hand-written split GEMM (forward + dx), 'fp32' = torch fp32 GEMMs,
    # 'bf16x3-lt' = the K-concatenated split through hipBLASLt (forward, dx and dW)
    from hotformerloc_amd.model import set_train_split, set_train_x3
    set_train_x3(linear == 'x3')
    set_train_split(linear == 'bf16x3-lt')
    set_gemm_mode('bf16x3' if linear == 'bf16x3-lt' else 'x3')
    try:
        y = model({'octree': build_batch_octree(clouds, depth, 2, 'cuda')})['global']
        (y * proj.cuda()).sum().backward()
    finally:
        set_train_split(False)
        set_train_x3(True)
        set_gemm_mode('x3')
    rel = _rel(y.detach().cpu().numpy(), y_ref.detach().numpy()).max()
    assert rel <= REL_TOL, rel
    worst = {}
    for name, p in model.named_parameters():
        gref = grads_ref[name]
        assert p.grad is not None, name
        err = (p.grad.cpu() - gref).norm().item() / max(gref.norm().item(), 1e-12)
        kind = name.split('.')[-1] if 'rpe_table' not in name else 'rpe_table'
        worst[kind] = max(worst.get(kind, 0.0), err)
        assert err < GRAD_TOL or gref.norm().item() < 1e-9, (name, err, gref.norm().item())
    print(cfg, linear, 'forward rel', rel, 'worst grad rel-L2 per kind', worst)


def test_drop_path_is_per_cloud_and_off_in_eval():
    """Stochastic depth (models/layers/octformer_layers.py:213-289): train-mode outputs differ from
    eval, a dropped branch is dropped for a whole cloud, eval ignores it."""
    params, depth = load_config('wild-places')
    assert params.drop_path == 0.5
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    clouds = syn.make_clouds(55, 3, 1200, params.coordinates)
    octree = build_batch_octree(clouds, depth, 2, 'cuda')
    model.eval()
    with torch.no_grad():
        e1 = model({'octree': octree})['global']
        e2 = model({'octree': octree})['global']
    assert torch.equal(e1, e2)
    model.train()
    torch.manual_seed(0)
    with torch.no_grad():
        t1 = model({'octree': octree})['global']
    assert torch.isfinite(t1).all() and not torch.allclose(t1, e1, atol=1e-4)
    from hotformerloc_amd.model import OctreeDropPath
    dp = OctreeDropPath(0.5).train()
    bid = torch.tensor([0] * 5 + [1] * 7 + [2] * 3, device='cuda')
    x = torch.ones(15, 4, device='cuda')
    torch.manual_seed(3)
    y = dp(x, bid, 3)
    for b in range(3):
        rows = y[bid == b]
        assert torch.all(rows == rows[0, 0]) and rows[0, 0].item() in (0.0, 2.0)


def test_stochastic_depth_inside_the_fused_branches_matches_the_unfused_path():
    """Train mode with the config's drop_path = 0.5: the fused residual-branch Functions apply the per-cloud factor in the
    proj / fc2 epilogues and to the incoming gradient (hfl_linear_x3_rows, hfl_split2_rows); with the same random draws the
    un-fused formulation (branch * factor, torch autograd) must give the same descriptors and parameter gradients."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    assert params.drop_path == 0.5
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().train()
    clouds = syn.make_clouds(77, 4, 1500, params.coordinates)
    octree = build_batch_octree(clouds, depth, 2, 'cuda')
    proj = torch.randn(4, params.output_dim, device='cuda', generator=torch.Generator(device='cuda').manual_seed(5))
    res = {}
    for fused in (True, False):
        M._TRAIN_MLP = fused
        try:
            model.zero_grad(set_to_none=True)
            torch.manual_seed(11)
            y = model({'octree': octree})['global']
            (y * proj).sum().backward()
            res[fused] = (y.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        finally:
            M._TRAIN_MLP = True
    ya, yb = res[True][0], res[False][0]
    assert (ya - yb).abs().max().item() < 1e-4 * yb.abs().max().item() + 1e-6
    worst = 0.0
    for n, gb in res[False][1].items():
        ga = res[True][1][n]
        if gb.norm().item() > 1e-9:
            worst = max(worst, ((ga - gb).norm() / gb.norm()).item())
    assert worst < 1e-3, worst


def test_native_block_executor_equals_the_python_launch_sequence():
    """hfl_block_forward_x3 issues the same kernels in the same order as the Python wrappers: bitwise equal descriptors."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().eval()
    octree = build_batch_octree(syn.make_clouds(91, 3, 2000, params.coordinates), depth, 2, 'cuda')
    out = {}
    for native in (True, False):
        M._NATIVE_BLOCK = native
        try:
            with torch.no_grad():
                out[native] = model({'octree': octree})['global']
        finally:
            M._NATIVE_BLOCK = True
    assert torch.equal(out[True], out[False])


def test_large_oxford_batch_completes_and_is_deterministic():
    """Regression for the stream-K dead-lock ("hipBLASLt schedule"): Oxford cfg, 48 clouds --
    every pyramid depth is chip-filling (92k-194k rows).  With stream-K GEMMs on three streams this configuration
    never returned from synchronize(); the data-parallel schedule + the side-stream row guard make it finish."""
    params, depth = load_config('oxford')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'init')
    model = model.cuda().eval()
    clouds = syn.make_clouds(5, 48, 4096, params.coordinates)
    octree = build_batch_octree(clouds, depth, 2, 'cuda')
    with torch.inference_mode():
        y1 = model({'octree': octree})['global']
        y2 = model({'octree': octree})['global']
    torch.cuda.synchronize()
    assert y1.shape == (48, 256) and torch.isfinite(y1).all()
    assert torch.equal(y1, y2)
    assert torch.allclose(y1.norm(dim=1), torch.ones(48, device='cuda'), atol=1e-5)


def test_grad_checkpoint_recomputes_the_same_gradients():
    """`grad_checkpoint` (default True, `misc/utils.py:89`; per-block non-reentrant checkpointing,
    `models/hotformerloc_backbone.py:596-618`, `models/octformer_backbone.py:415-416`): the custom autograd
    Functions are re-entrant-safe -- recomputation in the backward gives the gradients of the plain run, BITWISE, and less
    peak memory.  That equality is what lets the default policy ('auto', model.set_checkpoint_policy) keep the activations
    while the device has room and recompute like the reference only when memory is tight."""
    from hotformerloc_amd import model as M
    params, depth = load_config('cs-wild-places')
    params.drop_path = 0.0
    clouds = [syn.forest_cloud(300 + i, 5000) if i % 2 else syn.unit_ball_cloud(300 + i, 4096) for i in range(4)]
    proj = torch.from_numpy(syn.hash_uniform(11, 4 * 256).reshape(4, 256).astype(np.float32)).cuda()
    res = {}
    prev = M.set_checkpoint_policy('always')          # the reference's behaviour: grad_checkpoint decides
    try:
        for ck in (False, True):
            params.grad_checkpoint = ck
            model = model_factory(params)
            assert model.backbone.backbone.hotf_stage.grad_checkpoint is ck
            syn.fill_synthetic_weights(model, 'stress')
            model = model.cuda().train()
            octree = build_batch_octree(clouds, depth, 2, 'cuda')
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            y = model({'octree': octree})['global']
            (y * proj).sum().backward()
            torch.cuda.synchronize()
            res[ck] = (y.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()},
                       torch.cuda.max_memory_allocated())
        # policy 'auto' (the default): grad_checkpoint = True recomputes only when the device is short of memory
        stage, dev = model.backbone.backbone.hotf_stage, torch.device('cuda', 0)
        rc = 20000 * 256                                     # rows x channels of this batch's pyramid levels, roughly
        assert M._use_checkpoint(stage, rc, 10, dev)
        M.set_checkpoint_policy('auto')
        assert not M._use_checkpoint(stage, rc, 10, dev)     # 4 GB of activations, > 250 GB free
        assert M._use_checkpoint(stage, 100 * rc, 10, dev)   # 400 GB would not fit
        assert M._use_checkpoint(stage)                      # no estimate: as the reference
        frac, M._CHECKPOINT_FREE_FRACTION = M._CHECKPOINT_FREE_FRACTION, 1e-6
        try:
            assert M._use_checkpoint(stage, rc, 10, dev)     # nothing counts as fitting
        finally:
            M._CHECKPOINT_FREE_FRACTION = frac
        M.set_checkpoint_policy('never')
        assert not M._use_checkpoint(stage, rc, 10, dev)
        model.eval()
        M.set_checkpoint_policy('always')
        assert not M._use_checkpoint(stage, rc, 10, dev)     # inference never checkpoints
    finally:
        M.set_checkpoint_policy(prev)
    assert torch.equal(res[False][0], res[True][0])
    for k, g in res[False][1].items():
        h = res[True][1][k]
        assert torch.equal(g, h), (k, (g - h).abs().max().item())     # RPE-table gradients included (fixed-order reduction)
    print('peak memory: plain %.2f GiB, checkpointed %.2f GiB' % (res[False][2] / 2 ** 30, res[True][2] / 2 ** 30))
    assert res[True][2] < res[False][2]


def test_drop_forward_caches_rebuilds_the_same_plan():
    """`Octree.drop_forward_caches()` (the reference boundary of bench.py: OctreeT and the octree2col tables are rebuilt in
    every forward, `models/hotformerloc_backbone.py:712-716`) leaves keys / children / neighbour tables alone and the next
    forward derives everything again: bitwise the same descriptors, and new plan objects."""
    params, depth = load_config('wild-places')
    model = _device_model(params)
    octree = build_batch_octree(syn.make_clouds(17, 3, 3000, params.coordinates), depth, 2, 'cuda')
    with torch.inference_mode():
        y1 = model({'octree': octree})['global']
        plans = dict(octree._window_plans)
        taps = dict(octree._sparse_taps)
        assert plans and taps
        neighs = [None if t is None else t.data_ptr() for t in octree.neighs]
        octree.drop_forward_caches()
        for name in Octree._FORWARD_CACHES:
            assert name not in octree.__dict__
        assert [None if t is None else t.data_ptr() for t in octree.neighs] == neighs
        y2 = model({'octree': octree})['global']
    assert torch.equal(y1, y2)
    for k, p in octree._window_plans.items():
        assert p is not plans[k]
    assert set(octree._sparse_taps) >= set(taps)


def test_early_phase_schedule_equals_the_sequential_one():
    """The token-row half of every H-OSA block (CPE, LN1, qkv) issued before / beside the relay-token self-attention of the
    iteration, on per-level streams (hfl_block_io.phase 1 / 2), against RTSA-then-blocks: the same kernels on the same rows,
    bitwise equal descriptors -- also with relay-token propagation on the last block."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    for prop in (False, True):
        params.ct_propagation = prop
        model = model_factory(params)
        syn.fill_synthetic_weights(model, 'stress')
        model = model.cuda().eval()
        octree = build_batch_octree(syn.make_clouds(93, 4, 2500, params.coordinates), depth, 2, 'cuda')
        out = {}
        for early in (True, False, True):
            M._EARLY_PHASE = early
            try:
                with torch.no_grad():
                    y = model({'octree': octree})['global']
                torch.cuda.synchronize()
            finally:
                M._EARLY_PHASE = True
            if early in out:
                assert torch.equal(out[early], y)                   # and run to run
            out[early] = y
        assert torch.equal(out[True], out[False]), prop


@contextlib.contextmanager
def _recorded_schedules(M):
    """What `HOTFormerStage._schedule` chose, forward by forward."""
    seen, orig = [], M.HOTFormerStage._schedule
    M.HOTFormerStage._schedule = lambda self, *a: (seen.append(orig(self, *a)), seen[-1])[1]
    try:
        yield seen
    finally:
        M.HOTFormerStage._schedule = orig


@pytest.mark.gpu
def test_every_stream_setting_runs_its_schedule_with_the_same_result():
    """`set_pyramid_streams(True | 'serial' | False)` and the default streams without the early phase: the stage runs the
    early schedule, the early schedule on one stream, the sequential one and the forked one -- the same kernels on the same
    rows, bitwise equal descriptors."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    model = _device_model(params)
    octree = build_batch_octree(syn.make_clouds(93, 4, 2500, params.coordinates), depth, 2, 'cuda')
    out = []
    with _recorded_schedules(M) as seen:
        try:
            for streams, early in ((True, True), ('serial', True), (False, True), (True, False)):
                M.set_pyramid_streams(streams)
                M._EARLY_PHASE = early
                with torch.no_grad():
                    out.append(model({'octree': octree})['global'])
                torch.cuda.synchronize()
        finally:
            M.set_pyramid_streams(True)
            M._EARLY_PHASE = True
    assert seen == ['early', 'early', 'sequential', 'forked'], seen
    assert torch.isfinite(out[0]).all()
    for y in out[1:]:
        assert torch.equal(out[0], y)


@pytest.mark.gpu
def test_attn_ws_block_path_matches_the_two_launch_path():
    """LN1 -> qkv -> window attention of the relay-token blocks' token rows as ONE launch (hfl_attn_ws_fwd behind
    hfl_block_forward_x3, phase 1 = the CPE alone; the default for the finest level from 40 k token rows, here forced on every
    level) against the two launches: the same arithmetic per score except the relative-position term (three 1-D tables summed
    per score against the two-lookup form), so the descriptors agree to rounding.  The stage leaves the early-phase schedule
    by itself when the finest level takes the one-launch form; forced to keep it (block phases 1 / 2) the result is bitwise
    the sequential one."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().eval()
    octree = build_batch_octree(syn.make_clouds(93, 4, 2500, params.coordinates), depth, 2, 'cuda')
    out = {}
    saved = (M._ATTN_WS, M._ATTN_WS_MIN_ROWS, M._EARLY_PHASE, M._ATTN_WS_EARLY)
    with _recorded_schedules(M) as calls:
        try:
            # (two launches, early) | (one launch, early phases forced: block phases 1 / 2 with the CPE alone in phase 1) |
            # (one launch, sequential) | (one launch, default: the stage leaves the early-phase schedule by itself)
            for key, ws, early, keep in (((False, True), False, True, False), ((True, True), True, True, True),
                                         ((True, False), True, False, False), ('auto', True, True, False)):
                M._ATTN_WS, M._ATTN_WS_MIN_ROWS, M._EARLY_PHASE, M._ATTN_WS_EARLY = ws, 0, early, keep
                with torch.no_grad():
                    out[key] = model({'octree': octree})['global']
                torch.cuda.synchronize()
        finally:
            M._ATTN_WS, M._ATTN_WS_MIN_ROWS, M._EARLY_PHASE, M._ATTN_WS_EARLY = saved
    assert calls == ['early', 'early', 'forked', 'forked'], calls
    assert torch.equal(out['auto'], out[True, False])
    assert torch.equal(out[True, True], out[True, False])
    a, b = out[False, True].double(), out[True, True].double()
    rel = ((a - b).norm(dim=1) / a.norm(dim=1)).max().item()
    assert 0.0 < rel < 2e-5, rel            # (not the same launches: > 0; bar = 20 x what is observed)


@pytest.mark.gpu
def test_merged_window_attention_launch_equals_one_launch_per_level():
    """The window attention of an H-OSA iteration's three pyramid levels as ONE launch (hfl_block_attention_x3_multi between
    block phases 3 and 4) against one launch per level: the same windows through the same kernel, bitwise equal descriptors;
    also on a batch small enough that the coarsest level has fewer windows than its share of the grid."""
    from hotformerloc_amd import model as M
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().eval()
    for n_clouds, pts in ((4, 2500), (1, 700), (9, 4096)):
        octree = build_batch_octree(syn.make_clouds(17, n_clouds, pts, params.coordinates), depth, 2, 'cuda')
        out = {}
        for merged in (True, False, True):
            M._MERGED_ATTN = merged
            try:
                with torch.no_grad():
                    y = model({'octree': octree})['global']
                torch.cuda.synchronize()
            finally:
                M._MERGED_ATTN = True
            if merged in out:
                assert torch.equal(out[merged], y)
            out[merged] = y
        assert torch.isfinite(out[True]).all()
        assert torch.equal(out[True], out[False]), (n_clouds, pts)
