"""The relay-token transformer block as ONE launch (hfl_relay_block_fused_x3, csrc/relay_block.hip) against the five
launches it replaces (hfl_relay_block_forward_x3), against a float64 restatement of the block, and inside the model."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import _native, build_batch_octree, load_config, model_factory, ops
from hotformerloc_amd import synthetic as syn

DEV = 'cuda'
C, H = 256, 16
EPS = 1e-5
SENTINEL = 12345.0


def _weights(seed=5):
    """Random block parameters (the scales of test_ln_mlp_fused_*), every weight image of both paths, the filled struct."""
    g = torch.Generator().manual_seed(seed)
    p = {'qkv_w': torch.randn(3 * C, C, generator=g) * 0.05, 'proj_w': torch.randn(C, C, generator=g) * 0.05,
         'fc1_w': torch.randn(4 * C, C, generator=g) * 0.05, 'fc2_w': torch.randn(C, 4 * C, generator=g) * 0.05,
         'qkv_b': torch.randn(3 * C, generator=g) * 0.1, 'proj_b': torch.randn(C, generator=g) * 0.1,
         'fc1_b': torch.randn(4 * C, generator=g) * 0.1, 'fc2_b': torch.randn(C, generator=g) * 0.1,
         'g1': 1 + 0.1 * torch.randn(C, generator=g), 'b1': 0.1 * torch.randn(C, generator=g),
         'g2': 1 + 0.1 * torch.randn(C, generator=g), 'b2': 0.1 * torch.randn(C, generator=g)}
    d = {k: v.to(DEV) for k, v in p.items()}
    keep = {'w2': [ops.split2_weight(d[k]) for k in ('qkv_w', 'proj_w', 'fc1_w', 'fc2_w')],
            'mlp': ops.mlp_fused_pack(d['fc1_w'], d['fc2_w']), 'qkv': ops.qkv_fused_pack(d['qkv_w']),
            'relay': ops.relay_block_pack(d['qkv_w'], d['proj_w'], d['fc1_w'], d['fc2_w'])}
    w = _native.RelayBlockWeights(channels=C, n_heads=H, eps=EPS, norm1_gamma=d['g1'].data_ptr(), norm1_beta=d['b1'].data_ptr(),
                                  norm2_gamma=d['g2'].data_ptr(), norm2_beta=d['b2'].data_ptr(),
                                  qkv_w=keep['w2'][0].data_ptr(), proj_w=keep['w2'][1].data_ptr(),
                                  fc1_w=keep['w2'][2].data_ptr(), fc2_w=keep['w2'][3].data_ptr(),
                                  qkv_b=d['qkv_b'].data_ptr(), proj_b=d['proj_b'].data_ptr(), fc1_b=d['fc1_b'].data_ptr(),
                                  fc2_b=d['fc2_b'].data_ptr(), mlp_pack=keep['mlp'].data_ptr(), qkv_pack=keep['qkv'].data_ptr(),
                                  relay_pack=keep['relay'].data_ptr())
    return p, d, keep, w


def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (C,), g.double(), b.double(), EPS)


def _mlp64(p, x1):
    h = torch.nn.functional.gelu(_ln(x1, p['g2'], p['b2']) @ p['fc1_w'].double().t() + p['fc1_b'].double())
    return x1 + h @ p['fc2_w'].double().t() + p['fc2_b'].double()


def _block64(p, x, seqs):
    """float64 restatement: rows of no sequence get a zero attention output."""
    x = x.double()
    qkv = _ln(x, p['g1'], p['b1']) @ p['qkv_w'].double().t() + p['qkv_b'].double()
    att = torch.zeros_like(x)
    for rows in seqs:
        if len(rows) == 0:
            continue
        r = torch.as_tensor(rows)
        q, k, v = (qkv[r, i * C:(i + 1) * C].view(len(rows), H, 16).transpose(0, 1) for i in range(3))
        a = torch.softmax(q @ k.transpose(1, 2) * 0.25, dim=-1) @ v
        att[r] = a.transpose(0, 1).reshape(len(rows), C)
    x1 = x + att @ p['proj_w'].double().t() + p['proj_b'].double()
    return _mlp64(p, x1)


def _io(parts, out, seq_rows, seq_off, batch, max_seq_len, orphans, arena=None):
    """(hfl_relay_block_io, what it points to): `parts` = one tensor (x_in) or a list (x_segments)."""
    seg = None
    if isinstance(parts, (list, tuple)):
        seg, rows = ops.row_segments(list(parts))
    else:
        rows = parts.shape[0]
    io = _native.RelayBlockIO(x_in=None if seg is not None else parts.data_ptr(),
                              x_segments=None if seg is None else ctypes.addressof(seg), out=out.data_ptr(),
                              arena=None if arena is None else arena.data_ptr(), seq_rows=seq_rows.data_ptr(),
                              seq_off=seq_off.data_ptr(), n_rows=rows, batch=batch, max_seq_len=max_seq_len,
                              orphan_rows=None if orphans is None or orphans.numel() == 0 else orphans.data_ptr(),
                              n_orphans=0 if orphans is None else orphans.numel())
    return io, (seg, parts, out, arena, seq_rows, seq_off, orphans)


def _run(entry, w, parts, rows, seq_rows, seq_off, batch, max_seq_len, orphans):
    lib = _native.load()
    out = torch.full((rows, C), SENTINEL, dtype=torch.float32, device=DEV)
    arena = None
    if entry == 'hfl_relay_block_forward_x3':
        arena = torch.zeros(int(lib.hfl_relay_block_forward_x3_arena(rows, C)), dtype=torch.uint8, device=DEV)
    io, keep = _io(parts, out, seq_rows, seq_off, batch, max_seq_len, orphans, arena)
    ops.check(getattr(lib, entry)(ctypes.byref(w), ctypes.byref(io), ops._stream()), entry)
    torch.cuda.synchronize()
    return out


def _layouts():
    """name -> (x (rows, C) on the host, segment sizes or None, sequences (row lists), orphan rows, rows no table names)."""
    g = torch.Generator().manual_seed(11)
    # everything that can go wrong: sequence lengths 0, 1, 17, 64 with rows in no order over three unequal segments, two orphan
    # rows, one row that no table mentions
    lens = (0, 1, 17, 64)
    rows = sum(lens) + 3
    perm = torch.randperm(rows, generator=g).tolist()
    seqs, at = [], 0
    for n in lens:
        seqs.append(perm[at:at + n])
        at += n
    ragged = (torch.randn(rows, C, generator=g) * 2, (40, 13, rows - 53), seqs, perm[at:at + 2], perm[at + 2:])
    # a single contiguous input, no orphans, every row in a sequence
    lens = (33, 16, 48)
    rows = sum(lens)
    perm = torch.randperm(rows, generator=g).tolist()
    seqs, at = [], 0
    for n in lens:
        seqs.append(perm[at:at + n])
        at += n
    return {'ragged': ragged, 'contiguous': (torch.randn(rows, C, generator=g) * 2, None, seqs, [], [])}


_CACHE = {}


def _case(name):
    """Both paths and the float64 reference of a layout, computed once and shared (nothing below modifies them)."""
    if name not in _CACHE:
        p, d, keep, w = _weights()
        x, segs, seqs, orphans, unnamed = _layouts()[name]
        xd = x.to(DEV)
        parts = xd if segs is None else [t.contiguous() for t in torch.split(xd, list(segs))]
        seq_rows = torch.tensor([r for s in seqs for r in s], dtype=torch.int32, device=DEV)
        seq_off = torch.tensor(np.cumsum([0] + [len(s) for s in seqs]), dtype=torch.int32, device=DEV)
        orph = torch.tensor(orphans, dtype=torch.int32, device=DEV)
        args = (w, parts, x.shape[0], seq_rows, seq_off, len(seqs), max(len(s) for s in seqs), orph)
        fused = _run('hfl_relay_block_fused_x3', *args)
        fused2 = _run('hfl_relay_block_fused_x3', *args)
        five = _run('hfl_relay_block_forward_x3', *args)
        ref = _block64(p, x, seqs)
        named = sorted(set(range(x.shape[0])) - set(unnamed))
        _CACHE[name] = dict(p=p, x=x, fused=fused.cpu(), fused2=fused2.cpu(), five=five.cpu(), ref=ref, named=named,
                            orphans=orphans, unnamed=unnamed, keep=(d, keep, w, args))
    return _CACHE[name]


@pytest.mark.parametrize('name', ['ragged', 'contiguous'])
def test_fused_launch_matches_the_five_launches_and_float64(name):
    """Sequence lengths 0 / 1 / 17 / 64, rows in no order over three segments, orphan rows, a row no table names -- and a
    single contiguous input: (a) two fused calls are bitwise equal; (b) |fused - five launches| <= 2e-5 max|ref| (the bar of
    test_ln_mlp_fused_*); (c) relative L2 against float64 of the fused launch at most twice the five launches' (summation
    order is all that differs); (e) rows that no table names keep what `out` held."""
    c = _case(name)
    named = c['named']
    fused, five, ref = c['fused'][named].double(), c['five'][named].double(), c['ref'][named]
    assert torch.isfinite(fused).all()
    assert torch.equal(c['fused'], c['fused2'])                                        # (a)
    diff = (fused - five).abs().max().item()
    bar = 2e-5 * ref.abs().max().item()
    e_fused = ((fused - ref).norm() / ref.norm()).item()
    e_five = ((five - ref).norm() / ref.norm()).item()
    print('relay block %s: max|fused - five| %.3e (bar %.3e); rel L2 vs float64: fused %.3e, five launches %.3e'
          % (name, diff, bar, e_fused, e_five))
    assert diff <= bar, (diff, bar)                                                    # (b)
    assert e_fused <= 2 * e_five, (e_fused, e_five)                                    # (c)
    for r in c['unnamed']:                                                             # (e)
        assert torch.equal(c['fused'][r], torch.full((C,), SENTINEL))
    assert (c['fused'][named] != SENTINEL).any(dim=1).all()


def test_orphan_rows_are_x_plus_proj_bias_through_the_mlp():
    """(d) rows of no sequence: attention output zero, so x1 = x + proj bias, then the MLP -- the five-launch path's values."""
    c = _case('ragged')
    p, orph = c['p'], c['orphans']
    assert len(orph) == 2
    want = _mlp64(p, c['x'][orph].double() + p['proj_b'].double())
    got = c['fused'][orph].double()
    assert ((got - want).norm() / want.norm()).item() < 1e-5
    assert (got - c['five'][orph].double()).abs().max().item() <= 2e-5 * c['ref'].abs().max().item()


def test_fused_ok_refuses_what_the_kernel_does_not_take_and_the_dispatcher_falls_back(monkeypatch):
    """hfl_relay_block_fused_ok says no to max_seq_len 65, C = 128 and a missing pack; ops.relay_block_forward_x3 then issues
    the five launches (hfl_relay_block_forward_x3) and never the fused entry."""
    lib = _native.load()
    c = _case('contiguous')
    d, keep, w, args = c['keep']
    _, parts, rows, seq_rows, seq_off, batch, max_len, orph = args
    out = torch.empty((rows, C), dtype=torch.float32, device=DEV)

    def ok(weights, max_seq_len):
        io, _ = _io(parts, out, seq_rows, seq_off, batch, max_seq_len, orph)
        return lib.hfl_relay_block_fused_ok(ctypes.byref(weights), ctypes.byref(io))

    def clone(**changes):
        w2 = _native.RelayBlockWeights()
        ctypes.memmove(ctypes.byref(w2), ctypes.byref(w), ctypes.sizeof(w))
        for k, v in changes.items():
            setattr(w2, k, v)
        return w2

    assert ok(w, max_len) == 1 and ok(w, 64) == 1
    assert ok(w, 65) == 0
    assert ok(clone(channels=128, n_heads=8), max_len) == 0
    no_pack = clone(relay_pack=None)
    assert ok(no_pack, max_len) == 0
    io, _ = _io(parts, out, seq_rows, seq_off, batch, 65, orph)
    assert lib.hfl_relay_block_fused_x3(ctypes.byref(w), ctypes.byref(io), ops._stream()) == -1        # HFL_EINVAL, no launch

    calls = []
    five_launches = lib.hfl_relay_block_forward_x3

    def refuse(*a):
        raise AssertionError('the fused entry was called')

    def counted(*a):
        calls.append(1)
        return five_launches(*a)

    monkeypatch.setattr(lib, 'hfl_relay_block_fused_x3', refuse)
    monkeypatch.setattr(lib, 'hfl_relay_block_forward_x3', counted)
    for weights, msl in ((w, 65), (no_pack, max_len)):
        got = ops.relay_block_forward_x3(weights, None, parts, seq_rows, seq_off, batch, msl, orph)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), c['five'])
    assert len(calls) == 2
    got = ops.relay_block_forward_x3(w, None, parts, seq_rows, seq_off, batch, max_len, orph, fused=False)       # the switch
    assert len(calls) == 3 and torch.equal(got.cpu(), c['five'])


def test_out_aliasing_an_input_is_refused():
    """The kernel reads the other rows of a cloud after some were written: `out` overlapping x_in or any segment is
    HFL_EINVAL (nothing is launched, nothing is written)."""
    lib = _native.load()
    c = _case('ragged')
    d, keep, w, args = c['keep']
    _, parts, rows, seq_rows, seq_off, batch, max_len, orph = args
    sizes = [t.shape[0] for t in parts]
    pool = torch.zeros((3 * rows, C), dtype=torch.float32, device=DEV)
    segs = [pool[0:sizes[0]], pool[sizes[0]:sizes[0] + sizes[1]], pool[2 * rows:2 * rows + sizes[2]]]
    for t, src in zip(segs, parts):
        t.copy_(src)
    whole = pool[0:rows]
    before = pool.clone()
    cases = [(whole, whole),                                        # out is x_in
             (whole, pool[8:8 + rows]),                             # out overlaps x_in in part
             (segs, pool[sizes[0] + 5:sizes[0] + 5 + rows]),        # out overlaps the second segment (and no other)
             (segs, pool[rows + 10:2 * rows + 10])]                 # out overlaps the first rows of the third segment
    for x, out in cases:
        io, _ = _io(x, out, seq_rows, seq_off, batch, max_len, orph)
        assert lib.hfl_relay_block_fused_x3(ctypes.byref(w), ctypes.byref(io), ops._stream()) == -1          # HFL_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pool, before)


_MODEL = {}


def _model_and_octree():
    """The Wild-Places model (stress weights) and a batch octree of three small clouds, built once."""
    if not _MODEL:
        params, depth = load_config('wild-places')
        model = model_factory(params)
        syn.fill_synthetic_weights(model, 'stress')
        clouds = [c[:n] for c, n in zip(syn.make_clouds(23, 3, 2000, params.coordinates), (800, 1400, 2000))]
        _MODEL['m'] = (model.cuda().eval(), build_batch_octree(clouds, depth, 2, 'cuda'))
    return _MODEL['m']


def _descriptors(relay_fused, native_block=True):
    from hotformerloc_amd import model as M
    model, octree = _model_and_octree()
    M._RELAY_FUSED, M._NATIVE_BLOCK = relay_fused, native_block
    try:
        with torch.no_grad():
            return model({'octree': octree})['global'].cpu()
    finally:
        M._RELAY_FUSED, M._NATIVE_BLOCK = True, True


def test_model_descriptors_with_the_fused_relay_block_match_the_five_launch_path(monkeypatch):
    """Wild-Places forward of three small clouds in GEMM mode x3, relay-token block as one launch against five: relative L2 of
    the descriptors <= 1e-5 per cloud.  The fused entry really runs with the switch on (once per H-OSA iteration) and never
    with it off, and the two descriptor sets differ in their last bits (other summation orders), so neither side is the
    other in disguise."""
    lib = _native.load()
    fused_entry, calls = lib.hfl_relay_block_fused_x3, []

    def counted(*a):
        calls.append(1)
        return fused_entry(*a)

    monkeypatch.setattr(lib, 'hfl_relay_block_fused_x3', counted)
    on = _descriptors(True)
    n_on = len(calls)
    off = _descriptors(False)
    assert n_on >= 1 and len(calls) == n_on, (n_on, len(calls))
    rel = (on.double() - off.double()).norm(dim=1) / off.double().norm(dim=1)
    print('relay block fused on / off (%d fused launches), descriptors rel L2 per cloud:' % n_on, rel.tolist())
    assert torch.isfinite(on).all() and rel.max().item() <= 1e-5, rel
    assert not torch.equal(on, off)


def test_five_launch_fallback_native_executor_equals_the_python_launch_sequence():
    """With the one-launch block switched off, hfl_relay_block_forward_x3 (and hfl_block_forward_x3) issue the same kernels in
    the same order as the Python wrappers: bitwise equal descriptors.  (With it on, both settings of _NATIVE_BLOCK run the same
    single launch for the relay-token block, so tests/test_gpu_model.py's check of the executor no longer reaches the five
    launches, which every shape the fused launch refuses still takes.)"""
    assert torch.equal(_descriptors(False, native_block=True), _descriptors(False, native_block=False))
