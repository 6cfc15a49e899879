"""Host logic of `FusedAdam` (no GPU): state-dict exchange with torch.optim.Adam / AdamW, hyper-parameter slots, chunk cutting
of the launch table, constructor rejections."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hotformerloc_amd import FusedAdam, _native, ops            # noqa: E402
import hotformerloc_amd.optim as hoptim                          # noqa: E402


def _params(seed=0, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(dtype)) for n in (5, 17, 3)]


def _set_grads(params, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).to(p.dtype)


def _groups(params):
    return [{'params': params[:2], 'lr': 3e-3, 'weight_decay': 1e-4}, {'params': params[2:], 'lr': 1e-3, 'betas': (0.8, 0.99)}]


@pytest.mark.parametrize('decoupled', [False, True])
def test_state_dict_travels_both_ways(decoupled):
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    # torch -> FusedAdam
    pt = _params()
    ot = cls(_groups(pt), weight_decay=0.01)
    for s in range(3):
        _set_grads(pt, 10 + s)
        ot.step()
    sd = copy.deepcopy(ot.state_dict())          # as through a checkpoint file: load_state_dict may alias the tensors it is given
    pf = _params()
    of = FusedAdam(_groups(pf), weight_decay=0.01, decoupled_weight_decay=decoupled)
    assert set(of.param_groups[0]) == set(ot.param_groups[0]), 'the groups carry the same keys'
    assert of.param_groups[0]['amsgrad'] is False and of.param_groups[0]['maximize'] is False
    of.load_state_dict(sd)
    assert of.param_groups[0]['decoupled_weight_decay'] is decoupled
    for a, b in zip(pt, pf):
        st, sf = ot.state[a], of.state[b]
        assert set(sf) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert sf['step'].item() == 3 and sf['step'].dtype == st['step'].dtype and sf['step'].device.type == 'cpu'
        assert torch.equal(sf['exp_avg'], st['exp_avg']) and torch.equal(sf['exp_avg_sq'], st['exp_avg_sq'])
    out = copy.deepcopy(of.state_dict())
    assert out['param_groups'] == sd['param_groups']
    assert out['state'].keys() == sd['state'].keys()
    # FusedAdam -> torch: the loader takes a further step and lands where an optimizer that never left torch lands
    p2 = _params()
    with torch.no_grad():
        for a, b in zip(p2, pt):
            a.copy_(b)
    o2 = cls(_groups(p2), weight_decay=0.01)
    o2.load_state_dict(out)
    _set_grads(pt, 99)
    _set_grads(p2, 99)
    ot.step()
    o2.step()
    for a, b in zip(pt, p2):
        assert torch.equal(a, b)
        assert ot.state[a]['step'].item() == o2.state[b]['step'].item() == 4
        assert torch.equal(ot.state[a]['exp_avg_sq'], o2.state[b]['exp_avg_sq'])


def test_fresh_state_dict_loads_into_torch():
    """a FusedAdam that has not stepped: no state, torch's groups"""
    pf = _params()
    sd = FusedAdam(_groups(pf), decoupled_weight_decay=True).state_dict()
    assert sd['state'] == {}
    pt = _params()
    ot = torch.optim.Adam(_groups(pt))
    ot.load_state_dict(sd)
    assert ot.param_groups[0]['decoupled_weight_decay'] is True
    _set_grads(pt, 1)
    ot.step()


@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('decoupled', [False, True])
def test_slot_values(step, decoupled):
    lr, b1, b2, eps, wd = 8e-4, 0.9, 0.999, 1e-8, 1e-4
    got = ops.adam_slot(lr, b1, b2, eps, wd, decoupled, step)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    want = (lr / bc1, bc2 ** 0.5, 1 - b1, b2, 1 - b2, eps, (1 - lr * wd) if decoupled else wd, int(decoupled))
    assert got == want
    s = _native.AdamSlot(*got)
    assert s.step_size == np.float32(lr / bc1) and s.bias_correction2_sqrt == np.float32(bc2 ** 0.5)
    assert s.one_minus_beta1 == np.float32(0.1) and s.one_minus_beta1 != np.float32(1) - np.float32(0.9), \
        '1 - beta is rounded from double, not formed in float'
    assert s.decoupled == int(decoupled)
    if step == 1:
        assert abs(got[0] - lr / (1 - b1)) < 1e-18 and abs(got[1] - (1 - b2) ** 0.5) < 1e-18
    with pytest.raises(ValueError):
        ops.adam_slot(lr, b1, b2, eps, wd, decoupled, 0)


def test_chunk_layout_matches_the_c_header(tmp_path):
    """`hfl_adam_chunk` / `hfl_adam_slot` against their ctypes mirrors, and the int64 row layout `adam_chunk_rows` writes"""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    pairs = [('hfl_adam_chunk', _native.AdamChunk), ('hfl_adam_slot', _native.AdamSlot)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hotformerloc_hip.h"', 'int main(void) {',
             '  printf("chunk %d slots %d\\n", HFL_ADAM_CHUNK, HFL_ADAM_MAX_SLOTS);']
    for cname, cls in pairs:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0].split() == ['chunk', str(ops.ADAM_CHUNK), 'slots', str(ops.ADAM_MAX_SLOTS)]
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out[1:]}
    for cname, cls in pairs:
        assert got[cname, 'sizeof'] == ctypes.sizeof(cls)
        assert sum(1 for k in got if k[0] == cname) - 1 == len(cls._fields_)
        for fname, _ in cls._fields_:
            assert got[cname, fname] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(_native.AdamChunk) == 48
    rows, _, _ = ops.adam_chunk_rows([7], [1000], [2000], [3000], [4000], [5000], [3])
    c = _native.AdamChunk.from_buffer_copy(rows.tobytes())
    assert (c.param, c.grad, c.exp_avg, c.exp_avg_sq, c.ema, c.count, c.slot) == (1000, 2000, 3000, 4000, 5000, 7, 3)


def test_chunk_cutting():
    C = ops.ADAM_CHUNK
    numels = [1, C, C + 1, 0, 2 * C + 5, 9, 4]
    base = [(i + 1) << 32 for i in range(len(numels))]
    P = [b + 0x100 for b in base]
    G = [b + 0x200 for b in base]
    M = [b + 0x300 for b in base]
    V = [b + 0x400 for b in base]
    E = [b + 0x500 for b in base]
    G[1] = 0                       # EMA line only
    E[2] = 0                       # no teacher
    G[5] = E[5] = 0                # neither: not emitted
    slots = [0, 5, 1, 0, 2, 0, 1]
    rows, owner, launches = ops.adam_chunk_rows(numels, P, G, M, V, E, slots)
    assert rows.dtype == np.int64 and rows.shape == (1 + 1 + 2 + 3 + 1, 6)
    assert owner.tolist() == [0, 1, 2, 2, 4, 4, 4, 6]
    assert launches == [(0, 8, 0)]
    count, slot = rows[:, 5] & 0xffffffff, rows[:, 5] >> 32
    assert count.tolist() == [1, C, C, 1, C, C, 5, 4]
    assert slot.tolist() == [0, 0, 1, 1, 2, 2, 2, 1], 'a chunk without a gradient names slot 0'
    for r, i in zip(rows, owner):
        k = (r[0] - P[i]) // (4 * C)
        assert r[0] == P[i] + 4 * C * k, 'chunk starts are multiples of the chunk size from the tensor start'
        assert r[4] == (E[i] + 4 * C * k if E[i] else 0)
        if G[i]:
            assert (r[1], r[2], r[3]) == (G[i] + 4 * C * k, M[i] + 4 * C * k, V[i] + 4 * C * k)
        else:
            assert (r[1], r[2], r[3]) == (0, 0, 0), 'no gradient: the moments are not handed to the kernel'
    for i in set(owner.tolist()):
        assert count[owner == i].sum() == numels[i]
    # nothing to do
    rows, owner, launches = ops.adam_chunk_rows([0, 4], [0, 8], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0])
    assert rows.shape == (0, 6) and launches == []
    # more slots than one launch carries: contiguous runs of rows, slot numbers relative to the run's first slot
    n = 2 * ops.ADAM_MAX_SLOTS + 3
    order = list(reversed(range(n)))
    rows, owner, launches = ops.adam_chunk_rows([4] * n, [0x1000 * (i + 1) for i in range(n)], [0x100000 + 16 * i for i in range(n)],
                                                [0x200000 + 16 * i for i in range(n)], [0x300000 + 16 * i for i in range(n)],
                                                [0] * n, order)
    assert launches == [(0, 16, 0), (16, 16, 16), (32, 3, 32)]
    for first, cnt, slot0 in launches:
        for r, i in zip(rows[first:first + cnt], owner[first:first + cnt]):
            assert slot0 <= order[i] < slot0 + ops.ADAM_MAX_SLOTS and (r[5] >> 32) == order[i] - slot0
    with pytest.raises(ValueError):
        ops.adam_chunk_rows([4], [8], [8], [8], [8], [0], [-1])


def test_constructor_rejections():
    for kw in ({'amsgrad': True}, {'maximize': True}, {'capturable': True}, {'differentiable': True}):
        with pytest.raises(ValueError):
            FusedAdam(_params(), **kw)
    for kw in ({'lr': -1.0}, {'eps': -1e-8}, {'betas': (1.0, 0.999)}, {'betas': (0.9, -0.1)}, {'weight_decay': -1e-4}):
        with pytest.raises(ValueError):
            FusedAdam(_params(), **kw)
    with pytest.raises(TypeError):
        FusedAdam(_params(dtype=torch.float64))
    opt = FusedAdam(_params())
    with pytest.raises(TypeError):
        opt.add_param_group({'params': _params(dtype=torch.float16)})
    assert opt.ema is None
    # a group that arrives with amsgrad through a state dict is refused when it would be used
    p = _params()
    bad = torch.optim.Adam(p, amsgrad=True)
    opt = FusedAdam(_params())
    opt.load_state_dict(bad.state_dict())
    with pytest.raises(ValueError):
        opt._walk()


def test_step_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    p = _params()
    _set_grads(p, 0)
    opt = FusedAdam(p)
    with pytest.raises(_native.NativeLibraryError):
        opt.step()
    assert len(opt.state) == 0
    assert hoptim.FusedAdam is FusedAdam
