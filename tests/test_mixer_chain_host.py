"""Host side of the one-launch Mixer chain (csrc/mixer_chain.hip): the pack's size, the shape rule, and the model's fallback
for heads the launch does not take.  No GPU."""

import pytest
import torch

from hotformerloc_amd import _native, ops
from hotformerloc_amd import model as M


def test_pack_bytes():
    """bf16 (hi, lo) of fc1 (256, 256) and fc2 (256, 256) per layer: 512 KiB a layer; 0 for a layer count the launch refuses"""
    lib = _native.load()
    for layers in (1, 2, 3, 4):
        assert lib.hfl_mixer_chain_pack_bytes(layers) == layers * 2 * 256 * 256 * 2 * 2
    for layers in (-1, 0, 5, 64):
        assert lib.hfl_mixer_chain_pack_bytes(layers) == 0


@pytest.mark.parametrize('c,hidden,layers,d,ok', [
    (256, 256, 1, 0, True), (256, 256, 4, 8, True), (256, 256, 4, 4, True), (256, 256, 2, 1, True),
    (128, 128, 4, 4, False), (128, 256, 4, 4, False), (256, 512, 4, 4, False), (256, 1024, 1, 4, False), (512, 512, 4, 4, False),
    (256, 256, 0, 4, False), (256, 256, 5, 4, False), (256, 256, -1, 4, False), (256, 256, 4, 9, False), (256, 256, 4, -1, False)])
def test_ok_rule(c, hidden, layers, d, ok):
    assert ops.mixer_chain_ok(c, hidden, layers, d) is ok


def test_null_arguments_are_refused_before_anything_else():
    """(null checks come before any launch, so this needs no device)"""
    lib = _native.load()
    assert lib.hfl_mixer_chain_pack(None, None, None, 4, None) == _native.HFL_EINVAL
    assert lib.hfl_mixer_chain_x3(None, None, None, None, None, None, None, None, 1e-5, None, 8, 4, 4, None) == _native.HFL_EINVAL
    assert lib.hfl_descriptor_tail(None, None, None, None, None, None, 1, 8, 256, 2, 4, 1, None) == _native.HFL_EINVAL


@pytest.mark.parametrize('kw', [dict(mlp_ratio=2), dict(mix_depth=5), dict(in_d=128), dict(out_d=16)])
def test_model_falls_back_for_heads_the_launch_does_not_take(kw, monkeypatch):
    """mlp_ratio != 1, more than 4 layers, another width, out_d > 8: `chain_shapes_ok` says no and the forward calls no chain
    op; the shipped head (256 wide, 4 layers, ratio 1, out_d 4) is taken."""
    def refuse(*a, **k):
        raise AssertionError('a chain op was called')

    monkeypatch.setattr(ops, 'mixer_chain', refuse)
    monkeypatch.setattr(ops, 'descriptor_tail', refuse)
    monkeypatch.setattr(ops, 'mixer_chain_pack', refuse)
    shipped = dict(k_input_tokens=16, k_output_tokens=4, in_d=256, mix_depth=4, mlp_ratio=1, out_d=4)
    assert M.Mixer(**shipped).chain_shapes_ok()
    args = dict(shipped, **kw)
    mixer = M.Mixer(**args).eval()
    assert not mixer.chain_shapes_ok()
    with torch.no_grad():
        x = torch.randn(2, 16, args['in_d'])
        out = mixer(x, normalize=True)
        want = torch.nn.functional.normalize(mixer.row_proj(mixer.channel_proj(mixer.mix(x).permute(0, 2, 1)).permute(0, 2, 1))
                                             .flatten(1), dim=1)
    assert torch.equal(out, want)
