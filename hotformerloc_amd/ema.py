"""Exponential moving average of a model's weights: the teacher of the reference's MESA self-distillation
(`training/trainer.py:161-163, 360-361`: `ModelEmaV3(model, decay=0.9998)`, updated after every optimizer step).

Every floating-point entry of the state dict follows
    ema <- ema + (1 - decay) * (model - ema)
(the formula of `torch.lerp(ema, model, 1 - decay)`, which is what timm's `ModelEmaV3.update` applies through
`torch._foreach_lerp_` when no warm-up is configured; the reference configures none); every other entry is copied.
All float tensors move in ONE HIP launch (`hfl_ema_update`, csrc/ema.hip) instead of one per tensor.

`state_dict()` yields the keys `'module.' + k` for k in `model.state_dict()`: what the reference's checkpoints hold under
`model_ema_state_dict`."""

import copy

import torch
import torch.nn as nn

from . import _native
from . import ops

# Per-module caches of launch state that the encoder keeps in a module's __dict__ (ctypes structures of raw device pointers,
# HIP streams; the packed weights live in `weight_cache`, keyed by the parameters, so the copy's are its own).  They describe the ORIGINAL's tensors and some cannot be copied at all; the copy rebuilds its
# own on its first forward.
_DERIVED_STATE = ('_stream_cache', '_unit_taps', '_drop_path_mods', '_drop_path_cache')


def _copy_model(model: nn.Module) -> nn.Module:
    held = []
    for m in model.modules():
        for name in _DERIVED_STATE:
            if name in m.__dict__:
                held.append((m, name, m.__dict__.pop(name)))
    try:
        return copy.deepcopy(model)
    finally:
        for m, name, value in held:
            m.__dict__[name] = value


class ModelEma(nn.Module):
    def __init__(self, model: nn.Module, decay: float = 0.9998):
        super().__init__()
        if not 0.0 <= decay <= 1.0:
            raise ValueError('decay must lie in [0, 1], got %r' % (decay,))
        self.module = _copy_model(model)
        self.module.eval()
        self.module.requires_grad_(False)
        self.decay = float(decay)
        self._launch = None                    # (stamp of data pointers, device table, chunk count, float ema tensors)

    def train(self, mode: bool = True):
        """The teacher always runs in eval mode (`trainer.py:313`: it is only ever called for inference)."""
        self.training = mode
        return self

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    @torch.no_grad()
    def update(self, model: nn.Module):
        """One EMA step towards `model`'s current weights.  Data-parallel training needs no communication here: after the
        gradient all-reduce every rank holds identical weights, so every rank computes the identical average."""
        ema_sd = self.module.state_dict(keep_vars=True)
        src_sd = model.state_dict(keep_vars=True)
        if ema_sd.keys() != src_sd.keys():
            raise KeyError('ModelEma.update: the model\'s state dict keys differ from the averaged copy\'s (%d vs %d entries)'
                           % (len(src_sd), len(ema_sd)))
        f_ema, f_src = [], []
        for k, e in ema_sd.items():
            s = src_sd[k]
            if not (e.is_cuda and s.is_cuda):
                raise _native.NativeLibraryError(
                    'ModelEma.update needs GPU tensors (%s is on %s / %s); there is no CPU fallback' % (k, e.device, s.device))
            if e.is_floating_point():
                f_ema.append(e)
                f_src.append(s)
            else:
                e.copy_(s)
        stamp = tuple(t.data_ptr() for t in f_ema) + tuple(t.data_ptr() for t in f_src)
        if self._launch is None or self._launch[0] != stamp:
            table, n = ops.ema_table(f_ema, f_src)
            self._launch = (stamp, table, n)
        _, table, n = self._launch
        ops.ema_update(table, n, 1.0 - self.decay)
        # The launch wrote the weights behind autograd's back.  Every cached weight pack of the encoder (split / packed GEMM
        # operands, native block descriptors) is stamped with its parameter's version counter: bump it, or the teacher would
        # go on encoding with the packs of its old weights.
        torch.autograd.graph.increment_version(f_ema)
