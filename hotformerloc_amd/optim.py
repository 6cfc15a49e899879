"""`FusedAdam`: the reference trainer's optimizer (`training/trainer.py:140-156`: `torch.optim.Adam`, weight decay folded
into the gradient, or `AdamW`, decoupled) as ONE HIP launch over all parameters (`hfl_adam_step`, csrc/optim.hip), with the
EMA teacher of `hotformerloc_amd.ema.ModelEma` advanced in the same launch once `attach_ema` has paired them.

Parameter groups and per-parameter state (`step`, `exp_avg`, `exp_avg_sq`) are exactly `torch.optim.Adam`'s, so a
`state_dict()` of either class loads into the other: the reference's checkpoints resume here and the other way round.

What a step costs on the host is the point: the walk over parameters, state and teacher is done once and kept; a step
re-reads the gradients (new tensors after every `zero_grad()`), compares addresses and rewrites the table's gradient column
when they moved.  A learning-rate scheduler changes slot values only, never the table."""

import torch

from . import _native
from . import ops


class _Plan:
    """the cached walk: one row per parameter of every group, in group order"""
    __slots__ = ('params', 'group_of', 'states', 'steps', 'step_tensors', 'exp_avgs', 'exp_avg_sqs', 'emas', 'active', 'slot_of',
                 'stamp', 'grad_ptrs', 'table', 'written')


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *,
                 amsgrad=False, maximize=False, capturable=False, differentiable=False):
        for name, flag in (('amsgrad', amsgrad), ('maximize', maximize), ('capturable', capturable),
                           ('differentiable', differentiable)):
            if flag:
                raise ValueError('FusedAdam does not support %s=True' % name)
        if isinstance(lr, torch.Tensor):
            lr = lr.item()
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: %r' % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: %r' % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        # the keys of torch.optim.Adam's groups, so that state dicts travel both ways
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        self._plan = None
        self._ema = None                    # (ModelEma, model)
        self._ema_pairs = {}                # id(parameter) -> teacher tensor
        self._ema_rest = None               # ([float ema], [float src], [(ema, src) to copy], stamp, table, n)
        super().__init__(params, defaults)

    # ------------------------------------------------------------------ what invalidates the cached walk
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]['params']:
            if p.dtype != torch.float32:
                raise TypeError('FusedAdam takes float32 parameters, got %s' % p.dtype)
        self._plan = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plan = None

    # ------------------------------------------------------------------ teacher
    @property
    def ema(self):
        """the `ModelEma` that `step()` advances, or None"""
        return None if self._ema is None else self._ema[0]

    def attach_ema(self, model_ema, model):
        """From now on `step()` also applies `model_ema.update(model)`: every state-dict entry of `model` that is a parameter
        of this optimizer moves its teacher tensor inside the optimizer's launch; every other entry (float buffers, non-float
        entries, parameters this optimizer does not own) takes `ModelEma.update`'s route right after it.  The pairing is
        taken once: call `attach_ema` again after replacing a parameter or buffer OBJECT of either module (tensors that
        merely move, as under `.to(...)`, are followed).  `attach_ema(None, None)` detaches."""
        self._plan = None
        self._ema, self._ema_pairs, self._ema_rest = None, {}, None
        if model_ema is None:
            return
        ema_sd = model_ema.module.state_dict(keep_vars=True)
        src_sd = model.state_dict(keep_vars=True)
        if ema_sd.keys() != src_sd.keys():
            raise KeyError('attach_ema: the model\'s state dict keys differ from the averaged copy\'s (%d vs %d entries)'
                           % (len(src_sd), len(ema_sd)))
        mine = {id(p) for g in self.param_groups for p in g['params']}
        f_ema, f_src, copies, seen = [], [], [], set()
        for k, e in ema_sd.items():
            s = src_sd[k]
            if id(e) in seen:                           # tied weights: one tensor under two keys
                continue
            seen.add(id(e))
            if id(s) in mine and e.dtype == torch.float32 and id(s) not in self._ema_pairs:
                if e.shape != s.shape:
                    raise ValueError('attach_ema: %s has shape %s in the model, %s in the average' % (k, tuple(s.shape), tuple(e.shape)))
                self._ema_pairs[id(s)] = e
            elif e.is_floating_point():
                f_ema.append(e)
                f_src.append(s)
            else:
                copies.append((e, s))
        self._ema = (model_ema, model)
        self._ema_rest = [f_ema, f_src, copies, None, None, 0]

    def _update_rest_of_teacher(self, w):
        f_ema, f_src, copies = self._ema_rest[:3]
        for e, s in copies:
            if not (e.is_cuda and s.is_cuda):
                raise _native.NativeLibraryError('FusedAdam: the teacher needs GPU tensors; there is no CPU fallback')
            e.copy_(s)
        if f_ema:
            stamp = tuple(t.data_ptr() for t in f_ema) + tuple(t.data_ptr() for t in f_src)
            if self._ema_rest[3] != stamp:
                self._ema_rest[4], self._ema_rest[5] = ops.ema_table(f_ema, f_src)
                self._ema_rest[3] = stamp
            ops.ema_update(self._ema_rest[4], self._ema_rest[5], w)
            torch.autograd.graph.increment_version(f_ema)

    # ------------------------------------------------------------------ the walk
    def _walk(self):
        plan = _Plan()
        plan.params, plan.group_of = [], []
        for gi, group in enumerate(self.param_groups):
            if group.get('amsgrad') or group.get('maximize') or group.get('capturable') or group.get('differentiable'):
                raise ValueError('FusedAdam does not support amsgrad, maximize, capturable or differentiable (param group %d)' % gi)
            for p in group['params']:
                plan.params.append(p)
                plan.group_of.append(gi)
        ops._dev(*plan.params)
        for p in plan.params:
            if p.dtype != torch.float32:
                raise TypeError('FusedAdam takes float32 parameters, got %s' % p.dtype)
        plan.states = [self.state.get(p) for p in plan.params]    # None until the parameter's first step, as torch keeps it
        plan.emas = [self._ema_pairs.get(id(p)) for p in plan.params]
        plan.active = plan.slot_of = plan.stamp = plan.grad_ptrs = plan.table = None
        self._read_state(plan)
        return plan

    @staticmethod
    def _read_state(plan):
        plan.step_tensors = [None if s is None else s.get('step') for s in plan.states]
        plan.steps = [0 if t is None else int(t.item()) for t in plan.step_tensors]
        plan.exp_avgs = [None if s is None else s.get('exp_avg') for s in plan.states]
        plan.exp_avg_sqs = [None if s is None else s.get('exp_avg_sq') for s in plan.states]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._plan
        if plan is None:
            plan = self._plan = self._walk()
        params = plan.params
        grads = [p.grad for p in params]
        active = tuple(g is not None for g in grads)
        states = plan.states
        # state tensors are this class's own: a replaced OBJECT (somebody wrote into optimizer.state) re-reads them
        for i, s in enumerate(states):
            if s is None:
                continue
            if s.get('exp_avg') is not plan.exp_avgs[i] or s.get('exp_avg_sq') is not plan.exp_avg_sqs[i] \
                    or s.get('step') is not plan.step_tensors[i]:
                self._read_state(plan)
                plan.table = None
                break
        fresh = False
        for i, on in enumerate(active):
            if on and plan.exp_avgs[i] is None:                   # torch's lazy state initialisation
                g = grads[i]
                if g.is_sparse:
                    raise TypeError('FusedAdam does not support sparse gradients')
                if g.dtype != torch.float32:
                    raise TypeError('FusedAdam takes float32 gradients, got %s' % g.dtype)
                s = states[i] = self.state[params[i]]
                s['step'] = torch.tensor(0.0, dtype=torch.float32)
                s['exp_avg'] = torch.zeros_like(params[i], memory_format=torch.preserve_format)
                s['exp_avg_sq'] = torch.zeros_like(params[i], memory_format=torch.preserve_format)
                fresh = True
        if fresh:
            self._read_state(plan)
            plan.table = None
        # one slot per (param group, step count) among the parameters that step now
        keys, slot_of = {}, []
        for i, on in enumerate(active):
            slot_of.append(keys.setdefault((plan.group_of[i], plan.steps[i] + 1), len(keys)) if on else 0)
        slots = []
        for gi, step in keys:
            g = self.param_groups[gi]
            beta1, beta2 = g['betas']
            slots.append(ops.adam_slot(float(g['lr']), float(beta1), float(beta2), float(g['eps']), float(g['weight_decay']),
                                       bool(g.get('decoupled_weight_decay', False)), step))
        emas = plan.emas
        try:
            grad_ptrs = [0 if g is None else g.data_ptr() for g in grads]
        except RuntimeError:                                      # a tensor without storage
            for g in grads:
                if g is not None and g.is_sparse:
                    raise TypeError('FusedAdam does not support sparse gradients') from None
            raise
        stamp = tuple(p.data_ptr() for p in params) + tuple(0 if e is None else e.data_ptr() for e in emas) \
            + tuple(0 if (t is None or not on) else t.data_ptr() for t, on in zip(plan.exp_avgs, active)) \
            + tuple(0 if (t is None or not on) else t.data_ptr() for t, on in zip(plan.exp_avg_sqs, active))
        if plan.table is None or plan.active != active or plan.slot_of != slot_of or plan.stamp != stamp:
            plan.table = ops.adam_table(params, grads, [t if on else None for t, on in zip(plan.exp_avgs, active)],
                                        [t if on else None for t, on in zip(plan.exp_avg_sqs, active)], emas, slot_of)
            plan.active, plan.slot_of, plan.stamp, plan.grad_ptrs = active, slot_of, stamp, grad_ptrs
            plan.written = [p for p, on in zip(params, active) if on and p.numel()] + \
                [e for e in emas if e is not None and e.numel()]
        elif plan.grad_ptrs != grad_ptrs:
            ops.adam_refresh_grads(plan.table, grads)
            plan.grad_ptrs = grad_ptrs
        w = 0.0 if self._ema is None else 1.0 - self._ema[0].decay
        ops.adam_step(plan.table, slots, w)
        stepped = [t for t, on in zip(plan.step_tensors, active) if on]
        if stepped:
            torch._foreach_add_(stepped, 1)
            for i, on in enumerate(active):
                if on:
                    plan.steps[i] += 1
        # The launch wrote parameters and teacher behind autograd's back.  The encoder's weight packs (`weight_cache`) are
        # stamped with their parameter's version counter: bump it, or the next forward would encode with stale packs.
        if plan.written:
            torch.autograd.graph.increment_version(plan.written)
        if self._ema is not None:
            self._update_rest_of_teacher(w)
        return loss
