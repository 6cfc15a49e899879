"""The one cache of tensors (or ctypes structures) derived from parameters: split / packed GEMM operands of Linear weights,
fused-launch weight images, padded per-tap blocks, native block descriptors.

An image is as large as its weight, so it is released with the parameter (a model that ran inference must not leak its
Linear bytes for the life of the process), and it is never dropped while the parameter lives (no size limit: a limit
that empties the store drops the images of the live model in the middle of a step)."""

import weakref

_STORE = {}             # (kind, id(p) for p in params) -> [stamp, value]


def derived(kind, params: tuple, build):
    """`build()` for the parameters (or tensors; None allowed) `params`, kept while every one of them is the same object
    with the same `_version` and `data_ptr()`; rebuilt in place (no new entry) when one was updated, dropped when one of them
    dies.  `kind`: hashable, tells apart the images built from the same parameters.

    The lookup is on the launch path of every block (the host runs only just ahead of the GPU), so a hit costs the key and
    the stamp and nothing else: every parameter's finalizer drops the entry, hence an entry found under these ids belongs
    to these very objects (an id is reused only after its object, and with it the entry, is gone)."""
    key = (kind, *map(id, params))
    # data_ptr: `module.to(other_device)` swaps `.data` without bumping the version counter
    stamp = [(p._version, p.data_ptr()) for p in params if p is not None]
    hit = _STORE.get(key)
    if hit is None:
        for p in params:
            if p is not None:
                weakref.finalize(p, _STORE.pop, key, None)
        hit = _STORE[key] = [stamp, build()]
    elif hit[0] != stamp:
        hit[0], hit[1] = stamp, build()
    return hit[1]
