"""The batch families -- many independent solves of one problem per call -- as data: "small", one workgroup per solve
(``Problem.solve_many``), and "mid", several workgroups per solve (``Problem.solve_many_mid``, section
6.3).  A family's record says which shapes it takes, how it names its envelope in a note, how many solves one call of the
drivers takes and which ``Problem`` methods run them; ``solve_chunked`` is the one loop behind the bootstrap, the restarts
and the model-selection sweeps.  Nothing here opens a problem or a context, and ``device`` is imported only when asked.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

from . import _lib as L


class Family(NamedTuple):
    name: str
    supported: str  # the envelope test, a function of device.py
    whose: str  # how a note names the family's envelope
    called: str  # ... and the family itself
    limits: str  # the prefix of _lib's *_MAX_* constants
    chunk_rule: Callable  # (bootstrap module, N, S, n_c, n_u, masked) -> solves per call
    method: str  # the Problem method of plain and purity solves
    masked_method: str  # ... and of solves with a hold-out mask each

    @property
    def envelope(self):
        nu, k, s, elements = (getattr(L, f"{self.limits}_MAX_{what}") for what in ("NU", "K", "S", "ELEMENTS"))
        return f"outside {self.whose} envelope (n_u <= {nu}, K <= {k}, S <= {s}, N S <= {elements})"

    def outside(self, n_rows, n_samples, n_ct, n_u, mode):
        """The sentence that says why the family does not take the shape, or None where it does.  Touches no device."""
        from . import device

        if getattr(device, self.supported)(n_rows, n_samples, n_ct, n_u, mode):
            return None
        return f"the shape {n_rows} x {n_samples} with {n_ct} + {n_u} cell types is {self.envelope}"

    def chunk(self, n_rows, n_samples, n_ct, n_u, masked=False):
        """How many solves one call of the drivers takes: ``batch_chunk`` or ``mid_batch_chunk``, read through ``bootstrap`` at
        call time -- the module the tools and tests know the two rules by, and replace them in."""
        from . import bootstrap

        return self.chunk_rule(bootstrap, n_rows, n_samples, n_ct, n_u, masked)


def batch_chunk(n_rows, n_u):
    """How many solves one ``solve_many`` call of the drivers takes: enough to fill the GPU several times over, and at most
    256 MB for the stack of profiles."""
    return int(max(1, min(1024, (1 << 25) // max(1, n_rows * n_u))))


def mid_batch_chunk(n_rows, n_samples, n_ct, n_u, masked=False):
    """How many solves one ``solve_many_mid`` call of the drivers takes: as many as keep the slab workspace (W workgroups per
    solve, each with the larger of the known and the u-dependent Gram jobs times S doubles) and the stack of profiles
    together within 256 MB, at least 1 and at most 1024.  The purity variant (``solve_many_mid(purity=...)``) has the same
    workspace -- it adds nothing per slab or per solve, only the S purities per call -- so the bound holds for it as it is.
    ``masked``: a ``solve_many_mid_masked`` call, which adds a solve's train mask (N x ceil(S / 8) bytes) and its W count and
    W hold-out partials (8 bytes each) to what the bound counts."""
    from .device import mid_solve_plan

    _, n_slabs, _ = mid_solve_plan(n_rows, n_samples)
    K = n_ct + n_u
    known = n_ct * (n_ct + 1) // 2 + n_ct
    jobs = max(known, K * (K + 1) // 2 + K - known)
    per_solve = 8 * (n_slabs * jobs * n_samples + n_rows * n_u)
    if masked:
        per_solve += n_rows * ((n_samples + 7) // 8) + 16 * n_slabs
    return int(max(1, min(1024, (1 << 28) // per_solve)))


FAMILIES = {
    "small": Family("small", "small_solve_supported", "the batched kernel's", "the batch", "SMALL",
                    lambda rules, N, S, n_c, n_u, masked: rules.batch_chunk(N, n_u), "solve_many", "solve_many_masked"),
    "mid": Family("mid", "mid_solve_supported", "the mid-size batch's", "the mid-size batch", "MID",
                  lambda rules, N, S, n_c, n_u, masked: rules.mid_batch_chunk(N, S, n_c, n_u, masked=masked),
                  "solve_many_mid", "solve_many_mid_masked"),
}


def family(name, parameter="kernel"):
    """The record of the family ``name``; any other name raises ValueError naming the caller's ``parameter``."""
    if name not in FAMILIES:
        raise ValueError(f'{parameter} must be "small" or "mid", got {name!r}')
    return FAMILIES[name]


def solve_chunked(problem, fam, shape, items, stack, steps, purity=None, masked=False):
    """``items`` through the family's ``Problem`` method, ``fam.chunk(*shape)`` of them per call -> the method's results over
    all items, concatenated (an empty tuple where there are none).  ``shape`` = (N, S, n_c, n_u).  ``stack(part)`` -> (u0s,
    alpha0s, a third array or None) of a slice of the items: the third is ``idx``, or with ``masked`` the train masks.  It
    is called immediately before the slice's solve, so initialisers are drawn per chunk and in item order.  ``steps`` =
    (mode, n_iter1, n_iter2, tol); ``purity``: the vector shared by all solves, or None.  The method is looked up on the
    problem by name at every call."""
    chunk = fam.chunk(*shape, masked=masked)
    parts = []
    for c0 in range(0, len(items), chunk):
        u0s, alpha0s, third = stack(items[c0:c0 + chunk])
        if masked:
            parts.append(getattr(problem, fam.masked_method)(u0s, alpha0s, third, *steps))
        else:
            parts.append(getattr(problem, fam.method)(u0s, alpha0s, *steps, idx=third, purity=purity))
    return tuple(np.concatenate(column) for column in zip(*parts))
