"""Restatement of the parts update (csrc/parts.hip) in numpy and plain Python: what mcpt_update_parts leaves in the device's arrays,
given what each route's OWN call would have written (the deformers' restatements: transform_ref, skin_ref, skin_dq_ref, morph_ref, keyframes_ref),
and the host half -- the owner validation, the per-owner counts and the ordered route plan.  Nothing of the deformers is restated here.
"""
from __future__ import annotations

import numpy as np

NONE, GROUPS, SKIN, MORPH, KEYFRAMES = range(5)
OWNERS = 5
ROUTES = (1 << GROUPS) | (1 << SKIN) | (1 << MORPH) | (1 << KEYFRAMES)
MORPH_THEN_SKIN = 1
PLAN_OK, PLAN_NO_ROUTE, PLAN_UNKNOWN_ROUTE, PLAN_UNKNOWN_FLAG, PLAN_SKIN_WITHOUT_MORPH = range(5)


def route(owner):
    return 1 << owner


def combine(before, owners, outputs):
    """The array after a parts update: per record the output of its owner's route when that route ran -- `outputs` maps the owner ids of the
    routes that ran to the (n, 3) array the route's own call writes --, otherwise the bits it held `before`.  Bits are moved, never computed."""
    out = np.array(before, np.float64, copy=True).reshape(-1, 3)
    o = np.ascontiguousarray(owners, np.uint8).reshape(-1)
    assert o.shape[0] == out.shape[0] and NONE not in outputs
    for owner, array in outputs.items():
        a = np.ascontiguousarray(array, np.float64).reshape(-1, 3)
        assert a.shape == out.shape
        mine = o == owner
        out.view(np.uint64)[mine] = a.view(np.uint64)[mine]
    return out


def check_owners(vertex_owner, normal_owner, scene_vertex, scene_normal, n_vertex=None, n_normal=None):
    """mcpt_set_vertex_owners' rules in their order: (True, vertex counts, normal counts), or (False, what the message names).  normal_owner None:
    a NULL pointer; n_vertex / n_normal: the counts passed, when they are not the arrays' lengths."""
    vo = np.ascontiguousarray(vertex_owner, np.uint8).reshape(-1)
    no = None if normal_owner is None else np.ascontiguousarray(normal_owner, np.uint8).reshape(-1)
    nv = vo.shape[0] if n_vertex is None else n_vertex
    nn = (0 if no is None else no.shape[0]) if n_normal is None else n_normal
    if nv != scene_vertex or nn != scene_normal:
        return False, "n_vertex / n_normal differ from the scene's"
    if nn and no is None:
        return False, "null normal_owner"
    for what, a in (("vertex", vo), ("normal", no)):
        bad = np.flatnonzero(a >= OWNERS) if a is not None else np.zeros(0, int)
        if bad.size:
            return False, "%s %d: owner id %d > 4" % (what, bad[0], a[bad[0]])
    count = lambda a: np.bincount(a, minlength=OWNERS).tolist() if a is not None else [0] * OWNERS
    return True, count(vo), count(no)


def plan(routes, flags):
    """(status, steps, morph_then_skin, bones): the owner ids of the routes that run in ascending order; is the morph followed by the skin; do
    the bones travel.  The refusals in their order: no route, an unknown route bit, an unknown flag bit, the flag without the morph route."""
    if routes == 0:
        return PLAN_NO_ROUTE, [], False, False
    if routes & ~ROUTES:
        return PLAN_UNKNOWN_ROUTE, [], False, False
    if flags & ~MORPH_THEN_SKIN:
        return PLAN_UNKNOWN_FLAG, [], False, False
    if flags & MORPH_THEN_SKIN and not routes & route(MORPH):
        return PLAN_SKIN_WITHOUT_MORPH, [], False, False
    then_skin = bool(flags & MORPH_THEN_SKIN)
    return PLAN_OK, [o for o in (GROUPS, SKIN, MORPH, KEYFRAMES) if routes & route(o)], then_skin, bool(routes & route(SKIN)) or then_skin
