"""-m gpu: every ray of the families of tests/trace_ref.py -- axis-parallel and -0.0 directions, components either side of the 1e-30 switch, rays in
planes shared by child boxes, at shared edges and vertices, origins 1e-4 from a surface, shadow rays whose limit is the occluder's distance to the last
bit -- through wf_trace8_kernel (probe_trace4) and bvh_traverse (probe_trace), closest hit and any hit, against the fp64 restatement's admissible
answers.  There is no percentage: one ray outside its admissible set, or one t, u, v beyond its bound, fails.  Where both kernels name the same face
their t, u, v are equal bit for bit (tri_test spells its fma chains for that).  With the host-built tree and the device-built one, after a refit, and
on ONE block (every chunk from the atomic cursor).  The restatement of a scene is computed once per session and never changed.
Measured on an MI355X: DESIGN.md, "Every ray at box planes, edges and axes"."""
import os

import numpy as np
import pytest

from tests import trace_ref as R
from tests.kit import bits

pytestmark = pytest.mark.gpu


def _context(pkg, scene, tree, flags=0, grid=0):
    if grid: os.environ["MCPT_WF_GRID"] = str(grid)
    try:
        r = pkg.Renderer(scene, flags=flags | (pkg.FLAG_GPU_BVH_BUILD if tree == "device" else 0))
    finally:
        os.environ.pop("MCPT_WF_GRID", None)
    # (a scene of at most MCPT_LEAF_MAX = 2 triangles is one leaf: build_trees never calls the device builder for it, and bvh_builder stays 0)
    assert r.info().bvh_builder == (1 if tree == "device" and scene.face.shape[0] > 2 else 0), r.info().bvh_builder
    return r


def _assert_admissible(rs, rays, title, face, t, u, v, blocked):
    """One kernel's answers for the whole list: the per-family table, then every ray admissible."""
    bad, ratio = rs.check_closest(face, t, u, v)
    R.print_table(title, R.family_table(rs, rays, ratio))
    where = np.nonzero(bad)[0]
    assert where.size == 0, "%s, closest hit: %d rays outside their admissible set (error / bound %.3g); %s" % (
        title, where.size, ratio[where[0]], "; ".join(R.describe(rs, rays, i, face[i]) for i in where[:5]))
    bad = rs.check_any(blocked)
    where = np.nonzero(bad)[0]
    assert where.size == 0, "%s, any hit: %d verdicts not admissible; %s" % (title, where.size, "; ".join(
        "blocked %d with t2 %r (%s), %d triangles surely before it, %d possibly; %s" % (blocked[i], rays["t2"][i], rays["t2_kind"][i], rs.sure_any[i], rs.open_any[i],
                                                                                      R.describe(rs, rays, i, -1)) for i in where[:5]))


def _check_both_kernels(r, rs, rays, title):
    o, d, t2 = rays["origin"], rays["direction"], rays["t2"]
    t4, f4, u4, v4 = r.probe_trace4(o, d)
    any4 = r.probe_trace4(o, d, t2=t2, any_hit=True)[1]
    tb, fb, ub, vb = r.probe_trace(o, d)
    anyb = r.probe_trace(o, d, t2=t2, any_hit=True)[1]
    _assert_admissible(rs, rays, title + ", wf_trace8_kernel", f4, t4, u4, v4, any4)
    _assert_admissible(rs, rays, title + ", bvh_traverse", fb, tb, ub, vb, anyb)
    same = (f4 == fb) & (f4 >= 0)
    print("both kernels name the same face on %.4f of the rays, the same verdict on %.4f" % ((f4 == fb).mean(), (any4 == anyb).mean()))
    assert same.sum() > 0 or not (rs.sure_closest > 0).any()
    for a, b, what in ((t4, tb, "t"), (u4, ub, "u"), (v4, vb, "v")):
        diff = np.nonzero(same & (bits(a) != bits(b)))[0]
        assert diff.size == 0, "%s: %s differs between the kernels on %d rays, first %s: %r vs %r" % (title, what, diff.size, R.describe(rs, rays, diff[0], f4[diff[0]]), a[diff[0]], b[diff[0]])


@pytest.mark.parametrize("tree", ["host", "device"])
@pytest.mark.parametrize("name", list(R.SCENES))
def test_every_ray_is_admissible(pkg, name, tree):
    scene, rays, rs = R.case(pkg, name)
    r = _context(pkg, scene, tree)
    try:
        i = r.info()
        print("\n%s, %s tree: %d triangles, %d wide nodes, wide depth %d" % (name, tree, i.n_tris, i.wide_nodes, i.wide_depth))
        if name in R.ROOMS:
            assert i.wide_nodes > 160                                                  # records from the LDS image AND from global memory
        if name in ("one", "two"):
            assert i.wide_nodes == 1                                                   # a single-record tree
        _check_both_kernels(r, rs, rays, "%s, %s tree" % (name, tree))
    finally:
        r.close()


@pytest.mark.parametrize("tree", ["host", "device"])
def test_every_ray_is_admissible_after_a_refit(pkg, tree):
    """room16, then mcpt_update_vertices with the wall interiors displaced smoothly: both trees refitted on the device, the restatement recomputed for
    the moved vertices (the context keeps the centre it was created with; the displacement keeps the bounding box, so it is the same one)."""
    scene, rays, _ = R.case(pkg, "room16")
    moved = R.displaced(scene)
    rs = R.restate(moved, rays["origin"], rays["direction"], rays["t2"], centre=R.centre_of(scene))
    r = _context(pkg, scene, tree, flags=pkg.FLAG_DYNAMIC)
    try:
        r.update_vertices(moved.vertex)
        _check_both_kernels(r, rs, rays, "room16 refitted, %s tree" % tree)
    finally:
        r.close()


def test_every_ray_is_admissible_on_one_block(pkg):
    """room16 with MCPT_WF_GRID=1: one block, every chunk of the ray list from the atomic cursor.  The rays of axis_on_planes head the list in runs of
    one axis and sign, so whole waves carry same-octant closest-hit rays (the order_matters branch) and, in the any-hit launch, any-hit rays alone."""
    scene, rays, rs = R.case(pkg, "room16")
    r = _context(pkg, scene, "host", grid=1)
    try:
        _check_both_kernels(r, rs, rays, "room16 on one block")
    finally:
        r.close()
