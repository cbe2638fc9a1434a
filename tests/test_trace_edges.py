"""-m gpu: every ray of the families of tests/trace_ref.py -- axis-parallel and -0.0 directions, components either side of the 1e-30 switch, rays in
planes shared by child boxes, at shared edges and vertices, origins 1e-4 from a surface, shadow rays whose limit is the occluder's distance to the last
bit -- through wf_trace8_kernel (probe_trace4) and bvh_traverse (probe_trace), closest hit and any hit, against the fp64 restatement's admissible
answers.  There is no percentage: one ray outside its admissible set, or one t, u, v beyond its bound, fails.  Where both kernels name the same face
their t, u, v are equal bit for bit (tri_test spells its fma chains for that).  With the host-built tree and the device-built one, after a refit, and
on ONE block (every chunk from the atomic cursor).  The restatement of a scene is computed once per session and never changed.
Measured on an MI355X: DESIGN.md, "Every ray at box planes, edges and axes"."""
import pytest

from tests import trace_ref as R
from tests.kit import check_both_kernels as _check_both_kernels, trace_context as _context

pytestmark = pytest.mark.gpu


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
