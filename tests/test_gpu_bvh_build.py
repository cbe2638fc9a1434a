"""-m gpu: the device BVH builder (csrc/bvh_gpu.hip, MCPT_FLAG_GPU_BVH_BUILD) behind the same C ABI.

The traversal result does not depend on the tree (closest hit = min t, any hit = exists), so a device-built tree must
  (a) pass the host-side soundness walk of the quantised 8-wide tree (MCPT_VALIDATE_BVH=1: every triangle referenced once and
      inside every box on its root path),
  (b) return the reference's own hits on the reference's own random rays (tests/golden/ref_paths.npz), through both the binary
      tree (probe kernels) and the 8-wide tree (render),
  (c) render the image the host-built tree renders, sample for sample (deterministic mode), up to exact-tie pixels.
None of that depends on WHICH tree the builder makes, so
  (d) on exact-arithmetic inputs (tests/ploc_ref.py: integer lattices, where neither rounding nor contraction can change a comparison) the
      tree has the node count, depth and largest leaf of the numpy restatement of the builder -- what notices a wrong window at a block edge
      or a changed tie rule,
  (e) mcpt_scene_info.bvh_builder says whether the device tree was kept (1) or discarded for the host builder's (2): every context here states
      which it expects, so that no test silently runs on the host tree."""
import os

import numpy as np
import pytest

from tests import ploc_ref
from tests.kit import bits

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def paths():
    with np.load(os.path.join(G, "ref_paths.npz")) as z:
        return {k: z[k] for k in z.files}


def _gpu_tree_renderer(pkg, scene, expect_builder=1, **kw):
    """A context of MCPT_FLAG_GPU_BVH_BUILD, its wide tree walked for soundness at creation; expect_builder: 1 = the device tree is the one in
    use, 2 = it was discarded (too deep for this context, or the builder gave up) and the host builder's is."""
    os.environ["MCPT_VALIDATE_BVH"] = "1"
    try:
        r = pkg.Renderer(scene, flags=kw.pop("flags", 0) | pkg.FLAG_GPU_BVH_BUILD, **kw)
    finally:
        os.environ.pop("MCPT_VALIDATE_BVH", None)
    i = r.info()
    if i.bvh_builder != expect_builder:
        r.close()
        pytest.fail("bvh_builder %d (binary depth %d), expected %d" % (i.bvh_builder, i.bvh_depth, expect_builder))
    return r


def test_device_built_tree_returns_the_reference_hits(pkg, paths):
    p = paths
    r = _gpu_tree_renderer(pkg, pkg.scenes.cornell_box_small(64, 64))
    i = r.info()
    assert i.n_tris == pkg.scenes.cornell_box_small(64, 64).n_faces and 1 <= i.bvh_depth <= 63 and i.max_leaf <= 2
    t, tri, u, v = r.probe_trace(p["cs_ray_o"], p["cs_ray_d"])
    anyh = r.probe_trace(p["cs_ray_o"], p["cs_ray_d"], t2=p["cs_ray_t2"], any_hit=True)[1]
    r.close()
    ref_tri = p["cs_ray_rec"][:, 11].astype(np.int32); ref_hit = p["cs_ray_hit"] == 1
    same = (tri == np.where(ref_hit, ref_tri, -1))
    assert same.mean() >= 0.999, same.mean()
    ok = same & ref_hit
    assert np.allclose(t[ok], p["cs_ray_rec"][ok, 0], rtol=2e-5, atol=2e-6)
    assert (anyh == p["cs_ray_any"]).mean() >= 0.999


@pytest.mark.parametrize("name,kw,res,depth", [("cornell-box-small", {}, (48, 48), 5), ("veach-mis", {"light_lon": 12, "light_lat": 6, "plate_cells": 4}, (64, 36), 0),
                                               ("bathroom2", {"detail": 24, "tex_size": 32}, (64, 36), 6)])
def test_device_and_host_trees_render_the_same_samples(pkg, name, kw, res, depth):
    scene = pkg.scenes.SCENES[name](*res, **kw)
    imgs = []
    for gpu_tree in (False, True):
        if gpu_tree: r = _gpu_tree_renderer(pkg, scene, max_depth=depth, flags=pkg.FLAG_DETERMINISTIC)
        else: r = pkg.Renderer(scene, max_depth=depth, flags=pkg.FLAG_DETERMINISTIC)
        r.render(16, seed=21); imgs.append(r.read_accum()); r.close()
    a, b = imgs
    assert np.array_equal(a[..., 3], b[..., 3])                                  # sample counts
    differ = np.any(a[..., :3] != b[..., :3], axis=-1)
    # identical arithmetic per ray => identical samples, except where two triangles tie exactly (shared edges) or an any-hit ray
    # has several occluders and the trees find different ones first (same verdict)
    assert differ.mean() <= 0.01, differ.mean()
    assert abs(a[..., :3].mean() - b[..., :3].mean()) <= 2e-3 * a[..., :3].mean()


def test_device_builder_on_awkward_geometry(pkg):
    """Huge coordinate offsets, tiny and huge triangles side by side, flat boxes, many identical centroids (equal Morton codes).  The device
    tree itself (bvh_builder 1): with the builder's earlier tie rule the 400 copies made a chain 416 deep, the tree was discarded and this test
    ran on the host builder's."""
    scene, centres, rng = ploc_ref.awkward(pkg)                                   # (the restatement is run on the same scene: tests/test_ploc_ref.py)
    base = pkg.scenes.open_box(8, 8); n = 3000
    rg = _gpu_tree_renderer(pkg, scene); rh = pkg.Renderer(scene)
    assert rg.info().n_tris == base.n_faces + n and rg.info().bvh_depth <= 63 and rg.info().bvh_builder == 1 and rh.info().bvh_builder == 0
    m = 20000
    o = rng.uniform(-1, 1, (m, 3)) * np.array([1.2e3, 4.0, 4.0]) + np.array([5e4, -3.0, 0.25])
    tgt = centres[rng.randint(0, n, m)] + rng.normal(size=(m, 3)) * 0.5
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    tg, ig, _, _ = rg.probe_trace(o, d); th, ih, _, _ = rh.probe_trace(o, d)
    rg.close(); rh.close()
    assert (ih >= 0).mean() > 0.2                                                 # the rays do hit things
    assert ((ig >= 0) == (ih >= 0)).all()
    hit = ih >= 0
    assert np.array_equal(tg[hit], th[hit])                                       # same closest distance, bit for bit
    # the triangle may differ only between exact ties (the 400 coincident copies)
    assert ((ig == ih) | ((ig >= base.n_faces + 1000) & (ig < base.n_faces + 1400))).all()


def test_device_builder_is_faster_on_a_large_scene(pkg):
    scene = pkg.scenes.bathroom_stress(64, 36, detail=160, tex_size=16)          # 0.59 M triangles
    rh = pkg.Renderer(scene); ih = rh.info(); rh.close()
    rg = _gpu_tree_renderer(pkg, scene); ig = rg.info()
    rg.render(4, seed=3); a = rg.read_accum(); rg.close()
    assert np.isfinite(a).all() and (a[..., 3] == 4).all()
    print("\nBVH build, %d triangles: host SAH %.0f ms (depth %d, %d nodes) | device PLOC %.0f ms (depth %d, %d nodes)" % (
        ih.n_tris, ih.bvh_build_ms, ih.bvh_depth, ih.n_nodes, ig.bvh_build_ms, ig.bvh_depth, ig.n_nodes))
    assert ig.bvh_build_ms < ih.bvh_build_ms


def test_device_builder_is_sound_and_close_to_the_host_tree(pkg, paths):
    """MCPT_FLAG_GPU_BVH_BUILD builds a SAH-costed tree (PLOC: every merge minimises the merged box's area within a +-16 window of the
    Morton order).  It must pass the soundness walk, return the reference's hits through the production kernel, and cost at most
    1.15x the host binned-SAH tree's box tests per ray (measured on S-bath detail 24: host 1.00, PLOC ~1.0)."""
    r = _gpu_tree_renderer(pkg, pkg.scenes.cornell_box_small(64, 64))
    t, tri, u, v = r.probe_trace4(paths["cs_ray_o"], paths["cs_ray_d"]); r.close()
    ref_tri = paths["cs_ray_rec"][:, 11].astype(np.int32); ref_hit = paths["cs_ray_hit"] == 1
    assert (tri == np.where(ref_hit, ref_tri, -1)).mean() >= 0.999
    scene = pkg.scenes.bathroom_stress(96, 54, detail=24, tex_size=32)
    cost = {}
    for name, fl in (("host", 0), ("device", pkg.FLAG_GPU_BVH_BUILD)):
        rr = pkg.Renderer(scene, max_depth=6, flags=fl | pkg.FLAG_COUNT_TRAVERSAL | pkg.FLAG_CORRECT_SHADOW_T2)
        rr.render(8, seed=3); c = rr.counters(); i = rr.info(); rr.close()
        cost[name] = c.box_tests / c.rays
        assert i.bvh_depth <= 63 and i.bvh_builder == (1 if fl else 0)
    print("box tests per ray: host %.1f device %.1f" % (cost["host"], cost["device"]))
    assert cost["device"] <= 1.15 * cost["host"]


@pytest.mark.parametrize("name,kw,res", [("cornell-box-small", {}, (48, 48)), ("veach-mis", {"light_lon": 12, "light_lat": 6, "plate_cells": 4}, (64, 36)),
                                         ("bathroom2", {"detail": 24, "tex_size": 32}, (64, 36)), ("bathroom2", {"detail": 100, "tex_size": 32}, (64, 36)),
                                         # trees of one or two wide levels, a run of ties, and a chain 148 deep (tests/ploc_ref.py makes them)
                                         ("lattice_soup", {"n": 3}, None), ("lattice_soup", {"n": 5}, None), ("lattice_soup", {"n": 9}, None),
                                         ("lattice_soup", {"n": 17}, None), ("lattice_soup", {"n": 257}, None), ("coincident", {"n": 300}, None),
                                         ("shells", {"n": 150, "ratio": 1.2}, None)])
def test_device_collapse_reproduces_the_host_collapse(pkg, name, kw, res):
    """gpu_collapse_bvh8 (bvh_gpu.hip) against build_bvh8 (scene_build.cpp) on the same device-built binary tree: the same dynamic programme in the
    same double arithmetic, the same octant slots, the same level-by-level numbering -- so the 8-wide records and the leaf order must be the
    host's bit for bit (mcpt_scene_info.wide_tree_hash covers both), and a deterministic render the same film."""
    scene = pkg.scenes.SCENES[name](res[0], res[1], **kw) if res else getattr(ploc_ref, name)(pkg, **kw)
    out = []
    for host_collapse in (False, True):
        if host_collapse: os.environ["MCPT_HOST_COLLAPSE"] = "1"
        try:
            r = _gpu_tree_renderer(pkg, scene, max_depth=5, flags=pkg.FLAG_DETERMINISTIC)
        finally:
            os.environ.pop("MCPT_HOST_COLLAPSE", None)
        i = r.info(); r.render(4, seed=3); out.append(((i.wide_nodes, i.wide_depth, i.wide_tree_hash), r.read_accum())); r.close()
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------------------------------ shape
SHAPES = ([("lattice_soup", n) for n in (3, 4, 5, 8, 9, 16, 17, 33, 255, 256, 257, 272, 273, 513, 4099)] + [("grid", 64), ("strip", 1024), ("coincident", 300)]
          + [("coincident", 5), ("coincident", 17), ("coincident", 257)])


@pytest.mark.parametrize("maker,n", SHAPES)
def test_device_tree_has_the_shape_the_restatement_predicts(pkg, maker, n):
    """Sizes around the 2-triangle fallback, the +-16 window, the 256-thread block of ploc_nn_kernel (its LDS tile underfilled at 3 .. 255,
    straddling a block edge at 257 .. 273) and two blocks and more; a lattice, a strip and coincident copies for runs of exact ties.  Every
    coordinate, extent and merged area is exact in fp32, so the device tree equals the restatement's in every figure: no tolerance.
    What each case can notice: the soups up to 513 build the same tree under the earlier tie rule (lower index only), so they check the window
    and the block edges; the tie rule shows in lattice_soup(4099) (2412 nodes, depth 15; earlier rule 2411, 16) and in the coincident copies at
    every size -- 5 (2 nodes; earlier 3), 17 (depth 4; 15), 257 (depth 8; 255), 300 -- while grid(64) and strip(1024) differ in rounds only."""
    scene = getattr(ploc_ref, maker)(pkg, n)
    want = ploc_ref.predict(scene)
    r = _gpu_tree_renderer(pkg, scene); i = r.info(); r.close()
    print("\n%s(%d): device nodes %d depth %d max_leaf %d | restatement %s" % (maker, n, i.n_nodes, i.bvh_depth, i.max_leaf, want))
    assert i.n_tris == scene.face.shape[0] and not want["gave_up"]
    assert (i.n_nodes, i.bvh_depth, i.max_leaf) == (want["n_nodes"], want["depth"], want["max_leaf"])


# ------------------------------------------------------------------------------------------------------------------------ hits
def _check_hits(pkg, rg, rh, name, binary):
    """The rays of ploc_ref.hit_case(name) through the context of the device builder `rg` and the host-built `rh`: the same hit/miss and bit-equal
    t (the triangle test does not depend on the tree), the same face except between exact ties (coincident copies only), the fp64 brute force's
    hit/miss on >= 99.9 % and its t to rtol 2e-5, atol 2e-6 (this file's figures), and the same any-hit verdicts for a t2 just short of and just
    past the closest hit.  binary: also through the binary tree (mcpt_probe_trace)."""
    scene, o, d, t64, f64 = ploc_ref.hit_case(pkg, name)
    ties = name.startswith("coincident")
    for probe in ("probe_trace4",) + (("probe_trace",) if binary else ()):
        tg, ig, _, _ = getattr(rg, probe)(o, d); th, ih, _, _ = getattr(rh, probe)(o, d)
        assert np.array_equal(ig >= 0, ih >= 0), probe
        hit = ih >= 0
        assert np.array_equal(bits(tg[hit]), bits(th[hit])), probe
        assert ties or np.array_equal(ig, ih), probe
        same = hit == (f64 >= 0)
        both = hit & (f64 >= 0)
        print("%s %s: hit/miss as the fp64 brute force on %.4f of %d rays (%d hits), max |t - t64| / t64 = %.2e" % (
            name, probe, same.mean(), same.size, int(both.sum()), float(np.max(np.abs(tg[both] - t64[both]) / t64[both]))))
        assert same.mean() >= 0.999, (probe, same.mean())
        assert np.allclose(tg[both], t64[both], rtol=2e-5, atol=2e-6), probe
        assert ties or (ig[both] == f64[both]).mean() >= 0.999, probe
        for k in (0.999, 1.001):                                                  # shadow rays that stop just short of / just past the closest hit
            t2 = np.where(hit, th.astype(np.float64) * k, 1e30)
            ag = getattr(rg, probe)(o, d, t2=t2, any_hit=True)[1]; ah = getattr(rh, probe)(o, d, t2=t2, any_hit=True)[1]
            assert np.array_equal(ag, ah), (probe, k)
            # the closest hit itself lies before a t2 just past it; nothing lies before one just short of it -- but for the smallest shells, which the
            # any-hit rule (|det| >= 1e-6) accepts and the closest-hit rule (|det| >= 1e-5) does not
            assert (ah[hit] != 0).all() if k > 1 else (name.startswith("shells") or not (ah[hit] != 0).any()), (probe, k)


HITS = [("coincident-5000", 1), ("strip-9000", 1), ("grid-64", 1), ("soup-4099", 1), ("shells-40", 1), ("shells-150", 1), ("shells-300", 2), ("shells-5000", 2)]


@pytest.mark.parametrize("name,builder", HITS)
def test_hits_do_not_depend_on_the_tree(pkg, name, builder):
    """Default (wavefront) contexts.  coincident-5000 and strip-9000 were refused with the earlier tie rule (more than 4096 rounds); shells-150 keeps a
    tree 148 deep; shells-300 (298 deep) and shells-5000 (the builder gives up after 4096 rounds) fall back to the host builder: bvh_builder 2."""
    scene = ploc_ref.hit_case(pkg, name)[0]
    rg = _gpu_tree_renderer(pkg, scene, expect_builder=builder); rh = pkg.Renderer(scene)
    ig, ih = rg.info(), rh.info()
    print("\n%s: device context builder %d depth %d nodes %d wide depth %d | host depth %d" % (name, ig.bvh_builder, ig.bvh_depth, ig.n_nodes, ig.wide_depth, ih.bvh_depth))
    assert ih.bvh_builder == 0 and ih.bvh_depth <= 63
    try:
        _check_hits(pkg, rg, rh, name, binary=ig.bvh_depth <= 63)
    finally:
        rg.close(); rh.close()


@pytest.mark.parametrize("maker,n", [("coincident", 5000), ("strip", 9000)])
def test_runs_of_ties_create_a_shallow_device_tree(pkg, maker, n):
    """Refused before the tie rule changed ("did not converge"); now a device tree every kernel can walk."""
    r = _gpu_tree_renderer(pkg, getattr(ploc_ref, maker)(pkg, n)); i = r.info(); r.close()
    assert i.bvh_builder == 1 and i.bvh_depth <= 63 and i.max_leaf <= 2


# ------------------------------------------------------------------------------------------------------------------------ depth bands
def test_a_chain_below_the_stack_limit_is_walked_by_every_kernel(pkg):
    r = _gpu_tree_renderer(pkg, ploc_ref.shells(pkg, 40, 1.5)); i = r.info()
    assert i.bvh_depth == 38
    _, o, d, t64, f64 = ploc_ref.hit_case(pkg, "shells-40")
    t, f, _, _ = r.probe_trace(o, d); r.close()
    assert ((f >= 0) == (f64 >= 0)).mean() >= 0.999


def test_a_deep_tree_is_kept_by_a_wavefront_context_and_rebuilt_for_the_binary_kernels(pkg):
    """shells(150, 1.2): a chain 148 deep.  The default context walks the wide collapse only and keeps it (mcpt_probe_trace, which would walk the
    binary tree, refuses); a context of the recursive integrator walks the binary tree, so the device tree is discarded for the host builder's."""
    scene, o, d, t64, f64 = ploc_ref.hit_case(pkg, "shells-150")
    r = _gpu_tree_renderer(pkg, scene, flags=pkg.FLAG_COUNT_TRAVERSAL); i = r.info()
    assert 64 <= i.bvh_depth <= 255
    with pytest.raises(pkg.McptError, match="probe_trace4"):
        r.probe_trace(o[:1], d[:1])
    t4, f4, _, _ = r.probe_trace4(o, d)
    r.render(2, seed=1); c = r.counters(); film = r.read_accum(); r.close()
    print("\nshells(150, 1.2), wavefront context: binary depth %d, wide depth %d, stack spills %d" % (i.bvh_depth, i.wide_depth, c.stack_spills))
    assert np.isfinite(film).all() and (film[..., 3] == 2).all()
    both = (f4 >= 0) & (f64 >= 0)
    assert ((f4 >= 0) == (f64 >= 0)).mean() >= 0.999 and (f4[both] == f64[both]).mean() >= 0.999
    assert np.allclose(t4[both], t64[both], rtol=2e-5, atol=2e-6)
    rr = _gpu_tree_renderer(pkg, scene, expect_builder=2, integrator=pkg.INTEGRATOR_RECURSIVE_NEE)
    assert rr.info().bvh_depth <= 63
    t2, f2, _, _ = rr.probe_trace(o, d); rr.close()
    assert np.array_equal(f2, f4)                                                  # the same hits: no ties in this scene
    hit = f4 >= 0
    assert np.array_equal(bits(t2[hit]), bits(t4[hit]))
