"""-m gpu: the first and the last steps of every path -- cast_ray, load_hit_shade, tex_color (csrc/pt_device.h) and tonemap_kernel (csrc/kernels.hip)
-- at their edges, through the probes and the film calls of the C ABI, against the float64 restatements and the error models of
tests/endpoints_ref.py.  One test per function; every case is inside its bound or its admissible set, none is forgiven, and the worst ratio per
family is printed.  The constants of the models are measured on the CPU by tests/test_endpoints_ref.py; the device's own worst ratios on an MI355X
are in DESIGN.md section 5.1.
"""
import numpy as np
import pytest

from tests import endpoints_ref as E
from tests.kit import bits

pytestmark = pytest.mark.gpu


def test_cast_ray_edges(pkg):
    """Every camera of camera_cases through mcpt_set_camera on one context per film of FILMS: origin and direction within half an fp32 ulp (plus
    float64 slack) of cast_ref on every pixel of pixel_cases.  The context keeps the centre it was created with, whatever the eye."""
    S = pkg.scenes
    fams, ratios = [], []
    for w, h in E.FILMS:
        scene = S.open_box(w, h)
        r = pkg.Renderer(scene)
        centre = np.array(r.info().centre)
        xy, xi, pf = E.pixel_cases(w, h)
        assert set(pf) == {"corners", "last_column", "xi_edges", "random"} and (xy[:, 0] < w).all() and (xy[:, 1] < h).all()
        cams = E.camera_cases(scene.camera, centre)
        assert {c[0] for c in cams} == {"fovy", "up", "far_eye", "lookat_distance", "axis"}
        for family, name, c in cams:
            cam = S.Camera(c["eye"], c["lookat"], c["up"], c["fovy"], w, h)
            r.set_camera(cam)
            got = r.probe_cast_ray(xy, xi)
            origin, direction = E.cast_ref(cam, centre, w, h, xy, xi)
            ratio = E.cast_ratio(got, origin, direction)
            assert ratio.max() <= 1, "film %dx%d, camera %s, pixel %s xi %s (%s): error / bound %.3g" % (
                w, h, name, xy[ratio.argmax()], xi[ratio.argmax()], pf[ratio.argmax()], ratio.max())
            fams += [np.full(len(ratio), family), pf]; ratios += [ratio, ratio]
        assert np.array_equal(np.array(r.info().centre), centre)
        r.close()
    E.print_worst("cast_ray", np.concatenate(fams), np.concatenate(ratios))


def test_hit_shade_edges(pkg):
    """load_hit_shade on hit_mesh / hit_cases: normal and uv within K_HIT 2^-24 of their absolute-value forms, `front` equal off the marginal cases, a
    zero normal sum not finite."""
    scene, face_family = E.hit_mesh(pkg)
    case = E.hit_cases(scene, face_family)
    assert set(case["face_family"]) == {"distinct", "uv0", "cancel3", "cancel6", "equal", "zero_corner", "zero_sum"}
    assert set(case["family"]) == {"corners", "edge_mid", "sum_one", "w_negative", "target", "interior", "nd_0", "nd_1e-7", "nd_1e-4"}
    ref = E.hit_shade_ref(E.corner_records(scene), case["tri"], case["u"], case["v"], case["d"])
    r = pkg.Renderer(scene)
    out = r.probe_hit_shade(case["tri"], case["u"], case["v"], case["d"])
    r.close()
    ratio, marginal, bad = E.hit_check(ref, out)
    E.print_worst("load_hit_shade, by face", case["face_family"], ratio, E.K_HIT)
    E.print_worst("load_hit_shade, by point", case["family"], ratio, E.K_HIT)
    zero = ~np.isfinite(ref.n).all(1)
    print("%d cases, %d marginal in `front`, %d with a zero normal sum" % (len(ratio), marginal.sum(), zero.sum()))
    assert zero.sum() >= 8 and len(ratio) <= 20000
    i = int(np.flatnonzero(bad)[0]) if bad.any() else 0
    assert not bad.any(), "%d cases outside: first face %d (%s) at u %r v %r (%s): got %s, want n %s tu %r tv %r front %s, ratio %.3g" % (
        bad.sum(), case["tri"][i], case["face_family"][i], case["u"][i], case["v"][i], case["family"][i], out[i], ref.n[i], ref.tu[i], ref.tv[i], ref.front[i], ratio[i])


def test_texture_edges(pkg):
    """tex_color on every texture of TEXTURES in one scene (tex_off adds up across them): the texel is tex_ref's on every case, no tolerance.  A texel
    holds (x, y, material), so a wrong one names itself."""
    scene, first, dims = E.texture_scene(pkg)
    table = np.concatenate([pkg.material_texels(m).reshape(-1, 3) for m in scene.materials[first:]])
    r = pkg.Renderer(scene)
    seen = set()
    for k, (w, h, off) in enumerate(dims):
        uv, fam = E.texture_cases(w, h)
        assert set(fam) == {"texel_edges", "cap", "denormal", "huge", "uniform"} and len(uv) <= 20000
        got = r.probe_texture(first + k, uv)
        x, y, idx = E.tex_ref(w, h, off, uv)
        assert (x >= 0).all() and (x < w).all() and (y >= 0).all() and (y < h).all()
        bad = np.flatnonzero(np.any(bits(got) != bits(table[idx]), axis=1))
        assert bad.size == 0, "%dx%d image: %d of %d texels differ, first uv %r (%s): got (x, y, material) %s, want %s" % (
            w, h, bad.size, len(uv), uv[bad[0]], fam[bad[0]], got[bad[0]], table[idx[bad[0]]])
        print("tex_color %4dx%-4d at texel %5d: %5d cases, all equal; x in %d..%d, y in %d..%d" % (w, h, off, len(uv), x.min(), x.max(), y.min(), y.max()))
        seen.add((int(x.max()) == int(0.999 * w), int(y.max()) == int(0.999 * h)))
    r.close()
    assert seen == {(True, True)}                                            # the texel of the 0.999 cap, the last an image can give (1998 of 2000), was asked for on both axes


def _needed_k(level, y):
    """The smallest K at which `level` is admissible for y: 0 where it is floor(y)."""
    level = level.astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.where(level > y, level - y, np.where(level + 1 <= y, y - np.nextafter(level + 1, 0), 0.0))
        d = np.where((level >= 255) & (y >= 255), 0.0, np.maximum(d - E.Y_FLOOR, 0.0))
        return np.where(d == 0, 0.0, d / (E.EPS24 * y))


def test_tonemap_edges(pkg):
    """tonemap_kernel on tonemap_cases laid out as films of TONEMAP_FILMS (every case on the 37 x 21 film, one film's worth on the others): every
    level inside tonemap_ref's admissible set, mcpt_tonemap, mcpt_tonemap_map and mcpt_tonemap_buffer bit-equal, flip_y the same image reversed in y."""
    rgba, family = E.tonemap_cases()
    assert set(family.ravel()) == {"boundary", "special", "above_one", "denormal", "generic"}
    fams, need = [], []
    for w, h in E.TONEMAP_FILMS:
        r = pkg.Renderer(pkg.scenes.open_box(w, h))
        for n, (film, fam) in enumerate(E.tonemap_films(rgba, family, w, h)):
            if n and (w, h) != (37, 21):
                break
            r.write_accum(film)
            img = r.tonemap()
            assert np.array_equal(img, r.tonemap_map()) and np.array_equal(img, r.tonemap_buffer(r.accum_device_ptr()))
            flipped = r.tonemap(flip_y=True)
            assert np.array_equal(flipped, img[::-1]) and np.array_equal(flipped, r.tonemap_map(flip_y=True))
            assert np.array_equal(flipped, r.tonemap_buffer(r.accum_device_ptr(), flip_y=True))
            lo, hi, y = E.tonemap_ref(film)
            k = _needed_k(img, y)
            bad = np.argwhere((img < lo) | (img > hi))
            assert bad.size == 0, "film %dx%d: %d levels outside; first sum %r count %r (%s): level %d, admissible %d..%d (y = %.9g)" % (
                w, h, len(bad), film[bad[0][0], bad[0][1], bad[0][2]], film[bad[0][0], bad[0][1], 3], fam[tuple(bad[0])], img[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])], y[tuple(bad[0])])
            fams.append(fam.ravel()); need.append(k.ravel())
        r.close()
    E.print_worst("tonemap (K needed)", np.concatenate(fams), np.concatenate(need), E.TONEMAP_DEVICE_FACTOR * E.K_T)


def test_set_camera_refuses_an_up_parallel_to_the_view(pkg):
    """cross(front, up) exactly zero (up along the view, against it, or zero) is MCPT_ERR_INVALID_ARG and changes nothing; 1e-3 rad off is a camera."""
    S = pkg.scenes
    scene = S.open_box(8, 8)
    r = pkg.Renderer(scene)
    xy = np.array([[0, 0], [7, 7], [3, 4]], np.int32); xi = np.full((3, 2), 0.5, np.float32)
    before = r.probe_cast_ray(xy, xi)
    c = scene.camera
    for up in ((0.0, 0.0, -1.0), (0.0, 0.0, 3.5), (0.0, 0.0, 0.0), (0.0, 1e200, 0.0)):
        with pytest.raises(pkg.McptError, match="mcpt status 1: mcpt_set_camera"):
            r.set_camera(S.Camera(c.eye, c.lookat, up, c.fovy, 8, 8))
        assert np.array_equal(bits(r.probe_cast_ray(xy, xi)), bits(before))
    near = [cc for cc in E.camera_cases(c, r.info().centre) if cc[1] == "up 1e-3 rad from the view"][0][2]
    r.set_camera(S.Camera(near["eye"], near["lookat"], near["up"], near["fovy"], 8, 8))
    assert np.isfinite(r.probe_cast_ray(xy, xi)).all()
    r.close()
    with pytest.raises(pkg.McptError, match="mcpt status 1: camera"):
        pkg.Renderer(S.SceneData(scene.name, scene.vertex, scene.normal, scene.texcoord, scene.face, scene.materials, S.Camera(c.eye, c.lookat, (0.0, 0.0, -2.0), c.fovy, 8, 8)))
