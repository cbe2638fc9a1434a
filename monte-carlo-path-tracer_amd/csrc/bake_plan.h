// The host half of surface baking, pure functions without a device: the validation of a bake-point list and the texel-to-surface
// map of a lightmap.  mcpt_api.cpp calls them; tests/bake_host_check.cpp builds them into a stand-alone program.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/mcpt.h"

#define BK_MAX_POINTS 0x3ffffffu       // what one probe job of the wavefront pipeline takes (mcpt_probe_paths, mcpt_render_camera)

// mcpt_set_bake_points' rule for one list: "" or what is wrong with the first bad point.
inline std::string bk_check_points(const mcpt_bake_point* p, uint32_t n, uint32_t n_face) {
    if (n > BK_MAX_POINTS) return "more than 67 108 863 points";
    if (n && !p) return "null list";
    for (uint32_t i = 0; i < n; i++) {
        const std::string at = "point " + std::to_string(i) + ": ";
        if (p[i].face >= n_face) return at + "face out of range";
        if (!std::isfinite(p[i].u) || !std::isfinite(p[i].v)) return at + "u or v is not finite";
        if (p[i].u < 0.f || p[i].v < 0.f || double(p[i].u) + double(p[i].v) > 1.0) return at + "(u, v) lies outside the triangle";
        if (p[i].flags & ~MCPT_BAKE_BACK_SIDE) return at + "unknown flag bit";
    }
    return "";
}

// The barycentrics of a texel centre rounded to fp32, then clamped so that bk_check_points accepts them: u, v >= 0 and double(u) + double(v) <= 1.
inline void bk_clamp_uv(double u, double v, float& fu, float& fv) {
    fu = float(u); fv = float(v);
    if (!(fu > 0.f)) fu = 0.f;
    if (!(fv > 0.f)) fv = 0.f;
    while (double(fu) + double(fv) > 1.0) {                                   // (one fp32 step of the larger one at a time: a handful at the most)
        if (fv >= fu) fv = std::nextafterf(fv, 0.f); else fu = std::nextafterf(fu, 0.f);
    }
}

// The texel-to-surface map of a width x height lightmap over the scene's texcoords: texel (i, j) has the centre ((i + 0.5) / width,
// (j + 0.5) / height) and belongs to the LOWEST face (Model::face order) whose three fp64 edge functions, each divided by the face's uv area, are
// all >= 0.  A face whose uv area is 0 or not finite is skipped; uv is not wrapped.  Every face is rasterised over the texels its uv bound can
// reach (one more on every side: the edge functions decide) and a texel keeps its first owner -- the same map as testing every face per texel.
// points / texel: in texel order (j * width + i ascending).  Returns "" or what is wrong with the description.
inline std::string bk_lightmap_points(const mcpt_scene_desc* sc, uint32_t width, uint32_t height, std::vector<mcpt_bake_point>& points, std::vector<uint32_t>& texel) {
    points.clear(); texel.clear();
    if (!sc) return "null scene";
    if (width == 0 || height == 0 || uint64_t(width) * height > BK_MAX_POINTS) return "the lightmap has no texels or more than 67 108 863";
    if (sc->n_face && !sc->face) return "null face list";
    if (sc->n_texcoord && !sc->texcoord) return "null texcoord list";
    const size_t n = size_t(width) * height;
    std::vector<int64_t> owner(n, -1); std::vector<float> uv(2 * n, 0.f);
    const double W = double(width), H = double(height);
    for (uint32_t f = 0; f < sc->n_face; f++) {
        double t[3][2];
        for (int k = 0; k < 3; k++) {
            const int32_t ti = sc->face[12 * size_t(f) + 4 * k + 2];
            if (ti < 0 || uint32_t(ti) >= sc->n_texcoord) return "face " + std::to_string(f) + ": texcoord index out of range";
            t[k][0] = sc->texcoord[2 * size_t(ti)]; t[k][1] = sc->texcoord[2 * size_t(ti) + 1];
        }
        const double ax = t[0][0], ay = t[0][1], e1x = t[1][0] - ax, e1y = t[1][1] - ay, e2x = t[2][0] - ax, e2y = t[2][1] - ay;
        const double area = e1x * e2y - e2x * e1y;
        if (area == 0.0 || !std::isfinite(area)) continue;
        const double xlo = std::fmin(t[0][0], std::fmin(t[1][0], t[2][0])), xhi = std::fmax(t[0][0], std::fmax(t[1][0], t[2][0]));
        const double ylo = std::fmin(t[0][1], std::fmin(t[1][1], t[2][1])), yhi = std::fmax(t[0][1], std::fmax(t[1][1], t[2][1]));
        if (!(xhi >= 0.0 && xlo <= 1.0 && yhi >= 0.0 && ylo <= 1.0)) continue;                 // (also a bound that is not a number)
        auto first = [](double lo, double size) { const double x = std::floor(lo * size - 0.5) - 1.0; return x > 0.0 ? (x < size ? uint32_t(x) : uint32_t(size)) : 0u; };
        auto last = [](double hi, double size) { const double x = std::ceil(hi * size - 0.5) + 1.0; return x < size - 1.0 ? (x > 0.0 ? uint32_t(x) : 0u) : uint32_t(size) - 1u; };
        const uint32_t i0 = first(xlo, W), i1 = last(xhi, W), j0 = first(ylo, H), j1 = last(yhi, H);
        for (uint32_t j = j0; j <= j1 && j < height; j++)
            for (uint32_t i = i0; i <= i1 && i < width; i++) {
                const size_t k = size_t(j) * width + i;
                if (owner[k] >= 0) continue;
                const double px = (double(i) + 0.5) / W - ax, py = (double(j) + 0.5) / H - ay;
                const double u = (px * e2y - e2x * py) / area, v = (e1x * py - px * e1y) / area;
                const double w = ((e1x - px) * (e2y - py) - (e2x - px) * (e1y - py)) / area;     // cross(t1 - p, t2 - p): the edge opposite corner 0
                if (!(u >= 0.0 && v >= 0.0 && w >= 0.0)) continue;
                owner[k] = int64_t(f);
                bk_clamp_uv(u, v, uv[2 * k], uv[2 * k + 1]);
            }
    }
    for (size_t k = 0; k < n; k++) {
        if (owner[k] < 0) continue;
        mcpt_bake_point p; p.face = uint32_t(owner[k]); p.u = uv[2 * k]; p.v = uv[2 * k + 1]; p.flags = 0u;
        points.push_back(p); texel.push_back(uint32_t(k));
    }
    return "";
}
