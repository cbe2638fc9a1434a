// mcpt_cli -- headless replacement for the reference's GLFW shell (src/main.cpp:4-39): load a scene, render N frames
// (= spp), print the reference's per-frame line, save <name><frames>.png.  `--gpus N` shards the sample range over N
// devices of this node from ONE process and sums the films with RCCL (ncclAllReduce over xGMI).
#include <atomic>
#include <chrono>
#include <cmath>
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "Render.h"

static void usage() {
    std::cout << "usage: mcpt_cli scene.obj [--spp N] [--batch B] [--depth D] [--gpus G] [--shard samples|tiles] [--out prefix] [--seed S] [--recursive] [--corrected]\n"
                 "                          [--deterministic] [--ref-index-order] [--ref-tie-order] [--gpu-bvh] [--check] [--dump-model file] [--save-every K]\n"
                 "                          [--denoise]   (also writes <prefix><frames>_denoised.png, and one per --save-every image)\n"
                 "                          [--denoise-robust]   (--denoise with emitted light kept apart and fireflies clamped)\n"
                 "                          [--adaptive T [--min-spp N]]   adaptive sampling per 8x8 tile down to error T, --spp samples at most per pixel\n"
                 "                                        (one GPU; also writes <prefix>_spp.png, a grey map of log2(samples) / log2(spp))\n"
                 "                          [--turntable N]   N frames of --spp samples each, the camera rotated about lookat around up by 360/N degrees per frame\n"
                 "                                        (one GPU; writes <prefix>_turn<frame>.png)\n"
                 "                          [--reproject H]   with --turntable: frames after the first carry the film over (temporal reprojection, at most H samples\n"
                 "                                        of history per pixel) instead of starting empty\n"
                 "                          [--wobble A]   with --turntable: every frame after the first also displaces the vertices by\n"
                 "                                        A sin(2 pi frame / N) (sin 9y, sin 7z, sin 8x) (device-side refit; with --reproject the film follows the surfaces)\n"
                 "                          [--light-pulse A]   with --turntable: frame k scales the radiance of every emissive material by 1 + A sin(2 pi k / N)\n"
                 "                                        (materials and light list edited on the device, the film restarts every frame; not with --reproject)\n"
                 "                          [--spin MTLNAME]   with --turntable: the faces of that material turn as one rigid part, by 360 k / N degrees in frame k about\n"
                 "                                        the camera's up axis through their bounding box's centre (one 3x4 matrix per frame, applied on the device;\n"
                 "                                        honours --reproject; not with --wobble).  --spin may be given together with --bend and / or --swell, for\n"
                 "                                        different materials that share no vertex and no normal: each part is then driven by its own deformer and every\n"
                 "                                        frame is ONE parts update (DESIGN.md 23) -- --spin's faces by the groups, --bend's / --swell's by the skin\n"
                 "                                        (--bend alone) or the morph; nothing else moves\n"
                 "                          [--bend MTLNAME DEG]   with --turntable: the faces of that material bend as a two-bone part (linear-blend skinning on the\n"
                 "                                        device): a vertex follows the upper bone by its height inside the part's y-extent, the lower bone stays,\n"
                 "                                        the upper one turns by DEG sin(2 pi k / N) about z through the part's centre in frame k (honours --reproject;\n"
                 "                                        not with --wobble)\n"
                 "                          [--dual-quat]   with --bend: the bones are blended as unit dual quaternions instead of matrices (DESIGN.md 21): the bent\n"
                 "                                        part keeps its volume however far it turns; the bones must be rigid, as --bend's are\n"
                 "                          [--swell MTLNAME AMOUNT]   with --turntable: the faces of that material swell and shrink about the centroid of their\n"
                 "                                        vertices (one morph target on the device, delta = vertex - centroid, weight AMOUNT sin(2 pi k / N) in frame k:\n"
                 "                                        a uniform scaling, so the normals stay); combines with --bend (morph, then skin, one call per frame);\n"
                 "                                        honours --reproject; not with --wobble\n"
                 "                          [--sequence PATTERN COUNT [--slowdown S] [--smooth]]   with --turntable: baked vertex animation from an OBJ sequence.  PATTERN\n"
                 "                                        holds one printf integer conversion (cloth_%04d.obj); frames 0 .. COUNT - 1 are loaded, each with the scene's\n"
                 "                                        vertex and normal counts and its faces, and uploaded once as keyframes one time unit apart (DESIGN.md 22);\n"
                 "                                        turntable frame j plays time j / S (S = 1 by default), the in-between frames are interpolated on the device,\n"
                 "                                        linearly or with --smooth as a Catmull-Rom spline; past the last file the last frame stays; honours\n"
                 "                                        --reproject; not with --wobble, --spin, --bend or --swell\n"
                 "                          [--auto-normals]   with --turntable and --wobble, --bend, --swell or --sequence: the smooth normals are recomputed on the device\n"
                 "                                        after every frame's update, area-weighted, from the deformed faces -- all normals with --wobble and --sequence,\n"
                 "                                        otherwise those of the named material's faces (honours --reproject and --rebuild-above)\n"
                 "                          [--rebuild-above R]   with --turntable and --wobble, --spin, --bend, --swell or --sequence: after a frame's update the trees are built anew\n"
                 "                                        (mcpt_rebuild_trees, film kept) when wide_area_ratio exceeds R; prints frame, ratio and cost per rebuild\n"
                 "                          [--hide MTLNAME]   with --turntable: the faces of that material are hidden in every frame (DESIGN.md 24: a visibility mask\n"
                 "                                        on the device -- no ray hits them, they are no lights; same upload, same trees)\n"
                 "                          [--blink MTLNAME K]   with --turntable: the faces of that material are visible in the frames f with (f / K) % 2 == 0 and hidden\n"
                 "                                        in the others; the mask changes only where that changes.  --hide and --blink honour --reproject (the film is\n"
                 "                                        carried across the change) and go with the camera alone: not with --wobble, --light-pulse, --spin, --bend,\n"
                 "                                        --swell or --sequence, and not with each other\n"
                 "                          [--aperture R --focus D | --autofocus X Y [--blades N [--blade-rotation DEG]]]   a thin lens of radius R instead of the\n"
                 "                                        pinhole (DESIGN.md 25): sharp at distance D along the view direction, or where pixel (X, Y) -- row 0 at the\n"
                 "                                        top of the saved image -- looks (with --turntable: in the first frame); the aperture a disk, or a polygon of\n"
                 "                                        N in [3, 16] blades turned by DEG degrees\n"
                 "                          [--ortho H]   an orthographic camera whose film is H world units high    [--panorama]   a 360 x 180 degree equirectangular camera\n"
                 "                                        (these three exclude each other; they go with --turntable and --gpus, not with --adaptive or --shard tiles;\n"
                 "                                        one pass per sample; --denoise and --reproject keep describing the pinhole view)\n"
                 "                          [--sh-grid NX NY NZ OUT.txt [--sh-passes N] [--sh-irradiance]]   instead of a picture: NX x NY x NZ light probes at the cell centres of\n"
                 "                                        the scene's bounds, N passes (default 16) of 64 rays each; one line per probe: position, 27 spherical-harmonic\n"
                 "                                        coefficients (per channel k = l (l + 1) + m, l <= 2) of the radiance around it or, with --sh-irradiance, of the\n"
                 "                                        irradiance by normal, and the share of rays that met a surface from behind (not with --recursive)\n"
                 "                          [--bake-lightmap W H OUT.ppm [--bake-spp N] [--bake-irradiance] [--bake-direct]]   instead of a picture: a W x H lightmap over the scene's texture\n"
                 "                                        coordinates (DESIGN.md 27), N samples per texel (64 by default) started ON the surfaces: the radiance a diffuse texel\n"
                 "                                        sends out, or with --bake-irradiance the irradiance it receives; through the picture's transfer curve; texels no\n"
                 "                                        face covers are black; row 0 of the file is v = 0, as a Map_Kd image is read (one GPU; honours --depth, --seed,\n"
                 "                                        --corrected, --deterministic; not with --recursive).  --bake-direct: sample the lights at the texel itself,\n"
                 "                                        MIS-weighted against the cosine ray (less noise in direct light under small lamps)\n"
                 "       mcpt_cli --decode-image texture.(png|jpg|ppm|bmp|tga|hdr) out.(ppm|pfm)\n";
}

int main(int argc, char** argv) {
    if (argc < 2) { usage(); return 2; }
    if (std::string(argv[1]) == "--decode-image") {              // host-only helper: texture file -> binary PPM (what map_Kd textures decode to)
        if (argc != 4) { usage(); return 2; }
        int w = 0, h = 0; std::vector<unsigned char> rgb;
        {   // a Radiance .hdr decodes to linear floats: written as a binary PFM-like dump ("PF\nw h\n-1.0\n" + w*h*3 little-endian floats, top row first)
            std::vector<float> lin;
            if (load_image_hdr(argv[2], w, h, lin)) {
                FILE* f = std::fopen(argv[3], "wb");
                if (!f) return 1;
                std::fprintf(f, "PF\n%d %d\n-1.0\n", w, h); std::fwrite(lin.data(), 4, lin.size(), f); std::fclose(f);
                return 0;
            }
        }
        if (!load_image_rgb8(argv[2], w, h, rgb)) { std::cerr << "Error: cannot decode " << argv[2] << std::endl; return 1; }
        FILE* f = std::fopen(argv[3], "wb");
        if (!f) return 1;
        std::fprintf(f, "P6\n%d %d\n255\n", w, h); std::fwrite(rgb.data(), 1, rgb.size(), f); std::fclose(f);
        return 0;
    }
    std::string filename = argv[1], out, dump_model;
    uint32_t spp = 64, batch = 0, depth = 0, gpus = 1, save_every = 0; uint64_t seed = 20251004; uint32_t flags = 0, integrator = 0; bool ref_order = false, check_only = false, shard_tiles = false, denoise = false, denoise_robust = false;
    float adaptive = -1.f; uint32_t min_spp = 0, turntable = 0;
    bool reproject = false; float history = 0.f;
    bool wobble = false; double wobble_a = 0.0;
    bool pulse = false; double pulse_a = 0.0;
    std::string spin, bend, swell; double bend_deg = 0.0, swell_a = 0.0;
    bool rebuild = false; double rebuild_above = 0.0;
    bool auto_normals = false, dual_quat = false;
    std::string sequence; int sequence_n = 0; bool slowdown_set = false, smooth = false; double slowdown = 1.0;
    std::string hide, blink; int blink_k = 0;
    bool aperture_set = false, focus_set = false, autofocus_set = false, blades_set = false, rotation_set = false, ortho_set = false, panorama = false;
    double aperture = 0.0, focus = 0.0, blade_deg = 0.0, ortho_h = 0.0; int focus_x = 0, focus_y = 0, blades = 0;
    std::string sh_out; int sh_n[3] = {0, 0, 0}, sh_passes = 16; bool sh_grid = false, sh_irradiance = false, sh_opts = false;
    std::string bake_out; int bake_w = 0, bake_h = 0, bake_spp = 64; bool bake_irradiance = false, bake_opts = false, bake_direct = false;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i]; auto next = [&]() { return i + 1 < argc ? argv[++i] : (char*)"0"; };
        if (a == "--spp") spp = uint32_t(std::atoi(next())); else if (a == "--batch") batch = uint32_t(std::atoi(next()));
        else if (a == "--depth") depth = uint32_t(std::atoi(next())); else if (a == "--gpus") gpus = uint32_t(std::atoi(next()));
        else if (a == "--out") out = next(); else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
        else if (a == "--recursive") integrator = MCPT_INTEGRATOR_RECURSIVE_NEE; else if (a == "--corrected") flags |= MCPT_FLAG_CORRECT_SHADOW_T2;
        else if (a == "--deterministic") flags |= MCPT_FLAG_DETERMINISTIC; else if (a == "--ref-index-order") ref_order = true;
        else if (a == "--gpu-bvh") flags |= MCPT_FLAG_GPU_BVH_BUILD;
        else if (a == "--ref-tie-order") flags |= MCPT_FLAG_REFERENCE_TIE_ORDER;
        else if (a == "--check") check_only = true;
        else if (a == "--dump-model") dump_model = next();
        else if (a == "--save-every") save_every = uint32_t(std::atoi(next()));
        else if (a == "--shard") shard_tiles = std::string(next()) == "tiles";
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-robust") denoise = denoise_robust = true;
        else if (a == "--adaptive") adaptive = float(std::atof(next()));
        else if (a == "--min-spp") min_spp = uint32_t(std::atoi(next()));
        else if (a == "--turntable") turntable = uint32_t(std::atoi(next()));
        else if (a == "--reproject") { reproject = true; history = float(std::atof(next())); }
        else if (a == "--wobble") { wobble = true; wobble_a = std::atof(next()); }
        else if (a == "--light-pulse") { pulse = true; pulse_a = std::atof(next()); }
        else if (a == "--spin") spin = next();
        else if (a == "--bend") { bend = next(); bend_deg = std::atof(next()); }
        else if (a == "--dual-quat") dual_quat = true;
        else if (a == "--swell") { swell = next(); swell_a = std::atof(next()); }
        else if (a == "--sequence") { sequence = next(); sequence_n = std::atoi(next()); }
        else if (a == "--slowdown") { slowdown_set = true; slowdown = std::atof(next()); }
        else if (a == "--smooth") smooth = true;
        else if (a == "--auto-normals") auto_normals = true;
        else if (a == "--rebuild-above") { rebuild = true; rebuild_above = std::atof(next()); }
        else if (a == "--hide") hide = next();
        else if (a == "--blink") { blink = next(); blink_k = std::atoi(next()); }
        else if (a == "--aperture") { aperture_set = true; aperture = std::atof(next()); }
        else if (a == "--focus") { focus_set = true; focus = std::atof(next()); }
        else if (a == "--autofocus") { autofocus_set = true; focus_x = std::atoi(next()); focus_y = std::atoi(next()); }
        else if (a == "--blades") { blades_set = true; blades = std::atoi(next()); }
        else if (a == "--blade-rotation") { rotation_set = true; blade_deg = std::atof(next()); }
        else if (a == "--ortho") { ortho_set = true; ortho_h = std::atof(next()); }
        else if (a == "--panorama") panorama = true;
        else if (a == "--bake-lightmap") { bake_w = std::atoi(next()); bake_h = std::atoi(next()); bake_out = next(); }
        else if (a == "--sh-grid") { sh_grid = true; for (int k = 0; k < 3; k++) sh_n[k] = std::atoi(next()); sh_out = next(); }
        else if (a == "--sh-passes") { sh_opts = true; sh_passes = std::atoi(next()); }
        else if (a == "--sh-irradiance") sh_opts = sh_irradiance = true;
        else if (a == "--bake-spp") { bake_opts = true; bake_spp = std::atoi(next()); }
        else if (a == "--bake-irradiance") bake_opts = bake_irradiance = true;
        else if (a == "--bake-direct") bake_opts = bake_direct = true;
        else { usage(); return 2; }
    }
    if (adaptive >= 0.f && gpus > 1) { std::cerr << "Error: --adaptive renders on one GPU only (drop --gpus)" << std::endl; return 2; }
    if (turntable && (gpus > 1 || adaptive >= 0.f)) { std::cerr << "Error: --turntable renders on one GPU, without --adaptive" << std::endl; return 2; }
    if (reproject && (!turntable || !(history >= 1.f))) { std::cerr << "Error: --reproject H needs --turntable N and H >= 1" << std::endl; return 2; }
    if (wobble && (!turntable || !(std::fabs(wobble_a) <= 1e6))) { std::cerr << "Error: --wobble A needs --turntable N and a finite A" << std::endl; return 2; }
    if (pulse && (!turntable || !(std::fabs(pulse_a) <= 1e6))) { std::cerr << "Error: --light-pulse A needs --turntable N and a finite A" << std::endl; return 2; }
    if (pulse && reproject) { std::cerr << "Error: --light-pulse restarts the film every frame: radiance reprojected across it would be the old light's (drop --reproject)" << std::endl; return 2; }
    if (!spin.empty() && (!turntable || wobble)) { std::cerr << "Error: --spin MTLNAME needs --turntable N and no --wobble (both write the vertices)" << std::endl; return 2; }
    if (!bend.empty() && (!turntable || wobble || !(std::fabs(bend_deg) <= 1e6))) {
        std::cerr << "Error: --bend MTLNAME DEG needs --turntable N, a finite DEG and no --wobble (which writes every vertex)" << std::endl; return 2;
    }
    if (!spin.empty() && (spin == bend || spin == swell)) {
        std::cerr << "Error: --spin and --" << (spin == bend ? "bend" : "swell") << " name the same material (" << spin << "): a face has one deformer" << std::endl; return 2;
    }
    if (dual_quat && bend.empty()) { std::cerr << "Error: --dual-quat needs --bend MTLNAME DEG (it chooses how --bend's bones are blended)" << std::endl; return 2; }
    if (!swell.empty() && (!turntable || wobble || !(std::fabs(swell_a) <= 1e6))) {
        std::cerr << "Error: --swell MTLNAME AMOUNT needs --turntable N, a finite AMOUNT and no --wobble (which writes every vertex)" << std::endl; return 2;
    }
    if ((slowdown_set || smooth) && sequence.empty()) { std::cerr << "Error: --slowdown S and --smooth need --sequence PATTERN COUNT (they choose how it is played)" << std::endl; return 2; }
    if (!sequence.empty()) {
        if (!turntable || wobble || !spin.empty() || !bend.empty() || !swell.empty()) {
            std::cerr << "Error: --sequence PATTERN COUNT needs --turntable N and none of --wobble, --spin, --bend and --swell (all of them write the vertices)" << std::endl; return 2;
        }
        // exactly one conversion, %d with an optional zero flag and width: the pattern is handed to snprintf
        const size_t at = sequence.find('%');
        size_t end = at == std::string::npos ? at : at + 1;
        while (end != std::string::npos && end < sequence.size() && std::isdigit(static_cast<unsigned char>(sequence[end]))) end++;
        if (at == std::string::npos || end >= sequence.size() || sequence[end] != 'd' || end - at > 6 || sequence.find('%', end) != std::string::npos) {
            std::cerr << "Error: --sequence: PATTERN needs exactly one integer conversion such as %04d" << std::endl; return 2;
        }
        if (sequence_n < 2 || sequence_n > MCPT_KEYFRAMES_MAX) { std::cerr << "Error: --sequence: COUNT must be in [2, 65536]" << std::endl; return 2; }
        if (!(slowdown > 0.0 && slowdown <= 1e6)) { std::cerr << "Error: --sequence: --slowdown S needs a finite S > 0" << std::endl; return 2; }
    }
    if (rebuild && (!turntable || !(wobble || !spin.empty() || !bend.empty() || !swell.empty() || !sequence.empty()) || !(rebuild_above >= 0.0))) {
        std::cerr << "Error: --rebuild-above R needs --turntable N with --wobble, --spin, --bend, --swell or --sequence, and R >= 0" << std::endl; return 2;
    }
    if (auto_normals && (!turntable || !(wobble || !bend.empty() || !swell.empty() || !sequence.empty()))) {
        std::cerr << "Error: --auto-normals needs --turntable N with --wobble, --bend, --swell or --sequence (the updates whose normals it recomputes)" << std::endl; return 2;
    }
    if (!hide.empty() || !blink.empty()) {
        if (!turntable || wobble || pulse || !spin.empty() || !bend.empty() || !swell.empty() || !sequence.empty() || (!hide.empty() && !blink.empty())) {
            std::cerr << "Error: --hide MTLNAME and --blink MTLNAME K need --turntable N and none of --wobble, --light-pulse, --spin, --bend, --swell and --sequence, and exclude each other" << std::endl; return 2;
        }
        if (!blink.empty() && blink_k < 1) { std::cerr << "Error: --blink MTLNAME K needs K >= 1" << std::endl; return 2; }
    }
    // --aperture / --ortho / --panorama: the camera model of DESIGN.md 25; the render loops below then call render_camera
    const bool lens = aperture_set || focus_set || autofocus_set || blades_set || rotation_set;
    const bool camera_model = lens || ortho_set || panorama;
    if (int(lens) + int(ortho_set) + int(panorama) > 1) { std::cerr << "Error: --aperture, --ortho and --panorama exclude each other" << std::endl; return 2; }
    if (lens && (!aperture_set || focus_set == autofocus_set || !(aperture >= 0.0 && aperture <= 1e300) || (focus_set && !(focus > 0.0 && focus <= 1e300)))) {
        std::cerr << "Error: --aperture R needs R >= 0 and exactly one of --focus D (D > 0) and --autofocus X Y" << std::endl; return 2;
    }
    if (blades_set && (blades < 3 || blades > int(MCPT_CAMERA_MAX_BLADES))) { std::cerr << "Error: --blades N needs N in [3, 16]" << std::endl; return 2; }
    if (rotation_set && (!blades_set || !(std::fabs(blade_deg) <= 1e6))) { std::cerr << "Error: --blade-rotation DEG needs --blades N and a finite DEG" << std::endl; return 2; }
    if (ortho_set && !(ortho_h > 0.0 && ortho_h <= 1e300)) { std::cerr << "Error: --ortho H needs a finite H > 0" << std::endl; return 2; }
    if (camera_model && (adaptive >= 0.f || shard_tiles || integrator != MCPT_INTEGRATOR_MIS)) {
        std::cerr << "Error: --aperture, --ortho and --panorama render pass by pass through the wavefront pipeline: not with --adaptive, --shard tiles or --recursive" << std::endl; return 2;
    }
    if (camera_model && (denoise || reproject))
        std::cerr << "Note: --denoise and --reproject are guided by features of the pinhole view, whatever camera model renders the film" << std::endl;
    // --bake-lightmap W H OUT.ppm: the surface baking of DESIGN.md 27 instead of a picture
    const bool bake = bake_w != 0 || bake_h != 0 || !bake_out.empty();
    if (bake_opts && !bake) { std::cerr << "Error: --bake-spp N, --bake-irradiance and --bake-direct need --bake-lightmap W H OUT.ppm" << std::endl; return 2; }
    if (bake && (bake_w < 1 || bake_h < 1 || bake_w > 8192 || bake_h > 8192 || bake_out.empty() || bake_out == "0" || bake_spp < 1)) {
        std::cerr << "Error: --bake-lightmap W H OUT.ppm needs W and H in [1, 8192], a file name and --bake-spp N >= 1" << std::endl; return 2;
    }
    if (bake && (gpus > 1 || turntable || adaptive >= 0.f || camera_model || integrator != MCPT_INTEGRATOR_MIS)) {
        std::cerr << "Error: --bake-lightmap bakes on one GPU through the wavefront pipeline: not with --gpus, --turntable, --adaptive, a camera model or --recursive" << std::endl; return 2;
    }
    // --sh-grid NX NY NZ OUT.txt: the light probes of DESIGN.md 28 instead of a picture
    if (sh_opts && !sh_grid) { std::cerr << "Error: --sh-passes N and --sh-irradiance need --sh-grid NX NY NZ OUT.txt" << std::endl; return 2; }
    if (sh_grid && (sh_n[0] < 1 || sh_n[1] < 1 || sh_n[2] < 1 || sh_n[0] > 1024 || sh_n[1] > 1024 || sh_n[2] > 1024 || sh_out.empty() || sh_out == "0" || sh_passes < 1 ||
                    uint64_t(sh_n[0]) * uint64_t(sh_n[1]) * uint64_t(sh_n[2]) > MCPT_SH_MAX_PROBES)) {
        std::cerr << "Error: --sh-grid NX NY NZ OUT.txt needs NX, NY and NZ in [1, 1024] with at most 1 048 575 probes in all, a file name and --sh-passes N >= 1" << std::endl; return 2;
    }
    if (sh_grid && (bake || gpus > 1 || turntable || adaptive >= 0.f || camera_model || integrator != MCPT_INTEGRATOR_MIS)) {
        std::cerr << "Error: --sh-grid bakes on one GPU through the wavefront pipeline: not with --bake-lightmap, --gpus, --turntable, --adaptive, a camera model or --recursive" << std::endl; return 2;
    }
    if (wobble || !spin.empty() || !bend.empty() || !swell.empty() || !sequence.empty() || !hide.empty() || !blink.empty()) flags |= MCPT_FLAG_DYNAMIC;
    Model model(filename, ref_order);
    if (!model.ok) { std::cerr << "Error: scene did not load" << std::endl; return 1; }
    std::cout << model.face.size() << " " << model.normal.size() << " " << model.vertex.size() << std::endl;   // main.cpp:14
    // --sequence PATTERN COUNT: the frames' vertices and normals, checked against the scene before anything is created on a device
    std::vector<std::vector<dvec3>> seq_vertex, seq_normal;
    for (int j = 0; j < sequence_n && !sequence.empty(); j++) {
        char path[4096];
        if (std::snprintf(path, sizeof path, sequence.c_str(), j) >= int(sizeof path)) { std::cerr << "Error: --sequence: the path of frame " << j << " is too long" << std::endl; return 2; }
        Model frame(path, ref_order);
        if (!frame.ok) { std::cerr << "Error: --sequence: frame " << j << " (" << path << ") did not load" << std::endl; return 2; }
        if (frame.vertex.size() != model.vertex.size() || frame.normal.size() != model.normal.size()) {
            std::cerr << "Error: --sequence: frame " << j << " (" << path << ") has " << frame.vertex.size() << " vertices and " << frame.normal.size() << " normals, the scene "
                      << model.vertex.size() << " and " << model.normal.size() << std::endl; return 2;
        }
        if (frame.face != model.face) { std::cerr << "Error: --sequence: frame " << j << " (" << path << ") has other faces than the scene (the topology must not change)" << std::endl; return 2; }
        seq_vertex.push_back(frame.vertex); seq_normal.push_back(frame.normal);
    }
    if (!dump_model.empty()) {   // host-only: everything Model(filename) parsed, as text (tests compare it with the reference's own parse)
        FILE* f = std::fopen(dump_model.c_str(), "w");
        if (!f) { std::cerr << "Error: cannot write " << dump_model << std::endl; return 1; }
        std::fprintf(f, "counts %zu %zu %zu %zu %zu %d %d\n", model.vertex.size(), model.normal.size(), model.texture.size(), model.face.size(), model.materials.size(),
                     model.camerainfo.width, model.camerainfo.height);
        for (auto& v : model.vertex) std::fprintf(f, "v %.17g %.17g %.17g\n", v.x, v.y, v.z);
        for (auto& v : model.normal) std::fprintf(f, "vn %.17g %.17g %.17g\n", v.x, v.y, v.z);
        for (auto& v : model.texture) std::fprintf(f, "vt %.17g %.17g\n", v.x, v.y);
        for (auto& fc : model.face) { std::fprintf(f, "f"); for (int c = 0; c < 3; c++) for (int k = 0; k < 4; k++) std::fprintf(f, " %d", fc[c][k]); std::fprintf(f, "\n"); }
        for (auto& m : model.materials) {
            std::fprintf(f, "m %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %zu %d %d\n", m.Ks.x, m.Ks.y, m.Ks.z, m.Tr.x, m.Tr.y, m.Tr.z, m.Ns, m.Ni,
                         m.radiance.x, m.radiance.y, m.radiance.z, m.Map_Kd->image_color.size(), m.Map_Kd->image_w, m.Map_Kd->image_h);
            std::fprintf(f, "t"); for (auto& c : m.Map_Kd->image_color) std::fprintf(f, " %.9g %.9g %.9g", c.x, c.y, c.z); std::fprintf(f, "\n");
        }
        const CameraInfo& c = model.camerainfo;
        std::fprintf(f, "c %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", c.eye.x, c.eye.y, c.eye.z, c.lookat.x, c.lookat.y, c.lookat.z, c.up.x, c.up.y, c.up.z, c.fovy);
        std::fclose(f);
        if (!check_only) return 0;
    }
    if (check_only) {   // host-only: what the loader produced + what the library's flatten / BVH build makes of it (no GPU needed)
        std::vector<mcpt_material> mats; std::vector<mcpt_texture> texs; mcpt_scene_desc d; mcpt_scene_info info;
        model_to_desc(model, mats, texs, d);
        const mcpt_status st = mcpt_check_scene(&d, &info);
        double sv = 0, sn = 0, st_ = 0; long long sf = 0; double stex = 0;
        for (auto& v : model.vertex) sv += v.x + 2 * v.y + 3 * v.z;
        for (auto& v : model.normal) sn += v.x + 2 * v.y + 3 * v.z;
        for (auto& v : model.texture) st_ += v.x + 2 * v.y;
        for (auto& f : model.face) for (int i = 0; i < 3; i++) sf += f[i][0] + 3LL * f[i][1] + 5LL * f[i][2] + 7LL * f[i][3];
        for (auto& m : model.materials) for (auto& c : m.Map_Kd->image_color) stex += c.x + c.y + c.z;
        std::printf("{\"status\": %d, \"faces\": %zu, \"materials\": %zu, \"width\": %d, \"height\": %d, \"fovy\": %.17g, \"sum_v\": %.17g, \"sum_vn\": %.17g, "
                    "\"sum_vt\": %.17g, \"sum_f\": %lld, \"sum_tex\": %.9g, \"n_tris\": %u, \"n_lights\": %u, \"n_nodes\": %u, \"bvh_depth\": %u}\n",
                    int(st), model.face.size(), model.materials.size(), model.camerainfo.width, model.camerainfo.height, model.camerainfo.fovy, sv, sn, st_, sf, stex,
                    info.n_tris, info.n_lights, info.n_nodes, info.bvh_depth);
        return st == MCPT_OK ? 0 : 1;
    }
    const int w = model.camerainfo.width, h = model.camerainfo.height;
    Scene scene(w, h);
    const size_t slash = filename.rfind('/');
    const std::string file_name = filename.substr(slash == std::string::npos ? 0 : slash + 1);
    if (out.empty()) out = file_name;
    if (batch == 0) batch = spp;
    if (gpus < 1) gpus = 1;

    // The scene is flattened and its BVH built ONCE (Render::Render(Model&), Render.cpp:5-10); the other devices get device-to-device
    // copies of the finished streams (mcpt_clone_to_device): 8 GPUs cost one build + 8 uploads, not 8 builds.
    std::vector<Render*> renders(gpus, nullptr);
    for (uint32_t g = 0; g < gpus; g++) {
        if (g == 0) {
            mcpt_opts o; std::memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.device = 0; o.max_depth = depth; o.flags = flags; o.integrator = integrator;
            renders[0] = new Render(model, o); renders[0]->seed = seed;
        } else renders[g] = new Render(*renders[0], int(g));
        if (!renders[g]->ok()) return 1;
    }
    if (camera_model) {
        mcpt_camera_model cm; std::memset(&cm, 0, sizeof cm); cm.struct_size = sizeof cm;
        cm.model = lens ? MCPT_CAMERA_THIN_LENS : ortho_set ? MCPT_CAMERA_ORTHOGRAPHIC : MCPT_CAMERA_EQUIRECT;
        cm.lens_radius = aperture; cm.focus_distance = focus; cm.blades = uint32_t(blades); cm.blade_rotation = blade_deg * 3.14159265358979323846 / 180.0; cm.ortho_height = ortho_h;
        if (autofocus_set) {                                                 // (X, Y) as in the saved image, whose row 0 is the film's last
            if (!renders[0]->autofocus(scene, focus_x, h - 1 - focus_y, cm.focus_distance)) return 1;
            std::cout << "autofocus: pixel (" << focus_x << ", " << focus_y << ") is " << cm.focus_distance << " away along the view direction" << std::endl;
        }
        for (auto r : renders) if (!r->set_camera_model(scene, cm)) return 1;
    }
    if (bake) {
        std::vector<mcpt_material> mats; std::vector<mcpt_texture> texs; mcpt_scene_desc d;
        model_to_desc(model, mats, texs, d);
        const size_t n_texel = size_t(bake_w) * size_t(bake_h);
        std::vector<mcpt_bake_point> points(n_texel); std::vector<uint32_t> texel(n_texel); uint32_t n = 0;
        if (mcpt_lightmap_points(&d, uint32_t(bake_w), uint32_t(bake_h), uint32_t(n_texel), points.data(), texel.data(), &n) != MCPT_OK) {
            std::cerr << "Error: mcpt_lightmap_points: " << mcpt_last_error() << std::endl; return 1;
        }
        points.resize(n); texel.resize(n);
        std::vector<unsigned char> rgb(3 * n_texel, 0);                      // texels no face covers stay black
        if (n) {
            Render& r0 = *renders[0];
            if (bake_direct && !r0.set_bake_direct(scene, MCPT_BAKE_DIRECT_MIS)) return 1;
            if (!r0.set_bake_points(scene, points) || !r0.bake(scene, uint32_t(bake_spp))) return 1;
            const std::vector<float> lit = r0.read_bake(scene, bake_irradiance ? MCPT_BAKE_IRRADIANCE : MCPT_BAKE_DIFFUSE);
            if (lit.size() != 4 * size_t(n)) return 1;
            for (uint32_t k = 0; k < n; k++)
                for (int c = 0; c < 3; c++) {                                // mcpt_tonemap's transfer (Scene::getPixelsColor) on the resolved value
                    float m = std::fmin(std::fmax(lit[4 * size_t(k) + c], 0.f), 1.f);
                    m = std::pow(m, 0.5f);
                    rgb[3 * size_t(texel[k]) + c] = (unsigned char)(m * 255.99f);
                }
        }
        FILE* f = std::fopen(bake_out.c_str(), "wb");
        if (!f) { std::cerr << "Error: cannot write " << bake_out << std::endl; return 1; }
        std::fprintf(f, "P6\n%d %d\n255\n", bake_w, bake_h); std::fwrite(rgb.data(), 1, rgb.size(), f); std::fclose(f);
        std::cout << "baked " << n << " of " << n_texel << " texels, " << bake_spp << " samples each: " << bake_out << std::endl;
        for (auto r : renders) delete r;
        return 0;
    }
    if (sh_grid) {
        // the grid spans the bounds of the vertices the faces use; one line per probe: position, 27 coefficients (channel-major, k = l (l + 1) + m), back-hit share
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (auto& fc : model.face)
            for (int c = 0; c < 3; c++) {
                const dvec3& v = model.vertex[size_t(fc[c][0])];
                const double x[3] = {v.x, v.y, v.z};
                for (int k = 0; k < 3; k++) { lo[k] = std::fmin(lo[k], x[k]); hi[k] = std::fmax(hi[k], x[k]); }
            }
        uint32_t n = uint32_t(sh_n[0]) * uint32_t(sh_n[1]) * uint32_t(sh_n[2]);
        std::vector<double> pos(3 * size_t(n));
        if (mcpt_sh_grid(lo, hi, uint32_t(sh_n[0]), uint32_t(sh_n[1]), uint32_t(sh_n[2]), n, pos.data(), &n) != MCPT_OK) {
            std::cerr << "Error: mcpt_sh_grid: " << mcpt_last_error() << std::endl; return 1;
        }
        Render& r0 = *renders[0];
        if (!r0.set_sh_probes(scene, pos) || !r0.bake_sh(scene, uint32_t(sh_passes))) return 1;
        const std::vector<float> coeffs = r0.read_sh(scene, sh_irradiance ? MCPT_SH_IRRADIANCE : MCPT_SH_RADIANCE), back = r0.read_sh_back_share(scene);
        if (coeffs.size() != 27 * size_t(n) || back.size() != n) return 1;
        FILE* f = std::fopen(sh_out.c_str(), "w");
        if (!f) { std::cerr << "Error: cannot write " << sh_out << std::endl; return 1; }
        for (uint32_t p = 0; p < n; p++) {
            std::fprintf(f, "%.17g %.17g %.17g", pos[3 * size_t(p)], pos[3 * size_t(p) + 1], pos[3 * size_t(p) + 2]);
            for (int q = 0; q < 27; q++) std::fprintf(f, " %.9g", coeffs[27 * size_t(p) + q]);
            std::fprintf(f, " %.6g\n", back[p]);
        }
        std::fclose(f);
        std::cout << "baked " << n << " probes, " << sh_passes << " passes of 64 rays each: " << sh_out << std::endl;
        for (auto r : renders) delete r;
        return 0;
    }
    // --turntable N: the camera moves, the scene stays -- Render::set_camera per frame, no rebuild, no upload
    if (turntable) {
        const CameraInfo base = model.camerainfo;
        const std::vector<dvec3> rest = model.vertex;                        // --wobble displaces from these
        const std::vector<Material> lit = model.materials;                   // --light-pulse scales these
        const double ul = std::sqrt(base.up.x * base.up.x + base.up.y * base.up.y + base.up.z * base.up.z);
        if (!(ul > 0.0)) { std::cerr << "Error: --turntable needs a camera with an up vector" << std::endl; return 1; }
        const double k[3] = {base.up.x / ul, base.up.y / ul, base.up.z / ul}, v[3] = {base.eye.x - base.lookat.x, base.eye.y - base.lookat.y, base.eye.z - base.lookat.z};
        // --spin MTLNAME: that material's faces are group 1, everything else group 0
        double pivot[3] = {0.0, 0.0, 0.0}, spin_pivot[3] = {0.0, 0.0, 0.0};
        if (!spin.empty()) {
            const int mtl = model.material_index(spin);
            if (mtl < 0) { std::cerr << "Error: --spin: no material named " << spin << std::endl; return 1; }
            std::vector<uint32_t> face_group(model.face.size(), 0u);
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            size_t n_spin = 0;
            for (size_t i = 0; i < model.face.size(); i++) {
                if (model.face[i][0][3] != mtl) continue;
                face_group[i] = 1u; n_spin++;
                for (int c = 0; c < 3; c++) {
                    const int vi = model.face[i][c][0];
                    if (vi < 0 || size_t(vi) >= model.vertex.size()) continue;   // (mcpt_create has refused such a face already)
                    const dvec3& p = model.vertex[size_t(vi)]; const double q[3] = {p.x, p.y, p.z};
                    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], q[a]); hi[a] = std::max(hi[a], q[a]); }
                }
            }
            if (!n_spin) { std::cerr << "Error: --spin: no face uses material " << spin << std::endl; return 1; }
            for (int a = 0; a < 3; a++) spin_pivot[a] = 0.5 * (lo[a] + hi[a]);
            if (!renders[0]->set_groups(scene, model, face_group)) return 1;
        }
        // --bend MTLNAME DEG: that material's faces follow bones 1 and 2 by height, everything else bone 0
        if (!bend.empty()) {
            const int mtl = model.material_index(bend);
            if (mtl < 0) { std::cerr << "Error: --bend: no material named " << bend << std::endl; return 1; }
            std::vector<uint8_t> part(model.vertex.size(), 0);
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            size_t n_bend = 0;
            for (size_t i = 0; i < model.face.size(); i++) {
                if (model.face[i][0][3] != mtl) continue;
                n_bend++;
                for (int c = 0; c < 3; c++) {
                    const int vi = model.face[i][c][0];
                    if (vi < 0 || size_t(vi) >= model.vertex.size()) continue;   // (mcpt_create has refused such a face already)
                    part[size_t(vi)] = 1;
                    const dvec3& p = model.vertex[size_t(vi)]; const double q[3] = {p.x, p.y, p.z};
                    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], q[a]); hi[a] = std::max(hi[a], q[a]); }
                }
            }
            if (!n_bend) { std::cerr << "Error: --bend: no face uses material " << bend << std::endl; return 1; }
            for (int a = 0; a < 3; a++) pivot[a] = 0.5 * (lo[a] + hi[a]);
            std::vector<uint32_t> bone(4 * model.vertex.size(), 0u); std::vector<double> weight(4 * model.vertex.size(), 0.0);
            for (size_t i = 0; i < model.vertex.size(); i++) {
                if (!part[i]) { weight[4 * i] = 1.0; continue; }             // bone 0
                const double t = hi[1] > lo[1] ? std::min(1.0, std::max(0.0, (model.vertex[i].y - lo[1]) / (hi[1] - lo[1]))) : 0.0;
                bone[4 * i] = 1u; weight[4 * i] = 1.0 - t; bone[4 * i + 1] = 2u; weight[4 * i + 1] = t;
            }
            if (!renders[0]->set_skin(scene, model, bone, weight, 3u)) return 1;
            // --dual-quat: before the first frame.  The bones below are rotations about z through the pivot: rigid, as the mode asks; were they not,
            // the library's refusal names the bone and the rule, and it is printed as it is -- the bones are never changed to fit
            if (dual_quat && !renders[0]->set_skin_mode(scene, MCPT_SKIN_DUAL_QUATERNION)) return 1;
        }
        // --swell MTLNAME AMOUNT: ONE morph target over that material's vertices, delta = vertex - centroid: a uniform scaling about a
        // point leaves every normal as it is, so there is no normal target
        if (!swell.empty()) {
            const int mtl = model.material_index(swell);
            if (mtl < 0) { std::cerr << "Error: --swell: no material named " << swell << std::endl; return 1; }
            std::vector<uint8_t> part(model.vertex.size(), 0);
            size_t n_swell = 0;
            for (size_t i = 0; i < model.face.size(); i++) {
                if (model.face[i][0][3] != mtl) continue;
                n_swell++;
                for (int c = 0; c < 3; c++) {
                    const int vi = model.face[i][c][0];
                    if (vi >= 0 && size_t(vi) < model.vertex.size()) part[size_t(vi)] = 1;   // (mcpt_create has refused any other face already)
                }
            }
            if (!n_swell) { std::cerr << "Error: --swell: no face uses material " << swell << std::endl; return 1; }
            double centre[3] = {0.0, 0.0, 0.0}; size_t n_part = 0;
            for (size_t i = 0; i < model.vertex.size(); i++) if (part[i]) { centre[0] += model.vertex[i].x; centre[1] += model.vertex[i].y; centre[2] += model.vertex[i].z; n_part++; }
            for (int a = 0; a < 3; a++) centre[a] /= double(n_part);
            std::vector<MorphTarget> target(1);
            for (size_t i = 0; i < model.vertex.size(); i++) {               // ascending, as the library asks
                if (!part[i]) continue;
                target[0].index.push_back(uint32_t(i));
                target[0].delta.push_back(model.vertex[i].x - centre[0]); target[0].delta.push_back(model.vertex[i].y - centre[1]); target[0].delta.push_back(model.vertex[i].z - centre[2]);
            }
            if (!renders[0]->set_morph(scene, model, target)) return 1;
        }
        // --sequence PATTERN COUNT: the frames go to the device once, one time unit apart; past the last one the last frame stays
        if (!sequence.empty() && !renders[0]->set_keyframes(scene, model, seq_vertex, seq_normal, 0.0, 1.0, smooth ? MCPT_KEYFRAMES_CATMULL_ROM : MCPT_KEYFRAMES_LINEAR,
                                                            MCPT_KEYFRAMES_CLAMP)) return 1;
        // --spin with --bend and / or --swell: every record gets the one route that writes it and every frame below is one parts
        // update.  Without --spin, or with --spin alone, the CLI makes exactly the calls it always made.
        const bool parts = !spin.empty() && (!bend.empty() || !swell.empty());
        const uint32_t deform_owner = swell.empty() ? MCPT_OWNER_SKIN : MCPT_OWNER_MORPH;        // --bend alone: the skin; otherwise the morph (with --bend: morph, then skin)
        if (parts) {
            const int spin_mtl = spin.empty() ? -1 : model.material_index(spin), bend_mtl = bend.empty() ? -1 : model.material_index(bend),
                      swell_mtl = swell.empty() ? -1 : model.material_index(swell);
            std::vector<uint8_t> face_owner(model.face.size(), uint8_t(MCPT_OWNER_NONE));
            for (size_t i = 0; i < model.face.size(); i++) {
                const int mtl = model.face[i][0][3];
                if (mtl >= 0 && mtl == spin_mtl) face_owner[i] = uint8_t(MCPT_OWNER_GROUPS);
                else if (mtl >= 0 && (mtl == bend_mtl || mtl == swell_mtl)) face_owner[i] = uint8_t(deform_owner);
            }
            // (faces of two owners that share a vertex or a normal: set_owners names the record and refuses)
            if (!renders[0]->set_owners(scene, model, face_owner)) return 1;
        }
        // --spin: Rodrigues as a matrix, R = cos a I + sin a [k]x + (1 - cos a) k k^T, about the pivot; group 0 stays
        auto spin_matrices = [&](double ca, double sa) {
            const double R[3][3] = {{ca + k[0] * k[0] * (1.0 - ca), k[0] * k[1] * (1.0 - ca) - k[2] * sa, k[0] * k[2] * (1.0 - ca) + k[1] * sa},
                                    {k[1] * k[0] * (1.0 - ca) + k[2] * sa, ca + k[1] * k[1] * (1.0 - ca), k[1] * k[2] * (1.0 - ca) - k[0] * sa},
                                    {k[2] * k[0] * (1.0 - ca) - k[1] * sa, k[2] * k[1] * (1.0 - ca) + k[0] * sa, ca + k[2] * k[2] * (1.0 - ca)}};
            std::vector<double> m(24, 0.0);
            m[0] = m[5] = m[10] = 1.0;
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) m[12 + 4 * r + c] = R[r][c];
                m[12 + 4 * r + 3] = spin_pivot[r] - (R[r][0] * spin_pivot[0] + R[r][1] * spin_pivot[1] + R[r][2] * spin_pivot[2]);
            }
            return m;
        };
        // --bend: bones 0 and 1 stay; bone 2 turns about z through the part's centre
        auto bend_matrices = [&](double sa) {
            const double b = bend_deg * 3.14159265358979323846 / 180.0 * sa, cb = std::cos(b), sb = std::sin(b);
            std::vector<double> m(36, 0.0);
            for (int g = 0; g < 3; g++) m[12 * g] = m[12 * g + 5] = m[12 * g + 10] = 1.0;
            double* u = m.data() + 24;
            u[0] = cb; u[1] = -sb; u[3] = pivot[0] - (cb * pivot[0] - sb * pivot[1]);
            u[4] = sb; u[5] = cb; u[7] = pivot[1] - (sb * pivot[0] + cb * pivot[1]);
            return m;
        };
        // --auto-normals: every update below is followed by the normals pass -- over all normals with --wobble and --sequence, which
        // move every vertex, otherwise over the normals of the faces of --bend's and --swell's materials
        if (auto_normals) {
            std::vector<uint8_t> face_mask;                                  // empty: all
            if (!wobble && sequence.empty()) {
                const int bend_mtl = bend.empty() ? -1 : model.material_index(bend), swell_mtl = swell.empty() ? -1 : model.material_index(swell);
                face_mask.assign(model.face.size(), 0);
                for (size_t i = 0; i < model.face.size(); i++) {
                    const int mtl = model.face[i][0][3];
                    face_mask[i] = mtl >= 0 && (mtl == bend_mtl || mtl == swell_mtl);
                }
            }
            if (!renders[0]->set_auto_normals(scene, model, face_mask)) return 1;
        }
        // --hide / --blink MTLNAME: the mask that hides that material's faces, and whether it is in force
        std::vector<uint8_t> hide_mask; bool hidden_now = false;
        if (!hide.empty() || !blink.empty()) {
            const std::string& name = hide.empty() ? blink : hide; const char* const opt = hide.empty() ? "--blink" : "--hide";
            const int mtl = model.material_index(name);
            if (mtl < 0) { std::cerr << "Error: " << opt << ": no material named " << name << std::endl; return 1; }
            hide_mask.assign(model.face.size(), 1);
            size_t n_hide = 0;
            for (size_t i = 0; i < model.face.size(); i++) if (model.face[i][0][3] == mtl) { hide_mask[i] = 0; n_hide++; }
            if (!n_hide) { std::cerr << "Error: " << opt << ": no face uses material " << name << std::endl; return 1; }
        }
        for (uint32_t f = 0; f < turntable; f++) {
            const double a = 2.0 * 3.14159265358979323846 * double(f) / double(turntable), ca = std::cos(a), sa = std::sin(a);
            const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2], kx[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
            CameraInfo cam = base;                                           // Rodrigues: v cos a + (k x v) sin a + k (k . v)(1 - cos a)
            cam.eye.x = base.lookat.x + v[0] * ca + kx[0] * sa + k[0] * kv * (1.0 - ca);
            cam.eye.y = base.lookat.y + v[1] * ca + kx[1] * sa + k[1] * kv * (1.0 - ca);
            cam.eye.z = base.lookat.z + v[2] * ca + kx[2] * sa + k[2] * kv * (1.0 - ca);
            auto t0 = std::chrono::steady_clock::now();
            if (pulse) {                                                     // --light-pulse A: the lamps breathe; the camera call below restarts the film
                const double g = 1.0 + pulse_a * std::sin(2.0 * 3.14159265358979323846 * double(f) / double(turntable));
                for (size_t i = 0; i < lit.size(); i++) {
                    model.materials[i].radiance.x = lit[i].radiance.x * g; model.materials[i].radiance.y = lit[i].radiance.y * g;
                    model.materials[i].radiance.z = lit[i].radiance.z * g;
                }
                if (!renders[0]->update_materials(scene, model)) return 1;
            }
            // --reproject H: frames after the first keep what the previous frame saw of the same surfaces
            if (wobble && f > 0) {                                           // --wobble A: the vertices move too, and with --reproject the film follows them (§14)
                const double s = wobble_a * std::sin(2.0 * 3.14159265358979323846 * double(f) / double(turntable));
                for (size_t i = 0; i < rest.size(); i++) {
                    const dvec3& p = rest[i];
                    model.vertex[i] = dvec3{p.x + s * std::sin(9.0 * p.y), p.y + s * std::sin(7.0 * p.z), p.z + s * std::sin(8.0 * p.x)};
                }
                model.camerainfo = cam;
                if (reproject ? !renders[0]->update_reproject(scene, model, cam, history) : !renders[0]->update(scene, model)) return 1;
            } else if (parts) {                                              // one call per frame: each route's payload is what its own branch below sends
                PartsUpdate u;
                u.routes |= MCPT_ROUTE_GROUPS; u.group_matrices = spin_matrices(ca, sa);
                if (!bend.empty()) u.bone_matrices = bend_matrices(sa);
                if (!swell.empty()) { u.routes |= MCPT_ROUTE_MORPH; u.morph_weights = {swell_a * sa}; if (!bend.empty()) u.flags |= MCPT_PARTS_MORPH_THEN_SKIN; }
                else if (!bend.empty()) u.routes |= MCPT_ROUTE_SKIN;
                Render& r0 = *renders[0];
                if (reproject && f > 0 ? !r0.update_parts_reproject(scene, u, cam, history) : !(r0.update_parts(scene, u) && r0.set_camera(scene, cam))) return 1;
            } else if (!sequence.empty()) {                                  // --sequence: turntable frame j plays time j / S; only that number crosses the bus
                const double time = double(f) / slowdown;
                Render& r0 = *renders[0];
                if (reproject && f > 0 ? !r0.update_keyframes_reproject(scene, time, cam, history) : !(r0.update_keyframes(scene, time) && r0.set_camera(scene, cam))) return 1;
            } else if (!spin.empty()) {
                const std::vector<double> m = spin_matrices(ca, sa);
                if (reproject && f > 0 ? !renders[0]->update_transforms_reproject(scene, m, cam, history)
                                       : !(renders[0]->update_transforms(scene, m) && renders[0]->set_camera(scene, cam))) return 1;
            } else if (!bend.empty() || !swell.empty()) {
                const std::vector<double> m = bend_matrices(sa);
                const std::vector<double> weights{swell_a * sa};             // --swell: the one target's weight (with --bend: morph, then skin, in one call)
                Render& r0 = *renders[0];
                if (!swell.empty() && !bend.empty()) {
                    if (reproject && f > 0 ? !r0.update_morph_reproject(scene, weights, m, cam, history) : !(r0.update_morph(scene, weights, m) && r0.set_camera(scene, cam))) return 1;
                } else if (!swell.empty()) {
                    if (reproject && f > 0 ? !r0.update_morph_reproject(scene, weights, cam, history) : !(r0.update_morph(scene, weights) && r0.set_camera(scene, cam))) return 1;
                } else
                if (reproject && f > 0 ? !renders[0]->update_skin_reproject(scene, m, cam, history)
                                       : !(renders[0]->update_skin(scene, m) && renders[0]->set_camera(scene, cam))) return 1;
            } else if (!hide_mask.empty() && (!hide.empty() || (f / uint32_t(blink_k)) % 2 == 1) != hidden_now) {   // --hide / --blink: the mask changes in this frame
                hidden_now = !hidden_now;
                const std::vector<uint8_t> mask = hidden_now ? hide_mask : std::vector<uint8_t>();   // (empty: every face visible again)
                Render& r0 = *renders[0];
                if (reproject && f > 0 ? !r0.set_visible_reproject(scene, mask, cam, history) : !(r0.set_visible(scene, mask) && r0.set_camera(scene, cam))) return 1;
            } else
            if (reproject && f > 0 ? !renders[0]->set_camera_reproject(scene, cam, history) : !renders[0]->set_camera(scene, cam)) return 1;
            if (rebuild) {                                                   // --rebuild-above R: the refitted trees have grown past R times their built size
                mcpt_update_info ui; mcpt_rebuild_info ri;
                if (mcpt_get_update_info(renders[0]->handle(), &ui) != MCPT_OK) { std::cerr << "Error: mcpt_get_update_info: " << mcpt_last_error() << std::endl; return 1; }
                if (ui.wide_area_ratio > rebuild_above) {
                    if (!renders[0]->rebuild(scene) || mcpt_get_rebuild_info(renders[0]->handle(), &ri) != MCPT_OK) return 1;
                    std::cout << "rebuild: frame " << f << "    wide_area_ratio before: " << ri.area_ratio_before << "    cost: " << ri.last_ms << " ms\n";
                }
            }
            if (camera_model ? !renders[0]->render_camera(scene, spp) : (renders[0]->render(scene, spp), false)) return 1;
            scene.sync();
            std::cout << "frame: " << f << "    frame cost: " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "s\n";
            scene.save_image(int(f), out + "_turn");
        }
        for (auto r : renders) delete r;
        return 0;
    }
    std::vector<ncclComm_t> comms(gpus);
    if (gpus > 1) {
        std::vector<int> devs(gpus); for (uint32_t g = 0; g < gpus; g++) devs[g] = int(g);
        if (ncclCommInitAll(comms.data(), int(gpus), devs.data()) != ncclSuccess) { std::cerr << "Error: ncclCommInitAll" << std::endl; return 1; }
    }
    uint32_t frame = 0, batches_done = 0; uint64_t rays = 0; double total_s = 0;
    void* progress_film = nullptr;                    // device 0: the sum of all devices' films, for --save-every with several devices
    std::vector<float> film(size_t(w) * h * 4);
    std::atomic<int> failed{0};                       // any device error or failed collective: no image, non-zero exit
    auto fail_with = [&](const std::string& what) { std::cerr << "Error: " << what << std::endl; failed.store(1); };
    // --denoise: the a-trous preview filter of device 0's film -- or of the films summed on device 0 -- guided by first-hit
    // features rendered once, from 4 camera samples of the run's seed
    if (denoise && mcpt_render_features(renders[0]->handle(), 4, seed) != MCPT_OK) { std::cerr << "Error: mcpt_render_features: " << mcpt_last_error() << std::endl; return 1; }
    auto save_denoised = [&](const void* device_film, uint32_t at) {
        std::vector<uint8_t> rgb(size_t(w) * h * 3);
        void* den = nullptr;
        mcpt_ctx* c = renders[0]->handle();
        mcpt_denoise_opts dopts; std::memset(&dopts, 0, sizeof dopts); dopts.struct_size = sizeof dopts;
        if (denoise_robust) dopts.flags = MCPT_DENOISE_SPLIT_EMISSION | MCPT_DENOISE_CLAMP_FIREFLIES;
        if (mcpt_denoise(c, device_film, &dopts) != MCPT_OK || mcpt_denoised_device_ptr(c, &den) != MCPT_OK || mcpt_tonemap_buffer(c, den, rgb.data(), 1) != MCPT_OK)
            return fail_with(std::string("denoised image: ") + mcpt_last_error());
        const std::string file = out + std::to_string(at) + "_denoised.png";
        if (write_png_rgb8(file, w, h, rgb.data())) std::cout << "Image saved successfully: " << file << std::endl;
        else std::cerr << "Failed to save image: " << file << std::endl;
    };
    // --adaptive T: one mcpt_render_adaptive call instead of the batch loop -- --spp samples per pixel at most, --min-spp in pass 0
    if (adaptive >= 0.f) {
        mcpt_ctx* c = renders[0]->handle();
        mcpt_adaptive_opts ao; std::memset(&ao, 0, sizeof ao); ao.struct_size = sizeof ao; ao.min_spp = min_spp; ao.max_spp = spp; ao.threshold = adaptive;
        mcpt_adaptive_stats st;
        auto t0 = std::chrono::steady_clock::now();
        if (mcpt_render_adaptive(c, seed, 0, &ao, &st) != MCPT_OK || mcpt_sync(c) != MCPT_OK) { std::cerr << "Error: mcpt_render_adaptive: " << mcpt_last_error() << std::endl; return 1; }
        total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("adaptive: %u passes, %.1f samples per pixel, %u tiles converged, %u capped: %.3f s\n", st.passes,
                    double(st.pixel_samples) / (double(w) * h), st.tiles_converged, st.tiles_capped, total_s);
        if (denoise) save_denoised(nullptr, spp);
        if (failed.load() || mcpt_read_accum(c, film.data()) != MCPT_OK) { std::cerr << "Error: " << mcpt_last_error() << std::endl; return 1; }
        // the sample-count map: log2(count) / log2(spp) as grey, top row first like the saved image
        std::vector<uint8_t> grey(size_t(w) * h * 3);
        const double top = std::log2(std::max(2.0, double(spp)));
        for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
            const float n = film[4 * (size_t(h - 1 - y) * w + x) + 3];
            const double g = n > 0.f ? std::min(1.0, std::max(0.0, std::log2(double(n)) / top)) : 0.0;
            for (int k = 0; k < 3; k++) grey[3 * (size_t(y) * w + x) + k] = uint8_t(g * 255.0 + 0.5);
        }
        const std::string map = out + "_spp.png";
        if (write_png_rgb8(map, w, h, grey.data())) std::cout << "Image saved successfully: " << map << std::endl;
        else std::cerr << "Failed to save image: " << map << std::endl;
        scene.add_film(film.data());
        mcpt_counters cn;
        if (mcpt_get_counters(c, &cn) != MCPT_OK) { std::cerr << "Error: " << mcpt_last_error() << std::endl; return 1; }
        rays = cn.rays_primary + cn.rays_continuation + cn.rays_shadow;
        std::printf("%u spp max, %dx%d, 1 GPU(s): %.3f s, %.1f Mray/s\n", spp, w, h, total_s, rays / total_s / 1e6);
        scene.save_image(int(spp), out);
        for (auto r : renders) delete r;
        return 0;
    }
    // The films stay on the devices from batch to batch (the reference's loop reads its film every frame only to display it): per batch
    // one mcpt_render per device, at the end the path's one exchange step and one read-back.
    while (frame < spp && !failed.load()) {
        const uint32_t n = std::min(batch, spp - frame);
        auto t0 = std::chrono::steady_clock::now();
        // sample range [frame, frame+n) split contiguously over the devices; one host thread per device (mcpt_render blocks
        // until its device's work is enqueued and nearly finished)
        auto work = [&](uint32_t g) {
            const uint32_t lo = frame + uint32_t(uint64_t(n) * g / gpus), hi = frame + uint32_t(uint64_t(n) * (g + 1) / gpus);
            mcpt_ctx* c = renders[g]->handle();
            // --shard tiles: device g renders ALL n samples of its interleaved share of the 8x8 tiles (BASELINE.json's "pixel-tile shard");
            // default: its contiguous share of the sample range for every pixel.  Either way the films add up to the frame.
            const mcpt_status rs = shard_tiles ? mcpt_render_tiles(c, n, seed, frame, gpus, g) : (hi > lo ? (camera_model ? mcpt_render_camera : mcpt_render)(c, hi - lo, seed, lo) : MCPT_OK);
            if (rs != MCPT_OK) return fail_with(std::string("mcpt_render: ") + mcpt_last_error());
            if (mcpt_sync(c) != MCPT_OK) return fail_with(std::string("mcpt_sync: ") + mcpt_last_error());
        };
        if (gpus == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (uint32_t g = 0; g < gpus; g++) th.emplace_back(work, g);
            for (auto& t : th) t.join();
        }
        if (failed.load()) break;
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        total_s += s; frame += n;
        std::cout << "frame: " << frame << "    frame cost: " << s << "s\n";                       // main.cpp:31
        // --save-every K: a progressive image every K batches, like the reference's window shows every frame (main.cpp:33-36) -- tonemapped
        // on the device (Scene::getPixelsColor as a kernel: mean, clamp, sqrt, x255.99), 3 bytes per pixel read back
        batches_done++;
        if (save_every && batches_done % save_every == 0 && frame < spp) {
            std::vector<uint8_t> rgb(size_t(w) * h * 3);
            bool ok_img;
            if (gpus == 1) ok_img = mcpt_tonemap(renders[0]->handle(), rgb.data(), 1) == MCPT_OK;
            else {
                // the whole film so far, like the reference's window (main.cpp:26-36): the devices' films are summed into a scratch film on
                // device 0 (ncclReduce; the films themselves keep accumulating untouched) and that one is tonemapped
                bool ok = hipSetDevice(0) == hipSuccess && (progress_film || hipMalloc(&progress_film, size_t(w) * h * 16) == hipSuccess);
                ok = ok && ncclGroupStart() == ncclSuccess;
                for (uint32_t g = 0; g < gpus && ok; g++) {
                    void* p = nullptr;
                    ok = mcpt_accum_device_ptr(renders[g]->handle(), &p) == MCPT_OK && hipSetDevice(int(g)) == hipSuccess &&
                         ncclReduce(p, progress_film, size_t(w) * h * 4, ncclFloat, ncclSum, 0, comms[g], nullptr) == ncclSuccess;
                }
                ok = (ncclGroupEnd() == ncclSuccess) && ok;
                for (uint32_t g = 0; g < gpus && ok; g++) ok = hipSetDevice(int(g)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
                ok_img = ok && mcpt_tonemap_buffer(renders[0]->handle(), progress_film, rgb.data(), 1) == MCPT_OK;
            }
            if (!ok_img) { fail_with(std::string("progressive image: ") + mcpt_last_error()); break; }
            const std::string file = out + std::to_string(frame) + ".png";
            if (write_png_rgb8(file, w, h, rgb.data())) std::cout << "Image saved successfully: " << file << std::endl;
            else std::cerr << "Failed to save image: " << file << std::endl;
            if (denoise) { save_denoised(gpus == 1 ? nullptr : progress_film, frame); if (failed.load()) break; }
        }
    }
    if (!failed.load()) {
        auto t0 = std::chrono::steady_clock::now();
        if (gpus > 1) {                               // sum of the per-device films over xGMI
            bool ok = ncclGroupStart() == ncclSuccess;
            for (uint32_t g = 0; g < gpus && ok; g++) {
                void* p = nullptr;
                ok = mcpt_accum_device_ptr(renders[g]->handle(), &p) == MCPT_OK && hipSetDevice(int(g)) == hipSuccess &&
                     ncclAllReduce(p, p, size_t(w) * h * 4, ncclFloat, ncclSum, comms[g], nullptr) == ncclSuccess;
            }
            ok = (ncclGroupEnd() == ncclSuccess) && ok;
            for (uint32_t g = 0; g < gpus && ok; g++) ok = hipSetDevice(int(g)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
            if (!ok) fail_with("RCCL all-reduce of the films failed");
        }
        if (!failed.load() && denoise) {            // device 0's film is the whole image now (all-reduced in place with several devices)
            void* p = nullptr;
            if (mcpt_accum_device_ptr(renders[0]->handle(), &p) != MCPT_OK) fail_with(std::string("mcpt_accum_device_ptr: ") + mcpt_last_error());
            else save_denoised(gpus == 1 ? nullptr : p, frame);
        }
        if (!failed.load()) {
            if (mcpt_read_accum(renders[0]->handle(), film.data()) != MCPT_OK) fail_with(std::string("mcpt_read_accum: ") + mcpt_last_error());
            else scene.add_film(film.data());
        }
        total_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    if (progress_film) { (void)hipSetDevice(0); (void)hipFree(progress_film); }
    if (gpus > 1) for (auto& c : comms) (void)ncclCommDestroy(c);
    if (failed.load()) { for (auto r : renders) delete r; return 1; }
    for (uint32_t g = 0; g < gpus; g++) {
        mcpt_counters c;
        if (mcpt_get_counters(renders[g]->handle(), &c) != MCPT_OK) { std::cerr << "Error: " << mcpt_last_error() << std::endl; return 1; }
        rays += c.rays_primary + c.rays_continuation + c.rays_shadow;
    }
    std::printf("%u spp, %dx%d, %u GPU(s): %.3f s, %.1f Mray/s\n", spp, w, h, gpus, total_s, rays / total_s / 1e6);
    scene.save_image(int(frame), out);                                                              // main.cpp:37
    for (auto r : renders) delete r;
    return 0;
}
