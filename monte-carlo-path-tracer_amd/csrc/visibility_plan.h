// What a visibility mask means for a scene, on the host: how many faces it hides, how many of those are emitters, how many visible
// faces every material keeps and how long the light list is.  Pure: no device, no context -- mcpt_set_face_visibility and mcpt_update_materials both
// validate through it, and tests/visibility_plan_check.cpp holds it to tests/visibility_ref.py.
#pragma once
#include <cstdint>
#include <vector>

struct VsPlan {
    uint32_t n_hidden = 0;                 // faces whose byte is 0
    uint32_t n_hidden_emitters = 0;        // ... of a material that emits
    uint32_t n_lights = 0;                 // visible faces of a material that emits: the light list's length
    std::vector<uint32_t> visible_faces;   // per material: its faces that stay visible
};

// visible: one byte per face, != 0 = visible; null = every face visible.  face_material: per face its material, < n_materials (a face that names a
// material out of range counts as hidden or visible, but for no material and never as an emitter).  material_emits: per material != 0 = its faces
// pass the light list's test.
inline VsPlan vs_plan(const uint8_t* visible, const uint32_t* face_material, uint32_t n_face, const uint8_t* material_emits, uint32_t n_materials) {
    VsPlan p;
    p.visible_faces.assign(n_materials, 0u);
    for (uint32_t f = 0; f < n_face; f++) {
        const uint32_t m = face_material[f];
        const bool known = m < n_materials, emits = known && material_emits[m] != 0;
        if (visible && !visible[f]) { p.n_hidden++; if (emits) p.n_hidden_emitters++; continue; }
        if (known) p.visible_faces[m]++;
        if (emits) p.n_lights++;
    }
    return p;
}
