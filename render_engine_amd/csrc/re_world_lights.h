// re_world_lights.h -- what re_lighting_set_lights_from_world (re_lighting.hip) needs of a world context (re_api.hip): the light list in ascending
// EntityId, the columns the nearby test and the record gather read, and the LightInformation column.  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "re_hip.h"
#include "re_kernels.h"

namespace re {

constexpr uint32_t LI_HAS = 0x80000000u;   // (device column only) the light carries LightInformation; the RE_LI_* bits below it as given

struct WorldLightsView {
    hipStream_t stream = nullptr;          // the context's stream: the selection kernels run on it, behind the work already enqueued there
    uint32_t nl = 0;                       // entries of the light list (rows with a RE_F_LIGHT_* bit, removed ones included), ascending EntityId
    const uint32_t *light_rows = nullptr, *flags = nullptr, *row_id = nullptr, *row_cell = nullptr;
    const uint64_t *cell_key = nullptr; const uint8_t *cell_flags = nullptr; const int32_t *sh_cells = nullptr;
    const float *pos = nullptr;            // live Position column (3 floats per row)
    const re_light_information *info = nullptr;   // per light-list entry; present == 0: no component
    const re_light_information *h_info = nullptr; // the same column on the host (nl entries)
    uint64_t li_epoch = 0;                         // changes whenever the column (or the light list it follows) is rebuilt
    LightQuery Q{};                        // type_flag unused: the kernel tests all three types
    bool complete[3] = {};                 // [RE_WL_*]: every live light of the type carries what the type unwraps (no device check needed)
};

// checks (device of the lighting context, a world, no shard range), settles the context (resolve) and brings the light list and the LightInformation
// column up to date on the device.  On failure the code is returned and the message is in *err (prefixed with `who`).
int world_lights_view(re_ctx *c, int device, const re_camera *cam, const uint32_t need[3], WorldLightsView *v, std::string *err,
                      const char *who = "re_lighting_set_lights_from_world");

// what the shadow flow (re_shadow.hip) needs of a world context besides the light view: the directional candidates -- live entities whose sortable
// index is 1 (ecs.get_entities_with_sortable()[1], flows/shadow_flow.rs:156), ascending EntityId, with their rows and LightInformation (present == 0:
// none) --, whether a row of the light list was removed, and the tree's outline length.  Host mirrors only; call after world_lights_view (settled).
// The caller keeps the object between calls: it is recomputed only when rows or the LightInformation column changed since (changed = false otherwise).
struct ShadowWorld {
    std::vector<uint32_t> dir_id, dir_row; std::vector<re_light_information> dir_info;
    bool dead_light = false; uint32_t outline_length = 0;
    bool valid = false, changed = true; uint64_t rows_epoch = 0, li_epoch = 0; uint32_t n_groups = 0;
};
int shadow_world(re_ctx *c, ShadowWorld *w, std::string *err);
int world_device(const re_ctx *c);
hipStream_t world_stream(const re_ctx *c);

// the previous sets of a lighting context (re_lighting.hip): device arrays in ascending EntityId and the device word holding each count, NULL when the
// context never ran re_lighting_set_lights_from_world (empty sets)
struct LightingPrev { int device = 0; const uint32_t *prev[3] = {}; const uint32_t *n_prev = nullptr; };
void lighting_prev(const re_lighting *l, LightingPrev *p);

}  // namespace re
