// re_world_lights.h -- what re_lighting_set_lights_from_world (re_lighting.hip) needs of a world context (re_api.hip): the light list in ascending
// EntityId, the columns the nearby test and the record gather read, and the LightInformation column.  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
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
    LightQuery Q{};                        // type_flag unused: the kernel tests all three types
    bool complete[3] = {};                 // [RE_WL_*]: every live light of the type carries what the type unwraps (no device check needed)
};

// checks (device of the lighting context, a world, no shard range), settles the context (resolve) and brings the light list and the LightInformation
// column up to date on the device.  On failure the code is returned and the message is in *err.
int world_lights_view(re_ctx *c, int device, const re_camera *cam, const uint32_t need[3], WorldLightsView *v, std::string *err);

}  // namespace re
