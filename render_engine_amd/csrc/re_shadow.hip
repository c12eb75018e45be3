// re_shadow.hip -- ShadowFlow::calculate_shadow_maps (flows/shadow_flow.rs:111-453) on the device: the round-robin state machine that decides, once per
// frame, whether a light gets a new shadow map, which texture index it takes and from which light camera the map is seen.  The state (servicing type and
// light, the free-index queue, the point / spot maps, the upload lists) lives in device memory; one single-workgroup launch per frame on the world
// context's stream steps it.  Inputs the reference reads: the nearby lights of the type (find_nearby_lights: re_visible_lights' test), the lighting
// context's previous sets (RenderFlow's visible_*_lights, written by upload_*_lights of the frame before), the live positions and LightInformation.
// Hash-order stand-ins as everywhere in the library: sets and maps in ascending EntityId.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "re_hip.h"
#include "re_guard.h"
#include "re_world_lights.h"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t SH_MAX_MAPS = 32;
constexpr int SH_THREADS = 256;

// the state machine between frames (ServicingLightType + free_indexes + the map sizes + the upload count)
struct ShadowState {
    uint32_t type, cur;                 // RE_WL_*; cur = the Option<EntityId> (NONE = None)
    uint32_t free_head, free_n;         // VecDeque<usize> as a ring over n_maps entries
    uint32_t free_q[SH_MAX_MAPS];
    uint32_t n_map[3];                  // [RE_WL_POINT], [RE_WL_SPOT]: entries of point_lights / spotlights (directional_lights is never filled)
    uint32_t n_up;                      // entries ever pushed to upload_matrices / upload_view_matrices / upload_indexes
};

// what the kernel leaves for the host: the frame (re_shadow_frame) and the verdict of the checks
struct ShadowOut {
    re_shadow_frame f;
    uint32_t bad_id, bad_kind;          // NONE: the step went through; else the entity whose unwrap the reference would panic on (state left unchanged)
};

struct ShadowArgs {
    // the world (re_world_lights.h)
    uint32_t nl; const uint32_t *rows, *flags, *row_id, *row_cell; const uint64_t *cell_key; const uint8_t *cell_flags; const int32_t *sh_cells;
    const float *pos; const re_light_information *info; const float *m11;   // m11: 1 / tan(radians(fov) / 2) per light-list entry (host libm, as ro_perspective)
    // directional candidates: live entities with sortable index 1, ascending EntityId (ecs.get_entities_with_sortable()[1], shadow_flow.rs:156)
    uint32_t n_dir; const uint32_t *dir_id, *dir_row; const re_light_information *dir_info;
    // the lighting context's previous sets (NULL: empty)
    const uint32_t *prev[3]; const uint32_t *n_prev;
    // state and scratch
    ShadowState *state; uint32_t *map_id[3], *map_idx[3], *work_id[3], *work_idx[3], map_cap, n_maps;
    uint32_t *near_ids; float *up_mat, *up_view; uint32_t *up_idx, up_cap;
    ShadowOut *out;
    // the frame
    float cam_pv[16]; float aspect, outline, spot_m11;
};

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1u; else hi = m; }
    return lo;
}
__device__ __forceinline__ bool in_sorted_u32(const uint32_t *a, uint32_t n, uint32_t v) { const uint32_t p = lower_bound_u32(a, n, v); return p < n && a[p] == v; }

// nalgebra matrix product, the summation order of ro_mat4_mul
__device__ void mat4_mul(const float *a, const float *b, float *out) {
    for (int j = 0; j < 4; j++)
        for (int i = 0; i < 4; i++) {
            float y = a[0 * 4 + i] * b[j * 4 + 0];
            y = a[1 * 4 + i] * b[j * 4 + 1] + y;
            y = a[2 * 4 + i] * b[j * 4 + 2] + y;
            y = a[3 * 4 + i] * b[j * 4 + 3] + y;
            out[j * 4 + i] = y;
        }
}
// ro_perspective with m11 = 1 / tanf(fovy / 2) supplied
__device__ void perspective(float aspect, float m11, float znear, float zfar, float *out) {
    for (int i = 0; i < 16; i++) out[i] = 0.0f;
    out[5] = m11; out[0] = m11 / aspect;
    out[10] = (zfar + znear) / (znear - zfar);
    out[14] = zfar * znear * 2.0f / (znear - zfar);
    out[11] = -1.0f;
}
// nalgebra_glm::ortho (right-handed, depth -1..1): with left == right and top == bottom (shadow_flow.rs:183-186) the x / y terms divide by zero
__device__ void ortho(float l, float r, float b, float t, float n, float f, float *out) {
    for (int i = 0; i < 16; i++) out[i] = 0.0f;
    out[0] = 2.0f / (r - l); out[5] = 2.0f / (t - b); out[10] = -2.0f / (f - n);
    out[12] = -(r + l) / (r - l); out[13] = -(t + b) / (t - b); out[14] = -(f + n) / (f - n); out[15] = 1.0f;
}
// ro_look_at
__device__ void look_at(const float *eye, const float *target, const float *up, float *out) {
    float f[3] = { target[0] - eye[0], target[1] - eye[1], target[2] - eye[2] };
    const float fl = sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]); f[0] /= fl; f[1] /= fl; f[2] /= fl;
    float s[3] = { f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0] };
    const float sl = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]); s[0] /= sl; s[1] /= sl; s[2] /= sl;
    const float u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
    for (int i = 0; i < 16; i++) out[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    out[0] = s[0]; out[4] = s[1]; out[8] = s[2];
    out[1] = u[0]; out[5] = u[1]; out[9] = u[2];
    out[2] = -f[0]; out[6] = -f[1]; out[10] = -f[2];
    out[12] = -((s[0] * eye[0] + s[1] * eye[1]) + s[2] * eye[2]);
    out[13] = -((u[0] * eye[0] + u[1] * eye[1]) + u[2] * eye[2]);
    out[14] = ((f[0] * eye[0] + f[1] * eye[1]) + f[2] * eye[2]);
}
// ro_make_planes (render_frustum_culler.rs:59-78)
__device__ void make_planes(const float *pv, float *planes) {
    float p[6][4];
    for (int i = 0; i < 4; i++) {
        const float r0 = pv[i * 4 + 0], r1 = pv[i * 4 + 1], r2 = pv[i * 4 + 2], r3 = pv[i * 4 + 3];
        p[0][i] = r3 + r0; p[1][i] = r3 - r0; p[2][i] = r3 + r1; p[3][i] = r3 - r1; p[4][i] = r3 - 0.0f; p[5][i] = r3 - r2;
    }
    for (int k = 0; k < 6; k++) {
        const float len = sqrtf((p[k][0] * p[k][0] + p[k][1] * p[k][1]) + p[k][2] * p[k][2]);
        for (int i = 0; i < 4; i++) planes[k * 4 + i] = p[k][i] / len;
    }
}

// the light-list entry of a live light with this id (the list is in ascending EntityId; a removed row may share the id of the row that reused it)
__device__ uint32_t light_entry(const ShadowArgs &A, uint32_t id) {
    uint32_t lo = 0, hi = A.nl;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (A.row_id[A.rows[m]] < id) lo = m + 1u; else hi = m; }
    for (; lo < A.nl && A.row_id[A.rows[lo]] == id; lo++) if (!(A.flags[A.rows[lo]] & re::F_DEAD)) return lo;
    return NONE;
}

// find_next_light_to_have_shadow_map (shadow_flow.rs:364-452) on the working copy of the type's map; thread 0 only.  near: ascending ids.
__device__ uint32_t find_next(const ShadowArgs &A, ShadowState &S, int t, const uint32_t *near, uint32_t n_near) {
    if (S.free_n == 0) return NONE;
    uint32_t *mid = A.work_id[t], *midx = A.work_idx[t];
    // lights no longer nearby give their indexes back, in map order (ascending id) and slot order
    uint32_t w = 0;
    for (uint32_t e = 0; e < S.n_map[t]; e++) {
        if (in_sorted_u32(near, n_near, mid[e])) {
            if (w != e) { mid[w] = mid[e]; for (int k = 0; k < 6; k++) midx[w * 6 + k] = midx[e * 6 + k]; }
            w++;
        } else {
            for (int k = 0; k < 6; k++) { const uint32_t x = midx[e * 6 + k]; if (x != NONE) { S.free_q[(S.free_head + S.free_n) % A.n_maps] = x; S.free_n++; } }
        }
    }
    S.n_map[t] = w;
    const uint32_t np = A.prev[t] ? A.n_prev[t] : 0u;
    // priority: the LAST visible light without a map
    for (uint32_t i = np; i-- > 0;) { const uint32_t v = A.prev[t][i]; if (!in_sorted_u32(mid, w, v)) return v; }
    // else the first nearby light that is not visible
    for (uint32_t i = 0; i < n_near; i++) if (!np || !in_sorted_u32(A.prev[t], np, near[i])) return near[i];
    return NONE;
}

__device__ uint32_t pop_free(const ShadowArgs &A, ShadowState &S) {
    const uint32_t x = S.free_q[S.free_head]; S.free_head = (S.free_head + 1u) % A.n_maps; S.free_n--; return x;
}

// frustum_aabb box (visible_world_flow.rs:117-129): centre = front * draw / 2 + pos
__device__ void frustum_box(const float *pos, const float *dir, float far, float *box) {
    const float h = far / 2.0f;
    for (int a = 0; a < 3; a++) { const float c = dir[a] * h + pos[a]; box[2 * a] = fmaxf(c - h, 0.0f); box[2 * a + 1] = c + h; }
}

__global__ __launch_bounds__(SH_THREADS) void k_shadow_select(ShadowArgs A, re::LightQuery Qarg) {
    __shared__ re::LightQuery Q;
    __shared__ ShadowState S;
    __shared__ uint32_t s_cnt[SH_THREADS + 1], s_bad;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { Q = Qarg; S = *A.state; s_bad = NONE; }
    __syncthreads();
    // working copies of the maps: the state is written back only when the step goes through
    for (int t = 1; t < 3; t++)
        for (uint32_t e = tid; e < S.n_map[t]; e += SH_THREADS) { A.work_id[t][e] = A.map_id[t][e]; for (int k = 0; k < 6; k++) A.work_idx[t][e * 6 + k] = A.map_idx[t][e * 6 + k]; }
    // nearby lights of the type whose find runs this frame (Point(None) / Spot(None) with a free index), ascending: chunked order-preserving compaction
    const int ft = (S.cur == NONE && S.free_n > 0 && S.type != RE_WL_DIRECTIONAL) ? (int)S.type : -1;
    uint32_t n_near = 0;
    if (ft >= 0) {
        const uint32_t tbit = ft == RE_WL_POINT ? re::F_LIGHT_POINT : re::F_LIGHT_SPOT;
        const uint32_t chunk = (A.nl + SH_THREADS - 1) / SH_THREADS, b0 = min(A.nl, tid * chunk), b1 = min(A.nl, b0 + chunk);
        auto is_near = [&](uint32_t i) {
            const uint32_t r = A.rows[i], fl = A.flags[r], rc = A.row_cell[r];
            if ((fl & re::F_DEAD) || !(fl & tbit) || rc == re::ROW_CELL_NONE) return false;
            if (!(rc & re::ROW_CELL_SHARED)) return !(A.cell_flags[rc] & re::CF_PAD) && re::light_section_visible(A.cell_key[rc], Q);
            const uint32_t sh = rc & ~re::ROW_CELL_SHARED;
            for (int k = 0; k < 8; k++) { const int32_t c = A.sh_cells[sh * 8 + k]; if (c >= 0 && !(A.cell_flags[c] & re::CF_PAD) && re::light_section_visible(A.cell_key[c], Q)) return true; }
            return false;
        };
        uint32_t cnt = 0;
        for (uint32_t i = b0; i < b1; i++) cnt += is_near(i) ? 1u : 0u;
        s_cnt[tid] = cnt;
        __syncthreads();
        if (tid == 0) { uint32_t acc = 0; for (int k = 0; k < SH_THREADS; k++) { const uint32_t v = s_cnt[k]; s_cnt[k] = acc; acc += v; } s_cnt[SH_THREADS] = acc; }
        __syncthreads();
        uint32_t o = s_cnt[tid];
        for (uint32_t i = b0; i < b1; i++) if (is_near(i)) A.near_ids[o++] = A.row_id[A.rows[i]];
        n_near = s_cnt[SH_THREADS];
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        re_shadow_frame F;
        memset(&F, 0, sizeof F);
        F.entity_id = NONE; F.face = NONE; F.texture_index = NONE;
        F.light_type = S.type;
        uint32_t bad = NONE, bad_kind = 0;
        float pos[3] = { 0, 0, 0 }, dir[3] = { 0, 0, 0 }, far = 0.0f, view[16], proj[16], lpv[16];
        const float *culler = A.cam_pv;
        auto fetch_pos = [&](uint32_t row) { for (int a = 0; a < 3; a++) pos[a] = A.pos[(size_t)row * 3 + a]; };
        if (S.type == RE_WL_DIRECTIONAL) {                                     // handle_direction_light (:144-208)
            uint32_t cur = S.cur;
            if (cur == NONE) {
                if (S.free_n == 0) S.type = RE_WL_POINT;
                else if (A.n_dir) { cur = A.dir_id[0]; S.cur = cur; }       // directional_lights is never filled: the first candidate
                else S.type = RE_WL_POINT;
            }
            if (cur != NONE) {
                const uint32_t p = lower_bound_u32(A.dir_id, A.n_dir, cur);
                if (S.free_n == 0) { bad = cur; bad_kind = 1; }               // free_indexes.pop_front().unwrap() on an empty queue
                else if (p >= A.n_dir || A.dir_id[p] != cur) { bad = cur; bad_kind = 2; }
                else {
                    const re_light_information &I = A.dir_info[p];
                    if ((I.present & (re::LI_HAS | RE_LI_DIRECTION)) != (re::LI_HAS | RE_LI_DIRECTION)) { bad = cur; bad_kind = 2; }
                    else {
                        F.texture_index = pop_free(A, S);
                        fetch_pos(A.dir_row[p]);
                        for (int a = 0; a < 3; a++) dir[a] = I.direction[a];
                        far = I.radius;
                        const float tgt[3] = { pos[0] + dir[0], pos[1] + dir[1], pos[2] + dir[2] }, up[3] = { 0.0f, 1.0f, 0.0f };
                        look_at(pos, tgt, up, view);
                        ortho(A.outline, A.outline, A.outline, A.outline, 0.1f, I.radius, proj);
                        mat4_mul(proj, view, lpv);
                        F.new_map = 1; F.entity_id = cur;
                    }
                }
            }
        } else if (S.type == RE_WL_POINT) {                                    // handle_point_light (:215-266)
            uint32_t cur = S.cur;
            if (cur == NONE) {
                cur = find_next(A, S, RE_WL_POINT, A.near_ids, n_near);
                S.cur = cur;
                if (cur != NONE) {                                             // point_lights.insert(id, [None; 6]): sorted insert
                    uint32_t *mid = A.work_id[1], *midx = A.work_idx[1], w = S.n_map[1];
                    uint32_t p = lower_bound_u32(mid, w, cur);
                    for (uint32_t e = w; e > p; e--) { mid[e] = mid[e - 1]; for (int k = 0; k < 6; k++) midx[e * 6 + k] = midx[(e - 1) * 6 + k]; }
                    mid[p] = cur; for (int k = 0; k < 6; k++) midx[p * 6 + k] = NONE;
                    S.n_map[1] = w + 1;
                }
            }
            if (cur == NONE) { S.type = RE_WL_SPOT; }
            else if (S.free_n > 0) {
                const uint32_t li = light_entry(A, cur);
                const uint32_t need = re::LI_HAS | RE_LI_DIRECTION | RE_LI_FOV;
                if (li == NONE || (A.info[li].present & need) != need) { bad = cur; bad_kind = 2; }
                else {
                    const re_light_information &I = A.info[li];
                    F.texture_index = pop_free(A, S);
                    fetch_pos(A.rows[li]);
                    for (int a = 0; a < 3; a++) dir[a] = I.direction[a];
                    far = I.radius;
                    const float tgt[3] = { pos[0] + dir[0], pos[1] + dir[1], pos[2] + dir[2] }, up[3] = { 0.0f, 1.0f, 0.0f };
                    look_at(pos, tgt, up, view);
                    perspective(A.aspect, A.m11[li], 0.1f, I.radius, proj);
                    mat4_mul(proj, view, lpv);
                    F.new_map = 1; F.entity_id = cur;
                }
            }
        } else {                                                               // handle_spot_light (:273-357)
            uint32_t cur = S.cur;
            if (cur == NONE) {
                cur = find_next(A, S, RE_WL_SPOT, A.near_ids, n_near);
                S.cur = cur;
                if (cur != NONE) {
                    uint32_t *mid = A.work_id[2], *midx = A.work_idx[2], w = S.n_map[2];
                    uint32_t p = lower_bound_u32(mid, w, cur);
                    for (uint32_t e = w; e > p; e--) { mid[e] = mid[e - 1]; for (int k = 0; k < 6; k++) midx[e * 6 + k] = midx[(e - 1) * 6 + k]; }
                    mid[p] = cur; for (int k = 0; k < 6; k++) midx[p * 6 + k] = NONE;
                    S.n_map[2] = w + 1;
                }
            }
            if (cur == NONE) { S.type = RE_WL_DIRECTIONAL; }
            else {
                uint32_t *mid = A.work_id[2], *midx = A.work_idx[2];
                const uint32_t e = lower_bound_u32(mid, S.n_map[2], cur);   // (always present: only find removes entries, and find runs only while cur is None)
                int face = -1;
                for (int k = 0; k < 6 && face < 0; k++) if (midx[e * 6 + k] == NONE) face = k;
                if (face < 0) { S.type = RE_WL_DIRECTIONAL; S.cur = NONE; }
                else if (S.free_n > 0) {
                    const uint32_t li = light_entry(A, cur);
                    if (li == NONE || !(A.info[li].present & re::LI_HAS)) { bad = cur; bad_kind = 2; }
                    else {
                        const float dirs[6][3] = { { -1, 0, 0 }, { 0, -1, 0 }, { 0, 0, -1 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
                        const float ups[6][3] = { { 0, -1, 0 }, { 0, 0, -1 }, { 0, -1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, -1, 0 } };
                        const uint32_t ti = pop_free(A, S);
                        midx[e * 6 + face] = ti;
                        F.texture_index = ti; F.face = (uint32_t)face;
                        fetch_pos(A.rows[li]);
                        for (int a = 0; a < 3; a++) dir[a] = dirs[face][a];
                        far = A.info[li].radius;
                        const float tgt[3] = { pos[0] + dir[0], pos[1] + dir[1], pos[2] + dir[2] };
                        look_at(pos, tgt, ups[face], view);
                        perspective(1.0f, A.spot_m11, 0.10f, far, proj);     // CameraBuilder((1024, 1024)), fov 90
                        mat4_mul(proj, view, lpv);
                        culler = lpv;
                        const uint32_t u = S.n_up % A.up_cap;
                        for (int i = 0; i < 16; i++) { A.up_mat[u * 16 + i] = lpv[i]; A.up_view[u * 16 + i] = view[i]; }
                        A.up_idx[u] = ti; S.n_up++;
                        F.new_map = 1; F.entity_id = cur;
                    }
                }
            }
        }
        if (bad == NONE && F.new_map) {
            for (int i = 0; i < 16; i++) { F.light_projection_view[i] = lpv[i]; F.light_view[i] = view[i]; F.culler[i] = culler[i]; }
            make_planes(culler, F.planes);
            frustum_box(pos, dir, far, F.box);
            for (int a = 0; a < 3; a++) F.position[a] = pos[a];
            F.far_draw = far;
        }
        F.n_uploads = S.n_up;
        s_bad = bad;
        A.out->bad_id = bad; A.out->bad_kind = bad_kind;
        if (bad == NONE) { A.out->f = F; *A.state = S; }
    }
    __syncthreads();
    if (s_bad == NONE)
        for (int t = 1; t < 3; t++)
            for (uint32_t e = tid; e < S.n_map[t]; e += SH_THREADS) { A.map_id[t][e] = A.work_id[t][e]; for (int k = 0; k < 6; k++) A.map_idx[t][e * 6 + k] = A.work_idx[t][e * 6 + k]; }
}

}  // namespace

// a device column filled from host data ON THE WORLD STREAM, so that the copy is ordered behind the steps already enqueued there (a step in flight
// keeps reading the old contents).  The pinned source buffers alternate; one is rewritten only after the copy that last read it has run.
struct Staged {
    void *d = nullptr; size_t cap = 0;
    void *h[2] = {}; size_t hcap[2] = {}; hipEvent_t ev[2] = {}; int k = 0;
    hipError_t upload(const void *src, size_t bytes, hipStream_t st) {
        hipError_t e = hipSuccess;
        if (bytes > cap) {                                               // (rare: the column grew) the old buffer may still be read by a queued step
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            (void)hipFree(d); d = nullptr; cap = 0;
            if ((e = hipMalloc(&d, bytes)) != hipSuccess) return e;
            cap = bytes;
        }
        k ^= 1;
        if (!ev[k] && (e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(ev[k])) != hipSuccess) return e;
        if (bytes > hcap[k]) {
            (void)hipHostFree(h[k]); h[k] = nullptr; hcap[k] = 0;
            if ((e = hipHostMalloc(&h[k], bytes, hipHostMallocDefault)) != hipSuccess) return e;
            hcap[k] = bytes;
        }
        memcpy(h[k], src, bytes);
        if ((e = hipMemcpyAsync(d, h[k], bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
        return hipEventRecord(ev[k], st);
    }
    void release() { (void)hipFree(d); for (int i = 0; i < 2; i++) { (void)hipHostFree(h[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); } }
};

struct re_shadow {
    re_ctx *ctx = nullptr;
    int device = 0;
    re_shadow_config cfg{};
    std::string err;
    ShadowState *d_state = nullptr; ShadowOut *d_out = nullptr;
    uint32_t *d_map_id[3] = {}, *d_map_idx[3] = {}, *d_work_id[3] = {}, *d_work_idx[3] = {}, map_cap = 0;
    uint32_t *d_near = nullptr; uint32_t near_cap = 0;
    float *d_up_mat = nullptr, *d_up_view = nullptr; uint32_t *d_up_idx = nullptr;
    Staged m11, dir;                                                     // the fov column (1 / tan(radians(fov) / 2)) and the directional candidates
    uint64_t m11_epoch = ~0ull; uint32_t m11_n = 0, n_dir = 0;
    re::ShadowWorld W;                                                   // cached between steps (re::shadow_world recomputes it only on a change)
    bool dir_seen = false;                                               // a directional candidate existed at some step: from then on every step may be the one that panics
    re_shadow_stats stats{};
    int fail(int code, const char *fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); err = buf; return code; }
};
static thread_local std::string g_sh_error;
#define SCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (s)->fail(RE_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

extern "C" const char *re_shadow_last_error(const re_shadow *s) { return s ? s->err.c_str() : g_sh_error.c_str(); }

extern "C" int re_shadow_create(re_ctx *c, const re_shadow_config *cfg, re_shadow **out) try {
    if (!c || !cfg || !out) { g_sh_error = "re_shadow_create: NULL argument"; return RE_E_ARG; }
    if (cfg->n_shadow_maps == 0 || cfg->n_shadow_maps > SH_MAX_MAPS) { g_sh_error = "re_shadow_create: n_shadow_maps must be 1..32"; return RE_E_ARG; }
    re_shadow *s = new re_shadow(); s->ctx = c; s->cfg = *cfg;
    if (!s->cfg.upload_capacity) s->cfg.upload_capacity = 64;
    s->device = re::world_device(c);
    auto bail = [&](hipError_t e) { g_sh_error = std::string("re_shadow_create: ") + hipGetErrorString(e); re_shadow_destroy(s); return RE_E_HIP; };
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_state), sizeof(ShadowState));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_out), sizeof(ShadowOut));
    const size_t U = s->cfg.upload_capacity;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_up_mat), U * 64);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_up_view), U * 64);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_up_idx), U * 4);
    if (e != hipSuccess) return bail(e);
    ShadowState S{};                                                     // ShadowFlow::new(n): DirectionalLight(None), free_indexes 0..n
    S.type = RE_WL_DIRECTIONAL; S.cur = NONE; S.free_head = 0; S.free_n = cfg->n_shadow_maps;
    for (uint32_t i = 0; i < cfg->n_shadow_maps; i++) S.free_q[i] = i;
    e = hipMemcpy(s->d_state, &S, sizeof S, hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(e);
    *out = s;
    return RE_OK;
} RE_ABI_GUARD_NOCTX(g_sh_error, "re_shadow_create")

extern "C" void re_shadow_destroy(re_shadow *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(re::world_stream(s->ctx));               // (a step may still be in flight)
    void *ps[] = { s->d_state, s->d_out, s->d_near, s->d_up_mat, s->d_up_view, s->d_up_idx };
    for (void *p : ps) (void)hipFree(p);
    s->m11.release(); s->dir.release();
    for (int t = 0; t < 3; t++) { (void)hipFree(s->d_map_id[t]); (void)hipFree(s->d_map_idx[t]); (void)hipFree(s->d_work_id[t]); (void)hipFree(s->d_work_idx[t]); }
    delete s;
}

// grow a device array of 32-bit words, keeping the first `keep` words (the caller has synchronised the world stream: no step reads the old one)
static hipError_t grow_words(uint32_t **p, size_t words, size_t keep) {
    uint32_t *q = nullptr; hipError_t e = hipMalloc(reinterpret_cast<void **>(&q), words * 4);
    if (e != hipSuccess) return e;
    if (keep && *p) { e = hipMemcpy(q, *p, keep * 4, hipMemcpyDeviceToDevice); if (e != hipSuccess) { (void)hipFree(q); return e; } }
    (void)hipFree(*p); *p = q; return hipSuccess;
}

extern "C" int re_shadow_step(re_shadow *s, re_lighting *l, const re_camera *cam, const re_shadow_args *args, uint32_t flags, re_shadow_frame *out) try {
    if (!s) return RE_E_ARG;
    if (flags != 0) return s->fail(RE_E_ARG, "re_shadow_step: flags is reserved and must be 0");
    if (!cam || !args) return s->fail(RE_E_ARG, "re_shadow_step: NULL argument");
    if (!args->window_width || !args->window_height) return s->fail(RE_E_ARG, "re_shadow_step: window size must be non-zero");
    re::LightingPrev P{};
    if (l) { re::lighting_prev(l, &P); if (P.device != s->device) return s->fail(RE_E_ARG, "re_shadow_step: the world context and the lighting context are on different devices"); }
    // the need masks of re_lighting_set_lights_from_world (the completeness flags of the shared LightInformation column are computed with them);
    // each covers what the shadow path unwraps of that type
    static const uint32_t need[3] = { re::LI_HAS | RE_LI_DIRECTION, re::LI_HAS | RE_LI_CUTOFF | RE_LI_OUTER_CUTOFF | RE_LI_DIRECTION | RE_LI_FOV, re::LI_HAS };
    re::WorldLightsView V;
    { const int rc = re::world_lights_view(s->ctx, s->device, cam, need, &V, &s->err, "re_shadow_step"); if (rc != RE_OK) return rc; }
    re::ShadowWorld &W = s->W;
    { const int rc = re::shadow_world(s->ctx, &W, &s->err); if (rc != RE_OK) return rc; }
    SCHK(s, hipSetDevice(s->device));
    const uint32_t nl = V.nl;
    // map capacity: a map entry is a nearby light of the type, so the light list bounds it
    if (nl + 1 > s->map_cap || nl + 1 > s->near_cap) {
        SCHK(s, hipStreamSynchronize(V.stream));                         // (rare: the light list grew) no step in flight reads the old arrays
        if (nl + 1 > s->map_cap) {
            const uint32_t cap = std::max(nl + 1, 2 * s->map_cap);
            for (int t = 1; t < 3; t++) {
                SCHK(s, grow_words(&s->d_map_id[t], cap, s->map_cap)); SCHK(s, grow_words(&s->d_map_idx[t], (size_t)cap * 6, (size_t)s->map_cap * 6));
                SCHK(s, grow_words(&s->d_work_id[t], cap, 0)); SCHK(s, grow_words(&s->d_work_idx[t], (size_t)cap * 6, 0));
            }
            s->map_cap = cap;
        }
        if (nl + 1 > s->near_cap) { SCHK(s, grow_words(&s->d_near, nl + 1, 0)); s->near_cap = nl + 1; }
    }
    // m11 = 1 / tanf(radians(fov) / 2) of every light with a fov, by the host's libm as ro_perspective computes it; recomputed and uploaded only when
    // the LightInformation column was rebuilt
    if (V.li_epoch != s->m11_epoch || !s->m11.d) {
        std::vector<float> m(std::max(nl, 1u), 0.0f);
        const float rad = (float)M_PI / 180.0f;
        for (uint32_t i = 0; i < nl; i++) if (V.h_info[i].present & RE_LI_FOV) m[i] = 1.0f / tanf((V.h_info[i].fov * rad) / 2.0f);
        SCHK(s, s->m11.upload(m.data(), m.size() * 4, V.stream));
        s->m11_epoch = V.li_epoch; s->stats.n_column_uploads++;
    }
    // directional candidates: [ids | rows | LightInformation], uploaded when they changed
    if (W.changed) {
        s->n_dir = (uint32_t)W.dir_id.size();
        if (s->n_dir) {
            std::vector<uint8_t> buf((size_t)s->n_dir * (8 + sizeof(re_light_information)));
            memcpy(buf.data(), W.dir_id.data(), (size_t)s->n_dir * 4); memcpy(buf.data() + (size_t)s->n_dir * 4, W.dir_row.data(), (size_t)s->n_dir * 4);
            memcpy(buf.data() + (size_t)s->n_dir * 8, W.dir_info.data(), (size_t)s->n_dir * sizeof(re_light_information));
            SCHK(s, s->dir.upload(buf.data(), buf.size(), V.stream));
            s->dir_seen = true;
        }
    }
    const uint32_t nd = s->n_dir;
    const uint8_t *dir_base = static_cast<const uint8_t *>(s->dir.d);
    ShadowArgs A{};
    A.nl = nl; A.rows = V.light_rows; A.flags = V.flags; A.row_id = V.row_id; A.row_cell = V.row_cell; A.cell_key = V.cell_key; A.cell_flags = V.cell_flags; A.sh_cells = V.sh_cells;
    A.pos = V.pos; A.info = V.info; A.m11 = static_cast<const float *>(s->m11.d);
    A.n_dir = nd;
    if (nd) { A.dir_id = reinterpret_cast<const uint32_t *>(dir_base); A.dir_row = A.dir_id + nd; A.dir_info = reinterpret_cast<const re_light_information *>(dir_base + (size_t)nd * 8); }
    for (int t = 0; t < 3; t++) A.prev[t] = P.prev[t];
    A.n_prev = P.n_prev;
    A.state = s->d_state; A.map_cap = s->map_cap; A.n_maps = s->cfg.n_shadow_maps;
    for (int t = 0; t < 3; t++) { A.map_id[t] = s->d_map_id[t]; A.map_idx[t] = s->d_map_idx[t]; A.work_id[t] = s->d_work_id[t]; A.work_idx[t] = s->d_work_idx[t]; }
    A.near_ids = s->d_near; A.up_mat = s->d_up_mat; A.up_view = s->d_up_view; A.up_idx = s->d_up_idx; A.up_cap = s->cfg.upload_capacity; A.out = s->d_out;
    memcpy(A.cam_pv, cam->projection_view, sizeof A.cam_pv);
    A.aspect = (float)args->window_width / (float)args->window_height;
    A.outline = (float)W.outline_length;
    A.spot_m11 = 1.0f / tanf(((float)M_PI / 180.0f * 90.0f) / 2.0f);
    hipLaunchKernelGGL(k_shadow_select, dim3(1), dim3(SH_THREADS), 0, V.stream, A, V.Q);
    SCHK(s, hipGetLastError());
    s->stats.n_steps++;
    // A check is needed when some light the machine may take lacks what its path unwraps, when a light of the list was removed (a light the machine
    // still services may be gone), and once a directional candidate was seen (the directional path panics when the queue runs dry).
    const bool check = s->dir_seen || !V.complete[RE_WL_POINT] || !V.complete[RE_WL_SPOT] || W.dead_light;
    if (check || out) {
        ShadowOut h{};
        SCHK(s, hipMemcpyAsync(&h, s->d_out, sizeof h, hipMemcpyDeviceToHost, V.stream));
        SCHK(s, hipStreamSynchronize(V.stream));
        s->stats.n_host_waits++;
        if (h.bad_id != NONE) {
            if (h.bad_kind == 1) return s->fail(RE_E_STATE, "re_shadow_step: directional light %u needs a shadow map but no free index is left (the reference panics: free_indexes.pop_front().unwrap())", h.bad_id);
            return s->fail(RE_E_STATE, "re_shadow_step: light entity %u is chosen for a shadow map but is gone or lacks LightInformation or a field its path unwraps (the reference panics)", h.bad_id);
        }
        if (out) *out = h.f;
    }
    return RE_OK;
} RE_ABI_GUARD(s, "re_shadow_step")

extern "C" int re_shadow_uploads(re_shadow *s, float *matrices, float *view_matrices, uint32_t *indexes, uint32_t capacity, uint32_t *n) try {
    if (!s) return RE_E_ARG;
    if (!n || (capacity && (!matrices || !view_matrices || !indexes))) return s->fail(RE_E_ARG, "re_shadow_uploads: NULL argument");
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipStreamSynchronize(re::world_stream(s->ctx)));
    ShadowState S{};
    SCHK(s, hipMemcpy(&S, s->d_state, sizeof S, hipMemcpyDeviceToHost));
    const uint32_t U = s->cfg.upload_capacity, kept = std::min(S.n_up, U), m = std::min(kept, capacity);
    std::vector<float> mat((size_t)U * 16), view((size_t)U * 16); std::vector<uint32_t> idx(U);
    if (m) {
        SCHK(s, hipMemcpy(mat.data(), s->d_up_mat, (size_t)U * 64, hipMemcpyDeviceToHost));
        SCHK(s, hipMemcpy(view.data(), s->d_up_view, (size_t)U * 64, hipMemcpyDeviceToHost));
        SCHK(s, hipMemcpy(idx.data(), s->d_up_idx, (size_t)U * 4, hipMemcpyDeviceToHost));
    }
    for (uint32_t k = 0; k < m; k++) {                                   // the last m entries, oldest first
        const uint32_t u = (S.n_up - m + k) % U;
        memcpy(matrices + (size_t)k * 16, &mat[(size_t)u * 16], 64); memcpy(view_matrices + (size_t)k * 16, &view[(size_t)u * 16], 64); indexes[k] = idx[u];
    }
    *n = m;
    return RE_OK;
} RE_ABI_GUARD(s, "re_shadow_uploads")

extern "C" int re_shadow_get_stats(re_shadow *s, re_shadow_stats *out) {
    if (!s || !out) return RE_E_ARG;
    *out = s->stats;
    return RE_OK;
}
