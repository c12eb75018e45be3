// re_lighting.hip -- BASELINE.json configs[4]: the deferred-lighting second pass of render_engine
// (render_engine_assets/shaders/second_pass_frag.glsl:20-139) as a HIP compute kernel for gfx950, plus its C ABI.
//
// Tiled deferred shading.  One 256-thread workgroup owns a 32x16-pixel tile (2 pixels per lane; each wave a compact 16x8 block of it):
//   1. tile AABB of the G-buffer positions (wave shuffles + LDS),
//   2. exact-conservative culling of the radius ("spot") lights against the tile AABB, 256 lights per round, compacted
//      into an LDS list (ballot + prefix: the per-pixel summation order is deterministic).  Only the lights that can reach the
//      tile along one axis are tested: re_lighting_set_lights orders the records by LIGHT_BUCKETS slabs along the axis of the
//      lights' largest extent (ascending light index inside a slab), and a tile takes the slabs its AABB, grown by the largest
//      radius, overlaps -- 192 of the 4096 lights of configs[4] instead of all of them,
//   3. every lane shades its pixels over the list, a pair at a time as 2-vectors; the listed lights' records (64 B) are staged in LDS by the
//      whole workgroup and read as broadcasts, so the inner loop is pure f32 VALU -- the kernel is VALU-bound, not HBM-bound; a light that
//      reaches no pixel of the wave's block costs the wave its distance test only,
//   4. cone ("point") lights cannot be culled (no radius in the shader) and are evaluated for every pixel,
//   5. epilogue exactly as main(): (spot + point) + spot -- the spot term is added twice in the shader --, the
//      default-diffuse floor, clamp.
// gLightPosition is not read: the shadow value it feeds is computed and discarded by the shader (:105).
// Contract (tests/test_lighting_exact_gpu.py against the float64 restatement tests/lighting_ref.py):
//   * exact, as the CPU oracle decides them: the radius cut (sqrtf of the unfused (dx*dx + dy*dy) + dz*dz against the radius; NaN radius = every pixel,
//     negative radius = none, 0 / -0 = the pixel at the light's exact position), and a light at a pixel's exact position (its ambient part, attenuation 1);
//     not covered: a distance whose square overflows f32 (|d| >= ~1.8e19: a cone light, or a radius light under a +inf or NaN radius), which gets attenuation 1, not 0;
//   * within 1e-4 of the float64 value per channel (hardware reciprocals, fused multiply-adds); a channel that close to the default-diffuse cutoff
//     may take either side of the floor.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "re_hip.h"
#include "re_guard.h"
#include "re_world_lights.h"

namespace {

constexpr int TILE = 32, LT_THREADS = 256, LIST_CAP = 384;
constexpr int NPX = 2, NPAIR = NPX / 2, TILE_H = 8 * NPX;   // pixels per lane (pairs of them shaded as 2-vectors); a workgroup's tile is TILE x TILE_H pixels, a wave's share of it 16 x 4 NPX
constexpr uint32_t CULL_CHUNK = 1;      // rounds of 256 lights whose positions are in flight together (a tile of configs[4] tests 192 lights; more rounds in flight cost registers: 8 -> 152 VGPRs, 2 -> 128)
constexpr uint32_t LIGHT_BUCKETS = 4096; // slabs along the sort axis of the radius lights

struct LightParams {
    uint32_t width, height, n_spot, n_point;
    float cam[3]; float cutoff, default_diffuse; uint32_t any_visible;
    uint32_t axis; float kmin, inv_w, rmax;                                   // slab of a light: light_bucket(position[axis])
};
// the slab a coordinate falls into: monotone in `key` (subtraction, multiplication by a positive constant, clamp and floor all are), so every light whose
// coordinate lies in [a, b] has its slab in [light_bucket(a), light_bucket(b)] -- the host files the lights with this same function
__host__ __device__ inline uint32_t light_bucket(float key, float kmin, float inv_w) {
    float b = (key - kmin) * inv_w;
    b = b > 0.0f ? b : 0.0f;                                                    // (also NaN -> 0)
    b = b < (float)(LIGHT_BUCKETS - 1u) ? b : (float)(LIGHT_BUCKETS - 1u);
    return (uint32_t)b;
}

__device__ __forceinline__ float3 f3(float x, float y, float z) { return make_float3(x, y, z); }
__device__ __forceinline__ float dot3(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return f3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float3 norm3v(float3 v) { float n = sqrtf(dot3(v, v)); return f3(v.x / n, v.y / n, v.z / n); }
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }   // a value every lane holds alike -> a scalar register
__device__ __forceinline__ float pow64(float x) { x *= x; x *= x; x *= x; x *= x; x *= x; x *= x; return x; }

// the oracle's squared distance, (dx*dx + dy*dy) + dz*dz with every operation rounded: what the radius cut is decided on
__device__ __forceinline__ float d2_unfused(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    return (dx * dx + dy * dy) + dz * dz;
}

// a * b, but 0 when either operand is 0 (v_mul_legacy_f32: also 0 * inf and 0 * NaN)
__device__ __forceinline__ float mul_legacy(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));   // (no clang builtin for gfx950)
    return r;
#else
    return a == 0.0f || b == 0.0f ? 0.0f : a * b;
#endif
}

// one cone light's contribution to one pixel; A = (pos, unused), B = (diffuse, linear), C = (specular, quadratic), D = ambient rgba
__device__ __forceinline__ void shade(float3 frag, float3 nrm, float3 od, float3 camdir, float4 A, float4 B, float4 C, float4 D, float intensity, float3 &acc) {
#pragma clang fp contract(fast)          // this file's arithmetic is tolerance-bound (1e-4), not bit-exact like the cull path: multiply-adds may fuse here (the library is built with -ffp-contract=off)
    // The shader's divisions and square roots are GPU-precision operations in the reference too (GLSL gives no IEEE guarantee); here they are the
    // hardware's reciprocal / reciprocal square root (1 ulp) instead of the ~10-instruction IEEE sequences: the kernel is bound by the VALU work of
    // this function, and the result stays within 1e-6 of the f32 GLSL restatement (tolerance of the path: 1e-4).
    float3 d = sub3(f3(A.x, A.y, A.z), frag);
    const float d2 = dot3(d, d);
    // a light at the pixel's exact position (d2 = 0): rsq gives +inf, so the direction is NaN and the oracle's fmaxf drops the diffuse and specular parts;
    // the distance must come out 0 (attenuation 1), not 0 * inf = NaN -- v_mul_legacy_f32 returns 0 when either operand is 0 (as in shade_pair, an
    // overflowed d2 = +inf then gives attenuation 1 where the oracle's is 0)
    const float inv = __builtin_amdgcn_rsqf(d2), dist = mul_legacy(d2, inv);
    float3 nd = f3(d.x * inv, d.y * inv, d.z * inv);
    float att = __builtin_amdgcn_rcpf(1.0f + B.w * dist + C.w * dist * dist);  // calculateAttenuation :132-136
    float dc = fmaxf(dot3(nrm, nd), 0.0f);                                     // calculateDiffuse :118-122
    float3 hv = f3(nd.x + camdir.x, nd.y + camdir.y, nd.z + camdir.z);         // calculateSpecular :124-130
    const float invh = __builtin_amdgcn_rsqf(dot3(hv, hv));
    float sf = pow64(fmaxf(dot3(nrm, hv) * invh, 0.0f));
    acc.x += (od.x * D.x * D.w) * att; acc.x += (B.x * od.x * dc) * att * intensity; acc.x += (C.x * sf) * att;
    acc.y += (od.y * D.y * D.w) * att; acc.y += (B.y * od.y * dc) * att * intensity; acc.y += (C.y * sf) * att;
    acc.z += (od.z * D.z * D.w) * att; acc.z += (B.z * od.z * dc) * att * intensity; acc.z += (C.z * sf) * att;
}

// The radius lights' inner loop works on TWO pixels of a lane at a time, as 2-vectors: gfx950 issues v_pk_{add,mul,fma}_f32 on a register pair at the rate of
// the scalar forms, so everything but the reciprocals / reciprocal square roots costs half the instructions per pixel.  A pixel of the pair that is outside the
// radius (or outside the image) is computed along and its contribution dropped at the end (selected, not multiplied: its intermediate values may be inf / NaN).
typedef float f2 __attribute__((ext_vector_type(2)));
struct PixelPair { f2 fx, fy, fz, nx, ny, nz, ox, oy, oz, cx, cy, cz; };        // position, normal, albedo, direction to the camera
__device__ __forceinline__ f2 rsq2(f2 v) { f2 r; r.x = __builtin_amdgcn_rsqf(v.x); r.y = __builtin_amdgcn_rsqf(v.y); return r; }
__device__ __forceinline__ f2 rcp2(f2 v) { f2 r; r.x = __builtin_amdgcn_rcpf(v.x); r.y = __builtin_amdgcn_rcpf(v.y); return r; }
__device__ __forceinline__ f2 max0(f2 v) { f2 r; r.x = fmaxf(v.x, 0.0f); r.y = fmaxf(v.y, 0.0f); return r; }
__device__ __forceinline__ void shade_pair(const PixelPair &X, bool live0, bool live1, float4 A, float4 B, float4 C, float4 D, f2 &ax, f2 &ay, f2 &az) {
#pragma clang fp contract(fast)
    const f2 dx = A.x - X.fx, dy = A.y - X.fy, dz = A.z - X.fz;
    const f2 d2 = (dx * dx + dy * dy) + dz * dz;                               // (fused: one v_pk_mul, two v_pk_fma)
    // :97-100: dist > radius, decided exactly as the oracle decides it (the cut is a discontinuity): sqrtf of the UNFUSED d2 against the radius, the square
    // root only near the boundary.  The fast accept / reject may use the fused d2 above: it is a few ulp from the unfused one, and the margins of 1e-6 are ~8 ulp
    const float r2 = A.w * A.w, r2_out = r2 * 1.000001f, r2_in = r2 * 0.999999f;
    bool in0 = live0 && !(A.w < 0.0f) && !(d2.x > r2_out), in1 = live1 && !(A.w < 0.0f) && !(d2.y > r2_out);      // (a distance is never below a negative radius)
    const bool shell0 = in0 && d2.x > r2_in, shell1 = in1 && d2.y > r2_in;
    if (__builtin_amdgcn_ballot_w64(shell0 || shell1)) {                      // a wave-uniform branch the compiler cannot flatten (the asm pins the operands inside it): flattened,
        float x0 = dx.x, y0 = dy.x, z0 = dz.x, x1 = dx.y, y1 = dy.y, z1 = dz.y;  // the IEEE square root (22 instructions) ran for every pixel inside the radius
        asm volatile("" : "+v"(x0), "+v"(y0), "+v"(z0), "+v"(x1), "+v"(y1), "+v"(z1));
        if (shell0 && sqrtf(d2_unfused(x0, y0, z0)) > A.w) in0 = false;
        if (shell1 && sqrtf(d2_unfused(x1, y1, z1)) > A.w) in1 = false;
    }
    if (!(in0 || in1)) return;
    // a light at the pixel's exact position (d2 = 0): the oracle's term is the ambient part with attenuation 1 (its NaN direction is dropped by fmaxf, as
    // max0 below drops it here); v_mul_legacy_f32 makes the distance 0 there instead of 0 * rsq(0) = 0 * inf = NaN, and is the plain product for every
    // finite nonzero d2.  (Not for an overflowed d2 = +inf, |d| >= ~1.8e19, which only a +inf or NaN radius admits: rsq gives 0, so the distance is 0 and
    // the attenuation 1 where the oracle's is 0.)
    const f2 inv = rsq2(d2);
    f2 dist; dist.x = mul_legacy(d2.x, inv.x); dist.y = mul_legacy(d2.y, inv.y);
    const f2 ndx = dx * inv, ndy = dy * inv, ndz = dz * inv;
    const f2 att = rcp2(1.0f + B.w * dist + C.w * dist * dist);                // calculateAttenuation :132-136
    const f2 dc = max0((X.nx * ndx + X.ny * ndy) + X.nz * ndz);                // calculateDiffuse :118-122
    const f2 hx = ndx + X.cx, hy = ndy + X.cy, hz = ndz + X.cz;                // calculateSpecular :124-130
    const f2 invh = rsq2((hx * hx + hy * hy) + hz * hz);
    f2 sf = max0(((X.nx * hx + X.ny * hy) + X.nz * hz) * invh);
    sf *= sf; sf *= sf; sf *= sf; sf *= sf; sf *= sf; sf *= sf;                 // pow(., 64)
    // ambient * albedo + diffuse * albedo * dc + specular * sf, all times the attenuation
    const f2 tx = (X.ox * (B.x * dc + D.x * D.w) + C.x * sf) * att, ty = (X.oy * (B.y * dc + D.y * D.w) + C.y * sf) * att, tz = (X.oz * (B.z * dc + D.z * D.w) + C.z * sf) * att;
    f2 cx, cy, cz;
    cx.x = in0 ? tx.x : 0.0f; cx.y = in1 ? tx.y : 0.0f; cy.x = in0 ? ty.x : 0.0f; cy.y = in1 ? ty.y : 0.0f; cz.x = in0 ? tz.x : 0.0f; cz.y = in1 ? tz.y : 0.0f;
    ax += cx; ay += cy; az += cz;
}

// DEV = false: the parameters come with the launch (re_lighting_set_lights); DEV = true: the light counts, the slab parameters, the camera and the factors are
// read from the device block the from-world upload wrote (re_lighting_set_lights_from_world), so that nothing of them has to come back to the host.
template <bool DEV>
__global__ __launch_bounds__(LT_THREADS) void k_deferred_lighting(LightParams Parg, const float4 *__restrict__ gpos, const float4 *__restrict__ gnormal, const uchar4 *__restrict__ galbedo,
                                                                   const float4 *__restrict__ spot,     // 4 float4 per light: A, B, C, D (slab order)
                                                                   const uint32_t *__restrict__ slab_start,   // LIGHT_BUCKETS + 1: first record of each slab
                                                                   const float4 *__restrict__ point,    // 5 float4 per light: A(pos), B, C, D, E(dir.xyz normalised, -) + F(cutoff, outer, -, -) packed as 6
                                                                   float4 *__restrict__ out, const LightParams *__restrict__ dparams) {
    LightParams P = Parg;
    if constexpr (DEV) {
        const LightParams D = *dparams;
        P.n_spot = D.n_spot; P.n_point = D.n_point; P.cam[0] = D.cam[0]; P.cam[1] = D.cam[1]; P.cam[2] = D.cam[2]; P.cutoff = D.cutoff; P.default_diffuse = D.default_diffuse;
        P.any_visible = D.any_visible; P.axis = D.axis; P.kmin = D.kmin; P.inv_w = D.inv_w; P.rmax = D.rmax;
    }
    __shared__ float s_red[4][6];
    __shared__ float4 s_rec[LIST_CAP * 4];                                    // the listed lights' records (A, B, C, D)
    __shared__ uint32_t s_wcnt[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    // A wave owns a 16x16 QUADRANT of the tile (lane -> column lane & 15, rows (lane >> 4) + 4k): a listed light that misses the quadrant costs the wave its distance test only (shade_pair
    // returns with no lane inside).  With the rows of a wave spread over the whole tile (round 2: row (tid >> 5) + 8k) every wave went through the full evaluation of nearly every listed light.
    static_assert(TILE == 32 && LT_THREADS == 256 && NPX % 2 == 0, "four waves, one quadrant each; pixels in pairs");
    const uint32_t tx = blockIdx.x * TILE + 16u * (wid & 1u) + (lane & 15u), ty0 = blockIdx.y * TILE_H + (uint32_t)(4 * NPX) * (wid >> 1) + (lane >> 4);
    float3 frag[NPX], nrm[NPX], od[NPX], camdir[NPX], acc[NPX]; bool live[NPX];
    float lo[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, hi[3] = { -3.4e38f, -3.4e38f, -3.4e38f };
#pragma unroll
    for (int k = 0; k < NPX; k++) {
        uint32_t y = ty0 + 4u * k;
        live[k] = tx < P.width && y < P.height;
        frag[k] = nrm[k] = od[k] = camdir[k] = f3(0.f, 0.f, 0.f); acc[k] = f3(0.f, 0.f, 0.f);
        if (live[k]) {
            size_t p = (size_t)y * P.width + tx;
            // (streamed once: non-temporal, so the G-buffer does not push the light records and slab bounds out of the L2)
            typedef float v4f __attribute__((ext_vector_type(4)));
            const v4f gpv = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(gpos) + p), gnv = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(gnormal) + p);
            const uint32_t gaw = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(galbedo) + p);
            const float4 gp = make_float4(gpv.x, gpv.y, gpv.z, gpv.w), gn = make_float4(gnv.x, gnv.y, gnv.z, gnv.w);
            uchar4 ga; ga.x = (unsigned char)(gaw & 0xFFu); ga.y = (unsigned char)((gaw >> 8) & 0xFFu); ga.z = (unsigned char)((gaw >> 16) & 0xFFu); ga.w = (unsigned char)(gaw >> 24);
            frag[k] = f3(gp.x, gp.y, gp.z); nrm[k] = f3(gn.x, gn.y, gn.z);
            // (per-pixel setup with the hardware's 1-ulp operations, like the shading itself: the IEEE divisions and square root here were ~300 of a tile's ~1,900 instructions per wave)
            constexpr float k255 = 1.0f / 255.0f;
            od[k] = f3(ga.x * k255, ga.y * k255, ga.z * k255);
            const float3 tc = sub3(f3(P.cam[0], P.cam[1], P.cam[2]), frag[k]); const float itc = __builtin_amdgcn_rsqf(dot3(tc, tc));
            camdir[k] = f3(tc.x * itc, tc.y * itc, tc.z * itc);
            lo[0] = fminf(lo[0], gp.x); lo[1] = fminf(lo[1], gp.y); lo[2] = fminf(lo[2], gp.z);
            hi[0] = fmaxf(hi[0], gp.x); hi[1] = fmaxf(hi[1], gp.y); hi[2] = fmaxf(hi[2], gp.z);
        }
    }
    if (P.any_visible) {
        // ---- tile AABB ----
#pragma unroll
        for (int a = 0; a < 3; a++)
            for (int d = 32; d >= 1; d >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64)); }
        if (lane == 0) for (int a = 0; a < 3; a++) { s_red[wid][a] = lo[a]; s_red[wid][3 + a] = hi[a]; }
        __syncthreads();
        for (int a = 0; a < 3; a++) { lo[a] = uniform(fminf(fminf(s_red[0][a], s_red[1][a]), fminf(s_red[2][a], s_red[3][a]))); hi[a] = uniform(fmaxf(fmaxf(s_red[0][3 + a], s_red[1][3 + a]), fmaxf(s_red[2][3 + a], s_red[3][3 + a]))); }
        // ---- radius lights: cull 256 per round into the ordered LDS list, shade whenever the list could overflow ----
        // Two things keep a tile from waiting on one memory round trip after the other: the positions of CULL_CHUNK rounds of lights are requested
        // together before their tests, and the 64-byte records of the listed lights are fetched into LDS by the whole workgroup in one go, so the
        // per-pixel loop reads them as LDS broadcasts (round 1 loaded each light's record with scalar loads inside that loop: one exposed L2
        // latency per listed light and tile).
        PixelPair X[NPAIR]; f2 sax[NPAIR], say[NPAIR], saz[NPAIR];                // pixels (0, 1), (2, 3) .. of the lane
#pragma unroll
        for (int q = 0; q < NPAIR; q++) {
            const int k0 = 2 * q, k1 = 2 * q + 1;
            X[q].fx.x = frag[k0].x; X[q].fx.y = frag[k1].x; X[q].fy.x = frag[k0].y; X[q].fy.y = frag[k1].y; X[q].fz.x = frag[k0].z; X[q].fz.y = frag[k1].z;
            X[q].nx.x = nrm[k0].x; X[q].nx.y = nrm[k1].x; X[q].ny.x = nrm[k0].y; X[q].ny.y = nrm[k1].y; X[q].nz.x = nrm[k0].z; X[q].nz.y = nrm[k1].z;
            X[q].ox.x = od[k0].x; X[q].ox.y = od[k1].x; X[q].oy.x = od[k0].y; X[q].oy.y = od[k1].y; X[q].oz.x = od[k0].z; X[q].oz.y = od[k1].z;
            X[q].cx.x = camdir[k0].x; X[q].cx.y = camdir[k1].x; X[q].cy.x = camdir[k0].y; X[q].cy.y = camdir[k1].y; X[q].cz.x = camdir[k0].z; X[q].cz.y = camdir[k1].z;
            sax[q] = say[q] = saz[q] = (f2)(0.0f);
        }
        uint32_t n = 0;                                                        // listed lights (uniform)
        auto shade_list = [&]() {                                              // (the records are in s_rec: the lane that listed a light put its record there, behind the barrier of the round)
            for (uint32_t j = 0; j < n; j++) {
                const float4 A = s_rec[j * 4u], B = s_rec[j * 4u + 1u], C = s_rec[j * 4u + 2u], D = s_rec[j * 4u + 3u];
#pragma unroll
                for (int q = 0; q < NPAIR; q++) shade_pair(X[q], live[2 * q], live[2 * q + 1], A, B, C, D, sax[q], say[q], saz[q]);
            }
            __syncthreads();                                                   // (s_rec is refilled afterwards)
            n = 0;
        };
        // the records a light of this tile can be among: the slabs [lo - rmax, hi + rmax] along the sort axis (a light farther away along that axis alone misses the tile)
        const float reach = P.rmax * 1.00001f + 1e-3f;                         // (the margin of the test below)
        const float alo = P.axis == 0 ? lo[0] : (P.axis == 1 ? lo[1] : lo[2]), ahi = P.axis == 0 ? hi[0] : (P.axis == 1 ? hi[1] : hi[2]);
        uint32_t l_begin = 0, l_end = 0;
        if (P.n_spot && ahi >= alo) { l_begin = slab_start[light_bucket(alo - reach, P.kmin, P.inv_w)]; l_end = slab_start[light_bucket(ahi + reach, P.kmin, P.inv_w) + 1u]; }
        for (uint32_t c0 = l_begin; c0 < l_end; c0 += LT_THREADS * CULL_CHUNK) {
            // the WHOLE record of every light tested (64 B, L2-resident: 4,096 lights are 256 KB), not its position alone: a lane that lists its light stores the record into LDS at once,
            // and the tile does not wait for a second round trip (list -> records) before it can shade
            float4 Ac[CULL_CHUNK], Bc[CULL_CHUNK], Cc[CULL_CHUNK], Dc[CULL_CHUNK];
#pragma unroll
            for (uint32_t r = 0; r < CULL_CHUNK; r++) {
                const uint32_t li = c0 + r * LT_THREADS + tid;
                Ac[r] = make_float4(0.f, 0.f, 0.f, -1.f); Bc[r] = Cc[r] = Dc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (li < l_end) { Ac[r] = spot[(size_t)li * 4]; Bc[r] = spot[(size_t)li * 4 + 1]; Cc[r] = spot[(size_t)li * 4 + 2]; Dc[r] = spot[(size_t)li * 4 + 3]; }
            }
#pragma unroll
            for (uint32_t r = 0; r < CULL_CHUNK; r++) {
                const uint32_t i0 = c0 + r * LT_THREADS;
                if (i0 >= l_end) break;                                         // uniform
                const uint32_t li = i0 + tid; bool hit = false;
                if (li < l_end) {
                    const float4 A = Ac[r];
                    float dx = fmaxf(fmaxf(lo[0] - A.x, A.x - hi[0]), 0.0f), dy = fmaxf(fmaxf(lo[1] - A.y, A.y - hi[1]), 0.0f), dz = fmaxf(fmaxf(lo[2] - A.z, A.z - hi[2]), 0.0f);
                    float rr = A.w * 1.00001f + 1e-3f;                              // conservative: the exact per-pixel radius test follows
                    hit = !(((dx * dx + dy * dy) + dz * dz) > rr * rr);             // (a NaN radius is unbounded: no distance is > NaN in the oracle either)
                }
                const uint64_t m = __ballot(hit);
                if (lane == 0) s_wcnt[wid] = (uint32_t)__popcll(m);
                __syncthreads();
                uint32_t base = n, tot = 0;
                for (uint32_t w = 0; w < 4; w++) { if (w < wid) base += s_wcnt[w]; tot += s_wcnt[w]; }
                if (hit) {
                    const uint32_t at = (base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))) * 4u;
                    s_rec[at] = Ac[r]; s_rec[at + 1u] = Bc[r]; s_rec[at + 2u] = Cc[r]; s_rec[at + 3u] = Dc[r];
                }
                __syncthreads();
                n += tot;
                if (n + LT_THREADS > LIST_CAP) shade_list();                    // uniform decision: the next round could overflow the list
            }
        }
        if (n) shade_list();
        // ---- cone lights (calculatePointLights :72-91): no radius, every pixel evaluates every light ----
        float3 point_acc[NPX]; for (int k = 0; k < NPX; k++) point_acc[k] = f3(0.f, 0.f, 0.f);
        for (uint32_t l = 0; l < P.n_point; l++) {
            float4 A = point[(size_t)l * 6], B = point[(size_t)l * 6 + 1], C = point[(size_t)l * 6 + 2], D = point[(size_t)l * 6 + 3], E = point[(size_t)l * 6 + 4], F = point[(size_t)l * 6 + 5];
#pragma unroll
            for (int k = 0; k < NPX; k++) if (live[k]) {
                float3 fn = norm3v(frag[k]);
                float angle = dot3(sub3(fn, f3(A.x, A.y, A.z)), f3(E.x, E.y, E.z));
                float intensity = fminf(fmaxf((angle - F.y) / (F.x - F.y), 0.0f), 1.0f);
                shade(frag[k], nrm[k], od[k], camdir[k], A, B, C, D, intensity, point_acc[k]);
            }
        }
        float3 spot_acc[NPX];
#pragma unroll
        for (int q = 0; q < NPAIR; q++) { spot_acc[2 * q] = f3(sax[q].x, say[q].x, saz[q].x); spot_acc[2 * q + 1] = f3(sax[q].y, say[q].y, saz[q].y); }
#pragma unroll
        for (int k = 0; k < NPX; k++) {
            // main() :42-44: lightColour = spot; lightColour += point; lightColour += spot
            acc[k].x = (spot_acc[k].x + point_acc[k].x) + spot_acc[k].x; acc[k].y = (spot_acc[k].y + point_acc[k].y) + spot_acc[k].y; acc[k].z = (spot_acc[k].z + point_acc[k].z) + spot_acc[k].z;
            acc[k].x += (acc[k].x < P.cutoff ? 1.0f : 0.0f) * od[k].x * P.default_diffuse;
            acc[k].y += (acc[k].y < P.cutoff ? 1.0f : 0.0f) * od[k].y * P.default_diffuse;
            acc[k].z += (acc[k].z < P.cutoff ? 1.0f : 0.0f) * od[k].z * P.default_diffuse;
            acc[k].x = fminf(fmaxf(acc[k].x, 0.0f), 1.0f); acc[k].y = fminf(fmaxf(acc[k].y, 0.0f), 1.0f); acc[k].z = fminf(fmaxf(acc[k].z, 0.0f), 1.0f);
        }
    } else {
#pragma unroll
        for (int k = 0; k < NPX; k++) acc[k] = f3(od[k].x * 1.0f * P.default_diffuse, od[k].y * 1.0f * P.default_diffuse, od[k].z * 1.0f * P.default_diffuse);   // :30-34
    }
#pragma unroll
    for (int k = 0; k < NPX; k++) if (live[k]) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        v4f o; o.x = acc[k].x; o.y = acc[k].y; o.z = acc[k].z; o.w = 1.0f;
        __builtin_nontemporal_store(o, reinterpret_cast<v4f *>(out) + ((size_t)(ty0 + 4u * k) * P.width + tx));
    }
}

__global__ void k_gather_pixels(const float4 *img, const uint32_t *idx, uint32_t n, float4 *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = img[idx[i]];
}


// ---- from-world upload (re_lighting_set_lights_from_world): upload_directional_lights / upload_point_lights / upload_spot_lights of RenderSystem::draw
// (render_system/render_system.rs:681-845) on the device, two single-workgroup launches on the world context's stream:
//   k_world_select: the nearby test of every light of the list (ascending EntityId), previous ∩ nearby, the slots (existing ++ nearby, take N) and the
//                   next previous set, into scratch -- nothing the renderer reads is written, so a failed check leaves everything as it was;
//   k_world_commit: the previous sets, the records in K5's layouts (live positions), the slab table of the radius lights, the device parameter block.
// Type index t: 0 directional, 1 point ("cone"), 2 spot ("radius") -- RE_WL_*.
constexpr int WL_THREADS = 1024, WL_WAVES = WL_THREADS / 64, SEL_THREADS = 512, SEL_WAVES = SEL_THREADS / 64;   // (the selection at 1024 threads spilled: 128 VGPRs)
constexpr uint32_t WL_LDS_BUCKETS = 8192;   // spot slots whose slab index the stable placement reads from LDS (the rest from the scratch array)
struct WorldSel { uint32_t n_prev[3], n_nearby[3], n_slots[3], n_stage[3], bad_id, pad; };
struct WorldSelArgs {
    uint32_t nl; const uint32_t *rows, *flags, *row_id, *row_cell; const uint64_t *cell_key; const uint8_t *cell_flags; const int32_t *sh_cells;
    const re_light_information *info; uint32_t max[3], need[3];
    const uint32_t *prev[3]; uint32_t *stage[3], *slot_li[3], *slot_id[3], *lmask; WorldSel *sel;
};
struct WorldCommitArgs {
    WorldSel *sel; const uint32_t *slot_li[3], *stage[3]; uint32_t *prev[3];
    const uint32_t *rows; const float *pos; const re_light_information *info;
    uint32_t max_spot; float cam[3], cutoff, default_diffuse;
    float4 *spot; uint32_t *slab; float4 *point; LightParams *params; uint32_t *place;
};
__device__ __forceinline__ bool in_sorted(const uint32_t *a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1u; else hi = m; }
    return lo < n && a[lo] == v;
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

__global__ __launch_bounds__(SEL_THREADS) void k_world_select(WorldSelArgs A, re::LightQuery Qarg) {
    __shared__ uint32_t s_tot[6], s_wc[SEL_WAVES][6];
    __shared__ re::LightQuery Q;                                              // (the level boxes are indexed by a section's level: from LDS, not a private copy of the argument)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    if (tid == 0) Q = Qarg;
    const uint32_t type_bit[3] = { re::F_LIGHT_DIRECTIONAL, re::F_LIGHT_POINT, re::F_LIGHT_SPOT };
    uint32_t nprev[3];
    #pragma unroll
    for (int t = 0; t < 3; t++) nprev[t] = A.sel->n_prev[t];
    __syncthreads();                                                          // (every thread has read the counts before thread 0 resets the check)
    if (tid < 6) s_tot[tid] = 0u;
    if (tid == 0) A.sel->bad_id = 0xFFFFFFFFu;
    __syncthreads();
    // pass 1: per light, bit t = nearby light of type t (find_nearby_lights: re_visible_lights' test), bit 3 + t = also in previous_t
    for (uint32_t base = 0; base < A.nl; base += SEL_THREADS) {
        const uint32_t i = base + tid; uint32_t m = 0;
        if (i < A.nl) {
            const uint32_t r = A.rows[i], fl = A.flags[r], rc = A.row_cell[r];
            if (!(fl & re::F_DEAD) && (fl & re::F_LIGHT_ANY) && rc != re::ROW_CELL_NONE) {
                bool vis = false;
                if (!(rc & re::ROW_CELL_SHARED)) vis = !(A.cell_flags[rc] & re::CF_PAD) && re::light_section_visible(A.cell_key[rc], Q);
                else {
                    const uint32_t sh = rc & ~re::ROW_CELL_SHARED;
                    #pragma unroll
                    for (int k = 0; k < 8 && !vis; k++) { const int32_t c = A.sh_cells[sh * 8 + k]; if (c >= 0 && !(A.cell_flags[c] & re::CF_PAD)) vis = re::light_section_visible(A.cell_key[c], Q); }
                }
                if (vis) {
                    const uint32_t id = A.row_id[r];
                    #pragma unroll
                    for (int t = 0; t < 3; t++) if (fl & type_bit[t]) { m |= 1u << t; if (in_sorted(A.prev[t], nprev[t], id)) m |= 8u << t; }
                }
            }
            A.lmask[i] = m;
        }
        #pragma unroll
        for (int q = 0; q < 6; q++) { const uint64_t b = __ballot((m >> q) & 1u); if (lane == 0 && b) atomicAdd(&s_tot[q], (uint32_t)__popcll(b)); }
    }
    __syncthreads();
    // N = min(|nearby|, max); slots = existing[0 .. min(|existing|, N)) ++ nearby[0 .. K), K = N - min(|existing|, N)
    uint32_t take[3], ne[3], K[3];
    #pragma unroll
    for (int t = 0; t < 3; t++) { take[t] = min(s_tot[t], A.max[t]); ne[t] = min(s_tot[3 + t], take[t]); K[t] = take[t] - ne[t]; }
    // pass 2: order-preserving compaction (ballot ranks + per-wave counts; carries across rounds)
    uint32_t cj[3] = { 0, 0, 0 }, ce[3] = { 0, 0, 0 }, cp[3] = { 0, 0, 0 };
    for (uint32_t base = 0; base < A.nl; base += SEL_THREADS) {
        const uint32_t i = base + tid;
        const uint32_t m = i < A.nl ? A.lmask[i] : 0u;                        // (written by this thread in pass 1)
        uint64_t b[6];
        #pragma unroll
        for (int q = 0; q < 6; q++) b[q] = __ballot((m >> q) & 1u);
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < 6; q++) s_wc[wid][q] = (uint32_t)__popcll(b[q]);
        __syncthreads();
        uint32_t pre[6], tot[6];
        #pragma unroll
        for (int q = 0; q < 6; q++) { pre[q] = tot[q] = 0; for (uint32_t w = 0; w < SEL_WAVES; w++) { const uint32_t v = s_wc[w][q]; tot[q] += v; if (w < wid) pre[q] += v; } }
        __syncthreads();                                                      // (s_wc is reused below)
        uint32_t id = 0, present = 0, keep = 0;
        if (m) { id = A.row_id[A.rows[i]]; present = A.info[i].present; }
        #pragma unroll
        for (int t = 0; t < 3; t++) {
            const uint32_t j = cj[t] + pre[t] + lanes_below(b[t]), k = ce[t] + pre[3 + t] + lanes_below(b[3 + t]);
            const bool sel_e = ((m >> (3 + t)) & 1u) && k < take[t], sel_n = ((m >> t) & 1u) && j < K[t];
            if (sel_e) { A.slot_li[t][k] = i; A.slot_id[t][k] = id; }
            if (sel_n) { A.slot_li[t][ne[t] + j] = i; A.slot_id[t][ne[t] + j] = id; }
            if ((sel_e || sel_n) && (present & A.need[t]) != A.need[t]) atomicMin(&A.sel->bad_id, id);   // get_ref::<LightInformation>(id).unwrap() / an unwrapped field
            if (sel_e || sel_n) keep |= 1u << t;
            cj[t] += tot[t]; ce[t] += tot[3 + t];
        }
        uint64_t bk[3];
        #pragma unroll
        for (int t = 0; t < 3; t++) bk[t] = __ballot((keep >> t) & 1u);
        if (lane == 0)
#pragma unroll
            for (int t = 0; t < 3; t++) s_wc[wid][t] = (uint32_t)__popcll(bk[t]);
        __syncthreads();
        #pragma unroll
        for (int t = 0; t < 3; t++) {
            uint32_t p = 0, tt = 0;
            for (uint32_t w = 0; w < SEL_WAVES; w++) { const uint32_t v = s_wc[w][t]; tt += v; if (w < wid) p += v; }
            if ((keep >> t) & 1u) A.stage[t][cp[t] + p + lanes_below(bk[t])] = id;   // the next previous set, ascending
            cp[t] += tt;
        }
        __syncthreads();
    }
    if (tid == 0) for (int t = 0; t < 3; t++) { A.sel->n_nearby[t] = s_tot[t]; A.sel->n_slots[t] = s_tot[t] ? take[t] : 0u; A.sel->n_stage[t] = cp[t]; }
}

// a radius light's 64-byte record (A = position, radius; B = diffuse, linear; C = specular, quadratic; D = ambient), as re_lighting_set_lights writes it;
// the slots past the selection are all zeros (upload_spot_lights leaves them at their defaults, numberSpotLights = max_spot_lights)
__device__ __forceinline__ void spot_record(const WorldCommitArgs &A, uint32_t s, uint32_t n, float4 &a, float4 &b, float4 &c, float4 &d) {
    a = b = c = d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= n) return;
    const uint32_t li = A.slot_li[2][s], r = A.rows[li];
    const re_light_information &I = A.info[li];
    a = make_float4(A.pos[(size_t)r * 3], A.pos[(size_t)r * 3 + 1], A.pos[(size_t)r * 3 + 2], I.radius);
    b = make_float4(I.diffuse[0], I.diffuse[1], I.diffuse[2], I.linear);
    c = make_float4(I.specular[0], I.specular[1], I.specular[2], I.quadratic);
    d = make_float4(I.ambient[0], I.ambient[1], I.ambient[2], I.ambient[3]);
}

__global__ __launch_bounds__(WL_THREADS) void k_world_commit(WorldCommitArgs A) {
    __shared__ uint32_t s_hist[LIGHT_BUCKETS + 1u], s_fill[LIGHT_BUCKETS], s_wt[WL_WAVES], s_axis;
    __shared__ uint16_t s_b[WL_LDS_BUCKETS];
    __shared__ float s_red[WL_WAVES][7], s_par[3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    uint32_t nn[3], ns[3], nst[3];
    #pragma unroll
    for (int t = 0; t < 3; t++) { nn[t] = A.sel->n_nearby[t]; ns[t] = A.sel->n_slots[t]; nst[t] = A.sel->n_stage[t]; }
    // previous_t := the lights taken, for the types that found any (a type without nearby lights returns before it clears its set)
    #pragma unroll
    for (int t = 0; t < 3; t++) if (nn[t]) {
        for (uint32_t k = tid; k < nst[t]; k += WL_THREADS) A.prev[t][k] = A.stage[t][k];
        if (tid == 0) A.sel->n_prev[t] = nst[t];
    }
    if (tid == 0) {
        LightParams *P = A.params;
        P->cam[0] = A.cam[0]; P->cam[1] = A.cam[1]; P->cam[2] = A.cam[2]; P->cutoff = A.cutoff; P->default_diffuse = A.default_diffuse;
        P->any_visible = (nn[0] || nn[1] || nn[2]) ? 1u : 0u;               // anyLightSourceVisible: the OR of the three uploads, directional included
    }
    // cone lights (upload_point_lights :752-780): numberPointLights = N
    if (nn[1]) {
        for (uint32_t s = tid; s < ns[1]; s += WL_THREADS) {
            const uint32_t li = A.slot_li[1][s], r = A.rows[li];
            const re_light_information &I = A.info[li];
            float4 *o = A.point + (size_t)s * 6;
            o[0] = make_float4(A.pos[(size_t)r * 3], A.pos[(size_t)r * 3 + 1], A.pos[(size_t)r * 3 + 2], 0.f);
            o[1] = make_float4(I.diffuse[0], I.diffuse[1], I.diffuse[2], I.linear);
            o[2] = make_float4(I.specular[0], I.specular[1], I.specular[2], I.quadratic);
            o[3] = make_float4(I.ambient[0], I.ambient[1], I.ambient[2], I.ambient[3]);
            const float *d = I.direction; const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);     // normalize(pointLightDirection[i]), as re_lighting_set_lights
            o[4] = make_float4(d[0] / n, d[1] / n, d[2] / n, 0.f);
            o[5] = make_float4(I.cutoff, I.outer_cutoff, 0.f, 0.f);
        }
        if (tid == 0) A.params->n_point = ns[1];
    }
    if (!nn[2]) return;                                                       // (uniform)
    // radius lights (upload_spot_lights :814-839): all max_spot_lights slots, then the slab table exactly as re_lighting_set_lights builds it
    const uint32_t M = A.max_spot, N = ns[2];
    float mn[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, mx[3] = { -3.4e38f, -3.4e38f, -3.4e38f }, rm = 0.0f;
    for (uint32_t s = tid; s < M; s += WL_THREADS) {
        float4 a, b, c, d; spot_record(A, s, N, a, b, c, d);
        const float v[3] = { a.x, a.y, a.z };
        #pragma unroll
        for (int k = 0; k < 3; k++) { if (v[k] < mn[k]) mn[k] = v[k]; if (v[k] > mx[k]) mx[k] = v[k]; }   // (comparisons: NaN takes no part, as on the host)
        if (!(a.w <= rm)) rm = a.w == a.w ? a.w : __builtin_inff();            // (a NaN radius reaches everything: the slab reach becomes unbounded, as on the host)
    }
    for (int d = 32; d >= 1; d >>= 1)
        #pragma unroll
        for (int k = 0; k < 3; k++) {
            const float o1 = __shfl_xor(mn[k], d, 64), o2 = __shfl_xor(mx[k], d, 64); if (o1 < mn[k]) mn[k] = o1; if (o2 > mx[k]) mx[k] = o2;
            if (k == 0) { const float o3 = __shfl_xor(rm, d, 64); if (o3 > rm) rm = o3; }
        }
    if (lane == 0) { for (int k = 0; k < 3; k++) { s_red[wid][k] = mn[k]; s_red[wid][3 + k] = mx[k]; } s_red[wid][6] = rm; }
    for (uint32_t b = tid; b < LIGHT_BUCKETS + 1u; b += WL_THREADS) s_hist[b] = 0u;
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < WL_WAVES; w++) {
            #pragma unroll
            for (int k = 0; k < 3; k++) { if (s_red[w][k] < mn[k]) mn[k] = s_red[w][k]; if (s_red[w][3 + k] > mx[k]) mx[k] = s_red[w][3 + k]; }
            if (s_red[w][6] > rm) rm = s_red[w][6];
        }
        uint32_t axis = 0; float kmin = 0.0f, inv_w = 0.0f, best = -1.0f;
        #pragma unroll
        for (int k = 0; k < 3; k++) { const float e = mx[k] - mn[k]; if (e > best && e < 3.0e38f) { best = e; axis = (uint32_t)k; } }
        if (best > 0.0f) { kmin = mn[axis]; inv_w = (float)LIGHT_BUCKETS / best; if (!(inv_w < 3.0e38f)) inv_w = 0.0f; }
        s_axis = axis; s_par[0] = kmin; s_par[1] = inv_w; s_par[2] = rm;
        A.params->n_spot = M; A.params->axis = axis; A.params->kmin = kmin; A.params->inv_w = inv_w; A.params->rmax = rm;
    }
    __syncthreads();
    const uint32_t axis = s_axis; const float kmin = s_par[0], inv_w = s_par[1];
    for (uint32_t s = tid; s < M; s += WL_THREADS) {
        float4 a, b, c, d; spot_record(A, s, N, a, b, c, d);
        const uint32_t bk = light_bucket(axis == 0 ? a.x : (axis == 1 ? a.y : a.z), kmin, inv_w);
        atomicAdd(&s_hist[bk + 1u], 1u);
        if (s < WL_LDS_BUCKETS) s_b[s] = (uint16_t)bk; else A.place[s] = bk;
    }
    __syncthreads();
    // slab starts: inclusive prefix over s_hist[1 .. LIGHT_BUCKETS] (four entries per thread, then across the lanes and the waves)
    static_assert(LIGHT_BUCKETS == 4u * WL_THREADS, "four slabs per thread");
    uint32_t v[4], run = 0;
    #pragma unroll
    for (int k = 0; k < 4; k++) { run += s_hist[1u + 4u * tid + k]; v[k] = run; }
    uint32_t incl = run;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= (uint32_t)d) incl += o; }
    if (lane == 63) s_wt[wid] = incl;
    __syncthreads();
    uint32_t off = incl - run;
    for (uint32_t w = 0; w < wid; w++) off += s_wt[w];
    #pragma unroll
    for (int k = 0; k < 4; k++) s_hist[1u + 4u * tid + k] = off + v[k];
    __syncthreads();
    for (uint32_t b = tid; b < LIGHT_BUCKETS + 1u; b += WL_THREADS) { A.slab[b] = s_hist[b]; if (b < LIGHT_BUCKETS) s_fill[b] = s_hist[b]; }
    __syncthreads();
    // stable placement (ascending slot index inside a slab): one wave walks the slots 64 at a time; the lanes of one slab find each other with 12 ballots
    if (wid == 0) {
        for (uint32_t base = 0; base < M; base += 64u) {
            const uint32_t s = base + lane; const bool valid = s < M;
            const uint32_t bk = valid ? (s < WL_LDS_BUCKETS ? (uint32_t)s_b[s] : A.place[s]) : 0u;
            uint64_t peers = __ballot(valid);
            #pragma unroll
            for (int bit = 0; bit < 12; bit++) { const bool on = (bk >> bit) & 1u; const uint64_t bb = __ballot(on); peers &= on ? bb : ~bb; }
            static_assert(LIGHT_BUCKETS <= 4096u, "12 bits of slab index");
            const uint32_t f = valid ? s_fill[bk] : 0u;
            if (valid) {
                A.place[s] = f + lanes_below(peers);
                if ((peers >> lane) == 1ull) s_fill[bk] = f + (uint32_t)__popcll(peers);   // the slab's last lane of this step advances its fill
            }
        }
    }
    __syncthreads();
    for (uint32_t s = tid; s < M; s += WL_THREADS) {
        float4 a, b, c, d; spot_record(A, s, N, a, b, c, d);
        float4 *o = A.spot + (size_t)A.place[s] * 4;
        o[0] = a; o[1] = b; o[2] = c; o[3] = d;
    }
}
}  // namespace

struct re_lighting {
    re_lighting_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    float4 *d_pos = nullptr, *d_nrm = nullptr, *d_out = nullptr, *d_spot = nullptr, *d_point = nullptr; uchar4 *d_alb = nullptr; uint32_t *d_slab = nullptr;
    LightParams P{};
    // from-world uploads: K5 reads its light parameters from d_params after one (dev_params), from P after re_lighting_set_lights.  The previous sets of the three
    // types (ascending ids) and the selection scratch; cap[t] = slots of type t (max_directional_lights grows with the largest one asked for)
    LightParams *d_params = nullptr; bool dev_params = false;
    WorldSel *d_sel = nullptr;
    uint32_t *d_prev[3] = {}, *d_stage[3] = {}, *d_slot_li[3] = {}, *d_slot_id[3] = {}, cap[3] = {};
    uint32_t *d_lmask = nullptr, lmask_cap = 0, *d_place = nullptr;
    hipEvent_t ev_world = nullptr;
    std::vector<uint32_t> h_slot_ids[3];
    int fail(int code, const char *fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); err = buf; return code; }
};
static thread_local std::string g_lt_error;
#define LCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (ctx)->fail(RE_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

extern "C" const char *re_lighting_last_error(const re_lighting *l) { return l ? l->err.c_str() : g_lt_error.c_str(); }

extern "C" int re_lighting_create(const re_lighting_config *cfg, re_lighting **out) try {
    if (!cfg || !out || !cfg->width || !cfg->height) { g_lt_error = "re_lighting_create: bad argument"; return RE_E_ARG; }
    int ndev = 0; hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) { g_lt_error = std::string("re_lighting_create: no HIP device (") + hipGetErrorString(e) + "); no CPU path"; return RE_E_HIP; }
    if (cfg->device < 0 || cfg->device >= ndev) { g_lt_error = "re_lighting_create: device ordinal out of range"; return RE_E_ARG; }
    re_lighting *l = new re_lighting(); l->cfg = *cfg;
    size_t np = (size_t)cfg->width * cfg->height;
    if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&l->d_pos, np * 16) != hipSuccess || hipMalloc(&l->d_nrm, np * 16) != hipSuccess || hipMalloc(&l->d_out, np * 16) != hipSuccess || hipMalloc(&l->d_alb, np * 4) != hipSuccess ||
        hipMalloc(&l->d_spot, (size_t)(cfg->max_spot_lights + 1) * 64) != hipSuccess || hipMalloc(&l->d_slab, (size_t)(LIGHT_BUCKETS + 1u) * 4) != hipSuccess || hipMalloc(&l->d_point, (size_t)(cfg->max_point_lights + 1) * 96) != hipSuccess) {
        g_lt_error = "re_lighting_create: device allocation failed"; delete l; return RE_E_HIP;
    }
    l->P.width = cfg->width; l->P.height = cfg->height;
    *out = l; return RE_OK;
} RE_ABI_GUARD_NOCTX(g_lt_error, "re_lighting_create")
extern "C" void re_lighting_destroy(re_lighting *l) try {
    if (!l) return;
    (void)hipSetDevice(l->cfg.device);
    if (l->stream) (void)hipStreamSynchronize(l->stream);
    (void)hipFree(l->d_pos); (void)hipFree(l->d_nrm); (void)hipFree(l->d_out); (void)hipFree(l->d_alb); (void)hipFree(l->d_spot); (void)hipFree(l->d_point); (void)hipFree(l->d_slab);
    (void)hipFree(l->d_params); (void)hipFree(l->d_sel); (void)hipFree(l->d_lmask); (void)hipFree(l->d_place);
    for (int t = 0; t < 3; t++) { (void)hipFree(l->d_prev[t]); (void)hipFree(l->d_stage[t]); (void)hipFree(l->d_slot_li[t]); (void)hipFree(l->d_slot_id[t]); }
    if (l->ev_world) (void)hipEventDestroy(l->ev_world);
    if (l->stream) (void)hipStreamDestroy(l->stream);
    delete l;
} catch (...) {}
extern "C" int re_lighting_upload_gbuffer(re_lighting *l, const float *g_position, const float *g_normal, const uint8_t *g_albedo_spec) try {
    if (!l || !g_position || !g_normal || !g_albedo_spec) return RE_E_ARG;
    LCHK(l, hipSetDevice(l->cfg.device));
    size_t np = (size_t)l->cfg.width * l->cfg.height;
    LCHK(l, hipMemcpyAsync(l->d_pos, g_position, np * 16, hipMemcpyHostToDevice, l->stream));
    LCHK(l, hipMemcpyAsync(l->d_nrm, g_normal, np * 16, hipMemcpyHostToDevice, l->stream));
    LCHK(l, hipMemcpyAsync(l->d_alb, g_albedo_spec, np * 4, hipMemcpyHostToDevice, l->stream));
    LCHK(l, hipStreamSynchronize(l->stream));
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_upload_gbuffer")
extern "C" int re_lighting_set_lights(re_lighting *l, const re_lights *L) try {
    if (!l || !L) return RE_E_ARG;
    if (L->n_spot > l->cfg.max_spot_lights || L->n_point > l->cfg.max_point_lights) return l->fail(RE_E_CAPACITY, "more lights than configured");
    LCHK(l, hipSetDevice(l->cfg.device));
    std::vector<float> s((size_t)L->n_spot * 16), p((size_t)L->n_point * 24);
    // the radius lights go to the device in slab order along the axis of their largest extent (see k_deferred_lighting): counting sort by light_bucket,
    // ascending light index inside a slab
    uint32_t axis = 0; float kmin = 0.0f, inv_w = 0.0f, rmax = 0.0f;
    std::vector<uint32_t> slab_start(LIGHT_BUCKETS + 1u, 0u), place(L->n_spot);
    {
        float mn[3] = { 3.4e38f, 3.4e38f, 3.4e38f }, mx[3] = { -3.4e38f, -3.4e38f, -3.4e38f };
        for (uint32_t i = 0; i < L->n_spot; i++) {
            for (int k = 0; k < 3; k++) { const float v = L->spot_pos[3 * i + k]; if (v < mn[k]) mn[k] = v; if (v > mx[k]) mx[k] = v; }   // (comparisons with NaN are false: it takes no part)
            const float r = L->spot_radius[i];
            if (!(r <= rmax)) rmax = r == r ? r : __builtin_inff();                                                                            // (a NaN radius lights every pixel in the oracle: unbounded reach)
        }
        float best = -1.0f;
        for (int k = 0; k < 3; k++) { const float e = mx[k] - mn[k]; if (e > best && e < 3.0e38f) { best = e; axis = (uint32_t)k; } }
        if (best > 0.0f) { kmin = mn[axis]; inv_w = (float)LIGHT_BUCKETS / best; if (!(inv_w < 3.0e38f)) inv_w = 0.0f; }                // (all lights at one coordinate, or an extent too small to divide by: one slab)
        for (uint32_t i = 0; i < L->n_spot; i++) slab_start[light_bucket(L->spot_pos[3 * i + axis], kmin, inv_w) + 1u]++;
        for (uint32_t b = 0; b < LIGHT_BUCKETS; b++) slab_start[b + 1u] += slab_start[b];
        std::vector<uint32_t> fill(slab_start.begin(), slab_start.end() - 1);
        for (uint32_t i = 0; i < L->n_spot; i++) place[i] = fill[light_bucket(L->spot_pos[3 * i + axis], kmin, inv_w)]++;
    }
    for (uint32_t i = 0; i < L->n_spot; i++) {
        float *o = &s[(size_t)place[i] * 16];
        o[0] = L->spot_pos[3 * i]; o[1] = L->spot_pos[3 * i + 1]; o[2] = L->spot_pos[3 * i + 2]; o[3] = L->spot_radius[i];
        o[4] = L->spot_diffuse[3 * i]; o[5] = L->spot_diffuse[3 * i + 1]; o[6] = L->spot_diffuse[3 * i + 2]; o[7] = L->spot_linear[i];
        o[8] = L->spot_specular[3 * i]; o[9] = L->spot_specular[3 * i + 1]; o[10] = L->spot_specular[3 * i + 2]; o[11] = L->spot_quadratic[i];
        o[12] = L->spot_ambient[4 * i]; o[13] = L->spot_ambient[4 * i + 1]; o[14] = L->spot_ambient[4 * i + 2]; o[15] = L->spot_ambient[4 * i + 3];
    }
    for (uint32_t i = 0; i < L->n_point; i++) {
        float *o = &p[(size_t)i * 24];
        o[0] = L->point_pos[3 * i]; o[1] = L->point_pos[3 * i + 1]; o[2] = L->point_pos[3 * i + 2]; o[3] = 0.f;
        o[4] = L->point_diffuse[3 * i]; o[5] = L->point_diffuse[3 * i + 1]; o[6] = L->point_diffuse[3 * i + 2]; o[7] = L->point_linear[i];
        o[8] = L->point_specular[3 * i]; o[9] = L->point_specular[3 * i + 1]; o[10] = L->point_specular[3 * i + 2]; o[11] = L->point_quadratic[i];
        o[12] = L->point_ambient[4 * i]; o[13] = L->point_ambient[4 * i + 1]; o[14] = L->point_ambient[4 * i + 2]; o[15] = L->point_ambient[4 * i + 3];
        const float *d = L->point_dir + 3 * i; float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);     // normalize(pointLightDirection[i])
        o[16] = d[0] / n; o[17] = d[1] / n; o[18] = d[2] / n; o[19] = 0.f;
        o[20] = L->point_cutoff[i]; o[21] = L->point_outer_cutoff[i]; o[22] = o[23] = 0.f;
    }
    if (L->n_spot) LCHK(l, hipMemcpyAsync(l->d_spot, s.data(), s.size() * 4, hipMemcpyHostToDevice, l->stream));
    if (L->n_point) LCHK(l, hipMemcpyAsync(l->d_point, p.data(), p.size() * 4, hipMemcpyHostToDevice, l->stream));
    LCHK(l, hipMemcpyAsync(l->d_slab, slab_start.data(), slab_start.size() * 4, hipMemcpyHostToDevice, l->stream));
    LCHK(l, hipStreamSynchronize(l->stream));
    l->P.n_spot = L->n_spot; l->P.n_point = L->n_point; l->P.axis = axis; l->P.kmin = kmin; l->P.inv_w = inv_w; l->P.rmax = rmax;
    for (int k = 0; k < 3; k++) l->P.cam[k] = L->camera_pos[k];
    l->P.cutoff = L->no_light_source_cutoff; l->P.default_diffuse = L->default_diffuse_factor; l->P.any_visible = L->any_light_source_visible;
    l->dev_params = false;
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_set_lights")
extern "C" int re_lighting_run(re_lighting *l, float *kernel_us) try {
    if (!l) return RE_E_ARG;
    LCHK(l, hipSetDevice(l->cfg.device));
    hipEvent_t a = nullptr, b = nullptr;
    if (kernel_us) { LCHK(l, hipEventCreate(&a)); LCHK(l, hipEventCreate(&b)); }
    dim3 grid((l->cfg.width + TILE - 1) / TILE, (l->cfg.height + TILE_H - 1) / TILE_H);
    if (l->dev_params) hipExtLaunchKernelGGL(k_deferred_lighting<true>, grid, dim3(LT_THREADS), 0, l->stream, a, b, 0, l->P, l->d_pos, l->d_nrm, l->d_alb, l->d_spot, l->d_slab, l->d_point, l->d_out,
                                             (const LightParams *)l->d_params);
    else hipExtLaunchKernelGGL(k_deferred_lighting<false>, grid, dim3(LT_THREADS), 0, l->stream, a, b, 0, l->P, l->d_pos, l->d_nrm, l->d_alb, l->d_spot, l->d_slab, l->d_point, l->d_out,
                               (const LightParams *)nullptr);
    LCHK(l, hipGetLastError());
    LCHK(l, hipStreamSynchronize(l->stream));
    if (kernel_us) { float ms = 0; LCHK(l, hipEventElapsedTime(&ms, a, b)); *kernel_us = ms * 1000.f; (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_run")
extern "C" int re_lighting_read(re_lighting *l, float *out_rgba) try {
    if (!l || !out_rgba) return RE_E_ARG;
    LCHK(l, hipSetDevice(l->cfg.device));
    LCHK(l, hipMemcpy(out_rgba, l->d_out, (size_t)l->cfg.width * l->cfg.height * 16, hipMemcpyDeviceToHost));
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_read")
extern "C" int re_lighting_read_pixels(re_lighting *l, const uint32_t *idx, uint32_t n, float *out_rgba) try {
    if (!l || !idx || !out_rgba) return RE_E_ARG;
    LCHK(l, hipSetDevice(l->cfg.device));
    uint32_t *d_idx = nullptr; float4 *d_o = nullptr;
    LCHK(l, hipMalloc(&d_idx, (size_t)n * 4 + 4)); LCHK(l, hipMalloc(&d_o, (size_t)n * 16 + 16));
    LCHK(l, hipMemcpy(d_idx, idx, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gather_pixels, dim3((n + 255) / 256), dim3(256), 0, l->stream, l->d_out, d_idx, n, d_o);
    LCHK(l, hipStreamSynchronize(l->stream));
    LCHK(l, hipMemcpy(out_rgba, d_o, (size_t)n * 16, hipMemcpyDeviceToHost));
    (void)hipFree(d_idx); (void)hipFree(d_o);
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_read_pixels")

// the device buffers of the from-world path, allocated on first use; the directional slots grow with max_directional_lights (the previous set is kept)
static int world_buffers(re_lighting *l, uint32_t max_dir, uint32_t nl) {
    auto grow = [&](uint32_t **p, size_t words, size_t keep) -> hipError_t {
        uint32_t *q = nullptr; hipError_t e = hipMalloc(reinterpret_cast<void **>(&q), words * 4);
        if (e != hipSuccess) return e;
        if (keep && *p) { e = hipMemcpy(q, *p, keep * 4, hipMemcpyDeviceToDevice); if (e != hipSuccess) { (void)hipFree(q); return e; } }
        (void)hipFree(*p); *p = q; return hipSuccess;
    };
    if (!l->d_sel) {
        LCHK(l, hipMalloc(reinterpret_cast<void **>(&l->d_sel), sizeof(WorldSel))); LCHK(l, hipMemset(l->d_sel, 0, sizeof(WorldSel)));
        LCHK(l, hipMalloc(reinterpret_cast<void **>(&l->d_params), sizeof(LightParams)));
        LCHK(l, hipMalloc(reinterpret_cast<void **>(&l->d_place), ((size_t)l->cfg.max_spot_lights + 1) * 4));
        LCHK(l, hipEventCreateWithFlags(&l->ev_world, hipEventDisableTiming));
        const uint32_t caps[3] = { 0, l->cfg.max_point_lights, l->cfg.max_spot_lights };
        for (int t = 1; t < 3; t++) {
            const size_t w = (size_t)caps[t] + 1;
            LCHK(l, grow(&l->d_prev[t], w, 0)); LCHK(l, grow(&l->d_stage[t], w, 0)); LCHK(l, grow(&l->d_slot_li[t], w, 0)); LCHK(l, grow(&l->d_slot_id[t], w, 0));
            l->cap[t] = caps[t];
        }
    }
    if (!l->d_prev[0] || max_dir > l->cap[0]) {
        const size_t w = (size_t)max_dir + 1;
        LCHK(l, grow(&l->d_prev[0], w, l->d_prev[0] ? (size_t)l->cap[0] : 0)); LCHK(l, grow(&l->d_stage[0], w, 0)); LCHK(l, grow(&l->d_slot_li[0], w, 0)); LCHK(l, grow(&l->d_slot_id[0], w, 0));
        l->cap[0] = max_dir;
    }
    if (nl > l->lmask_cap || !l->d_lmask) { (void)hipFree(l->d_lmask); l->d_lmask = nullptr; LCHK(l, hipMalloc(reinterpret_cast<void **>(&l->d_lmask), ((size_t)nl + 1) * 4)); l->lmask_cap = nl; }
    return RE_OK;
}

// the previous sets for the shadow flow (re_world_lights.h)
void re::lighting_prev(const re_lighting *l, LightingPrev *p) {
    p->device = l->cfg.device;
    p->n_prev = l->d_sel ? l->d_sel->n_prev : nullptr;
    for (int t = 0; t < 3; t++) p->prev[t] = l->d_sel ? l->d_prev[t] : nullptr;
}

extern "C" int re_lighting_set_lights_from_world(re_lighting *l, re_ctx *c, const re_camera *cam, const re_world_light_args *a, re_world_lights *out) try {
    if (!l) return RE_E_ARG;
    if (!c || !cam || !a) return l->fail(RE_E_ARG, "re_lighting_set_lights_from_world: NULL argument");
    // what each type unwraps besides get_ref::<LightInformation>: direction (directional, :700-720), direction, fov, cutoff and outer cutoff (point, :752-780)
    static const uint32_t need[3] = { re::LI_HAS | RE_LI_DIRECTION, re::LI_HAS | RE_LI_CUTOFF | RE_LI_OUTER_CUTOFF | RE_LI_DIRECTION | RE_LI_FOV, re::LI_HAS };
    re::WorldLightsView V;
    { const int rc = re::world_lights_view(c, l->cfg.device, cam, need, &V, &l->err); if (rc != RE_OK) return rc; }
    LCHK(l, hipSetDevice(l->cfg.device));
    { const int rc = world_buffers(l, a->max_directional_lights, V.nl); if (rc != RE_OK) return rc; }
    const uint32_t maxs[3] = { a->max_directional_lights, l->cfg.max_point_lights, l->cfg.max_spot_lights };
    WorldSelArgs S{};
    S.nl = V.nl; S.rows = V.light_rows; S.flags = V.flags; S.row_id = V.row_id; S.row_cell = V.row_cell; S.cell_key = V.cell_key; S.cell_flags = V.cell_flags; S.sh_cells = V.sh_cells;
    S.info = V.info; S.lmask = l->d_lmask; S.sel = l->d_sel;
    for (int t = 0; t < 3; t++) { S.max[t] = maxs[t]; S.need[t] = need[t]; S.prev[t] = l->d_prev[t]; S.stage[t] = l->d_stage[t]; S.slot_li[t] = l->d_slot_li[t]; S.slot_id[t] = l->d_slot_id[t]; }
    hipLaunchKernelGGL(k_world_select, dim3(1), dim3(SEL_THREADS), 0, V.stream, S, V.Q);
    LCHK(l, hipGetLastError());
    WorldSel h{};
    if (!(V.complete[0] && V.complete[1] && V.complete[2])) {                 // some light lacks what its type unwraps: is one of them selected?
        LCHK(l, hipMemcpyAsync(&h, l->d_sel, sizeof h, hipMemcpyDeviceToHost, V.stream)); LCHK(l, hipStreamSynchronize(V.stream));
        if (h.bad_id != 0xFFFFFFFFu)
            return l->fail(RE_E_STATE, "re_lighting_set_lights_from_world: light entity %u is selected but lacks LightInformation or a field its type unwraps (the reference panics)", h.bad_id);
    }
    if (!l->dev_params) LCHK(l, hipMemcpyAsync(l->d_params, &l->P, sizeof(LightParams), hipMemcpyHostToDevice, V.stream));   // a type without nearby lights keeps what set_lights uploaded
    WorldCommitArgs W{};
    W.sel = l->d_sel; W.rows = V.light_rows; W.pos = V.pos; W.info = V.info; W.max_spot = l->cfg.max_spot_lights;
    for (int t = 0; t < 3; t++) { W.slot_li[t] = l->d_slot_li[t]; W.stage[t] = l->d_stage[t]; W.prev[t] = l->d_prev[t]; W.cam[t] = cam->position[t]; }
    W.cutoff = a->no_light_source_cutoff; W.default_diffuse = a->default_diffuse_factor;
    W.spot = l->d_spot; W.slab = l->d_slab; W.point = l->d_point; W.params = l->d_params; W.place = l->d_place;
    hipLaunchKernelGGL(k_world_commit, dim3(1), dim3(WL_THREADS), 0, V.stream, W);
    LCHK(l, hipGetLastError());
    LCHK(l, hipEventRecord(l->ev_world, V.stream));
    LCHK(l, hipStreamWaitEvent(l->stream, l->ev_world, 0));                   // re_lighting_run is ordered behind the upload
    l->dev_params = true;
    if (out) {
        LCHK(l, hipMemcpyAsync(&h, l->d_sel, sizeof h, hipMemcpyDeviceToHost, V.stream)); LCHK(l, hipStreamSynchronize(V.stream));
        out->any_light_source_visible = (h.n_nearby[0] || h.n_nearby[1] || h.n_nearby[2]) ? 1u : 0u;
        for (int t = 0; t < 3; t++) {
            out->n_nearby[t] = h.n_nearby[t]; out->n_slots[t] = h.n_slots[t];
            l->h_slot_ids[t].resize(h.n_slots[t]);
            if (h.n_slots[t]) LCHK(l, hipMemcpy(l->h_slot_ids[t].data(), l->d_slot_id[t], (size_t)h.n_slots[t] * 4, hipMemcpyDeviceToHost));
            out->slot_ids[t] = h.n_slots[t] ? l->h_slot_ids[t].data() : nullptr;
        }
    }
    return RE_OK;
} RE_ABI_GUARD(l, "re_lighting_set_lights_from_world")
