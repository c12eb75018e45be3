// Tree queries for user logic on the resident world, for gfx950: the entities along each segment of a batch -- a shot, a line of sight, a pick ray; the
// other question a LogicFunction / CollisionFunction / UserInputLogicFunction of the reference asks of its &BoundingBoxTree (re_boxquery.hip answers "who
// is near this box").
//
// The rule: (query i, entity, t_enter, t_exit) for every entity re_query_boxes would consider (live, in the tree, no F_PHANTOM replica, no ghost instance,
// the flag filter) other than the segment's excluded one whose stored, unclipped StaticAABB is met by the segment p0 + t * d, t in [0, 1], by the slab
// test below: plain f32, IEEE division, closed intervals, d == 0 on an axis a containment test.  Each pair once; tests/segment_rule.py restates it.
//
// The walk is the box query's over the segment's bounding box (inflated by the margin), with one test more in front of every
// probe: a candidate cell is looked up only when the segment meets the cell's own box -- inflated by the margin, and open-ended on an axis where the
// cell lies on a face of the world, because entities clipped to the world sit there and the exact test runs on unclipped boxes.
//   unique sections: one workgroup per segment enumerates the candidate cells of every level, prunes, looks the remaining keys up (rb_find) and walks the
//     rows of the sections that exist, one wave per section, one lane per row;
//   shared sections: workgroups behind the first n hold 256 shared sections each, one per lane, against a tile of segments in LDS -- a shared section is
//     walked once for a segment when ANY of its linked keys lies in the range of its level and the segment meets the bounding cell box of the linked
//     keys (inflated, open-ended as above), by the lane that owns it.  O(shared sections x segments) integer tests, as the box query's.
#include "re_kernels.h"

namespace re {

namespace {

__device__ __forceinline__ uint32_t segq_mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// one axis of the slab test; false: d == 0 and p outside [mn, mx]
__device__ __forceinline__ bool segq_axis(float p, float d, float mn, float mx, float &lo, float &hi) {
    if (d == 0.0f) return p >= mn && p <= mx;
    float u = (mn - p) / d, v = (mx - p) / d;
    if (u > v) { const float t = u; u = v; v = t; }
    if (u > lo) lo = u;
    if (v < hi) hi = v;
    return true;
}
// the slab test of the segment p + t * d, t in [0, 1], with a closed box (bounds may be infinite; p and d are finite, so no NaN arises)
__device__ __forceinline__ bool segq_slab(float px, float py, float pz, float dx, float dy, float dz, float x0, float x1, float y0, float y1, float z0, float z1,
                                          float &lo, float &hi) {
    lo = 0.0f; hi = 1.0f;
    if (!segq_axis(px, dx, x0, x1, lo, hi)) return false;
    if (!segq_axis(py, dy, y0, y1, lo, hi)) return false;
    if (!segq_axis(pz, dz, z0, z1, lo, hi)) return false;
    return lo <= hi;
}
// bounds of the cells [c0, c1] (world units) of one axis as the prune takes them: inflated by the margin, open-ended on a face of the world
__device__ __forceinline__ float segq_cell_min(uint32_t c0, float margin) { return c0 == 0u ? -__builtin_inff() : (float)c0 - margin; }
__device__ __forceinline__ float segq_cell_max(uint32_t c1, uint32_t outline, float margin) { return c1 >= outline ? __builtin_inff() : (float)c1 + margin; }

struct SegRec { uint32_t query, id; float t0, t1; };      // re_segment_hit

// Records are read by the host as soon as it has seen the count: write-through stores, as k_box_query's; two 8-byte halves, both below the capacity or neither
__device__ __forceinline__ void segq_store(const SegQueryArgs &A, uint32_t slot, const SegRec &r) {
    if (slot >= A.capacity) return;
    unsigned long long *o = A.out + (size_t)slot * 2u;
    __hip_atomic_store(o, (unsigned long long)r.query | ((unsigned long long)r.id << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(o + 1, (unsigned long long)__float_as_uint(r.t0) | ((unsigned long long)__float_as_uint(r.t1) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr uint32_t SEGQ_TILE_WORDS = 14;       // a segment in the LDS tile of the shared part: umin[3], umax[3], flags, p0[3], d[3], exclude

struct SegqShared {
    SegRec hits[BOXQ_HITBUF];                      // staged records
    uint32_t queue[BOXQ_TILE * SEGQ_TILE_WORDS];   // unique part: slots of the hit sections of a round; shared part: the segment tile
    uint32_t n_hits, n_queue, gbase;
    uint32_t prefix[MAX_LEVELS + 2], lo[3][MAX_LEVELS + 1], ext[3][MAX_LEVELS + 1];      // unique part: candidate cells before each level, first cell and extent per axis
    float p0[3], d[3]; uint32_t exclude;
};
static_assert(BOXQ_QUEUE <= BOXQ_TILE * SEGQ_TILE_WORDS, "the section queue shares the LDS of the segment tile");

// the staged records leave: ONE global atomicAdd per workgroup and flush.  Called by all 256 threads.
__device__ __forceinline__ void segq_flush(const SegQueryArgs &A, SegqShared &S) {
    __syncthreads();
    const uint32_t n = S.n_hits < BOXQ_HITBUF ? S.n_hits : BOXQ_HITBUF;
    if (n == 0u) return;                                                   // (uniform)
    if (threadIdx.x == 0) S.gbase = atomicAdd(&A.hdr->count, n);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += BOXQ_THREADS) segq_store(A, S.gbase + k, S.hits[k]);
    __syncthreads();
    if (threadIdx.x == 0) S.n_hits = 0u;
    __syncthreads();
}

// does the row belong to the rule for this segment?  expect: the row_cell word of a member of the section being walked
__device__ __forceinline__ bool segq_row_hit(const SegQueryArgs &A, uint32_t r, uint32_t expect, uint32_t exclude, float px, float py, float pz, float dx, float dy, float dz,
                                             SegRec &rec) {
    if (r >= A.nrows) return false;                                        // (ghost instances live beyond the entity rows)
    const uint32_t fl = A.row_flags[r], rc = A.row_cell[r];
    if ((fl & (F_DEAD | F_PHANTOM)) || rc != expect || (fl & A.need) != A.need || (fl & A.forbid)) return false;
    const Aabb a = A.row_aabb[r];
    rec.id = A.row_id[r];
    if (rec.id == exclude) return false;
    return segq_slab(px, py, pz, dx, dy, dz, a.xmin, a.xmax, a.ymin, a.ymax, a.zmin, a.zmax, rec.t0, rec.t1);
}

// one wave walks rows[begin .. begin + cnt): one lane per row, ballot + mbcnt compaction into the workgroup's staging buffer
__device__ __forceinline__ void segq_walk_wave(const SegQueryArgs &A, SegqShared &S, uint32_t query, uint32_t begin, uint32_t cnt, uint32_t expect) {
    const uint32_t lane = threadIdx.x & 63u;
    const float px = S.p0[0], py = S.p0[1], pz = S.p0[2], dx = S.d[0], dy = S.d[1], dz = S.d[2];
    const uint32_t exclude = S.exclude;
    for (uint32_t base = 0; base < cnt; base += 64u) {                     // (wave-uniform trip count)
        const uint32_t k = base + lane;
        SegRec rec = { query, 0u, 0.0f, 0.0f };
        bool hit = false;
        if (k < cnt) hit = segq_row_hit(A, A.rows[begin + k], expect, exclude, px, py, pz, dx, dy, dz, rec);
        const uint64_t mask = __ballot(hit);
        if (!mask) continue;
        uint32_t pos = 0;
        if (lane == 0u) pos = atomicAdd(&S.n_hits, (uint32_t)__popcll(mask));
        pos = __shfl(pos, 0) + segq_mbcnt(mask);
        if (hit && pos < BOXQ_HITBUF) S.hits[pos] = rec;
        const uint64_t over = __ballot(hit && pos >= BOXQ_HITBUF);        // the staging buffer is full: this wave's remainder goes out directly
        if (over) {
            uint32_t g = 0;
            if (lane == 0u) g = atomicAdd(&A.hdr->count, (uint32_t)__popcll(over));
            g = __shfl(g, 0) + segq_mbcnt(over);
            if (hit && pos >= BOXQ_HITBUF) segq_store(A, g, rec);
        }
    }
}

__device__ __forceinline__ void segq_unique_part(const SegQueryArgs &A, SegqShared &S) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, query = blockIdx.x;
    const SegQuery &Q = A.q[query];
    const uint32_t nlev = A.max_level + 1u;                                // an entity longer than half the outline sits at level max_level
    if (tid < 3u) { S.p0[tid] = Q.p0[tid]; S.d[tid] = Q.d[tid]; }
    if (tid == 3u) S.exclude = Q.exclude;
    if (tid < nlev) {
        const uint32_t len = A.atomic << tid;
        for (uint32_t a = 0; a < 3u; a++) {
            uint32_t lo, hi; box_level_range(Q.umin[a], Q.umax[a], (Q.flags >> a) & 1u, len, &lo, &hi);
            S.lo[a][tid] = lo; S.ext[a][tid] = hi - lo + 1u;
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t sum = 0;
        for (uint32_t l = 0; l < nlev; l++) { S.prefix[l] = sum; sum += S.ext[0][l] * S.ext[1][l] * S.ext[2][l]; }      // (<= RE_BOX_QUERY_MAX_CELLS: the host refused the segment otherwise)
        S.prefix[nlev] = sum;
    }
    __syncthreads();
    const uint32_t total = S.prefix[nlev];
    const float px = S.p0[0], py = S.p0[1], pz = S.p0[2], dx = S.d[0], dy = S.d[1], dz = S.d[2];
    for (uint32_t base = 0; base < total; base += BOXQ_QUEUE) {            // rounds of 1024 candidate cells
        for (uint32_t j = 0; j < BOXQ_PROBES; j++) {
            const uint32_t g = base + j * BOXQ_THREADS + tid;
            if (g >= total) break;
            uint32_t l = 0;
            while (g >= S.prefix[l + 1u]) l++;                             // (l < nlev: g < prefix[nlev])
            const uint32_t idx = g - S.prefix[l], nx = S.ext[0][l], ny = S.ext[1][l];
            const uint32_t ix = idx % nx, rest = idx / nx, iy = rest % ny, iz = rest / ny;
            const uint32_t cx = S.lo[0][l] + ix, cy = S.lo[1][l] + iy, cz = S.lo[2][l] + iz, len = A.atomic << l;
            // the prune: the cell's closed box holds the clipped AABB of every entity of a unique section there
            float t0, t1;
            if (!segq_slab(px, py, pz, dx, dy, dz, segq_cell_min(cx * len, A.margin), segq_cell_max(cx * len + len, A.outline, A.margin),
                           segq_cell_min(cy * len, A.margin), segq_cell_max(cy * len + len, A.outline, A.margin),
                           segq_cell_min(cz * len, A.margin), segq_cell_max(cz * len + len, A.outline, A.margin), t0, t1)) continue;
            const uint64_t key = pack_key(l, cx, cz, cy);
            const int32_t slot = rb_find(A.T, A.cell_key, key);
            if (slot >= 0 && A.cell_nl[slot] + A.cell_ns[slot] != 0u) S.queue[atomicAdd(&S.n_queue, 1u)] = (uint32_t)slot;
        }
        __syncthreads();
        const uint32_t nq = S.n_queue;
        for (uint32_t e = wave; e < nq; e += BOXQ_THREADS / 64u) {          // one wave per hit section: active rows, then static rows; the ghost tail is not walked
            const uint32_t slot = S.queue[e];
            segq_walk_wave(A, S, query, A.cell_begin[slot], A.cell_nl[slot] + A.cell_ns[slot], slot);
        }
        segq_flush(A, S);
        if (tid == 0) S.n_queue = 0u;
        __syncthreads();
    }
}

// the cell of one linked key against one segment's bounding box: is the cell inside the range of the key's level?  (the integer form of box_level_range, re_boxquery.hip)
__device__ __forceinline__ bool segq_cell_in_range(uint32_t c0, uint32_t c1, uint32_t umin, uint32_t umax, uint32_t whole) {
    return c0 <= umax && c1 + whole > umin;
}

__device__ __forceinline__ void segq_shared_part(const SegQueryArgs &A, SegqShared &S) {
    const uint32_t tid = threadIdx.x, sb = blockIdx.x - A.n;
    const uint32_t chunk = sb % A.n_sh_chunks, q0 = (sb / A.n_sh_chunks) * BOXQ_TILE;
    const uint32_t nq = A.n - q0 < BOXQ_TILE ? A.n - q0 : BOXQ_TILE;
    uint32_t *tile = S.queue;
    if (tid < nq) {
        const SegQuery &Q = A.q[q0 + tid];
        uint32_t *t = tile + tid * SEGQ_TILE_WORDS;
        for (uint32_t a = 0; a < 3u; a++) { t[a] = Q.umin[a]; t[3u + a] = Q.umax[a]; t[7u + a] = __float_as_uint(Q.p0[a]); t[10u + a] = __float_as_uint(Q.d[a]); }
        t[6] = Q.flags; t[13] = Q.exclude;
    }
    __syncthreads();
    const uint32_t s = chunk * BOXQ_THREADS + tid;
    const uint32_t nk = s < A.nsh ? A.sh_nk[s] : 0u;                        // holes: nk == 0
    const uint32_t cnt = nk ? A.sh_nact[s] + A.sh_nstat[s] : 0u;
    if (cnt) {
        uint64_t keys[8];
#pragma unroll
        for (int k = 0; k < 8; k++) keys[k] = A.sh_keys[(size_t)s * 8u + k];
        // the bounding cell box of the linked keys, in world units: most (segment, shared section) pairs end at its integer test, the rest at its prune
        uint32_t b0[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, b1[3] = { 0u, 0u, 0u };
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)k < nk) {
                const uint32_t len = A.atomic << key_level(keys[k]);
                const uint32_t c[3] = { key_x(keys[k]) * len, key_y(keys[k]) * len, key_z(keys[k]) * len };
#pragma unroll
                for (int a = 0; a < 3; a++) { b0[a] = c[a] < b0[a] ? c[a] : b0[a]; b1[a] = c[a] + len > b1[a] ? c[a] + len : b1[a]; }
            }
        const float bx0 = segq_cell_min(b0[0], A.margin), bx1 = segq_cell_max(b1[0], A.outline, A.margin);
        const float by0 = segq_cell_min(b0[1], A.margin), by1 = segq_cell_max(b1[1], A.outline, A.margin);
        const float bz0 = segq_cell_min(b0[2], A.margin), bz1 = segq_cell_max(b1[2], A.outline, A.margin);
        // the first member (most shared sections hold one entity) is fetched ONCE, in front of the loop over the segments
        const uint32_t begin = A.sh_begin[s], expect = ROW_CELL_SHARED | s;
        const uint32_t r0 = A.rows[begin];
        bool live0 = false; Aabb a0 = {}; uint32_t id0 = 0;
        if (r0 < A.nrows) {
            const uint32_t fl = A.row_flags[r0], rc = A.row_cell[r0];
            live0 = !(fl & (F_DEAD | F_PHANTOM)) && rc == expect && (fl & A.need) == A.need && !(fl & A.forbid);
            a0 = A.row_aabb[r0]; id0 = A.row_id[r0];
        }
        for (uint32_t i = 0; i < nq; i++) {
            const uint32_t *t = tile + i * SEGQ_TILE_WORDS;
            const uint32_t fl = t[6];
            if (!(segq_cell_in_range(b0[0], b1[0], t[0], t[3], fl & 1u) && segq_cell_in_range(b0[1], b1[1], t[1], t[4], (fl >> 1) & 1u) &&
                  segq_cell_in_range(b0[2], b1[2], t[2], t[5], (fl >> 2) & 1u))) continue;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if ((uint32_t)k < nk) {
                    const uint32_t len = A.atomic << key_level(keys[k]);
                    const uint32_t cx = key_x(keys[k]) * len, cy = key_y(keys[k]) * len, cz = key_z(keys[k]) * len;
                    any = any || (segq_cell_in_range(cx, cx + len, t[0], t[3], fl & 1u) && segq_cell_in_range(cy, cy + len, t[1], t[4], (fl >> 1) & 1u) &&
                                  segq_cell_in_range(cz, cz + len, t[2], t[5], (fl >> 2) & 1u));
                }
            if (!any) continue;
            const float px = __uint_as_float(t[7]), py = __uint_as_float(t[8]), pz = __uint_as_float(t[9]);
            const float dx = __uint_as_float(t[10]), dy = __uint_as_float(t[11]), dz = __uint_as_float(t[12]);
            const uint32_t exclude = t[13];
            SegRec rec = { q0 + i, 0u, 0.0f, 0.0f };
            if (!segq_slab(px, py, pz, dx, dy, dz, bx0, bx1, by0, by1, bz0, bz1, rec.t0, rec.t1)) continue;      // (S.aabb is not a bound: the cell box is)
            // walked ONCE for this segment, however many of its linked keys lie in the range
            for (uint32_t m = 0; m < cnt; m++) {
                if (m == 0u) {
                    rec.id = id0;
                    if (!(live0 && id0 != exclude && segq_slab(px, py, pz, dx, dy, dz, a0.xmin, a0.xmax, a0.ymin, a0.ymax, a0.zmin, a0.zmax, rec.t0, rec.t1))) continue;
                } else if (!segq_row_hit(A, A.rows[begin + m], expect, exclude, px, py, pz, dx, dy, dz, rec)) continue;
                const uint32_t pos = atomicAdd(&S.n_hits, 1u);
                if (pos < BOXQ_HITBUF) S.hits[pos] = rec;
                else segq_store(A, atomicAdd(&A.hdr->count, 1u), rec);
            }
        }
    }
    segq_flush(A, S);
}

}  // namespace

// Grid: workgroups [0, n) take one segment each through the unique sections; the workgroups behind them take (256 shared sections) x (256 segments) each.
// 256 threads, 64-wide waves, no recursion; every loop is bounded (candidate cells by the host's cap, rb_find's probe by an empty slot of an overlay that is
// never full and a binary search, the row walks by the sections' counts).
// Publication: write-through records, every wave waits for its own stores, then the workgroup signs off (list_sign_off, re_kernels.h).
__global__ __launch_bounds__(BOXQ_THREADS) void k_segment_query(SegQueryArgs A) {
    __shared__ SegqShared S;
    if (threadIdx.x == 0) { S.n_hits = 0u; S.n_queue = 0u; }
    __syncthreads();
    if (blockIdx.x < A.n) segq_unique_part(A, S); else segq_shared_part(A, S);
    wait_own_stores();
    __syncthreads();                                                          // every wave's records have left; the count atomics have returned
    if (threadIdx.x == 0) list_sign_off(A.hdr, A.h_pub, A.seq);
}

}  // namespace re
