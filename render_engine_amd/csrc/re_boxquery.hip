// Tree queries for user logic on the resident world, for gfx950: the entities whose StaticAABB intersects each box of a batch -- what a
// LogicFunction / CollisionFunction / UserInputLogicFunction of the reference (exports/logic_components.rs:14-18) reads out of its
// &BoundingBoxTree (find_all_unique_world_section_ids, stored_entities_indexes, shared_section_indexes).
//
// The rule: (query i, entity) for every live entity in the tree (not F_DEAD, not an F_PHANTOM replica, row_cell set; ghost instances of the frozen
// static cache are no entities) whose stored StaticAABB intersects box i by StaticAABB::intersect (aabb.rs:68-73: closed intervals, plain f32
// compares), optionally filtered by flag bits.  Each pair once.
//
// The walk: an entity's sections are a function of its AABB clipped to the world (normalize_aabb); clipping is monotone per axis, so two
// intersecting intervals still intersect after it, and every entity of the rule has a section key inside the query's cell range of that key's level
// (box_level_range, re_kernels.h; tests/test_box_query_rule.py shows it against the oracle).  The exact test then runs on the stored boxes.
//   unique sections: one workgroup per query enumerates the candidate cells of every level, looks each key up (rb_find) and walks the rows of the
//     sections that exist, one wave per section, one lane per row;
//   shared sections: their links to the unique sections are not on the device, so they are taken from their own side: workgroups behind the first n
//     hold 256 shared sections each, one per lane, and test them against a tile of queries in LDS -- a shared section is walked once for a query
//     when ANY of its linked keys lies in the query's range (that is the dedupe), by the lane that owns it.  O(shared sections x queries) integer tests.
#include "re_kernels.h"

namespace re {

namespace {

__device__ __forceinline__ uint32_t boxq_mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ bool boxq_intersect(const Aabb &a, const float *q) {      // StaticAABB::intersect: a.min <= b.max && a.max >= b.min per axis
    return a.xmin <= q[1] && a.xmax >= q[0] && a.ymin <= q[3] && a.ymax >= q[2] && a.zmin <= q[5] && a.zmax >= q[4];
}
// Records are read by the host as soon as it has seen the count: write-through stores (sc1), as k_logic_list's.
__device__ __forceinline__ void boxq_store(const BoxQueryArgs &A, uint32_t slot, unsigned long long rec) {
    if (slot < A.capacity) __hip_atomic_store(&A.out[slot], rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// does the row belong to the rule for this box?  expect: the row_cell word of a member of the section being walked
__device__ __forceinline__ bool boxq_row_hit(const BoxQueryArgs &A, uint32_t r, uint32_t expect, const float *q) {
    if (r >= A.nrows) return false;                                        // (ghost instances live beyond the entity rows; they are not walked, and not read if they were)
    const uint32_t fl = A.row_flags[r], rc = A.row_cell[r];
    if ((fl & (F_DEAD | F_PHANTOM)) || rc != expect || (fl & A.need) != A.need || (fl & A.forbid)) return false;
    return boxq_intersect(A.row_aabb[r], q);
}

struct BoxqShared {
    unsigned long long hits[BOXQ_HITBUF];          // staged records
    uint32_t queue[BOXQ_TILE * 13u];               // unique part: slots of the hit sections of a round; shared part: the query tile, 13 words a query
    uint32_t n_hits, n_queue, gbase;
    uint32_t prefix[MAX_LEVELS + 2], lo[3][MAX_LEVELS + 1], ext[3][MAX_LEVELS + 1];      // unique part: candidate cells before each level, first cell and extent per axis
    float box[6];
};
static_assert(BOXQ_QUEUE <= BOXQ_TILE * 13u, "the section queue shares the LDS of the query tile");

// the staged records leave: ONE global atomicAdd per workgroup and flush.  Called by all 256 threads.
__device__ __forceinline__ void boxq_flush(const BoxQueryArgs &A, BoxqShared &S) {
    __syncthreads();
    const uint32_t n = S.n_hits < BOXQ_HITBUF ? S.n_hits : BOXQ_HITBUF;
    if (n == 0u) return;                                                   // (uniform)
    if (threadIdx.x == 0) S.gbase = atomicAdd(&A.hdr->count, n);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += BOXQ_THREADS) boxq_store(A, S.gbase + k, S.hits[k]);
    __syncthreads();
    if (threadIdx.x == 0) S.n_hits = 0u;
    __syncthreads();
}

// one wave walks rows[begin .. begin + cnt): one lane per row, ballot + mbcnt compaction into the workgroup's staging buffer
__device__ __forceinline__ void boxq_walk_wave(const BoxQueryArgs &A, BoxqShared &S, uint32_t query, uint32_t begin, uint32_t cnt, uint32_t expect) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = 0; base < cnt; base += 64u) {                     // (wave-uniform trip count)
        const uint32_t k = base + lane;
        uint32_t r = 0; bool hit = false;
        if (k < cnt) { r = A.rows[begin + k]; hit = boxq_row_hit(A, r, expect, S.box); }
        const uint64_t mask = __ballot(hit);
        if (!mask) continue;
        uint32_t pos = 0;
        if (lane == 0u) pos = atomicAdd(&S.n_hits, (uint32_t)__popcll(mask));
        pos = __shfl(pos, 0) + boxq_mbcnt(mask);
        const unsigned long long rec = hit ? ((unsigned long long)query | ((unsigned long long)A.row_id[r] << 32)) : 0ull;
        if (hit && pos < BOXQ_HITBUF) S.hits[pos] = rec;
        const uint64_t over = __ballot(hit && pos >= BOXQ_HITBUF);        // the staging buffer is full: this wave's remainder goes out directly
        if (over) {
            uint32_t g = 0;
            if (lane == 0u) g = atomicAdd(&A.hdr->count, (uint32_t)__popcll(over));
            g = __shfl(g, 0) + boxq_mbcnt(over);
            if (hit && pos >= BOXQ_HITBUF) boxq_store(A, g, rec);
        }
    }
}

__device__ __forceinline__ void boxq_unique_part(const BoxQueryArgs &A, BoxqShared &S) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, query = blockIdx.x;
    const BoxQuery &Q = A.q[query];
    const uint32_t nlev = A.max_level + 1u;                                // an entity longer than half the outline sits at level max_level
    if (tid < 6u) S.box[tid] = Q.box[tid];
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
        for (uint32_t l = 0; l < nlev; l++) { S.prefix[l] = sum; sum += S.ext[0][l] * S.ext[1][l] * S.ext[2][l]; }      // (<= RE_BOX_QUERY_MAX_CELLS: the host refused the box otherwise)
        S.prefix[nlev] = sum;
    }
    __syncthreads();
    const uint32_t total = S.prefix[nlev];
    for (uint32_t base = 0; base < total; base += BOXQ_QUEUE) {            // rounds of 1024 candidate cells
        for (uint32_t j = 0; j < BOXQ_PROBES; j++) {
            const uint32_t g = base + j * BOXQ_THREADS + tid;
            if (g >= total) break;
            uint32_t l = 0;
            while (g >= S.prefix[l + 1u]) l++;                             // (l < nlev: g < prefix[nlev])
            const uint32_t idx = g - S.prefix[l], nx = S.ext[0][l], ny = S.ext[1][l];
            const uint32_t ix = idx % nx, rest = idx / nx, iy = rest % ny, iz = rest / ny;
            const uint64_t key = pack_key(l, S.lo[0][l] + ix, S.lo[2][l] + iz, S.lo[1][l] + iy);
            const int32_t slot = rb_find(A.T, A.cell_key, key);
            if (slot >= 0 && A.cell_nl[slot] + A.cell_ns[slot] != 0u) S.queue[atomicAdd(&S.n_queue, 1u)] = (uint32_t)slot;
        }
        __syncthreads();
        const uint32_t nq = S.n_queue;
        for (uint32_t e = wave; e < nq; e += BOXQ_THREADS / 64u) {          // one wave per hit section: active rows, then static rows; the ghost tail is not walked
            const uint32_t slot = S.queue[e];
            boxq_walk_wave(A, S, query, A.cell_begin[slot], A.cell_nl[slot] + A.cell_ns[slot], slot);
        }
        boxq_flush(A, S);
        if (tid == 0) S.n_queue = 0u;
        __syncthreads();
    }
}

// the cell of one linked key against one query: is the cell inside the query's range of the key's level?  Integer form of box_level_range:
// x <= umax / len  <=>  x * len <= umax;   x >= lo  <=>  (x + 1) * len + whole > umin  (lo = umin / len, one less when umin is a whole multiple of len)
__device__ __forceinline__ bool boxq_cell_in_range(uint32_t c0, uint32_t c1, uint32_t umin, uint32_t umax, uint32_t whole) {
    return c0 <= umax && c1 + whole > umin;
}

constexpr uint32_t BOXQ_TILE_WORDS = 13;       // a query in the LDS tile of the shared part: umin[3], umax[3], flags, then the box itself (6 floats)

__device__ __forceinline__ void boxq_shared_part(const BoxQueryArgs &A, BoxqShared &S) {
    const uint32_t tid = threadIdx.x, sb = blockIdx.x - A.n;
    const uint32_t chunk = sb % A.n_sh_chunks, q0 = (sb / A.n_sh_chunks) * BOXQ_TILE;
    const uint32_t nq = A.n - q0 < BOXQ_TILE ? A.n - q0 : BOXQ_TILE;
    uint32_t *tile = S.queue;
    if (tid < nq) {
        const BoxQuery &Q = A.q[q0 + tid];
        uint32_t *t = tile + tid * BOXQ_TILE_WORDS;
        for (uint32_t a = 0; a < 3u; a++) { t[a] = Q.umin[a]; t[3u + a] = Q.umax[a]; }
        t[6] = Q.flags;
        for (uint32_t a = 0; a < 6u; a++) t[7u + a] = __float_as_uint(Q.box[a]);
    }
    __syncthreads();
    const uint32_t s = chunk * BOXQ_THREADS + tid;
    const uint32_t nk = s < A.nsh ? A.sh_nk[s] : 0u;                        // holes: nk == 0
    const uint32_t cnt = nk ? A.sh_nact[s] + A.sh_nstat[s] : 0u;
    if (cnt) {
        uint64_t keys[8];
#pragma unroll
        for (int k = 0; k < 8; k++) keys[k] = A.sh_keys[(size_t)s * 8u + k];
        // the bounding cell box of the linked keys, in world units: most (query, shared section) pairs end at this one test
        uint32_t b0[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, b1[3] = { 0u, 0u, 0u };
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)k < nk) {
                const uint32_t len = A.atomic << key_level(keys[k]);
                const uint32_t c[3] = { key_x(keys[k]) * len, key_y(keys[k]) * len, key_z(keys[k]) * len };
#pragma unroll
                for (int a = 0; a < 3; a++) { b0[a] = c[a] < b0[a] ? c[a] : b0[a]; b1[a] = c[a] + len > b1[a] ? c[a] + len : b1[a]; }
            }
        // the first member (most shared sections hold one entity) is fetched ONCE, in front of the loop over the queries: a section of a high level is a
        // candidate of every query, and a lane that gathered its row per query would spend four dependent round trips on each
        const uint32_t begin = A.sh_begin[s], expect = ROW_CELL_SHARED | s;
        const uint32_t r0 = A.rows[begin];
        bool live0 = false; Aabb a0 = {}; uint32_t id0 = 0;
        if (r0 < A.nrows) {
            const uint32_t fl = A.row_flags[r0], rc = A.row_cell[r0];
            live0 = !(fl & (F_DEAD | F_PHANTOM)) && rc == expect && (fl & A.need) == A.need && !(fl & A.forbid);
            a0 = A.row_aabb[r0]; id0 = A.row_id[r0];
        }
        for (uint32_t i = 0; i < nq; i++) {
            const uint32_t *t = tile + i * BOXQ_TILE_WORDS;
            const uint32_t fl = t[6];
            if (!(boxq_cell_in_range(b0[0], b1[0], t[0], t[3], fl & 1u) && boxq_cell_in_range(b0[1], b1[1], t[1], t[4], (fl >> 1) & 1u) &&
                  boxq_cell_in_range(b0[2], b1[2], t[2], t[5], (fl >> 2) & 1u))) continue;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if ((uint32_t)k < nk) {
                    const uint32_t len = A.atomic << key_level(keys[k]);
                    const uint32_t cx = key_x(keys[k]) * len, cy = key_y(keys[k]) * len, cz = key_z(keys[k]) * len;
                    any = any || (boxq_cell_in_range(cx, cx + len, t[0], t[3], fl & 1u) && boxq_cell_in_range(cy, cy + len, t[1], t[4], (fl >> 1) & 1u) &&
                                  boxq_cell_in_range(cz, cz + len, t[2], t[5], (fl >> 2) & 1u));
                }
            if (!any) continue;
            // walked ONCE for this query, however many of its linked keys lie in the range
            float qb[6];
#pragma unroll
            for (int a = 0; a < 6; a++) qb[a] = __uint_as_float(t[7 + a]);
            for (uint32_t m = 0; m < cnt; m++) {
                uint32_t id = id0;
                if (m == 0u) { if (!(live0 && boxq_intersect(a0, qb))) continue; }
                else {
                    const uint32_t r = A.rows[begin + m];
                    if (!boxq_row_hit(A, r, expect, qb)) continue;
                    id = A.row_id[r];
                }
                const unsigned long long rec = (unsigned long long)(q0 + i) | ((unsigned long long)id << 32);
                const uint32_t pos = atomicAdd(&S.n_hits, 1u);
                if (pos < BOXQ_HITBUF) S.hits[pos] = rec;
                else boxq_store(A, atomicAdd(&A.hdr->count, 1u), rec);
            }
        }
    }
    boxq_flush(A, S);
}

}  // namespace

// Grid: workgroups [0, n) take one query each through the unique sections; the workgroups behind them take (256 shared sections) x (256 queries) each.
// 256 threads, 64-wide waves, no recursion; every loop is bounded (candidate cells by the host's cap, rb_find's probe by an empty slot of an overlay that is
// never full and a binary search, the row walks by the sections' counts).
// Publication: write-through records, every wave waits for its own stores, then the workgroup signs off (list_sign_off, re_kernels.h).
__global__ __launch_bounds__(BOXQ_THREADS) void k_box_query(BoxQueryArgs A) {
    __shared__ BoxqShared S;
    if (threadIdx.x == 0) { S.n_hits = 0u; S.n_queue = 0u; }
    __syncthreads();
    if (blockIdx.x < A.n) boxq_unique_part(A, S); else boxq_shared_part(A, S);
    wait_own_stores();
    __syncthreads();                                                          // every wave's records have left; the count atomics have returned
    if (threadIdx.x == 0) list_sign_off(A.hdr, A.h_pub, A.seq);
}

}  // namespace re
