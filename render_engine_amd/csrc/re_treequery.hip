// Tree queries for user logic on the resident world, for gfx950 -- what a LogicFunction / CollisionFunction / UserInputLogicFunction of the reference
// (exports/logic_components.rs:14-18) reads out of its &BoundingBoxTree (find_all_unique_world_section_ids, stored_entities_indexes,
// shared_section_indexes): "who is near this box" (k_box_query), "who lies along this segment" -- a shot, a line of sight, a pick ray (k_segment_query) --
// and "who is within r of this point" -- an explosion, a proximity trigger (k_sphere_query).
// One walk of the tree, written once over a query shape and a mode of storing hits; the three kernels instantiate it with the default mode (every hit a record), and
// the four kernels of re_query_segments_first / re_query_spheres_nearest with the other two: reduce the hits' keys per query, then pick the winners (TreeqMode, below).
// The same questions asked by entity (re_query_boxes_around, re_query_spheres_around) have their records built here, from the askers' rows
// (k_around_build_*, at the end), and are walked by k_box_query_around -- the boxes' shape with the asker left out -- and by k_sphere_query as it is.
//
// The rule of the boxes: (query i, entity) for every live entity in the tree (not F_DEAD, not an F_PHANTOM replica, row_cell set; ghost instances of the
// frozen static cache are no entities) whose stored StaticAABB intersects box i by StaticAABB::intersect (aabb.rs:68-73: closed intervals, plain f32
// compares), optionally filtered by flag bits.  Each pair once.
// The rule of the segments: (query i, entity, t_enter, t_exit) for every entity the box query would consider other than the segment's excluded one whose
// stored, unclipped StaticAABB is met by the segment p0 + t * d, t in [0, 1], by the slab test below: plain f32, IEEE division, closed intervals, d == 0 on
// an axis a containment test.  Each pair once; tests/segment_rule.py restates it.
// The rule of the spheres: (query i, entity, dist_sq, side) for every entity the box query would consider other than the sphere's excluded one whose
// stored, unclipped StaticAABB lies within the radius of the centre by sphq_dist_sq below: plain f32, every operation rounded once, compares written as
// compares, dist_sq <= r2 with r2 = r * r multiplied once on the host.  Each pair once; tests/sphere_rule.py restates it.
//
// The walk: an entity's sections are a function of its AABB clipped to the world (normalize_aabb); clipping is monotone per axis, so two
// intersecting intervals still intersect after it, and every entity of the rule has a section key inside the query's cell range of that key's level
// (box_level_range, re_kernels.h; tests/test_box_query_rule.py shows it against the oracle).  The exact test then runs on the stored boxes.  A segment
// walks the cell ranges of its bounding box (inflated by the margin), with one test more in front of every probe: a candidate
// cell is looked up only when the segment meets the cell's own box -- inflated by the margin, and open-ended on an axis where the cell lies on a face of
// the world, because entities clipped to the world sit there and the exact test runs on unclipped boxes.  A sphere walks the cell ranges of its bounding
// cube (inflated likewise) and prunes a cell whose box -- the segments' cell box -- lies further from the centre than the radius, by the exact test's own
// function: f32 subtract, multiply and add are monotone, so the distance to a box that contains an entity's clipped AABB never exceeds the entity's.
//   unique sections: one workgroup per query enumerates the candidate cells of every level, prunes (segments), looks the remaining keys up (rb_find) and
//     walks the rows of the sections that exist, one wave per section, one lane per row;
//   shared sections: their links to the unique sections are not on the device, so they are taken from their own side: workgroups behind the first n
//     hold 256 shared sections each, one per lane, and test them against a tile of queries in LDS -- a shared section is walked once for a query
//     when ANY of its linked keys lies in the query's range (that is the dedupe) and the query's prune lets the bounding cell box of the linked keys
//     through (segments; inflated, open-ended as above), by the lane that owns it.  O(shared sections x queries) integer tests.
//
// A shape is the query as a lane holds it (a small value type: it sits in LDS for the workgroup's own query, in registers during a walk) and supplies
//   Args, Query, Rec, TILE_WORDS      the kernel's argument block, the host's query record, the output record, the words of a query in the LDS tile
//   stage / to_tile / from_tile       the payload out of the query record: into LDS by the first lanes of a workgroup, into and out of the tile
//   cell_box / misses                 the prune of a candidate cell and of a shared section's bounding cell box ([c0, c1] per axis in world units)
//   test                              the exact test on a row's AABB and id, which fills the record
//   store                             the record's write-through store below the capacity
//   value_bits / misses_beyond        (segments, spheres) the value of a record's key -- t_enter, dist_sq --, and the prune of the pick pass: the query shrunk to its best value
#include "re_kernels.h"

namespace re {

namespace {

__device__ __forceinline__ uint32_t treeq_mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool boxq_intersect(const Aabb &a, const float *q) {      // StaticAABB::intersect: a.min <= b.max && a.max >= b.min per axis
    return a.xmin <= q[1] && a.xmax >= q[0] && a.ymin <= q[3] && a.ymax >= q[2] && a.zmin <= q[5] && a.zmax >= q[4];
}
struct BoxShape {
    using Args = BoxQueryArgs; using Query = BoxQuery; using Rec = unsigned long long;      // re_box_hit: query | entity << 32
    struct CellBox {};                                                                      // no prune: every candidate cell is probed
    static constexpr uint32_t TILE_WORDS = 13;     // a query in the LDS tile of the shared part: umin[3], umax[3], flags, then the box itself (6 floats)
    float box[6];
    static __device__ __forceinline__ void stage(BoxShape &L, const Query &Q, uint32_t tid) { if (tid < 6u) L.box[tid] = Q.box[tid]; }
    static __device__ __forceinline__ void to_tile(const Query &Q, uint32_t *t) { for (uint32_t a = 0; a < 6u; a++) t[a] = __float_as_uint(Q.box[a]); }
    static __device__ __forceinline__ BoxShape from_tile(const uint32_t *t) {
        BoxShape P;
#pragma unroll
        for (int a = 0; a < 6; a++) P.box[a] = __uint_as_float(t[a]);
        return P;
    }
    static __device__ __forceinline__ CellBox cell_box(const Args &, const uint32_t *, const uint32_t *) { return {}; }
    __device__ __forceinline__ bool misses(const CellBox &) const { return false; }
    __device__ __forceinline__ bool test(const Aabb &a, const uint32_t *id, uint32_t query, Rec &rec) const {
        if (!boxq_intersect(a, box)) return false;
        rec = (unsigned long long)query | ((unsigned long long)*id << 32);
        return true;
    }
    // Records are read by the host as soon as it has seen the count: write-through stores (sc1), as k_logic_list's.
    static __device__ __forceinline__ void store(const Args &A, uint32_t slot, const Rec &rec) {
        if (slot < A.capacity) __hip_atomic_store(&A.out[slot], rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ... and the box of an asking entity (re_query_boxes_around): the same records, the same test, minus the asker, whose id the device builder left in pad[0].
// A shape of its own, so that k_box_query stays the code object it is.  The prune lets everything through but the builder's empty record (an inverted box),
// which walks nothing.
struct BoxAroundShape : BoxShape {
    static constexpr uint32_t TILE_WORDS = 14;     // umin[3], umax[3], flags, the box (6 floats), exclude
    uint32_t exclude;
    static __device__ __forceinline__ void stage(BoxAroundShape &L, const Query &Q, uint32_t tid) {
        if (tid < 6u) L.box[tid] = Q.box[tid];
        if (tid == 6u) L.exclude = Q.pad[0];
    }
    static __device__ __forceinline__ void to_tile(const Query &Q, uint32_t *t) { BoxShape::to_tile(Q, t); t[6] = Q.pad[0]; }
    static __device__ __forceinline__ BoxAroundShape from_tile(const uint32_t *t) {
        BoxAroundShape P;
#pragma unroll
        for (int a = 0; a < 6; a++) P.box[a] = __uint_as_float(t[a]);
        P.exclude = t[6];
        return P;
    }
    __device__ __forceinline__ bool misses(const CellBox &) const { return box[0] > box[1]; }
    __device__ __forceinline__ bool test(const Aabb &a, const uint32_t *id, uint32_t query, Rec &rec) const {
        return *id != exclude && BoxShape::test(a, id, query, rec);
    }
};

// ---- segments ---------------------------------------------------------------------------------------------------------------------------------------
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

struct SegShape {
    using Args = SegQueryArgs; using Query = SegQuery; using Rec = SegRec;
    struct CellBox { float x0, x1, y0, y1, z0, z1; };
    static constexpr uint32_t TILE_WORDS = 14;     // a segment in the LDS tile of the shared part: umin[3], umax[3], flags, p0[3], d[3], exclude
    float p0[3], d[3]; uint32_t exclude;
    static __device__ __forceinline__ void stage(SegShape &L, const Query &Q, uint32_t tid) {
        if (tid < 3u) { L.p0[tid] = Q.p0[tid]; L.d[tid] = Q.d[tid]; }
        if (tid == 3u) L.exclude = Q.exclude;
    }
    static __device__ __forceinline__ void to_tile(const Query &Q, uint32_t *t) {
        for (uint32_t a = 0; a < 3u; a++) { t[a] = __float_as_uint(Q.p0[a]); t[3u + a] = __float_as_uint(Q.d[a]); }
        t[6] = Q.exclude;
    }
    static __device__ __forceinline__ SegShape from_tile(const uint32_t *t) {
        SegShape P;
#pragma unroll
        for (int a = 0; a < 3; a++) { P.p0[a] = __uint_as_float(t[a]); P.d[a] = __uint_as_float(t[3 + a]); }
        P.exclude = t[6];
        return P;
    }
    static __device__ __forceinline__ CellBox cell_box(const Args &A, const uint32_t *c0, const uint32_t *c1) {
        return { segq_cell_min(c0[0], A.margin), segq_cell_max(c1[0], A.outline, A.margin), segq_cell_min(c0[1], A.margin), segq_cell_max(c1[1], A.outline, A.margin),
                 segq_cell_min(c0[2], A.margin), segq_cell_max(c1[2], A.outline, A.margin) };
    }
    // the prune: the cell's closed box holds the clipped AABB of every entity of a unique section there (of a shared section: the bounding cell box does)
    __device__ __forceinline__ bool misses(const CellBox &b) const {
        float t0, t1;
        return !segq_slab(p0[0], p0[1], p0[2], d[0], d[1], d[2], b.x0, b.x1, b.y0, b.y1, b.z0, b.z1, t0, t1);
    }
    __device__ __forceinline__ bool test(const Aabb &a, const uint32_t *id, uint32_t query, Rec &rec) const {
        rec.query = query; rec.id = *id;
        if (rec.id == exclude) return false;
        return segq_slab(p0[0], p0[1], p0[2], d[0], d[1], d[2], a.xmin, a.xmax, a.ymin, a.ymax, a.zmin, a.zmax, rec.t0, rec.t1);
    }
    // first hit: the value of a record's key, and the prune of the pick pass -- a cell whose slab lo exceeds the best t_enter holds neither the winner nor
    // anything tied with it.  Per axis with d > 0 the cell's near bound mn is no greater than the entity's, and (mn - p) / d is monotone in mn (f32 subtract
    // and divide by a positive number keep order; mirrored for d < 0 with the far bound; d == 0 adds nothing to lo); the maximum over the axes keeps the
    // order: lo(cell) <= t_enter(entity).
    static __device__ __forceinline__ uint32_t value_bits(const Rec &r) { return __float_as_uint(r.t0); }
    __device__ __forceinline__ bool misses_beyond(const CellBox &b, float best) const {
        float t0, t1;
        return !segq_slab(p0[0], p0[1], p0[2], d[0], d[1], d[2], b.x0, b.x1, b.y0, b.y1, b.z0, b.z1, t0, t1) || t0 > best;
    }
    // write-through stores, as the box query's; two 8-byte halves, both below the capacity or neither
    static __device__ __forceinline__ void store(const Args &A, uint32_t slot, const Rec &r) {
        if (slot >= A.capacity) return;
        unsigned long long *o = A.out + (size_t)slot * 2u;
        __hip_atomic_store(o, (unsigned long long)r.query | ((unsigned long long)r.id << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, (unsigned long long)__float_as_uint(r.t0) | ((unsigned long long)__float_as_uint(r.t1) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- spheres ----------------------------------------------------------------------------------------------------------------------------------------
// one axis of the distance from a point to a closed interval (bounds may be infinite: both compares are false then and e = 0); the side bit a the minimum
// face, 16 << a the maximum face
__device__ __forceinline__ float sphq_axis(float c, float mn, float mx, uint32_t lo_bit, uint32_t hi_bit, uint32_t &side) {
    if (c < mn) { side |= lo_bit; return mn - c; }
    if (c > mx) { side |= hi_bit; return c - mx; }
    return 0.0f;
}
// the squared distance from the point c to a closed box, (ex * ex + ey * ey) + ez * ez, every operation rounded once (the library is built without
// contraction); side == 0 exactly when the point is inside
__device__ __forceinline__ float sphq_dist_sq(const float *c, float x0, float x1, float y0, float y1, float z0, float z1, uint32_t &side) {
    side = 0u;
    const float ex = sphq_axis(c[0], x0, x1, 1u, 16u, side), ey = sphq_axis(c[1], y0, y1, 2u, 32u, side), ez = sphq_axis(c[2], z0, z1, 4u, 64u, side);
    return (ex * ex + ey * ey) + ez * ez;
}

struct SphRec { uint32_t query, id; float dist_sq; uint32_t side; };      // re_sphere_hit

struct SphShape {
    using Args = SphQueryArgs; using Query = SphQuery; using Rec = SphRec;
    using CellBox = SegShape::CellBox;
    static constexpr uint32_t TILE_WORDS = 12;     // a sphere in the LDS tile of the shared part: umin[3], umax[3], flags, c[3], r2, exclude
    float c[3], r2; uint32_t exclude;
    static __device__ __forceinline__ void stage(SphShape &L, const Query &Q, uint32_t tid) {
        if (tid < 3u) L.c[tid] = Q.c[tid];
        if (tid == 3u) { L.r2 = Q.r2; L.exclude = Q.exclude; }
    }
    static __device__ __forceinline__ void to_tile(const Query &Q, uint32_t *t) {
        for (uint32_t a = 0; a < 3u; a++) t[a] = __float_as_uint(Q.c[a]);
        t[3] = __float_as_uint(Q.r2); t[4] = Q.exclude;
    }
    static __device__ __forceinline__ SphShape from_tile(const uint32_t *t) {
        SphShape P;
#pragma unroll
        for (int a = 0; a < 3; a++) P.c[a] = __uint_as_float(t[a]);
        P.r2 = __uint_as_float(t[3]); P.exclude = t[4];
        return P;
    }
    static __device__ __forceinline__ CellBox cell_box(const Args &A, const uint32_t *c0, const uint32_t *c1) {      // the segments' cell box
        return { segq_cell_min(c0[0], A.margin), segq_cell_max(c1[0], A.outline, A.margin), segq_cell_min(c0[1], A.margin), segq_cell_max(c1[1], A.outline, A.margin),
                 segq_cell_min(c0[2], A.margin), segq_cell_max(c1[2], A.outline, A.margin) };
    }
    // the prune, by the exact test's own function: the cell's box holds the clipped AABB of every entity there and is open-ended where they were clipped,
    // and f32 subtract, multiply and add are monotone, so dist_sq(cell) <= dist_sq(entity)
    __device__ __forceinline__ bool misses(const CellBox &b) const {
        uint32_t side;
        return sphq_dist_sq(c, b.x0, b.x1, b.y0, b.y1, b.z0, b.z1, side) > r2;
    }
    __device__ __forceinline__ bool test(const Aabb &a, const uint32_t *id, uint32_t query, Rec &rec) const {
        rec.query = query; rec.id = *id;
        if (rec.id == exclude) return false;
        rec.dist_sq = sphq_dist_sq(c, a.xmin, a.xmax, a.ymin, a.ymax, a.zmin, a.zmax, rec.side);
        return rec.dist_sq <= r2;
    }
    // nearest: the value of a record's key, and the prune of the pick pass -- the prune above with r2 := the best dist_sq (its monotonicity argument holds for
    // any bound: dist_sq(cell) <= dist_sq(entity), so a cell further away than the best holds neither the winner nor anything tied with it)
    static __device__ __forceinline__ uint32_t value_bits(const Rec &r) { return __float_as_uint(r.dist_sq); }
    __device__ __forceinline__ bool misses_beyond(const CellBox &b, float best) const {
        SphShape P = *this;
        P.r2 = best;
        return P.misses(b);
    }
    // write-through stores, as the segment query's; two 8-byte halves, both below the capacity or neither
    static __device__ __forceinline__ void store(const Args &A, uint32_t slot, const Rec &r) {
        if (slot >= A.capacity) return;
        unsigned long long *o = A.out + (size_t)slot * 2u;
        __hip_atomic_store(o, (unsigned long long)r.query | ((unsigned long long)r.id << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(o + 1, (unsigned long long)__float_as_uint(r.dist_sq) | ((unsigned long long)r.side << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t TREEQ_TILE_HEAD = 7;        // every shape's tile entry starts with umin[3], umax[3], flags; the shape's payload follows

// What the walk does with a hit (a mode beside the shape; the argument block of the two new modes carries best[n] behind the sibling's members):
//   TREEQ_ALL     every hit is a record: staged in LDS, flushed into the list, the launch signs off (the three queries above)
//   TREEQ_REDUCE  pass 1 of first hit / nearest: no record -- the hit's key (hit_key, re_kernels.h) is reduced into best[query]: a wave minimum and one LDS
//                 atomicMin per wave iteration in the row walk, one LDS atomicMin per hit in the shared part, one global atomicMin per workgroup and query
//                 that found anything.  Counts nothing, does not touch the header, does not sign off.
//   TREEQ_PICK    pass 2: every query shrunk to its best value (Shape::misses_beyond), a query without a hit walks nothing; the one hit whose key equals
//                 best[query] is a record and leaves as in TREEQ_ALL.  Entity ids are unique and the rule yields each pair once: one record per query with a hit.
enum TreeqMode { TREEQ_ALL = 0, TREEQ_REDUCE = 1, TREEQ_PICK = 2 };

template <class Shape, int Mode> struct TreeqStore {                     // TREEQ_ALL
    static constexpr uint32_t NHIT = BOXQ_HITBUF;
    typename Shape::Rec hits[NHIT];                // staged records
};
template <class Shape> struct TreeqStore<Shape, TREEQ_REDUCE> {          // no staging buffer: its LDS is free
    unsigned long long best[BOXQ_TILE];            // unique part: [0] the workgroup's own best key; shared part: the best key of every tile query
};
template <class Shape> struct TreeqStore<Shape, TREEQ_PICK> {
    static constexpr uint32_t NHIT = BOXQ_TILE;    // (a workgroup keeps at most one record per query: one in the unique part, one per tile query in the shared part)
    typename Shape::Rec hits[NHIT];
    unsigned long long best[BOXQ_TILE];            // shared part: best[q0 + i] of every tile query
};
template <class Shape, int Mode = TREEQ_ALL> struct TreeqShared : TreeqStore<Shape, Mode> {
    uint32_t queue[BOXQ_TILE * Shape::TILE_WORDS]; // unique part: slots of the hit sections of a round; shared part: the query tile
    uint32_t n_hits, n_queue, gbase;
    uint32_t prefix[MAX_LEVELS + 2], lo[3][MAX_LEVELS + 1], ext[3][MAX_LEVELS + 1];      // unique part: candidate cells before each level, first cell and extent per axis
    Shape own;                                     // unique part: the workgroup's query
    static_assert(BOXQ_QUEUE <= BOXQ_TILE * Shape::TILE_WORDS, "the section queue shares the LDS of the query tile");
};

// the staged records leave: ONE global atomicAdd per workgroup and flush.  Called by all 256 threads.
template <class Shape, int Mode> __device__ __forceinline__ void treeq_flush(const typename Shape::Args &A, TreeqShared<Shape, Mode> &S) {
    __syncthreads();
    const uint32_t n = S.n_hits < S.NHIT ? S.n_hits : S.NHIT;
    if (n == 0u) return;                                                   // (uniform)
    if (threadIdx.x == 0) S.gbase = atomicAdd(&A.hdr->count, n);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < n; k += BOXQ_THREADS) Shape::store(A, S.gbase + k, S.hits[k]);
    __syncthreads();
    if (threadIdx.x == 0) S.n_hits = 0u;
    __syncthreads();
}

// is the row an entity of the tree that passes the filter?  expect: the row_cell word of a member of the section being walked
template <class Args> __device__ __forceinline__ bool treeq_row_live(const Args &A, uint32_t r, uint32_t expect) {
    if (r >= A.nrows) return false;                                        // (ghost instances live beyond the entity rows; they are not walked, and not read if they were)
    const uint32_t fl = A.row_flags[r], rc = A.row_cell[r];
    return !(fl & (F_DEAD | F_PHANTOM)) && rc == expect && (fl & A.need) == A.need && !(fl & A.forbid);
}
// does the row belong to the rule for this query?
template <class Shape> __device__ __forceinline__ bool treeq_row_hit(const typename Shape::Args &A, const Shape &P, uint32_t r, uint32_t expect, uint32_t query, typename Shape::Rec &rec) {
    return treeq_row_live(A, r, expect) && P.test(A.row_aabb[r], &A.row_id[r], query, rec);
}

template <class Shape> __device__ __forceinline__ unsigned long long treeq_key(const typename Shape::Rec &rec) { return hit_key(Shape::value_bits(rec), rec.id); }
__device__ __forceinline__ float treeq_key_value(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
// the minimum of a 64-bit key over the lanes of a wave, by shuffles (every lane ends with it)
__device__ __forceinline__ unsigned long long treeq_wave_min(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = ((unsigned long long)__shfl_xor((uint32_t)(k >> 32), off) << 32) | __shfl_xor((uint32_t)k, off);
        k = o < k ? o : k;
    }
    return k;
}

// the hits of one wave iteration go into the workgroup's staging buffer: ballot + mbcnt compaction
template <class Shape, int Mode> __device__ __forceinline__ void treeq_stage_wave(const typename Shape::Args &A, TreeqShared<Shape, Mode> &S, bool hit, const typename Shape::Rec &rec, uint64_t mask, uint32_t lane) {
    uint32_t pos = 0;
    if (lane == 0u) pos = atomicAdd(&S.n_hits, (uint32_t)__popcll(mask));
    pos = __shfl(pos, 0) + treeq_mbcnt(mask);
    if (hit && pos < S.NHIT) S.hits[pos] = rec;
    const uint64_t over = __ballot(hit && pos >= S.NHIT);                  // the staging buffer is full: this wave's remainder goes out directly
    if (over) {
        uint32_t g = 0;
        if (lane == 0u) g = atomicAdd(&A.hdr->count, (uint32_t)__popcll(over));
        g = __shfl(g, 0) + treeq_mbcnt(over);
        if (hit && pos >= S.NHIT) Shape::store(A, g, rec);
    }
}

// one wave walks rows[begin .. begin + cnt): one lane per row
// (bk: TREEQ_PICK: the query's best key, the only one kept.  TREEQ_REDUCE: every lane holds the same query, so the wave's minimum goes into the workgroup's best)
template <class Shape, int Mode> __device__ __forceinline__ void treeq_walk_wave(const typename Shape::Args &A, TreeqShared<Shape, Mode> &S, const Shape &P, uint32_t query, uint32_t begin, uint32_t cnt, uint32_t expect,
                                                                                 unsigned long long bk) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = 0; base < cnt; base += 64u) {                     // (wave-uniform trip count)
        const uint32_t k = base + lane;
        typename Shape::Rec rec{};
        bool hit = false;
        if (k < cnt) hit = treeq_row_hit(A, P, A.rows[begin + k], expect, query, rec);
        if constexpr (Mode == TREEQ_PICK) hit = hit && treeq_key<Shape>(rec) == bk;
        const uint64_t mask = __ballot(hit);
        if (!mask) continue;
        if constexpr (Mode == TREEQ_REDUCE) {
            const unsigned long long m = treeq_wave_min(hit ? treeq_key<Shape>(rec) : HIT_KEY_NONE);
            if (lane == 0u) atomicMin(&S.best[0], m);
        } else treeq_stage_wave(A, S, hit, rec, mask, lane);
    }
}

template <class Shape, int Mode, class KArgs> __device__ __forceinline__ void treeq_unique_part(const KArgs &A, TreeqShared<Shape, Mode> &S) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, query = blockIdx.x;
    unsigned long long bk = HIT_KEY_NONE;
    if constexpr (Mode == TREEQ_PICK) {
        bk = A.best[query];                                                // (pass 1 has ended: the launches follow each other in the stream)
        if (bk == HIT_KEY_NONE) return;                                    // (uniform) no hit: nothing to walk, the workgroup still signs off
    }
    const typename Shape::Query &Q = A.q[query];
    const uint32_t nlev = A.max_level + 1u;                                // an entity longer than half the outline sits at level max_level
    Shape::stage(S.own, Q, tid);
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
        for (uint32_t l = 0; l < nlev; l++) { S.prefix[l] = sum; sum += S.ext[0][l] * S.ext[1][l] * S.ext[2][l]; }      // (<= RE_BOX_QUERY_MAX_CELLS: the host refused the query otherwise)
        S.prefix[nlev] = sum;
    }
    __syncthreads();
    const uint32_t total = S.prefix[nlev];
    const Shape P = S.own;
    for (uint32_t base = 0; base < total; base += BOXQ_QUEUE) {            // rounds of 1024 candidate cells
        for (uint32_t j = 0; j < BOXQ_PROBES; j++) {
            const uint32_t g = base + j * BOXQ_THREADS + tid;
            if (g >= total) break;
            uint32_t l = 0;
            while (g >= S.prefix[l + 1u]) l++;                             // (l < nlev: g < prefix[nlev])
            const uint32_t idx = g - S.prefix[l], nx = S.ext[0][l], ny = S.ext[1][l];
            const uint32_t ix = idx % nx, rest = idx / nx, iy = rest % ny, iz = rest / ny;
            const uint32_t cx = S.lo[0][l] + ix, cy = S.lo[1][l] + iy, cz = S.lo[2][l] + iz, len = A.atomic << l;
            const uint32_t c0[3] = { cx * len, cy * len, cz * len }, c1[3] = { cx * len + len, cy * len + len, cz * len + len };
            if constexpr (Mode == TREEQ_PICK) { if (P.misses_beyond(Shape::cell_box(A, c0, c1), treeq_key_value(bk))) continue; }
            else if (P.misses(Shape::cell_box(A, c0, c1))) continue;
            const uint64_t key = pack_key(l, cx, cz, cy);
            const int32_t slot = rb_find(A.T, A.cell_key, key);
            if (slot >= 0 && A.cell_nl[slot] + A.cell_ns[slot] != 0u) S.queue[atomicAdd(&S.n_queue, 1u)] = (uint32_t)slot;
        }
        __syncthreads();
        const uint32_t nq = S.n_queue;
        for (uint32_t e = wave; e < nq; e += BOXQ_THREADS / 64u) {          // one wave per hit section: active rows, then static rows; the ghost tail is not walked
            const uint32_t slot = S.queue[e];
            treeq_walk_wave(A, S, P, query, A.cell_begin[slot], A.cell_nl[slot] + A.cell_ns[slot], slot, bk);
        }
        if constexpr (Mode == TREEQ_REDUCE) __syncthreads(); else treeq_flush<Shape, Mode>(A, S);
        if (tid == 0) S.n_queue = 0u;
        __syncthreads();
    }
    if constexpr (Mode == TREEQ_REDUCE) {                                  // (the barrier above: every wave's LDS minimum is in)
        if (tid == 0 && S.best[0] != HIT_KEY_NONE) atomicMin(&A.best[query], S.best[0]);      // ONE global atomic, only if the workgroup found anything
    }
}

// the cell of one linked key against one query: is the cell inside the query's range of the key's level?  Integer form of box_level_range:
// x <= umax / len  <=>  x * len <= umax;   x >= lo  <=>  (x + 1) * len + whole > umin  (lo = umin / len, one less when umin is a whole multiple of len)
__device__ __forceinline__ bool treeq_cell_in_range(uint32_t c0, uint32_t c1, uint32_t umin, uint32_t umax, uint32_t whole) {
    return c0 <= umax && c1 + whole > umin;
}
__device__ __forceinline__ bool treeq_cells_in_range(const uint32_t *c0, const uint32_t *c1, const uint32_t *t) {      // t: the head of a tile entry
    const uint32_t fl = t[6];
    return treeq_cell_in_range(c0[0], c1[0], t[0], t[3], fl & 1u) && treeq_cell_in_range(c0[1], c1[1], t[1], t[4], (fl >> 1) & 1u) &&
           treeq_cell_in_range(c0[2], c1[2], t[2], t[5], (fl >> 2) & 1u);
}

template <class Shape, int Mode, class KArgs> __device__ __forceinline__ void treeq_shared_part(const KArgs &A, TreeqShared<Shape, Mode> &S) {
    const uint32_t tid = threadIdx.x, sb = blockIdx.x - A.n;
    const uint32_t chunk = sb % A.n_sh_chunks, q0 = (sb / A.n_sh_chunks) * BOXQ_TILE;
    const uint32_t nq = A.n - q0 < BOXQ_TILE ? A.n - q0 : BOXQ_TILE;
    uint32_t *tile = S.queue;
    if (tid < nq) {
        const typename Shape::Query &Q = A.q[q0 + tid];
        uint32_t *t = tile + tid * Shape::TILE_WORDS;
        for (uint32_t a = 0; a < 3u; a++) { t[a] = Q.umin[a]; t[3u + a] = Q.umax[a]; }
        t[6] = Q.flags;
        Shape::to_tile(Q, t + TREEQ_TILE_HEAD);
        if constexpr (Mode == TREEQ_PICK) S.best[tid] = A.best[q0 + tid];
    }
    __syncthreads();
    const uint32_t s = chunk * BOXQ_THREADS + tid;
    const uint32_t nk = s < A.nsh ? A.sh_nk[s] : 0u;                        // holes: nk == 0
    const uint32_t cnt = nk ? A.sh_nact[s] + A.sh_nstat[s] : 0u;
    if (cnt) {
        uint64_t keys[8];
#pragma unroll
        for (int k = 0; k < 8; k++) keys[k] = A.sh_keys[(size_t)s * 8u + k];
        // the bounding cell box of the linked keys, in world units: most (query, shared section) pairs end at its integer test, the rest at the shape's prune
        uint32_t b0[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, b1[3] = { 0u, 0u, 0u };
#pragma unroll
        for (int k = 0; k < 8; k++)
            if ((uint32_t)k < nk) {
                const uint32_t len = A.atomic << key_level(keys[k]);
                const uint32_t c[3] = { key_x(keys[k]) * len, key_y(keys[k]) * len, key_z(keys[k]) * len };
#pragma unroll
                for (int a = 0; a < 3; a++) { b0[a] = c[a] < b0[a] ? c[a] : b0[a]; b1[a] = c[a] + len > b1[a] ? c[a] + len : b1[a]; }
            }
        const typename Shape::CellBox bound = Shape::cell_box(A, b0, b1);
        // the first member (most shared sections hold one entity) is fetched ONCE, in front of the loop over the queries: a section of a high level is a
        // candidate of every query, and a lane that gathered its row per query would spend four dependent round trips on each
        const uint32_t begin = A.sh_begin[s], expect = ROW_CELL_SHARED | s;
        const uint32_t r0 = A.rows[begin];
        const bool live0 = treeq_row_live(A, r0, expect);
        Aabb a0 = {}; uint32_t id0 = 0;
        if (r0 < A.nrows) { a0 = A.row_aabb[r0]; id0 = A.row_id[r0]; }
        for (uint32_t i = 0; i < nq; i++) {
            unsigned long long bk = HIT_KEY_NONE;
            if constexpr (Mode == TREEQ_PICK) { bk = S.best[i]; if (bk == HIT_KEY_NONE) continue; }      // a tile entry without a hit walks nothing
            const uint32_t *t = tile + i * Shape::TILE_WORDS;
            if (!treeq_cells_in_range(b0, b1, t)) continue;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if ((uint32_t)k < nk) {
                    const uint32_t len = A.atomic << key_level(keys[k]);
                    const uint32_t c0[3] = { key_x(keys[k]) * len, key_y(keys[k]) * len, key_z(keys[k]) * len }, c1[3] = { c0[0] + len, c0[1] + len, c0[2] + len };
                    any = any || treeq_cells_in_range(c0, c1, t);
                }
            if (!any) continue;
            const Shape P = Shape::from_tile(t + TREEQ_TILE_HEAD);
            if constexpr (Mode == TREEQ_PICK) { if (P.misses_beyond(bound, treeq_key_value(bk))) continue; }
            else if (P.misses(bound)) continue;
            // walked ONCE for this query, however many of its linked keys lie in the range
            for (uint32_t m = 0; m < cnt; m++) {
                typename Shape::Rec rec{};
                if (m == 0u ? !(live0 && P.test(a0, &id0, q0 + i, rec)) : !treeq_row_hit(A, P, A.rows[begin + m], expect, q0 + i, rec)) continue;
                if constexpr (Mode == TREEQ_REDUCE) atomicMin(&S.best[i], treeq_key<Shape>(rec));
                else {
                    if constexpr (Mode == TREEQ_PICK) { if (treeq_key<Shape>(rec) != bk) continue; }
                    const uint32_t pos = atomicAdd(&S.n_hits, 1u);
                    if (pos < S.NHIT) S.hits[pos] = rec;
                    else Shape::store(A, atomicAdd(&A.hdr->count, 1u), rec);
                }
            }
        }
    }
    if constexpr (Mode == TREEQ_REDUCE) {
        __syncthreads();
        if (tid < nq && S.best[tid] != HIT_KEY_NONE) atomicMin(&A.best[q0 + tid], S.best[tid]);      // one global atomic per tile query that has a key
    } else treeq_flush<Shape, Mode>(A, S);
}

// Grid: workgroups [0, n) take one query each through the unique sections; the workgroups behind them take (256 shared sections) x (256 queries) each.
// 256 threads, 64-wide waves, no recursion; every loop is bounded (candidate cells by the host's cap, rb_find's probe by an empty slot of an overlay that is
// never full and a binary search, the row walks by the sections' counts).
// Publication: write-through records, every wave waits for its own stores, then the workgroup signs off (list_sign_off, re_kernels.h).
template <class Shape, int Mode = TREEQ_ALL, class KArgs> __device__ __forceinline__ void treeq_kernel(const KArgs &A, TreeqShared<Shape, Mode> &S) {
    if (threadIdx.x == 0) { S.n_hits = 0u; S.n_queue = 0u; }
    if constexpr (Mode == TREEQ_REDUCE) S.best[threadIdx.x] = HIT_KEY_NONE;      // (BOXQ_TILE == BOXQ_THREADS)
    __syncthreads();
    if (blockIdx.x < A.n) treeq_unique_part<Shape, Mode>(A, S); else treeq_shared_part<Shape, Mode>(A, S);
    if constexpr (Mode == TREEQ_REDUCE) return;                               // nothing counted, nothing published: the pick pass answers
    wait_own_stores();
    __syncthreads();                                                          // every wave's records have left; the count atomics have returned
    if (threadIdx.x == 0) list_sign_off(A.hdr, A.h_pub, A.seq);
}
static_assert(BOXQ_TILE == BOXQ_THREADS, "one lane per tile query");

// ---- the queries asked by entity: the records are built here ---------------------------------------------------------------------------------------
// One lane per ask (AroundAsk, re_kernels.h): the row's live flags, row_cell and StaticAABB / Position make the record the host builders would make for the
// same geometry -- box_query_record is theirs --, written over the ask.  The box and cube bounds and r2 are single rounded operations (__fsub_rn, __fadd_rn,
// __fmul_rn: what the host's plain f32 arithmetic does).  No loop but the levels', no LDS, nothing shared between lanes.
template <bool Spheres> __device__ __forceinline__ void around_build(const AroundBuildArgs &B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    void *rec = static_cast<char *>(B.q) + (size_t)i * 64u;
    const AroundAsk ask = *static_cast<const AroundAsk *>(rec);            // (read before the record takes its place)
    const float inf = __builtin_inff();
    uint8_t status = AROUND_NOT_IN_TREE;
    uint32_t id = AROUND_NO_ENTITY;
    float bb[6] = { inf, -inf, inf, -inf, inf, -inf }, ctr[3] = { 0.0f, 0.0f, 0.0f };
    if (ask.row < B.nrows && !(B.row_flags[ask.row] & (F_DEAD | F_PHANTOM)) && B.row_cell[ask.row] != ROW_CELL_NONE) {      // an entity of the tree (a halo replica's owner answers)
        status = AROUND_OK;
        id = B.row_id[ask.row];
        if constexpr (Spheres) {
            const float limit = 64.0f * (float)B.outline;                  // re_query_spheres refuses a centre beyond it: the margin covers the rounding below it only
#pragma unroll
            for (int a = 0; a < 3; a++) {
                ctr[a] = B.row_pos[(size_t)ask.row * 3u + a];
                if (!(fabsf(ctr[a]) <= limit)) status = AROUND_TOO_LARGE;
                bb[2 * a] = __fsub_rn(__fsub_rn(ctr[a], ask.reach), B.margin); bb[2 * a + 1] = __fadd_rn(__fadd_rn(ctr[a], ask.reach), B.margin);
            }
        } else {
            const Aabb s = B.row_aabb[ask.row];
            bb[0] = __fsub_rn(s.xmin, ask.reach); bb[1] = __fadd_rn(s.xmax, ask.reach); bb[2] = __fsub_rn(s.ymin, ask.reach); bb[3] = __fadd_rn(s.ymax, ask.reach);
            bb[4] = __fsub_rn(s.zmin, ask.reach); bb[5] = __fadd_rn(s.zmax, ask.reach);
        }
    }
    uint32_t umin[3], umax[3], flags = 0u, ncells = 0u;
    if (status == AROUND_OK) {
        const uint64_t cells = box_query_record(bb, B.outline, B.atomic, B.max_level, umin, umax, &flags);
        if (cells > B.max_cells) status = AROUND_TOO_LARGE; else ncells = (uint32_t)cells;
    }
    if (status != AROUND_OK) {                                             // the empty record (re_kernels.h)
        const uint32_t top = 2u * (B.atomic << B.max_level);
#pragma unroll
        for (int a = 0; a < 3; a++) { umin[a] = top; umax[a] = top - 1u; bb[2 * a] = inf; bb[2 * a + 1] = -inf; }
        flags = 0u; ncells = 0u;
    }
    const uint32_t exclude = (ask.flags & AROUND_INCLUDE_SELF) ? AROUND_NO_ENTITY : id;
    if constexpr (Spheres) {
        SphQuery q;
        q.r2 = status == AROUND_OK ? __fmul_rn(ask.reach, ask.reach) : -1.0f;
        q.exclude = exclude; q.flags = flags; q.ncells = ncells; q.pad[0] = q.pad[1] = q.pad[2] = 0u;
#pragma unroll
        for (int a = 0; a < 3; a++) { q.c[a] = ctr[a]; q.umin[a] = umin[a]; q.umax[a] = umax[a]; }
        *static_cast<SphQuery *>(rec) = q;
    } else {
        BoxQuery q;
#pragma unroll
        for (int a = 0; a < 6; a++) q.box[a] = bb[a];
#pragma unroll
        for (int a = 0; a < 3; a++) { q.umin[a] = umin[a]; q.umax[a] = umax[a]; }
        q.flags = flags; q.ncells = ncells; q.pad[0] = exclude; q.pad[1] = 0u;
        *static_cast<BoxQuery *>(rec) = q;
    }
    B.status[i] = status;
}
static_assert(sizeof(BoxQuery) == 64 && sizeof(SphQuery) == 64 && sizeof(AroundAsk) == 16, "an ask lies in the head of its 64-byte query record");

}  // namespace

__global__ __launch_bounds__(256) void k_around_build_boxes(AroundBuildArgs B) { around_build<false>(B); }
__global__ __launch_bounds__(256) void k_around_build_spheres(AroundBuildArgs B) { around_build<true>(B); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_box_query_around(BoxQueryArgs A) { __shared__ TreeqShared<BoxAroundShape> S; treeq_kernel<BoxAroundShape>(A, S); }

__global__ __launch_bounds__(BOXQ_THREADS) void k_box_query(BoxQueryArgs A) { __shared__ TreeqShared<BoxShape> S; treeq_kernel<BoxShape>(A, S); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_segment_query(SegQueryArgs A) { __shared__ TreeqShared<SegShape> S; treeq_kernel<SegShape>(A, S); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_sphere_query(SphQueryArgs A) { __shared__ TreeqShared<SphShape> S; treeq_kernel<SphShape>(A, S); }
// first hit per segment, nearest per sphere: reduce, then pick (two launches in the stream, no host round trip between them)
__global__ __launch_bounds__(BOXQ_THREADS) void k_segment_first_reduce(SegBestArgs A) { __shared__ TreeqShared<SegShape, TREEQ_REDUCE> S; treeq_kernel<SegShape, TREEQ_REDUCE>(A, S); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_segment_first_pick(SegBestArgs A) { __shared__ TreeqShared<SegShape, TREEQ_PICK> S; treeq_kernel<SegShape, TREEQ_PICK>(A, S); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_sphere_nearest_reduce(SphBestArgs A) { __shared__ TreeqShared<SphShape, TREEQ_REDUCE> S; treeq_kernel<SphShape, TREEQ_REDUCE>(A, S); }
__global__ __launch_bounds__(BOXQ_THREADS) void k_sphere_nearest_pick(SphBestArgs A) { __shared__ TreeqShared<SphShape, TREEQ_PICK> S; treeq_kernel<SphShape, TREEQ_PICK>(A, S); }

}  // namespace re
