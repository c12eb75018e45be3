// The frame's entity-logic call list on the resident world: LogicFlow::update_logic (flows/logic_flow.rs:245, body :662-734, with
// find_always_execute_entities :801-837) up to the callbacks, for gfx950.
//
// The reference walks the tree: the local entities of the active visible sections (once per listing of the section in
// visible_sections_vec), the entities of the shared sections those link (once, if the shared AABB is in view of either culler), and the
// always-execute entities of sections that are not visible; apply_entity_logic then calls entity_logic[type] / random_entity_logic[type]
// where the type has one.  Here the walk is turned round: the host keeps the rows whose entity type is in the logic table (ascending row,
// with the table index and the function bits of each), and one lane per listed row asks the frame's cull stamps whether -- and how often --
// the walk would reach it (logic_gate_times, re_kernels.h: the gate of k_tick and k_col_moved).  No tree, no hash probes.
#include "re_kernels.h"

namespace re {

__device__ __forceinline__ uint32_t logic_mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// One lane per listed row, 256 threads.
//   round trip 1: the row and its word (logic_index | which << 16), coalesced
//   round trip 2: flags[r] and row_cell[r]; a wave without a live candidate does nothing more
//   then the gathered stamp of the row's section (or the eight sh_cells entries and sh_aabb of its shared section), and id[r] for the lanes that are listed
// Compaction: ballot + mbcnt inside the wave, the four waves' counts summed in LDS, ONE global atomicAdd per workgroup that lists anything.  Each listed row
// yields at most one record, so a list of n records cannot overflow.
// The records are read by the host as soon as it has seen the count -- while other workgroups' plain stores could still sit in their XCD's L2 --, so they
// are write-through stores (sc1), and every storing wave waits for its own (s_waitcnt vmcnt(0)) before its workgroup signs off (list_sign_off, re_kernels.h).
__global__ __launch_bounds__(256) void k_logic_list(uint32_t n, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ words, const uint32_t *__restrict__ row_flags,
                                                    const uint32_t *__restrict__ row_id, const uint32_t *__restrict__ row_cell, const uint32_t *__restrict__ cell_stamp,
                                                    const uint8_t *__restrict__ cell_flags, const int32_t *__restrict__ sh_cells, const Aabb *__restrict__ sh_aabb,
                                                    const FrameParams *__restrict__ Pp, LogicHeader *hdr, unsigned long long *__restrict__ out, LogicPublished *h_pub, uint32_t seq) {
    __shared__ uint32_t s_count[4], s_base;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, wave = threadIdx.x >> 6;
    const bool in = i < n;
    const uint32_t r = in ? rows[i] : 0u, word = in ? words[i] : 0u;
    const uint32_t fl = in ? row_flags[r] : F_DEAD, rc = in ? row_cell[r] : ROW_CELL_NONE;
    // a static entity is reached through RE_F_ALWAYS_EXEC only
    const bool candidate = !(fl & (F_DEAD | F_PHANTOM)) && rc != ROW_CELL_NONE && (!(fl & F_STATIC) || (fl & F_ALWAYS_EXEC));
    uint32_t times = 0;
    if (__ballot(candidate)) {                                                // wave-uniform
        if (candidate) times = logic_gate_times(fl, rc, cell_stamp, cell_flags, sh_cells, sh_aabb, *Pp);
    }
    const uint64_t listed = __ballot(times != 0u);
    if ((threadIdx.x & 63u) == 0u) s_count[wave] = (uint32_t)__popcll(listed);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = s_count[0] + s_count[1] + s_count[2] + s_count[3];
        s_base = total ? atomicAdd(&hdr->count, total) : 0u;
    }
    __syncthreads();
    if (times) {
        uint32_t slot = s_base + logic_mbcnt(listed);
        for (uint32_t w = 0; w < wave; w++) slot += s_count[w];
        // re_logic_call: entity_id | logic_index:16 | which:8 | times:8
        const unsigned long long rec = (unsigned long long)row_id[r] | ((unsigned long long)((word & 0xFFFFu) | (((word >> 16) & 0xFFu) << 16) | (times << 24)) << 32);
        __hip_atomic_store(&out[slot], rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // global_store_dwordx2 ... sc1
    }
    if (listed) wait_own_stores();
    __syncthreads();                                                          // every wave's records have left; the count atomic has returned
    if (threadIdx.x == 0) list_sign_off(hdr, h_pub, seq);
}

}  // namespace re
