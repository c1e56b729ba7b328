// rl_path_list.hip.h -- the kernels behind rl_scene_step_path_list*: one segment for the path states an index list names, in place,
// and the list of those that are still live afterwards, in the order the list had them.  Included by rl_api.hip after
// rl_step.hip.h (rl_step_chunk), rl_paths.hip.h (rl_opaque, RlChunkCursor) and rl_film.hip.h (RlFilmQueue).
//
// Three launches on one stream: rl_list_step_kernel steps the listed states and leaves, per chunk of 64 list positions, the
// chunk's survivors (compacted in list order) and their number; rl_list_scan_kernel turns the numbers into running totals, in
// place; rl_list_pack_kernel copies every chunk's survivors to their place in the caller's list.  The survivors go through scratch
// memory of the call's own, so the caller's output may be the list that was read.  Nothing here takes an atomic per chunk beyond
// the step kernel's share of the chunk counter: the order of the survivors is the list's, whatever wave stepped a chunk.
#pragma once

// What a list-step launch reads beside the scene, the states and the hits.  The host writes it behind the launch's chunk counter,
// as the film's constants are (RlFilmQueue, rl_film.hip.h), instead of passing it as kernel arguments, and a chunk loads each word
// where it uses it.  With the list, its length and the survivors' scratch as arguments, five more scalar registers held across the
// persistent loop spilled (37, 42, 31 and 29 spilled SGPRs in the variants that do not stage the whole scene, against the step
// kernel's 27, 30, 20 and 21); with those three in the block the chunk index that the compaction needs behind the scan still cost
// 30, 31, 22 and 23, so the step's own launch constants (n_states, seed, stream, flags) are in the block too.
struct RlPathList {
    const uint32_t* list; // null: the identity list
    uint32_t* survivors;  // null: no compaction; else n_list slots, and the chunks' counts in the ceil(n_list / 64) words in front of them
    uint32_t n_list;
    uint32_t n_states;
    uint64_t seed;
    uint32_t stream;
    uint32_t flags;
};
struct RlPathListQueue {
    unsigned long long next; // the chunk counter: zero at launch
    RlPathList job;
};

// A launch's seed, stream and flags for rl_step_chunk (rl_step.hip.h): words of the block, loaded through an opaque copy of the
// pointer where the body uses them, so that nothing of the block is held across the scan.
struct RlPathListConsts {
    unsigned long long* queue;
    __device__ __forceinline__ const RlPathList* job() const { return &((const RlPathListQueue*)rl_opaque(queue))->job; }
    // (the same in every lane: rl_rng.h wants the launch constants in scalar registers)
    __device__ __forceinline__ uint64_t seed() const {
        const uint64_t seed = job()->seed;
        return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(seed >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)seed);
    }
    __device__ __forceinline__ uint32_t stream() const { return __builtin_amdgcn_readfirstlane(job()->stream); }
    __device__ __forceinline__ uint32_t flags() const { return job()->flags; }
};

// A list position as a state index: `listed` when k is below n_list and the entry there (k itself when the list is null: the
// identity list) is below n_states; i = 0 otherwise, so that no address is formed from an entry that was not checked.  `job` is
// a launch's block with the words list, n_list and n_states (RlPathList, RlLightJob): each is loaded where it is tested, n_states
// only under the lanes that are listed so far.  (Handed the three words as values the light kernels loaded them all up front and
// ran 3.5 % slower: DESIGN.md section 4.)
struct RlListed {
    bool listed;
    uint32_t i;
};
template <class JOB>
__device__ __forceinline__ RlListed rl_listed_index(const JOB* job, uint32_t k) {
    RlListed at;
    at.i = k;
    at.listed = k < job->n_list;
    if (const uint32_t* entries = job->list) {
        if (at.listed) at.i = entries[k];
    }
    at.listed = at.listed && at.i < job->n_states;
    if (!at.listed) at.i = 0u;
    return at;
}

// rl_step_kernel on a list: chunk c is list positions c * 64 .. c * 64 + 63, lane l steps states[list[c * 64 + l]] (or state
// c * 64 + l when the list is null: the identity list).  An entry that is not below n_states is skipped like a position past the
// end of the list: the lane idles through the scan and touches no memory (rl_listed_index).  The chunk counter, the slice rule
// and the body of a chunk are the step kernel's (RlChunkCursor, rl_step_chunk).  `queue` is the counter of an RlPathListQueue,
// written before the launch and, but for the counter, never by the kernel; its block is loaded through an opaque copy of the
// pointer where it is used, so that nothing of it is held across the scan.  When `survivors` is not null: the lanes whose state
// is live after the step write its index to survivors[c * 64 + rank], rank = the number of such lanes below (ballot + mbcnt), and
// the chunk's count of them goes to counts[c].  Slot c * 64 + rank is below n_list: a chunk has no more survivors than list
// positions.
template <int STAGE, bool CYL>
__global__ __launch_bounds__(RL_TRACE_BLOCK, RL_TRACE_WPS) __attribute__((amdgpu_num_vgpr(RL_TRACE_VGPRS / 2))) void rl_list_step_kernel(
    const RlF4* __restrict__ scene, RlSceneLayout lay, RlPathState* __restrict__ states, RlRayHit* __restrict__ hits,
    unsigned long long* __restrict__ queue) {
    const RlStagedScene staged = rl_stage_scene<STAGE>(scene, lay);
    const uint32_t lane = threadIdx.x & 63u;
    RlWaveScratch* ws = &staged.scratch[threadIdx.x >> 6];
#ifdef RL_STATS
    unsigned long long st[RL_ST_COUNT] = {};
#endif
    RlChunkCursor chunks(__builtin_amdgcn_readfirstlane(((const RlPathListQueue*)queue)->job.n_list)); // (n_list: used up before the loop)
    const RlPathListConsts consts = {queue};
    RL_T0(t_total);
    for (;;) {
        RL_T0(t_refill);
        uint32_t c;
        if (!chunks.next(queue, lane, &c)) break;
        const RlPathList* job = consts.job();
        const RlListed at = rl_listed_index(job, c * 64u + lane);
        RL_T1(RL_ST_T_REFILL, t_refill);
        const bool survives = rl_step_chunk<STAGE, CYL>(staged, lay, ws, lane, states, hits, at.i, at.listed, consts RL_TACC_ARG);
        RL_T0(t_pack);
        if (uint32_t* out = consts.job()->survivors) {
            const uint32_t done = chunks.last(); // (`c` itself would be one more register held across the scan)
            const uint64_t m = __builtin_amdgcn_ballot_w64(survives);
            if (survives) out[done * 64u + rl_mbcnt(m)] = at.i;
            if (lane == 0) (out - chunks.n_chunks)[done] = (uint32_t)__popcll(m);
        }
        RL_T1(RL_ST_T_TAIL, t_pack); // (the diagnostic build: the scan's tail-flush timer is free in this kernel)
        rl_wave_sync(); // (the next chunk's scan rewrites the wave's scratch)
    }
    RL_T1(RL_ST_T_TOTAL, t_total);
#ifdef RL_STATS
    if (lane == 0)
        for (int k = 0; k < RL_ST_COUNT; ++k) atomicAdd(&rl_stat_counters[k], st[k]);
#endif
}

#define RL_LIST_SCAN_BLOCK 1024 // one workgroup of 16 waves
#define RL_LIST_SCAN_TILE 16384 // counts per turn of its loop: 1024 per wave, four 16-byte loads per lane

// counts[0, n) become their running totals, in place: counts[c] = the survivors of chunks 0 .. c, so the last one is the call's
// n_live.  ONE workgroup (the launch has one): n is a 64th of the list, at most 2^26, and a turn of the loop moves 64 KB.  Per
// turn every wave takes 1,024 consecutive counts, four per lane and load: the lane's own four are summed in registers, the lanes'
// sums by a shuffle scan, the waves' totals through LDS (two buffers, alternating: one barrier per turn).  `counts` is 16-byte
// aligned; four counts that would reach past n are loaded and stored one by one.
__global__ __launch_bounds__(RL_LIST_SCAN_BLOCK) void rl_list_scan_kernel(uint32_t* __restrict__ counts, uint32_t n) {
    __shared__ uint32_t wave_total[2][RL_LIST_SCAN_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0; // the total of every turn before this one
    uint32_t phase = 0;
    for (uint32_t tile = 0; tile < n; tile += RL_LIST_SCAN_TILE, phase ^= 1u) {
        uint32_t v[4][4], before[4];
        uint32_t run = 0; // the wave's total so far in this turn
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = tile + wave * 1024u + (uint32_t)k * 256u + lane * 4u;
            if (e + 4u <= n) {
                const uint4 q = *(const uint4*)(counts + e);
                v[k][0] = q.x, v[k][1] = q.y, v[k][2] = q.z, v[k][3] = q.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[k][j] = e + (uint32_t)j < n ? counts[e + (uint32_t)j] : 0u;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k][1] += v[k][0];
            v[k][2] += v[k][1];
            v[k][3] += v[k][2];
            uint32_t x = v[k][3]; // the lane's four; then the inclusive scan over the lanes
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t below = __shfl_up(x, d);
                if (lane >= d) x += below;
            }
            before[k] = run + x - v[k][3];
            run += __shfl(x, 63);
        }
        if (lane == 0) wave_total[phase][wave] = run;
        __syncthreads();
        uint32_t mine = carry, all = carry;
#pragma unroll
        for (uint32_t w = 0; w < RL_LIST_SCAN_BLOCK / 64; ++w) {
            const uint32_t t = wave_total[phase][w];
            if (w < wave) mine += t;
            all += t;
        }
        carry = all;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t e = tile + wave * 1024u + (uint32_t)k * 256u + lane * 4u;
            const uint32_t base = mine + before[k];
            if (e + 4u <= n) {
                *(uint4*)(counts + e) = make_uint4(v[k][0] + base, v[k][1] + base, v[k][2] + base, v[k][3] + base);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + (uint32_t)j < n) counts[e + (uint32_t)j] = v[k][j] + base;
            }
        }
    }
}

// live_list = the chunks' survivors one behind the other: a wave per chunk (grid-stride), chunk c's survivors[c * 64 ..] to
// live_list[totals[c - 1] ..], as many as totals[c] - totals[c - 1] (at most 64, and the last ends at n_live <= n_list).  Nothing
// is written behind n_live.  live_list may be the list the step kernel read: that kernel is done.
__global__ __launch_bounds__(RL_BLOCK) void rl_list_pack_kernel(const uint32_t* __restrict__ totals, const uint32_t* __restrict__ survivors,
                                                                uint32_t n_chunks, uint32_t* __restrict__ live_list) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (RL_BLOCK / 64u);
#pragma unroll 4
    for (uint32_t c = blockIdx.x * (RL_BLOCK / 64u) + (threadIdx.x >> 6); c < n_chunks; c += waves) {
        const uint32_t base = c != 0u ? totals[c - 1u] : 0u;
        const uint32_t count = totals[c] - base;
        if (lane < count) live_list[base + lane] = survivors[c * 64u + lane];
    }
}
