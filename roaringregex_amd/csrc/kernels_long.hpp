// kernels_long.hpp — the chunk maps of one long string on a plain DFA, shared by kernels_long.hip (rrx_match_string: the state the
// string ENDS in) and kernels_long_search.hip (rrx_search_longest_string: the state every chunk is ENTERED in): the widened table,
// the walks, the four-step map build in WALKING order (BACK = false: chunk 0 holds the string's first bytes and is walked left to
// right; BACK = true: chunk 0 holds its last bytes and is walked right to left), and the composition of a group of maps.
// Everything here sits in the unnamed namespace, as in kernels_common.hpp: each of the two units compiles its own copy of what it
// launches (kernels_long.hip the forward map kernels and long_compose_kernel, kernels_long_search.hip both directions and
// long_compose_kernel again), with its own LDS slots.  The duplication is intended: the units share source, not device symbols.
#pragma once
#include "kernels_common.hpp"

namespace rrx {
namespace dev {
namespace {

// Chunk maps.  LDS: the plain DFA widened to one u16 entry per (state, byte value 0..127 | >= 0x80), entry = row
// offset of the next state (state * 129), so a step is one clamp, one add and one ds_read_u16.
constexpr int kLongThreads = 256;
//
// Convergence (round 2): stepping a chunk from EVERY state costs D times the text.  But a DFA forgets where it started:
// after a few dozen bytes the D runs of a chunk sit in one, two, three different states (a whole-string match against
// running text is dead almost at once).  So the chunk maps are built in four steps:
//   A  long_maps_kernel with limit = kLongPrefix: the state after the first 64 bytes walked of the chunk, from every state;
//   B  long_continue_kernel: lane = (chunk, slot j < kLongSlots): the j-th DISTINCT state among those D, stepped through
//      the rest of the chunk - 4 lanes per chunk instead of D; a chunk with more distinct states is flagged;
//   A' long_maps_kernel with limit = chunk for the flagged chunks only (the old way: automata that count, a{1,200} on a's);
//   C  long_expand_kernel: map[s] = result of the slot that holds prefix_state[s].
constexpr uint32_t kLongPrefix = 64, kLongSlots = 4;
__device__ __forceinline__ void long_load_wide(const DfaDevice &p, uint16_t *wide) {
    const uint32_t D = p.nstates;
    for (uint32_t i = threadIdx.x; i < D * kWideColumns; i += blockDim.x) {
        const uint32_t s = i / kWideColumns, c = i % kWideColumns;
        wide[i] = (uint16_t)(p.next[s * p.ncls + p.cls[c]] * kWideColumns);     // column 128 stands for every byte >= 0x80
    }
}
// the row after bytes [pos, b) from `row` (pos 16-byte aligned if the base pointer is)
__device__ __forceinline__ uint32_t long_walk(const uint16_t *wide, const uint8_t *__restrict__ bytes, size_t pos, size_t b, uint32_t row) {
    if ((reinterpret_cast<uintptr_t>(bytes + pos) & 15) == 0) {
        for (; pos + 16 <= b; pos += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
                row = wide[row + (c < 128 ? c : 128)];
            }
        }
    }
    for (; pos < b; pos++) {
        const uint32_t c = bytes[pos];
        row = wide[row + (c < 128 ? c : 128)];
    }
    return row;
}
// the row after bytes [a, q) walked RIGHT TO LEFT from `row`: single bytes down to a 16-byte aligned address (b itself may sit
// anywhere: the chunks of a backward run are counted from the string's end), then 16 bytes per load, the high byte first
__device__ __forceinline__ uint32_t long_walk_back(const uint16_t *wide, const uint8_t *__restrict__ bytes, size_t a, size_t q, uint32_t row) {
    for (; q > a && (reinterpret_cast<uintptr_t>(bytes + q) & 15); q--) {
        const uint32_t c = bytes[q - 1];
        row = wide[row + (c < 128 ? c : 128)];
    }
    for (; q >= a + 16; q -= 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 15; i >= 0; i--) {
            const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
            row = wide[row + (c < 128 ? c : 128)];
        }
    }
    for (; q > a; q--) {
        const uint32_t c = bytes[q - 1];
        row = wide[row + (c < 128 ? c : 128)];
    }
    return row;
}
// Bytes [a, b) of chunk k in walking order: forwards they are counted from the string's first byte, backwards from its last
template <bool BACK>
__device__ __forceinline__ void long_chunk_span(size_t k, uint32_t chunk, size_t nbytes, size_t &a, size_t &b) {
    if constexpr (BACK) {
        b = nbytes - k * (size_t)chunk;
        a = b > chunk ? b - chunk : 0;
    } else {
        a = k * (size_t)chunk;
        b = a + chunk < nbytes ? a + chunk : nbytes;
    }
}
// maps[k][s] = state after the first `limit` bytes walked of chunk k from state s; with `only`: just the chunks flagged there
template <bool BACK>
__global__ __launch_bounds__(kLongThreads) void long_maps_kernel(DfaDevice p, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t chunk,
                                                                 uint32_t nchunks, uint16_t *__restrict__ maps, uint32_t limit,
                                                                 const uint8_t *__restrict__ only) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *wide = reinterpret_cast<uint16_t *>(smem);
    const uint32_t D = p.nstates;
    const uint32_t per_block = kLongThreads / D, ci = threadIdx.x / D, s0 = threadIdx.x % D;
    // the workgroups take batch after batch of per_block chunks: the table (D * 129 entries, two dependent loads and a
    // division each) is built once per workgroup, not once per batch
    bool loaded = false;
    for (size_t k0 = (size_t)blockIdx.x * per_block; k0 < nchunks; k0 += (size_t)gridDim.x * per_block) {
        const size_t k = k0 + ci;
        const bool mine = ci < per_block && k < nchunks && (!only || only[k]);
        if (only && !__syncthreads_or(mine ? 1 : 0)) continue;       // nothing flagged in this batch
        if (!loaded) { long_load_wide(p, wide); __syncthreads(); loaded = true; }
        if (!mine) continue;
        size_t a, b;
        long_chunk_span<BACK>(k, chunk, nbytes, a, b);
        if constexpr (BACK) {
            if (a + limit < b) a = b - limit;
            maps[k * D + s0] = (uint16_t)(long_walk_back(wide, bytes, a, b, s0 * kWideColumns) / kWideColumns);
        } else {
            if (a + limit < b) b = a + limit;
            maps[k * D + s0] = (uint16_t)(long_walk(wide, bytes, a, b, s0 * kWideColumns) / kWideColumns);
        }
    }
}
// B: lane = (chunk, slot).  pre[k][*] = the D prefix states of chunk k (step A).  dist[k][j] = j-th distinct one (0xffff: none),
// res[k][j] = the state it reaches at the end of the chunk; flags[k] = 1 if there are more than kLongSlots.
template <bool BACK>
__global__ __launch_bounds__(kLongThreads) void long_continue_kernel(DfaDevice p, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t chunk,
                                                                     uint32_t nchunks, const uint16_t *__restrict__ pre, uint16_t *__restrict__ dist,
                                                                     uint16_t *__restrict__ res, uint8_t *__restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *wide = reinterpret_cast<uint16_t *>(smem);
    const uint32_t D = p.nstates;
    long_load_wide(p, wide);
    __syncthreads();
    const size_t lane = (size_t)blockIdx.x * kLongThreads + threadIdx.x;
    const size_t k = lane / kLongSlots;
    const uint32_t j = (uint32_t)(lane % kLongSlots);
    if (k >= nchunks) return;
    uint32_t list[kLongSlots];
    uint32_t cnt = 0;                                                // distinct prefix states seen, in order of first appearance
#pragma unroll
    for (uint32_t i = 0; i < kLongSlots; i++) list[i] = 0xffffu;
    for (uint32_t s = 0; s < D && cnt <= kLongSlots; s++) {
        const uint32_t v = pre[k * D + s];
        bool seen = false;
#pragma unroll
        for (uint32_t i = 0; i < kLongSlots; i++) seen |= i < cnt && list[i] == v;
        if (!seen) {
#pragma unroll
            for (uint32_t i = 0; i < kLongSlots; i++)
                if (i == cnt) list[i] = v;
            cnt++;
        }
    }
    if (cnt > kLongSlots) { if (j == 0) flags[k] = 1; return; }
    uint32_t mine = 0xffffu;
#pragma unroll
    for (uint32_t i = 0; i < kLongSlots; i++)
        if (i == j) mine = list[i];
    dist[k * kLongSlots + j] = (uint16_t)mine;
    if (j == 0) flags[k] = 0;
    if (mine == 0xffffu) return;
    size_t a, b;
    long_chunk_span<BACK>(k, chunk, nbytes, a, b);
    if constexpr (BACK) {
        const size_t upto = a + kLongPrefix < b ? b - kLongPrefix : a;
        res[k * kLongSlots + j] = (uint16_t)(long_walk_back(wide, bytes, a, upto, mine * kWideColumns) / kWideColumns);
    } else {
        const size_t from = a + kLongPrefix < b ? a + kLongPrefix : b;
        res[k * kLongSlots + j] = (uint16_t)(long_walk(wide, bytes, from, b, mine * kWideColumns) / kWideColumns);
    }
}
// C: lane = (chunk, state), in place: maps[k][s] holds the prefix state and receives the chunk's map entry
__global__ __launch_bounds__(kLongThreads) void long_expand_kernel(uint16_t *__restrict__ maps, uint32_t D, uint32_t nchunks,
                                                                   const uint16_t *__restrict__ dist, const uint16_t *__restrict__ res,
                                                                   const uint8_t *__restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * kLongThreads + threadIdx.x;
    if (i >= (size_t)nchunks * D) return;
    const size_t k = i / D;
    if (flags[k]) return;                                            // built the old way (step A')
    const uint32_t v = maps[i];
    uint32_t out = 0;
#pragma unroll
    for (uint32_t j = 0; j < kLongSlots; j++)
        if (dist[k * kLongSlots + j] == v) out = res[k * kLongSlots + j];
    maps[i] = (uint16_t)out;
}
// out[g] = in[g*group + group-1] o ... o in[g*group]   (one lane per start state).  The group's maps are copied into LDS
// first (coalesced) and composed from there: composing straight from HBM/L2 was `group` dependent round trips per level,
// 90 us for 128, and three levels were most of the time of a string of a few MiB.
__global__ __launch_bounds__(kLongThreads) void long_compose_kernel(const uint16_t *__restrict__ in, uint32_t nin, uint32_t D, uint32_t group,
                                                                    uint16_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *sm = reinterpret_cast<uint16_t *>(smem);
    const size_t lo = (size_t)blockIdx.x * group, hi = lo + group < nin ? lo + group : nin;
    const uint32_t cnt = (uint32_t)(hi - lo);
    for (uint32_t i = threadIdx.x; i < cnt * D; i += kLongThreads) sm[i] = in[lo * D + i];
    __syncthreads();
    const uint32_t j = threadIdx.x;
    if (j >= D) return;
    uint32_t s = j;
    for (uint32_t k = 0; k < cnt; k++) s = sm[k * D + s];
    out[(size_t)blockIdx.x * D + j] = (uint16_t)s;
}

// The four steps on the stream: level 0 of the maps into `maps` (n * D entries), on dist / res (n * kLongSlots entries each) and
// flags (n bytes).  The LDS attributes of the two table kernels are the caller's (ensure_dynamic_lds, once per instantiation).
template <bool BACK>
void long_build_maps(const DfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t chunk, uint32_t n, uint16_t *maps, uint16_t *dist, uint16_t *res,
                     uint8_t *flags, hipStream_t st) {
    const uint32_t D = p.nstates;
    const size_t lds = (size_t)D * kWideColumns * sizeof(uint16_t);
    const uint32_t per_block = kLongThreads / D;
    const uint32_t batches = (n + per_block - 1) / per_block;
    const dim3 by_state(batches < 2048 ? batches : 2048);
    if (chunk > 2 * kLongPrefix) {
        hipLaunchKernelGGL(long_maps_kernel<BACK>, by_state, dim3(kLongThreads), lds, st, p, bytes, nbytes, chunk, n, maps, kLongPrefix, nullptr);
        hipLaunchKernelGGL(long_continue_kernel<BACK>, dim3((unsigned)(((size_t)n * kLongSlots + kLongThreads - 1) / kLongThreads)), dim3(kLongThreads), lds, st,
                           p, bytes, nbytes, chunk, n, maps, dist, res, flags);
        hipLaunchKernelGGL(long_maps_kernel<BACK>, by_state, dim3(kLongThreads), lds, st, p, bytes, nbytes, chunk, n, maps, chunk, flags);
        hipLaunchKernelGGL(long_expand_kernel, dim3((unsigned)(((size_t)n * D + kLongThreads - 1) / kLongThreads)), dim3(kLongThreads), 0, st, maps, D, n, dist,
                           res, flags);
    } else {
        hipLaunchKernelGGL(long_maps_kernel<BACK>, by_state, dim3(kLongThreads), lds, st, p, bytes, nbytes, chunk, n, maps, chunk, nullptr);
    }
}
// The dynamic LDS of the kernels above that have some: ONE high-water slot per kernel - long_compose_kernel is no template, so its
// slot sits in no template either (a slot per direction would each believe it had set the kernel's size last).
inline hipError_t long_compose_lds(uint32_t D) {
    static LdsAttr attr;
    return ensure_dynamic_lds(attr, reinterpret_cast<const void *>(long_compose_kernel), (size_t)kLongGroup * D * sizeof(uint16_t));
}
template <bool BACK>
hipError_t long_maps_lds(uint32_t D) {
    const size_t lds = (size_t)D * kWideColumns * sizeof(uint16_t);
    static LdsAttr attr, attr2;                          // (the two kernels of this direction)
    hipError_t e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(long_maps_kernel<BACK>), lds);
    if (e == hipSuccess) e = ensure_dynamic_lds(attr2, reinterpret_cast<const void *>(long_continue_kernel<BACK>), lds);
    return e == hipSuccess ? long_compose_lds(D) : e;
}

}  // namespace
}  // namespace dev
}  // namespace rrx
