// kernels_multi_items.hip — "which patterns of a set does each item contain" (rrx_multi_contains_extents / _items): the
// lane-per-item kernel on the product table of a group of members (lower.hpp: MultiProgram), and the two small kernels that read a
// column of masks: per-pattern totals (rrx_multi_counts) and one pattern's bit as a bitmap (rrx_multi_plane).
#include "item_lanes.hpp"
#include "multi_engines.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item: contains_extents_kernel's walk (item_lanes.hpp: aligned on the offset, nothing kills), with a mask in the place
// of the verdict.  Per byte the row steps and, on the rows that carry a mask (s >= first_hit) only, the mask is ORed in - that read
// is off the dependent chain of the row lookups.  A lane stops reading once it holds every bit this table can give (m == full).
// FIRST: the lane stores its word; the launches of a set's later groups OR theirs in.  The lane owns the word either way: plain
// loads and stores, a wave's 64 stores one contiguous 256-byte row, nothing to clear beforehand.
template <class Engine, bool FIRST>
__global__ __launch_bounds__(kThreads) void multi_contains_extents_kernel(MultiDevice prog, const uint8_t *__restrict__ bytes,
                                                                           const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                           uint32_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Engine eng;
    eng.load(prog, smem);
    __syncthreads();
    const uint32_t first_hit = prog.first_hit, full = prog.full;
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim);
        uint32_t s = prog.start;
        uint32_t m = eng.mask[s];
        bool done = m == full;
        size_t p = b;
        auto one = [&](uint32_t c) {
            s = eng.step(s, c);
            if (s >= first_hit) m |= eng.mask[s];
            done = m == full;
        };
        for (; p < e && (p & 15) && !done; p++) one(bytes[p]);                 // up to 16-byte alignment
        for (; p + 16 <= e && !done; p += 16) {                                // 16 bytes per load
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (!done) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        }
        for (; p < e && !done; p++) one(bytes[p]);
        out[i] = FIRST ? m : out[i] | m;
    });
}

// Per-pattern totals of a mask column.  A pass gives a wave 64 consecutive masks; for every pattern one ballot and one popcount,
// kept by lane k for pattern k.  At the end the wave adds its 32 totals with one 64-bit atomic per pattern (lanes 0 .. 31, one
// instruction), the zero ones left out.
__global__ __launch_bounds__(kThreads) void multi_counts_kernel(const uint32_t *__restrict__ mask, size_t nitems, unsigned long long *__restrict__ counts) {
    unsigned long long mine = 0;
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        const uint32_t v = i < nitems ? mask[i] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < 32; k++) {
            const uint32_t n = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((v >> k) & 1u));
            if (lane == k) mine += n;
        }
    });
    if (mine) atomicAdd(&counts[threadIdx.x & 63u], mine);         // (mine != 0 only in a lane below 32)
}

// Bit `pattern` of every mask as a bitmap: one ballot per pass, lane 0 stores the wave's two words as contains_extents_kernel does
// (the second one only where it holds an item).
__global__ __launch_bounds__(kThreads) void multi_plane_kernel(const uint32_t *__restrict__ mask, size_t nitems, uint32_t pattern, uint32_t *__restrict__ bits) {
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        const bool hit = i < nitems && ((mask[i] >> pattern) & 1u);
        const uint64_t verdicts = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) {
            bits[first >> 5] = (uint32_t)verdicts;
            if (first + 32 < nitems) bits[(first >> 5) + 1] = (uint32_t)(verdicts >> 32);
        }
    });
}

template <class Engine>
int launch_multi(const MultiDevice &p, bool first, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *out, void *stream) {
    if (first) return launch_item_lanes<multi_contains_extents_kernel<Engine, true>>(Engine::lds_bytes(p), nitems, 0, stream, p, bytes, off, nitems, trim, out);
    return launch_item_lanes<multi_contains_extents_kernel<Engine, false>>(Engine::lds_bytes(p), nitems, 0, stream, p, bytes, off, nitems, trim, out);
}

}  // namespace

int multi_contains_extents(const MultiDevice &p, bool in_global, bool first, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                           uint32_t *out, void *stream) {
    if (!nitems) return 0;
    if (!p.nstates || !p.next || !p.cls || !p.mask || p.start >= p.nstates) return (int)hipErrorInvalidValue;
    if (in_global || MultiLdsEngine::lds_bytes(p) > kPlainDfaLdsBudget) return launch_multi<MultiGlobalEngine>(p, first, bytes, off, nitems, trim, out, stream);
    return launch_multi<MultiLdsEngine>(p, first, bytes, off, nitems, trim, out, stream);
}

int multi_counts(const uint32_t *mask, size_t nitems, unsigned long long *counts, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<multi_counts_kernel>(0, nitems, kItemLanesMaxBlocks, stream, mask, nitems, counts);
}

int multi_plane(const uint32_t *mask, size_t nitems, uint32_t pattern, uint32_t *bits, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<multi_plane_kernel>(0, nitems, kItemLanesMaxBlocks, stream, mask, nitems, pattern, bits);
}

}  // namespace dev
}  // namespace rrx
