// kernels_search_longest_items.hip — "where is the LEFTMOST-LONGEST match of every item" (rrx_search_longest_extents /
// rrx_search_longest_items): a lane per item on the starts table and the anchored table (lower.hpp: search_longest_dfas),
// search_extents_kernel's grid shape.  '\n' is a byte like any other.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item, a pass of the grid-stride loop per 64 consecutive items (item_lanes.hpp: the loop, the item's span, the
// walks).  Two phases per pass, each run by all lanes of the wave before the next begins:
//  * backward on starts ("any bytes, then the pattern right to left": never dies, so the WHOLE item is read - there is no early
//    exit) from the item's last byte down to its first.  Accepting after the byte at offset s: some match starts at s; `start` is
//    the last such s seen, i.e. the smallest.  No state ever accepts: no match.  Skipped where `nullable` (launch-uniform): start = 0.
//  * forward on anchored (the pattern's own DFA) from the byte at `start` to the item's end or to row 0, which is dead and absorbing
//    (pack_search_longest checks it).  Accepting after the byte at offset p: item[start, p + 1) is accepted; `end` is the last such
//    p + 1 seen, i.e. the largest.  A hit of the first phase guarantees one (the CPU replay test asserts it); a nullable pattern
//    begins with end = start = 0.
// Alignment is that of the ADDRESS (d_bytes itself may sit anywhere).  NUL and bytes >= 0x80 go through the tables' own byte ->
// class maps like every other byte.
// (8 waves per SIMD asked for: the backward loop has no exit inside its 16 bytes, and without the bound the compiler spreads the
// HBM/L2 form's lookups over 65 VGPRs - 7 waves per SIMD, which is ONE workgroup of 16 waves per CU instead of two.)
template <class StartsEngine, class AnchoredEngine>
__global__ __launch_bounds__(kThreads, 8) void search_longest_extents_kernel(SearchLongestDevice prog, uint32_t anchored_lds_off, uint32_t nullable,
                                                                              const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off,
                                                                              size_t nitems, uint32_t trim, uint32_t *__restrict__ match_start,
                                                                              uint32_t *__restrict__ match_end) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    StartsEngine starts;
    AnchoredEngine anchored;
    starts.load(prog.starts, smem);
    anchored.load(prog.anchored, smem + anchored_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;      // (p + skew) & 15 == 0: bytes + p is 16-byte aligned
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim, kMaxItemOffset);
        // ---- backward over the whole item: the smallest start
        size_t start = b;
        bool hit = nullable != 0;
        if (!nullable) {
            typename StartsEngine::State st;
            starts.reset(st);
            size_t q = e;                                // bytes [q, e) have been consumed
            auto one = [&](uint32_t c, size_t at) {
                starts.step(st, c);
                if (starts.accepting(st)) { hit = true; start = at; }
            };
            for (; q > b && ((q + skew) & 15); q--) one(bytes[q - 1], q - 1);             // down to 16-byte alignment
            for (; q >= b + 16; q -= 16) {                                               // 16 bytes per load, the high byte first
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 15; k >= 0; k--) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, q - 16 + k);
            }
            for (; q > b; q--) one(bytes[q - 1], q - 1);
        }
        // ---- forward from the start: the largest end
        uint32_t s_out = kNoMatch, e_out = kNoMatch;
        if (hit) {
            typename AnchoredEngine::State st;
            anchored.reset(st);
            size_t p = start, end = start;               // bytes [start, p) have been consumed
            bool dead = false;
            auto one = [&](uint32_t c, size_t next_p) {
                anchored.step(st, c);
                if (anchored.accepting(st)) end = next_p;
                dead = st.s == 0;
            };
            for (; p < e && ((p + skew) & 15) && !dead; p++) one(bytes[p], p + 1);       // up to 16-byte alignment
            for (; p + 16 <= e && !dead; p += 16) {                                      // 16 bytes per load
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (!dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, p + k + 1);
            }
            for (; p < e && !dead; p++) one(bytes[p], p + 1);
            s_out = (uint32_t)(start - b);
            e_out = (uint32_t)(end - b);
        }
        match_start[i] = s_out;
        match_end[i] = e_out;
    });
}

template <class StartsEngine, class AnchoredEngine>
int launch_search_longest(const SearchLongestDevice &p, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                          uint32_t *match_start, uint32_t *match_end, void *stream) {
    const size_t anchored_off = (StartsEngine::lds_bytes(p.starts) + 15) & ~(size_t)15, lds = anchored_off + AnchoredEngine::lds_bytes(p.anchored);
    return launch_item_lanes<search_longest_extents_kernel<StartsEngine, AnchoredEngine>>(lds, nitems, kItemLanesMaxBlocks, stream, p, (uint32_t)anchored_off,
                                                                                          nullable ? 1u : 0u, bytes, off, nitems, trim, match_start, match_end);
}

}  // namespace

int search_longest_extents_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                               uint32_t trim, uint32_t *match_start, uint32_t *match_end, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(p.starts) || !plain_table_ok(p.anchored)) return (int)hipErrorInvalidValue;
    if (!two_tables_in_lds(p.starts, p.anchored, in_global))
        return launch_search_longest<PlainDfaGlobalEngine, PlainDfaGlobalEngine>(p, nullable, bytes, off, nitems, trim, match_start, match_end, stream);
    return launch_search_longest<PlainDfaEngine, PlainDfaEngine>(p, nullable, bytes, off, nitems, trim, match_start, match_end, stream);
}

}  // namespace dev
}  // namespace rrx
