// kernels_search_items.hip — "where is the first match of every item" (rrx_search_extents / rrx_search_items): a lane per item on
// the two plain search tables (lower.hpp: search_dfas).  The stripe-wise search kernel (kernels_search.hip) is tied to '\n' through
// its product table's columns and its chunk index; this one knows items only, and '\n' is a byte like any other.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item, a pass of the grid-stride loop per 64 consecutive items (item_lanes.hpp: the loop, the item's span, the
// walks).  Two phases per pass, each run by all lanes of the wave before the next begins (a lane without a hit idles through the
// second one once per pass, not once per byte):
//  * forward on fwd ("any bytes, then the pattern": never dies, accepting exactly where a match ends) from the item's first
//    byte until the first byte after which the state accepts: that byte's offset + 1 is `end`.  No state ever accepts: no match.
//  * backward on rev (the pattern right to left) from the byte at end - 1 down to the item's first byte.  Accepting after the byte
//    at offset s: item[s, end) is accepted; `start` is the last such s seen, i.e. the smallest.  Row 0 of rev is dead and absorbing
//    (pack_search_items checks it): a lane stops reading there.  A hit guarantees at least one accepting position (the CPU replay
//    test asserts it).
// Alignment is that of the ADDRESS (d_bytes itself may sit anywhere).  NUL and bytes >= 0x80 go through the tables' own byte ->
// class maps like every other byte.
template <class FwdEngine, class RevEngine>
__global__ __launch_bounds__(kThreads) void search_extents_kernel(SearchItemsDevice prog, uint32_t rev_lds_off, const uint8_t *__restrict__ bytes,
                                                                   const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                   uint32_t *__restrict__ match_start, uint32_t *__restrict__ match_end) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    FwdEngine fwd;
    RevEngine rev;
    fwd.load(prog.fwd, smem);
    rev.load(prog.rev, smem + rev_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;      // (p + skew) & 15 == 0: bytes + p is 16-byte aligned
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim, kMaxItemOffset);
        // ---- forward: the smallest end
        size_t hit_end = 0;                              // one past the byte that made fwd accept
        bool hit = false;
        {
            typename FwdEngine::State st;
            fwd.reset(st);
            size_t p = b;
            auto one = [&](uint32_t c, size_t next_p) {
                fwd.step(st, c);
                if (fwd.accepting(st)) { hit = true; hit_end = next_p; }
            };
            for (; p < e && ((p + skew) & 15) && !hit; p++) one(bytes[p], p + 1);      // up to 16-byte alignment
            for (; p + 16 <= e && !hit; p += 16) {                                     // 16 bytes per load
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (!hit) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, p + k + 1);
            }
            for (; p < e && !hit; p++) one(bytes[p], p + 1);
        }
        // ---- backward from the hit: the smallest start
        uint32_t s_out = kNoMatch, e_out = kNoMatch;
        if (hit) {
            typename RevEngine::State st;
            rev.reset(st);
            size_t q = hit_end, start = hit_end;         // bytes [q, hit_end) have been consumed
            bool dead = false;
            auto one = [&](uint32_t c, size_t at) {
                rev.step(st, c);
                if (rev.accepting(st)) start = at;
                dead = st.s == 0;
            };
            for (; q > b && ((q + skew) & 15) && !dead; q--) one(bytes[q - 1], q - 1);   // down to 16-byte alignment
            for (; q >= b + 16 && !dead; q -= 16) {                                      // 16 bytes per load, the high byte first
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 15; k >= 0; k--)
                    if (!dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, q - 16 + k);
            }
            for (; q > b && !dead; q--) one(bytes[q - 1], q - 1);
            s_out = (uint32_t)(start - b);
            e_out = (uint32_t)(hit_end - b);
        }
        match_start[i] = s_out;
        match_end[i] = e_out;
    });
}

template <class FwdEngine, class RevEngine>
int launch_search_extents(const SearchItemsDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *match_start,
                          uint32_t *match_end, void *stream) {
    const size_t rev_off = (FwdEngine::lds_bytes(p.fwd) + 15) & ~(size_t)15, lds = rev_off + RevEngine::lds_bytes(p.rev);
    return launch_item_lanes<search_extents_kernel<FwdEngine, RevEngine>>(lds, nitems, kItemLanesMaxBlocks, stream, p, (uint32_t)rev_off, bytes, off, nitems, trim,
                                                                          match_start, match_end);
}

}  // namespace

int search_extents_dfa(const SearchItemsDevice &p, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                       uint32_t *match_start, uint32_t *match_end, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(p.fwd) || !plain_table_ok(p.rev)) return (int)hipErrorInvalidValue;
    if (!two_tables_in_lds(p.fwd, p.rev, in_global))
        return launch_search_extents<PlainDfaGlobalEngine, PlainDfaGlobalEngine>(p, bytes, off, nitems, trim, match_start, match_end, stream);
    return launch_search_extents<PlainDfaEngine, PlainDfaEngine>(p, bytes, off, nitems, trim, match_start, match_end, stream);
}

}  // namespace dev
}  // namespace rrx
