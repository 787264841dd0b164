// kernels_search_all_items.hip — "where is EVERY match of every item" (rrx_search_all_extents* / rrx_search_all_items*): a lane per
// item on the two plain search tables (lower.hpp: search_dfas), search_extents_kernel's grid shape.  The matches of an item are
// those of rrx_search_extents applied again and again to the rest of the item behind the previous match.  The stripe-wise
// all-matches kernels (kernels_search.hip) are tied to '\n'; here '\n' is a byte like any other.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item, a pass gives every wave 64 CONSECUTIVE items.  One body, two modes, for patterns that do NOT accept the empty
// string (every match then has at least one byte, and the next search begins at the match end wherever the match starts):
//  * COUNT (FILL = false): forward only.  fwd ("any bytes, then the pattern") accepts exactly where a match of the text behind the
//    last reset ends; after every accepting byte the state goes back to the start row.  count[i] = the number of accepts.  The
//    reverse table is neither placed nor stepped.
//  * FILL: the same forward stream - a head up to 16-byte alignment, 16 bytes per load, a tail.  A hit does not restart the loads:
//    the state is reset and the stream goes on with the next byte of the vector already in registers (`k`: the first byte of `v`
//    not yet consumed).  After each hit the lane walks back on rev (the pattern right to left) from the hit end down to the FLOOR -
//    the end of the previous match, the item's first byte for the first one - as search_extents_kernel does down to the item's
//    first byte; it stops in dead row 0; the last accepting position is the start.  A hit guarantees an accepting position at or
//    above the floor: fwd was reset there.  Match n of item i goes to slot first[i] + n if that slot is below `cap`.
// No byte outside the item is ever read: a wide load is used only where all its 16 bytes lie inside [item start, item end), and,
// walking back, inside [floor, hit end).  Alignment is that of the ADDRESS (d_bytes itself may sit anywhere).
// A wave takes as long as its longest item, and a lane's result stores are scattered (one slot run per item).
template <class Engine, bool FILL>
__global__ __launch_bounds__(kThreads) void search_all_extents_kernel(SearchItemsDevice prog, uint32_t rev_lds_off, const uint8_t *__restrict__ bytes,
                                                                       const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                       uint32_t *__restrict__ count, const uint64_t *__restrict__ first,
                                                                       uint32_t *__restrict__ match_start, uint32_t *__restrict__ match_end, uint64_t cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Engine fwd, rev;
    fwd.load(prog.fwd, smem);
    if constexpr (FILL) rev.load(prog.rev, smem + rev_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;      // (p + skew) & 15 == 0: bytes + p is 16-byte aligned
    // (for_each_wave_pass, written out: through the helper's lambda the compiler lays the FILL body out differently)
    const uint32_t lane = threadIdx.x & 63u;
    const size_t per_pass = (size_t)gridDim.x * kThreads;
    for (size_t first_item = (size_t)blockIdx.x * kThreads + (threadIdx.x - lane); first_item < nitems; first_item += per_pass) {
        const size_t i = first_item + lane;
        if (i >= nitems) continue;
        const auto [b, e] = item_span(off, i, trim, kMaxItemOffset);
        uint64_t slot = 0;                               // FILL: where this item's next match goes
        if constexpr (FILL) slot = first[i];
        uint32_t n = 0;                                  // matches so far
        typename Engine::State st;
        fwd.reset(st);
        size_t p = b, floor = b;
        uint4 v = make_uint4(0, 0, 0, 0);
        uint32_t k = 0;                                  // FILL: bytes of `v` (loaded from p) already consumed; 0: nothing loaded
        for (;;) {
            // ---- forward to the next hit (COUNT: to the end of the item - `hit` is never set)
            bool hit = false;
            size_t hit_end = 0;                          // one past the byte that made fwd accept
            auto one = [&](uint32_t c, size_t next_p) {
                fwd.step(st, c);
                if (fwd.accepting(st)) {
                    fwd.reset(st);
                    if constexpr (FILL) { hit = true; hit_end = next_p; }
                    else n++;
                }
            };
            for (; p < e && ((p + skew) & 15) && !hit; p++) one(bytes[p], p + 1);      // up to 16-byte alignment (and on through a short tail)
            while (p + 16 <= e && !hit) {                                              // 16 bytes per load
                if (k == 0) v = *reinterpret_cast<const uint4 *>(bytes + p);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                uint32_t next_k = 16;
#pragma unroll
                for (uint32_t j = 0; j < 16; j++)
                    if (j >= k && !hit) { one((w[j >> 2] >> (8 * (j & 3))) & 0xffu, p + j + 1); if (hit) next_k = j + 1; }
                k = next_k & 15u;                        // (16: the vector is used up)
                if (k == 0) p += 16;
            }
            for (; p < e && !hit; p++) one(bytes[p], p + 1);
            if (!FILL || !hit) break;
            // ---- backward from the hit down to the floor: the smallest start
            {
                typename Engine::State rs;
                rev.reset(rs);
                size_t q = hit_end, start = hit_end;     // bytes [q, hit_end) have been consumed
                bool dead = false;
                auto back = [&](uint32_t c, size_t at) {
                    rev.step(rs, c);
                    if (rev.accepting(rs)) start = at;
                    dead = rs.s == 0;
                };
                for (; q > floor && ((q + skew) & 15) && !dead; q--) back(bytes[q - 1], q - 1);   // down to 16-byte alignment
                for (; q >= floor + 16 && !dead; q -= 16) {                                       // 16 bytes per load, the high byte first
                    const uint4 u = *reinterpret_cast<const uint4 *>(bytes + q - 16);
                    const uint32_t x[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                    for (int j = 15; j >= 0; j--)
                        if (!dead) back((x[j >> 2] >> (8 * (j & 3))) & 0xffu, q - 16 + j);
                }
                for (; q > floor && !dead; q--) back(bytes[q - 1], q - 1);
                if (slot + n < cap) {
                    match_start[slot + n] = (uint32_t)(start - b);
                    match_end[slot + n] = (uint32_t)(hit_end - b);
                }
                n++;
                floor = hit_end;
            }
        }
        if constexpr (!FILL) count[i] = n;
    }
}

// A pattern that accepts the empty string: the matches of an item are [k, k) for k = 0 .. its trimmed length - no table, no text.
// FILL = false: count[i] = length + 1.  FILL = true: the slots first[i], first[i] + 1, ... below `cap`.
template <bool FILL>
__global__ __launch_bounds__(256) void empty_item_matches_kernel(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim, uint32_t *__restrict__ count,
                                                                 const uint64_t *__restrict__ first, uint32_t *__restrict__ match_start,
                                                                 uint32_t *__restrict__ match_end, uint64_t cap) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nitems) return;
    const uint64_t b = off[i], e = off[i + 1];
    uint64_t len = e - b >= trim ? e - b - trim : 0;
    if (len > kMaxItemOffset) len = kMaxItemOffset;         // (matches that end beyond offset 0xFFFFFFFE are not reported)
    if constexpr (!FILL) { count[i] = (uint32_t)(len + 1); return; }
    const uint64_t slot = first[i];
    for (uint64_t k = 0; k <= len && slot + k < cap; k++) { match_start[slot + k] = (uint32_t)k; match_end[slot + k] = (uint32_t)k; }
}

template <class Engine, bool FILL>
int launch_search_all_extents(const SearchItemsDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *count,
                              const uint64_t *first, uint32_t *match_start, uint32_t *match_end, size_t cap, void *stream) {
    // COUNT places the forward table only
    const size_t rev_off = (Engine::lds_bytes(p.fwd) + 15) & ~(size_t)15, lds = FILL ? rev_off + Engine::lds_bytes(p.rev) : Engine::lds_bytes(p.fwd);
    return launch_item_lanes<search_all_extents_kernel<Engine, FILL>>(lds, nitems, kItemLanesMaxBlocks, stream, p, (uint32_t)rev_off, bytes, off, nitems, trim,
                                                                      count, first, match_start, match_end, (uint64_t)cap);
}

}  // namespace

int search_all_extents_dfa(const SearchItemsDevice &p, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                           uint32_t *count, const uint64_t *first, uint32_t *match_start, uint32_t *match_end, size_t cap, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(p.fwd) || !plain_table_ok(p.rev)) return (int)hipErrorInvalidValue;
    // search_extents_dfa's placement rule, for both modes
    const bool global = !two_tables_in_lds(p.fwd, p.rev, in_global);
    if (!first)
        return global ? launch_search_all_extents<PlainDfaGlobalEngine, false>(p, bytes, off, nitems, trim, count, first, match_start, match_end, cap, stream)
                      : launch_search_all_extents<PlainDfaEngine, false>(p, bytes, off, nitems, trim, count, first, match_start, match_end, cap, stream);
    return global ? launch_search_all_extents<PlainDfaGlobalEngine, true>(p, bytes, off, nitems, trim, count, first, match_start, match_end, cap, stream)
                  : launch_search_all_extents<PlainDfaEngine, true>(p, bytes, off, nitems, trim, count, first, match_start, match_end, cap, stream);
}

int empty_item_matches(const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *count, const uint64_t *first, uint32_t *match_start,
                       uint32_t *match_end, size_t cap, void *stream) {
    if (!nitems) return 0;
    const dim3 grid((unsigned)((nitems + 255) / 256));
    if (first) hipLaunchKernelGGL(empty_item_matches_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, off, nitems, trim, count, first, match_start, match_end, (uint64_t)cap);
    else hipLaunchKernelGGL(empty_item_matches_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, off, nitems, trim, count, first, match_start, match_end, (uint64_t)cap);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
