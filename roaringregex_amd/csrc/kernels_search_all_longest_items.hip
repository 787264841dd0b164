// kernels_search_all_longest_items.hip — "where is EVERY LEFTMOST-LONGEST match of every item" (rrx_search_all_longest_extents* /
// rrx_search_all_longest_items*): a lane per item on the starts table and the anchored table of the leftmost-longest first match
// (lower.hpp: search_longest_dfas), search_longest_extents_kernel's grid shape.  The matches of an item are those of
// rrx_search_longest_extents applied again and again to the rest of the item behind the previous match.  '\n' is a byte like any other.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item, a pass of the grid-stride loop per 64 consecutive items (item_lanes.hpp: the loop, the item's span, the
// walks).  One body, two modes:
//  * COUNT (FILL = false): first the backward walk of search_longest_extents_kernel on starts, over the WHOLE item (that table
//    never dies).  Accepting after the byte at offset s: some match starts at s - its MARK bit is set.  The marks of 32 consecutive
//    offsets are gathered in a register (`acc`) and stored each time the walk crosses a mark-word boundary downwards, and once more
//    at the item's first byte: every word of the item's range is stored, all-zero words included, nothing is cleared beforehand.
//    Then the forward phase, which counts: count[i] = n.
//  * FILL: the forward phase alone on the marks COUNT left; match n of item i goes to slot first[i] + n if that slot is below `cap`.
//    The starts table is neither placed nor stepped.
// The forward phase, from p = the item's first byte: the next mark s >= p (the lane's own mark words, the bits below p masked off,
// the first set bit; the next word when there is none), then anchored (the pattern's own DFA) from the byte at s to the item's end
// or to row 0, which is dead and absorbing (pack_search_longest checks it), tested before every byte; the last accepting position
// is the end.  p = that end (one byte further after an empty match), and again.
// MARKS.  base = off[0].  The bit of byte g of item i is bit (g - base) & 31 of word ((g - base) >> 5) + i.  Offsets are monotone:
// item i's last word, ((e_i - 1 - base) >> 5) + i, lies below item i + 1's first, ((b_{i+1} - base) >> 5) + i + 1 - no two items
// share a word (no atomics, no memset), an empty item has none.  A lane reads back only words it stored itself (COUNT) or that the
// same lane of the COUNT launch stored (FILL): no fence; `marks` must stay free of const and __restrict__ for that.  Words at or
// beyond marks_words are neither stored nor read (a buffer shorter than rrx_search_all_longest_marks_words is the caller's error:
// its result is wrong, no byte outside the buffer is touched).
// `nullable` (launch-uniform: the pattern accepts the empty string): every offset 0 .. length is a start, `marks` is never touched
// and the starts table never stepped; anchored restarts at every offset that no non-empty match covers.
// Alignment is that of the ADDRESS (d_bytes itself may sit anywhere); no byte outside the item is ever read.
template <class Engine, bool FILL>
__global__ __launch_bounds__(kThreads, 8) void search_all_longest_extents_kernel(SearchLongestDevice prog, uint32_t anchored_lds_off, uint32_t nullable,
                                                                                  const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off,
                                                                                  size_t nitems, uint32_t trim, uint32_t *marks, uint64_t marks_words,
                                                                                  uint32_t *__restrict__ count, const uint64_t *__restrict__ first,
                                                                                  uint32_t *__restrict__ match_start, uint32_t *__restrict__ match_end,
                                                                                  uint64_t cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Engine starts, anchored;
    if constexpr (!FILL) starts.load(prog.starts, smem);
    anchored.load(prog.anchored, smem + anchored_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;      // (p + skew) & 15 == 0: bytes + p is 16-byte aligned
    const size_t base = off[0];                                       // (uniform)
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim, kMaxItemOffset);
        auto word_of = [&](size_t g) { return (uint64_t)((g - base) >> 5) + i; };
        // ---- COUNT, backward over the whole item: a mark wherever some match starts
        if constexpr (!FILL) {
            if (!nullable) {
                typename Engine::State st;
                starts.reset(st);
                uint32_t acc = 0;                            // the marks of the word that holds byte q - 1, of the bytes consumed so far
                size_t q = e;                                // bytes [q, e) have been consumed
                auto put = [&](uint64_t w, uint32_t v) { if (w < marks_words) marks[w] = v; };
                auto one = [&](uint32_t c, size_t at) {
                    starts.step(st, c);
                    const uint32_t bit = (uint32_t)(at - base) & 31u;
                    if (starts.accepting(st)) acc |= 1u << bit;
                    if (bit == 0) { put(word_of(at), acc); acc = 0; }
                };
                for (; q > b && ((q + skew) & 15); q--) one(bytes[q - 1], q - 1);             // down to 16-byte alignment
                for (; q >= b + 16; q -= 16) {                                               // 16 bytes per load, the high byte first
                    const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    uint32_t m16 = 0;                        // bit k: accepting after the byte at q - 16 + k
#pragma unroll
                    for (int k = 15; k >= 0; k--) {
                        starts.step(st, (w[k >> 2] >> (8 * (k & 3))) & 0xffu);
                        if (starts.accepting(st)) m16 |= 1u << k;
                    }
                    const size_t lo = q - 16;
                    const uint32_t bit = (uint32_t)(lo - base) & 31u;
                    const uint64_t x = (uint64_t)m16 << bit; // the 16 marks where they sit in the word of `lo` and, beyond bit 31, the next one
                    if (bit > 16) { put(word_of(lo) + 1, acc | (uint32_t)(x >> 32)); acc = (uint32_t)x; }     // (the boundary lies inside the 16 bytes)
                    else {
                        acc |= (uint32_t)x;
                        if (bit == 0) { put(word_of(lo), acc); acc = 0; }
                    }
                }
                for (; q > b; q--) one(bytes[q - 1], q - 1);
                if (e > b && ((b - base) & 31)) put(word_of(b), acc);                        // the item's first byte (bit 0: stored already)
            }
        }
        // ---- forward: mark, anchored walk to the largest end, again from that end
        uint64_t slot = 0;                                   // FILL: where this item's first match goes
        if constexpr (FILL) slot = first[i];
        uint32_t n = 0;                                      // matches so far
        size_t p = b;                                        // the search position
        for (;;) {
            size_t s = p;
            if (nullable) {
                if (p > e) break;
            } else {
                bool found = false;
                while (p < e) {
                    const uint64_t w = word_of(p);
                    const uint32_t bit = (uint32_t)(p - base) & 31u;
                    const uint32_t m = (w < marks_words ? marks[w] : 0u) & (~0u << bit);
                    if (m) { s = p - bit + (uint32_t)__builtin_ctz(m); found = true; break; }
                    p = p - bit + 32;
                }
                if (!found || s >= e) break;                 // (a mark at or behind the item's end: not this lane's marks)
            }
            typename Engine::State st;
            anchored.reset(st);
            size_t r = s, end = s;                           // bytes [s, r) have been consumed
            bool dead = false;
            auto one = [&](uint32_t c, size_t next_r) {
                anchored.step(st, c);
                if (anchored.accepting(st)) end = next_r;
                dead = st.s == 0;
            };
            for (; r < e && ((r + skew) & 15) && !dead; r++) one(bytes[r], r + 1);           // up to 16-byte alignment
            for (; r + 16 <= e && !dead; r += 16) {                                          // 16 bytes per load
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + r);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (!dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, r + k + 1);
            }
            for (; r < e && !dead; r++) one(bytes[r], r + 1);
            if constexpr (FILL) {
                if (slot + n < cap) {
                    match_start[slot + n] = (uint32_t)(s - b);
                    match_end[slot + n] = (uint32_t)(end - b);
                }
            }
            n++;
            p = end > s ? end : s + 1;                       // (an empty match: one byte further)
        }
        if constexpr (!FILL) count[i] = n;
    });
}

template <class Engine, bool FILL>
int launch_search_all_longest(const SearchLongestDevice &p, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                              uint32_t *marks, size_t marks_words, uint32_t *count, const uint64_t *first, uint32_t *match_start, uint32_t *match_end,
                              size_t cap, void *stream) {
    // FILL places the anchored table only
    const size_t anchored_off = FILL ? 0 : (Engine::lds_bytes(p.starts) + 15) & ~(size_t)15, lds = anchored_off + Engine::lds_bytes(p.anchored);
    return launch_item_lanes<search_all_longest_extents_kernel<Engine, FILL>>(lds, nitems, kItemLanesMaxBlocks, stream, p, (uint32_t)anchored_off,
                                                                              nullable ? 1u : 0u, bytes, off, nitems, trim, marks, (uint64_t)marks_words,
                                                                              count, first, match_start, match_end, (uint64_t)cap);
}

}  // namespace

size_t search_all_longest_marks_words(size_t extent_bytes, size_t nitems) { return extent_bytes / 32 + nitems + 1; }

int search_all_longest_extents_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                                   uint32_t trim, uint32_t *marks, size_t marks_words, uint32_t *count, const uint64_t *first, uint32_t *match_start,
                                   uint32_t *match_end, size_t cap, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(p.starts) || !plain_table_ok(p.anchored)) return (int)hipErrorInvalidValue;
    // search_longest_extents_dfa's placement rule, for both modes
    const bool global = !two_tables_in_lds(p.starts, p.anchored, in_global);
    if (!first)
        return global ? launch_search_all_longest<PlainDfaGlobalEngine, false>(p, nullable, bytes, off, nitems, trim, marks, marks_words, count, first,
                                                                               match_start, match_end, cap, stream)
                      : launch_search_all_longest<PlainDfaEngine, false>(p, nullable, bytes, off, nitems, trim, marks, marks_words, count, first, match_start,
                                                                         match_end, cap, stream);
    return global ? launch_search_all_longest<PlainDfaGlobalEngine, true>(p, nullable, bytes, off, nitems, trim, marks, marks_words, count, first, match_start,
                                                                          match_end, cap, stream)
                  : launch_search_all_longest<PlainDfaEngine, true>(p, nullable, bytes, off, nitems, trim, marks, marks_words, count, first, match_start,
                                                                    match_end, cap, stream);
}

}  // namespace dev
}  // namespace rrx
