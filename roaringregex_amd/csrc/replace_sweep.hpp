// replace_sweep.hpp — what the two regexp_replace units share, kernels_replace_items.hip (a literal replacement R) and
// kernels_replace_template_items.hip (a replacement R_k per match, put together from a template): the SIZES walk and the FILL sweep,
// each over what a unit knows about its replacement.  Included by these two units only.  Output item i = t[0:s_0] + R_0 + t[e_0:s_1]
// + R_1 + ... + R_{m-1} + t[e_{m-1}:], t = the item without its separator.
#pragma once
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// SIZES.  One lane per item (item_lanes.hpp: the loop, the item's span), walking its matches in order: pos[slot] = where the R of
// that match begins inside the OUTPUT item = s_k - (what the matches before it removed) + (the replacements before it), len[i] = the
// output item's length, saturated at ~0u.  `shift` is (the replacements so far - removed) mod 2^64.  Every one of the nitems words of
// `len` and exactly the slots first[i] .. first[i + 1] of `pos` are written with plain stores; a lane is as slow as its item has
// matches, and its loads of match_start / match_end are scattered.  too_long (may be null): set to 1 by every lane whose item's
// output has 2^30 bytes or more - the same value from every lane, a plain store (the one-call form zeroes the word and reads it
// back: scan_counts carries 30 bits).  rep_len_of(slot, L): the length of the replacement of `slot` in an item of L bytes.
template <class RepLen>
__device__ __forceinline__ void replace_sizes_walk(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim, const uint64_t *__restrict__ first,
                                                   const uint32_t *__restrict__ match_start, const uint32_t *__restrict__ match_end,
                                                   uint32_t *__restrict__ len, uint32_t *__restrict__ pos, uint32_t *__restrict__ too_long,
                                                   const RepLen &rep_len_of) {
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim);
        const uint64_t f0 = first[i], f1 = first[i + 1];
        uint64_t shift = 0;
        for (uint64_t slot = f0; slot < f1; slot++) {
            const uint64_t s = match_start[slot], en = match_end[slot];
            pos[slot] = (uint32_t)(s + shift);
            shift += rep_len_of(slot, e - b) - (en - s);
        }
        uint64_t total = (uint64_t)(e - b) + shift;
        if ((int64_t)total < 0) total = 0;                   // (a list that removes more than the item holds: not a list of this item)
        len[i] = total > 0xffffffffu ? 0xffffffffu : (uint32_t)total;
        if (too_long && total >= ((uint64_t)1 << 30)) *too_long = 1;
    });
}

// FILL.  Driven by output bytes: a lane-per-item copy loop stores 64 scattered bytes per instruction, this one 256 contiguous ones.
// A wave takes the 64 consecutive items of a pass, F .. F + 63.  Lane l stages out_off[min(F + l, nitems)] into the wave's own LDS
// row (entry 64: the pass's end; the entries behind the last item repeat it, so they are never found), then the wave sweeps the
// pass's output range [lo, hi) = [out_off[F], out_off[min(F + 64, nitems)]) in turns of 256 bytes, lane l the four bytes of one
// dword ALIGNED BY ADDRESS: the sweep starts at the dword that holds out + lo, `mis` bytes before it.  A dword that lies wholly
// inside [lo, hi) is stored as one; the partial first and last dwords byte by byte - the neighbouring wave owns the rest of them.
// For an output byte q (locate): its item = the last staged offset <= q (six steps over the 64 entries: items with empty output drop
// out); r = q - out_off[item]; k = how many of the item's pos entries are <= r (a binary search over its slots, mostly zero or one
// step); k = 0: byte r of the item; else, j the last such slot and d = r - pos[j]: the replacement says whether R_j holds byte d and
// where that byte comes from (Replacement::holds, below); if not, it is byte match_end[j] + d - |R_j| of the item.  A source offset
// at or beyond the item's end gives 0: no byte outside an item is read, whatever the lists hold, and nothing outside [lo, hi) is
// written.  What locate found holds up to `lim`, the end of the segment (the item's output, the R or a part of it, the text up to
// the next R): the bytes of a dword behind the first reuse it while q < lim.
// The span and first[] of an item are read from global memory (L1/L2 hits: neighbouring lanes ask for the same item).
// No atomics, no memset; every lane of a wave makes every turn of the pass loop, none returns early (the row is the wave's).
//
// A Replacement has two operations:
//   holds(j, at, q, item_len, in_rep, origin, lim, rep_len)   R_j begins at output byte `at` <= q in an item of item_len bytes.  If
//       it holds q: true, with in_rep = whether the byte is one of the replacement's own (byte(q - origin)) or one of the item's
//       (byte q - origin of it), origin set, lim lowered to the end of what holds q.  If not: false, with rep_len = |R_j|.
//   byte(at)                                                   byte `at` of the replacement's own bytes
constexpr uint32_t kWavesPerBlock = kThreads / 64;
// a value that every lane of the wave holds alike, into scalar registers (what comes out of LDS is a vector register to the compiler)
__device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// row: the 65 words of the calling wave in LDS
template <class Replacement>
__device__ __forceinline__ void replace_fill_sweep(uint64_t *row, const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, size_t nitems,
                                                   uint32_t trim, const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_end,
                                                   const uint32_t *__restrict__ pos, const Replacement &R, const uint64_t *__restrict__ out_off,
                                                   uint8_t *__restrict__ out) {
    for_each_wave_pass(nitems, [&](size_t first_of_lane, uint32_t lane) {
        const size_t first_item = wave_uniform(first_of_lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (the previous pass has read the row)
        __builtin_amdgcn_wave_barrier();
        row[lane] = out_off[first_item + lane < nitems ? first_item + lane : nitems];
        if (lane == 0) row[64] = out_off[first_item + 64 < nitems ? first_item + 64 : nitems];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t lo = wave_uniform(row[0]), hi = wave_uniform(row[64]);
        if (hi <= lo) return;
        const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(out) + lo) & 3u);
        const uint64_t span = (hi - lo) + mis;                      // the sweep: bytes [0, span) from the aligned dword of out + lo on
        for (uint64_t rel = (uint64_t)lane * 4; rel < span; rel += 256) {
            const uint32_t c0 = rel < mis ? mis - (uint32_t)rel : 0u;                         // (rel < mis: rel == 0)
            const uint32_t c1 = span - rel < 4 ? (uint32_t)(span - rel) : 4u;
            // the segment that holds the byte located last: output bytes below lim; R.byte(q - origin) or byte q - origin of the item at b
            uint64_t lim = 0, origin = 0, b = 0, item_len = 0;
            bool in_rep = false;
            auto locate = [&](uint64_t q) {
                uint32_t idx = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if (row[idx + step] <= q) idx += step;
                const uint64_t o0 = row[idx], o1 = row[idx + 1], r = q - o0;
                const auto [ib, ie] = item_span(off, first_item + idx, trim);
                b = ib;
                item_len = ie - ib;
                const uint64_t f0 = first[first_item + idx], f1 = first[first_item + idx + 1];
                uint64_t below = f0, above = f1 > f0 ? f1 : f0;     // slots below `below` have pos <= r, those from `above` on pos > r
                while (below < above) {
                    const uint64_t mid = below + ((above - below) >> 1);
                    if (pos[mid] <= r) below = mid + 1;
                    else above = mid;
                }
                lim = o1;
                if (below < f1) { const uint64_t next = o0 + pos[below]; if (next < lim) lim = next; }
                in_rep = false;
                origin = o0;
                if (below > f0) {
                    const uint64_t j = below - 1, at = o0 + pos[j];  // where R_j begins in the output
                    uint64_t rep_len = 0;
                    if (!R.holds(j, at, q, item_len, in_rep, origin, lim, rep_len)) origin = at + rep_len - match_end[j];
                }
            };
            uint32_t word = 0;
            for (uint32_t c = c0; c < c1; c++) {
                const uint64_t q = lo + (rel + c - mis);
                if (c == c0 || q >= lim) locate(q);
                const uint64_t at = q - origin;
                const uint32_t v = in_rep ? R.byte(at) : at < item_len ? bytes[b + at] : 0u;
                word |= v << (8 * c);
            }
            uint8_t *dst = out + lo + (rel - mis);                   // (4-byte aligned; below out + lo only where c0 > 0: not stored to)
            if (c0 == 0 && c1 == 4) *reinterpret_cast<uint32_t *>(dst) = word;
            else for (uint32_t c = c0; c < c1; c++) dst[c] = (uint8_t)(word >> (8 * c));
        }
    });
}

}  // namespace
}  // namespace dev
}  // namespace rrx
