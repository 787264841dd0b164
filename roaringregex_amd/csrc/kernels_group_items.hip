// kernels_group_items.hip — "where, inside a known stretch of every item, is the LONGEST SPLIT POINT between two languages"
// (rrx_group_spans_* / rrx_extract_group_longest_*: the span of a top-level capture group A(B)C inside the whole match, two launches
// of one kernel; rrx_group_spans_list_*: the same for every match of a match list, longest_split_list_kernel): a lane per item on an
// anchored reverse table and an anchored forward table, search_longest_extents_kernel's grid shape.  '\n' is a byte like any other.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item, a pass of the grid-stride loop per 64 consecutive items (item_lanes.hpp: the loop, the item's span, the walks).
// The lane is given the stretch [lo, hi] of its item (offsets relative to the item, clamped here: lo = min(lo, L), hi = clamp(hi,
// lo, L) for an item of L bytes - no byte outside the item is read whatever the arrays hold) and answers the LARGEST offset x in
// [lo, hi] with  fwd accepts item[lo, x)  and  rev accepts item[x, hi) read right to left.  Two phases:
//  * backward on rev (anchored: row 0 dead and absorbing, pack_group checks it) from hi down to lo.  Offset p is MARKED iff rev
//    accepts item[p, hi), hi itself iff the start state accepts.  The marks of 32 consecutive offsets are gathered in a register and
//    stored each time the walk crosses a mark-word boundary downwards, and once more at lo: EVERY word of [lo, hi] is stored, all-zero
//    words included, nothing is cleared beforehand.  In row 0 the walk stops reading text and stores the zero words that are left.
//    (Inside a 16-byte load the dead row is stepped on: it stays where it is and accepts nothing.)
//  * forward on fwd from lo to hi or to row 0, tested before every byte: lo is a candidate iff the start state accepts and lo is
//    marked, p + 1 after the byte at p iff the table accepts and p + 1 is marked; the last candidate is the answer.
// MARKS.  base = off[0].  The bit of absolute offset g in [b + lo, b + hi] of item i (b = off[i]) is bit (g - base) & 31 of word
// ((g - base) >> 5) + i - the layout of search_all_longest_extents_kernel with one position more, the item's end.  Offsets are
// monotone: item i's last word, ((e_i - base) >> 5) + i, lies below item i + 1's first, ((b_{i+1} - base) >> 5) + i + 1 - no two
// items share a word (no atomics, no memset).  A lane reads back only words it stored itself: no fence; `marks` must stay free of
// const and __restrict__ for that.  Words at or beyond marks_words are neither stored nor read.
// lo_in / hi_in / out / on_none may be the same arrays in any combination (none is __restrict__): a lane reads its own two entries
// before it writes.  out[i] = the answer relative to the item, ~0u where there is none or lo_in[i] == ~0u (such an item touches
// neither text nor marks); on_none (may be null): on_none[i] = ~0u as well in that case, and is left alone otherwise.
// Alignment is that of the ADDRESS (d_bytes itself may sit anywhere).
//
// longest_split_of: the two phases for ONE stretch [lo_raw, hi_raw] of item i (its span: `item`) -> the answer, ~0u where there is none.  Shared by
// longest_split_kernel (a stretch per item) and longest_split_list_kernel (a stretch per slot of the item's match list).
template <class RevEngine, class FwdEngine>
__device__ __forceinline__ uint32_t longest_split_of(const RevEngine &rev, const FwdEngine &fwd, const uint8_t *__restrict__ bytes, size_t skew, size_t base,
                                                     size_t i, const ItemSpan item, uint32_t lo_raw, uint32_t hi_raw, uint32_t *marks, uint64_t marks_words) {
    const size_t b = item.b, len = item.e - b, lo = lo_raw < len ? lo_raw : len, hi = hi_raw < lo ? lo : hi_raw < len ? hi_raw : len;
    const size_t gl = b + lo, gh = b + hi;                        // the stretch in absolute offsets
    auto word_of = [&](size_t g) { return (uint64_t)((g - base) >> 5) + i; };
    auto put = [&](uint64_t w, uint32_t v) { if (w < marks_words) marks[w] = v; };
    // ---- backward on rev from gh down to gl: a mark wherever the right-hand language accepts item[p, hi)
    {
        typename RevEngine::State st;
        rev.reset(st);
        uint32_t acc = 0;                                // the marks of the word that holds offset q, of the offsets >= q (0 once stored)
        size_t q = gh;                                   // offsets [q, gh] have their marks
        auto mark = [&](size_t at) {
            const uint32_t bit = (uint32_t)(at - base) & 31u;
            if (rev.accepting(st)) acc |= 1u << bit;
            if (bit == 0) { put(word_of(at), acc); acc = 0; }
        };
        mark(gh);
        bool dead = st.s == 0;
        auto one = [&](uint32_t c, size_t at) {
            rev.step(st, c);
            mark(at);
            dead = st.s == 0;
        };
        for (; q > gl && ((q + skew) & 15) && !dead; q--) one(bytes[q - 1], q - 1);       // down to 16-byte alignment
        for (; q >= gl + 16 && !dead; q -= 16) {                                         // 16 bytes per load, the high byte first
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t m16 = 0;                            // bit k: accepting after the byte at q - 16 + k
#pragma unroll
            for (int k = 15; k >= 0; k--) {
                rev.step(st, (w[k >> 2] >> (8 * (k & 3))) & 0xffu);
                if (rev.accepting(st)) m16 |= 1u << k;
            }
            dead = st.s == 0;
            const size_t at = q - 16;
            const uint32_t bit = (uint32_t)(at - base) & 31u;
            const uint64_t x = (uint64_t)m16 << bit;     // the 16 marks where they sit in the word of `at` and, beyond bit 31, the next one
            if (bit > 16) { put(word_of(at) + 1, acc | (uint32_t)(x >> 32)); acc = (uint32_t)x; }     // (the boundary lies inside the 16 bytes)
            else {
                acc |= (uint32_t)x;
                if (bit == 0) { put(word_of(at), acc); acc = 0; }
            }
        }
        for (; q > gl && !dead; q--) one(bytes[q - 1], q - 1);
        if (q > gl) {                                    // dead above gl: no offset below q is marked - the words left, without the text
            if ((q - base) & 31) put(word_of(q), acc);
            for (uint64_t w = word_of(q), w0 = word_of(gl); w > w0;) put(--w, 0u);
        } else if ((gl - base) & 31) put(word_of(gl), acc);                              // (bit 0: stored already)
    }
    // ---- forward on fwd from gl: the last marked offset at which the left-hand language accepts item[lo, x)
    uint32_t answer = kNoMatch;
    {
        typename FwdEngine::State st;
        fwd.reset(st);
        uint64_t held = ~(uint64_t)0;                    // the mark word in `word` (none yet)
        uint32_t word = 0;
        auto marked = [&](size_t g) {
            const uint64_t w = word_of(g);
            if (w != held) { held = w; word = w < marks_words ? marks[w] : 0u; }
            return (word >> ((uint32_t)(g - base) & 31u)) & 1u;
        };
        size_t p = gl;                                   // bytes [gl, p) have been consumed
        if (fwd.accepting(st) && marked(gl)) answer = (uint32_t)lo;
        bool dead = st.s == 0;
        auto one = [&](uint32_t c, size_t next_p) {
            fwd.step(st, c);
            if (fwd.accepting(st) && marked(next_p)) answer = (uint32_t)(next_p - b);
            dead = st.s == 0;
        };
        for (; p < gh && ((p + skew) & 15) && !dead; p++) one(bytes[p], p + 1);          // up to 16-byte alignment
        for (; p + 16 <= gh && !dead; p += 16) {                                         // 16 bytes per load
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (!dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, p + k + 1);
        }
        for (; p < gh && !dead; p++) one(bytes[p], p + 1);
    }
    return answer;
}

template <class RevEngine, class FwdEngine>
__global__ __launch_bounds__(kThreads, 8) void longest_split_kernel(DfaDevice rev_table, DfaDevice fwd_table, uint32_t fwd_lds_off,
                                                                     const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, size_t nitems,
                                                                     uint32_t trim, const uint32_t *lo_in, const uint32_t *hi_in, uint32_t *marks,
                                                                     uint64_t marks_words, uint32_t *out, uint32_t *on_none) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RevEngine rev;
    FwdEngine fwd;
    rev.load(rev_table, smem);
    fwd.load(fwd_table, smem + fwd_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;      // (p + skew) & 15 == 0: bytes + p is 16-byte aligned
    const size_t base = off[0];                                       // (uniform)
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const uint32_t lo_raw = lo_in[i], hi_raw = hi_in[i];          // (before any store: the arrays may be `out` / `on_none`)
        if (lo_raw == kNoMatch) {
            out[i] = kNoMatch;
            if (on_none) on_none[i] = kNoMatch;
            return;
        }
        const uint32_t answer = longest_split_of(rev, fwd, bytes, skew, base, i, item_span(off, i, trim, kMaxItemOffset), lo_raw, hi_raw, marks, marks_words);
        out[i] = answer;
        if (answer == kNoMatch && on_none) on_none[i] = kNoMatch;
    });
}

// THE LIST FORM.  The same answer for every SLOT of a match list (first: nitems + 1 entries, match k of item i is slot first[i] + k;
// lo_in / hi_in / out / on_none are indexed by the slot itself): still a lane per ITEM, walking its slots in order, the two phases
// per slot.  A lane per item and not per match because consecutive matches of an item share mark words - and the bit of the offset
// e_k == s_{k+1}: within a lane those stores are sequential and stay plain, no atomics, no memset.  What holds of the marks here:
// NO WORD OF ANOTHER ITEM is touched and the LARGEST INDEX lies below the bound, as above; "no word stored twice" does NOT hold - a
// slot's backward phase stores every word of its own stretch again, over what the previous slot left, and its forward phase reads
// only those (its cached mark word starts empty for every slot).  A slot whose lo is ~0u touches neither text nor marks.  Exactly
// the slots first[0] .. first[nitems] of out (and of on_none, where the answer is none) are written; a lane reads a slot's two
// entries before it writes them, so all four arrays may be the same.
template <class RevEngine, class FwdEngine>
__global__ __launch_bounds__(kThreads, 8) void longest_split_list_kernel(DfaDevice rev_table, DfaDevice fwd_table, uint32_t fwd_lds_off,
                                                                          const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, size_t nitems,
                                                                          uint32_t trim, const uint64_t *__restrict__ first, const uint32_t *lo_in,
                                                                          const uint32_t *hi_in, uint32_t *marks, uint64_t marks_words, uint32_t *out,
                                                                          uint32_t *on_none) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RevEngine rev;
    FwdEngine fwd;
    rev.load(rev_table, smem);
    fwd.load(fwd_table, smem + fwd_lds_off);
    __syncthreads();
    const size_t skew = reinterpret_cast<uintptr_t>(bytes) & 15;
    const size_t base = off[0];                                       // (uniform)
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        for (uint64_t slot = first[i], f1 = first[i + 1]; slot < f1; slot++) {
            const uint32_t lo_raw = lo_in[slot], hi_raw = hi_in[slot];   // (before any store: the arrays may be `out` / `on_none`)
            uint32_t answer = kNoMatch;
            // (the span is read again per slot - an L1 hit - rather than kept: two 64-bit registers less across the walks)
            if (lo_raw != kNoMatch)
                answer = longest_split_of(rev, fwd, bytes, skew, base, i, item_span(off, i, trim, kMaxItemOffset), lo_raw, hi_raw, marks, marks_words);
            out[slot] = answer;
            if (answer == kNoMatch && on_none) on_none[slot] = kNoMatch;
        }
    });
}

// The slots first[0] .. first[nitems] of up to two arrays, copied (src != nullptr) or filled with ~0u (src == nullptr): what a
// launch that is skipped leaves to do.  The slot range is on the device only; a pair whose dst is null is left out.
__global__ __launch_bounds__(kThreads) void slot_range_kernel(const uint64_t *__restrict__ first, size_t nitems, const uint32_t *src_a, uint32_t *dst_a,
                                                              const uint32_t *src_b, uint32_t *dst_b) {
    const uint64_t f0 = first[0], f1 = first[nitems];
    for (uint64_t q = f0 + (uint64_t)blockIdx.x * kThreads + threadIdx.x; q < f1; q += (uint64_t)gridDim.x * kThreads) {
        if (dst_a) dst_a[q] = src_a ? src_a[q] : kNoMatch;
        if (dst_b) dst_b[q] = src_b ? src_b[q] : kNoMatch;
    }
}

template <class RevEngine, class FwdEngine>
int launch_longest_split(const DfaDevice &rev, const DfaDevice &fwd, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                         const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out, uint32_t *on_none, void *stream) {
    const size_t fwd_off = (RevEngine::lds_bytes(rev) + 15) & ~(size_t)15, lds = fwd_off + FwdEngine::lds_bytes(fwd);
    return launch_item_lanes<longest_split_kernel<RevEngine, FwdEngine>>(lds, nitems, kItemLanesMaxBlocks, stream, rev, fwd, (uint32_t)fwd_off, bytes, off,
                                                                         nitems, trim, lo, hi, marks, (uint64_t)marks_words, out, on_none);
}

template <class RevEngine, class FwdEngine>
int launch_longest_split_list(const DfaDevice &rev, const DfaDevice &fwd, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                              const uint64_t *first, const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out,
                              uint32_t *on_none, void *stream) {
    const size_t fwd_off = (RevEngine::lds_bytes(rev) + 15) & ~(size_t)15, lds = fwd_off + FwdEngine::lds_bytes(fwd);
    return launch_item_lanes<longest_split_list_kernel<RevEngine, FwdEngine>>(lds, nitems, kItemLanesMaxBlocks, stream, rev, fwd, (uint32_t)fwd_off, bytes,
                                                                              off, nitems, trim, first, lo, hi, marks, (uint64_t)marks_words, out, on_none);
}

}  // namespace

int longest_split_dfa(const DfaDevice &rev, const DfaDevice &fwd, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                      const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out, uint32_t *on_none, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(rev) || !plain_table_ok(fwd)) return (int)hipErrorInvalidValue;
    // search_longest_extents_dfa's placement rule
    if (!two_tables_in_lds(rev, fwd, in_global))
        return launch_longest_split<PlainDfaGlobalEngine, PlainDfaGlobalEngine>(rev, fwd, bytes, off, nitems, trim, lo, hi, marks, marks_words, out, on_none,
                                                                               stream);
    return launch_longest_split<PlainDfaEngine, PlainDfaEngine>(rev, fwd, bytes, off, nitems, trim, lo, hi, marks, marks_words, out, on_none, stream);
}

int longest_split_list_dfa(const DfaDevice &rev, const DfaDevice &fwd, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                           uint32_t trim, const uint64_t *first, const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out,
                           uint32_t *on_none, void *stream) {
    if (!nitems) return 0;
    if (!plain_table_ok(rev) || !plain_table_ok(fwd)) return (int)hipErrorInvalidValue;
    if (!two_tables_in_lds(rev, fwd, in_global))
        return launch_longest_split_list<PlainDfaGlobalEngine, PlainDfaGlobalEngine>(rev, fwd, bytes, off, nitems, trim, first, lo, hi, marks, marks_words,
                                                                                    out, on_none, stream);
    return launch_longest_split_list<PlainDfaEngine, PlainDfaEngine>(rev, fwd, bytes, off, nitems, trim, first, lo, hi, marks, marks_words, out, on_none, stream);
}

int slot_range_copy(const uint64_t *first, size_t nitems, const uint32_t *src_a, uint32_t *dst_a, const uint32_t *src_b, uint32_t *dst_b, void *stream) {
    if (!nitems || (!dst_a && !dst_b)) return 0;
    return launch_item_lanes<slot_range_kernel>(0, nitems, kItemLanesMaxBlocks, stream, first, nitems, src_a, dst_a, src_b, dst_b);
}

}  // namespace dev
}  // namespace rrx
