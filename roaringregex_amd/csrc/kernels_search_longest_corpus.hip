// kernels_search_longest_corpus.hip — "where is the LEFTMOST-LONGEST match of every line" (rrx_search_longest_corpus): the starts
// table and the anchored table of kernels_search_longest_items.hip (lower.hpp: search_longest_dfas) stepped stripe-wise over a
// '\n'-corpus, a lane per stripe.  The starts table runs right to left: the mirror image of multi_contains_corpus_kernel.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

constexpr uint32_t kLongLine = 0xffffffffu;      // the length word of a line of 0xFFFFFFFF bytes or more (between the two phases)

// The anchored table forwards over bytes [from, limit), limit <= nbytes: the largest end of a match that starts at `from` (`from`
// itself where nothing is accepted: the empty match of a nullable pattern).  Stops in row 0, dead and absorbing.  The text comes in
// pieces of 16 bytes counted from `from` itself, one load each - at whatever alignment `from` has: every lane of the wave begins
// its match with byte 0 of a piece, and a match of up to 16 bytes is one load.  The bytes of a piece behind `limit` are loaded
// (they lie inside the data) and not consumed; single bytes only in a last piece that the data does not fill.
template <class Engine>
__device__ __forceinline__ size_t longest_end(const Engine &anchored, const uint8_t *__restrict__ bytes, size_t nbytes, size_t from, size_t limit) {
    typename Engine::State st;
    anchored.reset(st);
    size_t end = from;
    bool dead = false;
    auto one = [&](uint32_t c, size_t next_p) {
        anchored.step(st, c);
        if (anchored.accepting(st)) end = next_p;
        dead = st.s == 0;
    };
    for (size_t a = from; a < limit && !dead; a += 16) {
        const uint32_t k1 = limit - a < 16 ? (uint32_t)(limit - a) : 16u;        // bytes 0 .. k1 - 1 of the piece
        if (a + 16 <= nbytes) {
            const uint4 v = load_text(reinterpret_cast<const uint4 *>(bytes + a));
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; k++)
                if (k < k1 && !dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu, a + k + 1);
        } else {
            for (uint32_t k = 0; k < k1 && !dead; k++) one(bytes[a + k], a + k + 1);
        }
    }
    return end;
}

// Lane g owns the lines that END in stripe g - the lines whose '\n' lies there: lines line_of(stripe_base[g]) ..
// line_of(stripe_base[g + 1]) - 1 of the corpus' stripe index, and for the last stripe of a corpus that does not end in '\n' the
// final fragment as well.  Every line ends in exactly one stripe, so each of its two words has one writer: plain stores, no atomics,
// nothing to clear beforehand.  A lane without a line of its own leaves at once.  `line` counts the lane's lines from 0.
//  * Phase 1, backward on starts ("any bytes, then the pattern right to left"; it never dies): from the end of the stripe (of the
//    data) downwards.  Bytes behind the stripe's last '\n' are somebody else's line - the table rests and the text is tested for
//    '\n' a 32-bit word at a time - unless they are the final fragment.  From a line's '\n' on the table is reset and stepped per
//    byte; accepting after the byte at offset s: some match starts at s, `start32` is the last such s seen, i.e. the smallest (its
//    low 32 bits: start - begin fits a word).  The next '\n' going down, or offset 0, completes the line.  The lane's first line is
//    followed below the stripe to its beginning; a fresh stripe (kFreshStripe) begins with it, and nothing below is read.  A
//    completed line leaves start - begin (~0u: none) in its start word and its LENGTH in its end word, and the lane keeps the offset
//    at which its first line begins.  nullable (launch-uniform): the table rests throughout, only the line starts are found,
//    start = 0.
//  * Phase 2, forward on anchored, once phase 1 is through for every lane of the wave: the lane takes its lines in ascending order -
//    each begins behind the one before, whose length it has just read back from its own words - and for a line with a start runs
//    longest_end from there to the line's '\n' (to the end of the data), then stores the line's end word: the match's end, or ~0u.
//    Run instead inside phase 1, at the moment a line completes, the forward walk of ONE lane would hold up the other 63 for every
//    line with a hit; here the lanes of a wave walk their k-th lines together.
// Loads of phase 1: 16 bytes from 16-byte aligned addresses (the corpus' base is aligned, a stripe is a power of two >= 512),
// consumed high byte first; a whole 128-byte round through TextRound's named slots while one lies inside the stripe, single
// 16-byte loads below the stripe, single bytes only above the last 16-byte boundary of the data.  Nothing is indexed at run time:
// nothing lives in scratch.  No byte below offset 0 or at or beyond nbytes is read.
// A line longer than 0xFFFFFFFE bytes is searched as if it ended at its offset 0xFFFFFFFE: its start is found again by a walk of
// its own in phase 2 (phase 1 has seen the bytes behind that offset too).
template <class StartsEngine, class AnchoredEngine>
__global__ __launch_bounds__(kThreads, 8) void search_longest_corpus_kernel(SearchLongestDevice prog, uint32_t anchored_lds_off, uint32_t nullable,
                                                                          const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                                          const uint64_t *__restrict__ stripe_base, size_t nstripes,
                                                                          uint32_t *__restrict__ match_start, uint32_t *__restrict__ match_end) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    StartsEngine starts;
    AnchoredEngine anchored;
    starts.load(prog.starts, smem);
    anchored.load(prog.anchored, smem + anchored_lds_off);
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= nstripes) return;
    const uint64_t b0 = stripe_base[g], b1 = stripe_base[g + 1];
    const bool fragment = g + 1 == nstripes && bytes[nbytes - 1] != '\n';         // the data ends inside a line: mine
    const int32_t n = (int32_t)(line_of(b1) - line_of(b0)) + (fragment ? 1 : 0);  // (a stripe holds at most kMaxStripe '\n')
    if (n <= 0) return;
    uint32_t *__restrict__ const start_of = match_start + line_of(b0), *__restrict__ const end_of = match_end + line_of(b0);
    const size_t lo = g * (size_t)stripe;
    const size_t floor = (b0 & kFreshStripe) ? lo : 0;                            // no byte below is read

    // ---- phase 1: backward
    typename StartsEngine::State st;
    starts.reset(st);
    int32_t line = fragment ? n - 1 : n;           // n: behind my last '\n', in somebody else's line; < 0: my first line is complete
    bool stepping = fragment && !nullable, hit = false;
    uint32_t start32 = 0;
    size_t line_end = nbytes, first_begin = 0;
    auto complete = [&](size_t begin) {
        const size_t len = line_end - begin;
        start_of[line] = nullable ? 0u : hit ? start32 - (uint32_t)begin : kNoMatch;
        end_of[line] = len < kLongLine ? (uint32_t)len : kLongLine;
        first_begin = begin;
    };
    auto one = [&](uint32_t c, size_t at) {        // the byte at offset `at`
        if (c == '\n') {
            if (line < 0) return;
            if (line < n) complete(at + 1);
            line--;
            stepping = !nullable && line >= 0;
            line_end = at;
            hit = false;
            starts.reset(st);
        } else if (stepping) {
            starts.step(st, c);
            if (starts.accepting(st)) { hit = true; start32 = (uint32_t)at; }
        }
    };
    auto four = [&](uint32_t w, size_t at) {       // the bytes at offsets at + 3 .. at
        if (!newline_flags(w)) {
            if (!stepping) return;
#pragma unroll
            for (int k = 3; k >= 0; k--) {
                starts.step(st, (w >> (8 * k)) & 0xffu);
                if (starts.accepting(st)) { hit = true; start32 = (uint32_t)at + k; }
            }
            return;
        }
#pragma unroll
        for (int k = 3; k >= 0; k--) one((w >> (8 * k)) & 0xffu, at + k);
    };
    auto sixteen = [&](const uint4 &v, size_t at) { four(v.w, at + 12); four(v.z, at + 8); four(v.y, at + 4); four(v.x, at); };

    size_t q = lo + stripe < nbytes ? lo + stripe : nbytes;                       // bytes [q, end of my stripe) have been consumed
    for (; q & 15; q--) one(bytes[q - 1], q - 1);                                 // (the last stripe of data that is no multiple of 16)
    while (q >= lo + kRound) {                                                    // (inside my stripe my first line does not complete)
        q -= kRound;
        TextRound<kRound / 16> buf;
        buf.load(reinterpret_cast<const uint4 *>(bytes + q));
        size_t at = q + kRound;
        buf.for_each_slot_down([&](const uint4 &v) { at -= 16; sixteen(v, at); });
    }
    for (; line >= 0 && q >= floor + 16; q -= 16) sixteen(load_text(reinterpret_cast<const uint4 *>(bytes + q - 16)), q - 16);
    if (line >= 0 && line < n) complete(floor);                                   // my first line begins with the stripe, or with the data

    // ---- phase 2: forward, line by line
    size_t begin = first_begin;
    for (int32_t j = 0; j < n; j++) {
        size_t len = end_of[j];
        uint32_t s = start_of[j];
        if (len == kLongLine) {                                                   // longer than a result word can say: its real end, its start again
            while (begin + len < nbytes && bytes[begin + len] != '\n') len++;
            if (!nullable) {
                s = kNoMatch;
                starts.reset(st);
                for (size_t x = begin + kMaxItemOffset; x > begin; x--) {
                    starts.step(st, bytes[x - 1]);
                    if (starts.accepting(st)) s = (uint32_t)(x - 1 - begin);
                }
                start_of[j] = s;
            }
        }
        uint32_t e_out = kNoMatch;
        if (s != kNoMatch) e_out = (uint32_t)(longest_end(anchored, bytes, nbytes, begin + s, begin + (len < kMaxItemOffset ? len : kMaxItemOffset)) - begin);
        end_of[j] = e_out;
        begin += len + 1;
    }
}

template <class StartsEngine, class AnchoredEngine>
int launch_search_longest_corpus(const SearchLongestDevice &p, bool nullable, const uint8_t *bytes, size_t nbytes, uint32_t stripe,
                                 const uint64_t *stripe_base, size_t nstripes, uint32_t *match_start, uint32_t *match_end, void *stream) {
    const size_t anchored_off = (StartsEngine::lds_bytes(p.starts) + 15) & ~(size_t)15, lds = anchored_off + AnchoredEngine::lds_bytes(p.anchored);
    return launch_item_lanes<search_longest_corpus_kernel<StartsEngine, AnchoredEngine>>(lds, nstripes, 0, stream, p, (uint32_t)anchored_off,
                                                                                         nullable ? 1u : 0u, bytes, nbytes, stripe, stripe_base, nstripes,
                                                                                         match_start, match_end);
}

}  // namespace

int search_longest_corpus_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, size_t nbytes, uint32_t stripe,
                              const uint64_t *stripe_base, size_t nstripes, uint32_t *match_start, uint32_t *match_end, void *stream) {
    if (!nstripes || !nbytes) return 0;
    if (!plain_table_ok(p.starts) || !plain_table_ok(p.anchored)) return (int)hipErrorInvalidValue;
    if (!two_tables_in_lds(p.starts, p.anchored, in_global))
        return launch_search_longest_corpus<PlainDfaGlobalEngine, PlainDfaGlobalEngine>(p, nullable, bytes, nbytes, stripe, stripe_base, nstripes, match_start,
                                                                                        match_end, stream);
    return launch_search_longest_corpus<PlainDfaEngine, PlainDfaEngine>(p, nullable, bytes, nbytes, stripe, stripe_base, nstripes, match_start, match_end,
                                                                        stream);
}

}  // namespace dev
}  // namespace rrx
