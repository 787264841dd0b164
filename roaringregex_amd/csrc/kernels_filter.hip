// kernels_filter.hip — the rows a result bitmap selects, as a new column (rrx_bitmap_rank, rrx_filter_sizes, rrx_filter_corpus_sizes,
// rrx_filter_contains_*): from any bitmap in the result layout (bit i & 31 of word i >> 5 = row i) to the RANK of every selected row
// and its triple (row number, absolute source offset, length) - what dev::pieces_fill takes once the lengths are prefixed.  No
// table, no regex.  The selection rule: with inv = 0 a row is selected iff its bit is 1, with inv = ~0u iff it is 0; the bits of the
// last word beyond nbits are never selected.
// Three kernels.  POPCOUNTS (a lane per bitmap word) feeds dev::scan_counts, whose output is rank[w] = selected bits in front of word
// w.  SELECT FOR ITEMS (a lane per row) takes the triple from an offsets array.  SELECT FOR CORPUS LINES (a lane per stripe) takes it
// from the text and the stripe index alone: no offsets array exists.  Every slot is written by exactly one lane with plain stores:
// no atomics, nothing to clear beforehand, no workgroup waits for another.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

__device__ __forceinline__ uint32_t low_mask(uint32_t n) { return (1u << n) - 1u; }      // bits 0 .. n - 1, n < 32

// counts[w] = selected bits of word w, the last word cut at nbits: what scan_counts sums (a count is 32 at most: no flag bit)
__global__ __launch_bounds__(256) void filter_popcounts_kernel(const uint32_t *__restrict__ bits, size_t nbits, uint32_t inv, uint32_t *__restrict__ counts) {
    const size_t words = (nbits + 31) / 32;
    const uint32_t tail = (uint32_t)(nbits & 31u);
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
        uint32_t v = bits[w] ^ inv;
        if (w + 1 == words && tail) v &= low_mask(tail);
        counts[w] = (uint32_t)__popc(v);
    }
}

// The number of selected rows in front of row x, x <= nbits: the rank of its word and the word's bits below it.  x a multiple of 32
// reads no bitmap word (x == nbits may name the word behind the last one); the bits below x are rows, never spare tail bits.
__device__ __forceinline__ uint64_t selected_before(const uint32_t *__restrict__ bits, uint32_t inv, const uint64_t *__restrict__ rank, uint64_t x) {
    const uint32_t r = (uint32_t)x & 31u;
    uint64_t n = rank[x >> 5];
    if (r) n += (uint32_t)__popc((bits[x >> 5] ^ inv) & low_mask(r));
    return n;
}
__device__ __forceinline__ void store_triple(uint64_t slot, uint64_t r, uint64_t src, uint64_t n, uint64_t *__restrict__ row, uint32_t *__restrict__ piece_len,
                                             uint64_t *__restrict__ piece_src, uint32_t *__restrict__ too_long) {
    if (row) row[slot] = r;
    piece_src[slot] = src;
    piece_len[slot] = n > 0xffffffffu ? 0xffffffffu : (uint32_t)n;
    if (too_long && n >= ((uint64_t)1 << 30)) *too_long = 1;      // the same value from every lane, a plain store
}

// SELECT FOR ITEMS.  One lane per row (item_lanes.hpp: the loop, the item's span): a selected row i goes to the slot
// rank[i >> 5] + popc(word & low_mask(i & 31)) - bit i and the bits below it are rows, so the tail needs no mask here.  A wave's 64
// rows are two bitmap words and its slots ascend with the lane: the loads of off and the stores are coalesced.  row may be null
// (the one-call forms beyond rows_cap).  Exactly the slots 0 .. nsel - 1 are written.
__global__ __launch_bounds__(kThreads) void filter_items_kernel(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim, const uint32_t *__restrict__ bits,
                                                                uint32_t inv, const uint64_t *__restrict__ rank, uint64_t *__restrict__ row,
                                                                uint32_t *__restrict__ piece_len, uint64_t *__restrict__ piece_src, uint32_t *__restrict__ too_long) {
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const uint32_t w = bits[i >> 5] ^ inv, r = (uint32_t)i & 31u;
        if (!((w >> r) & 1u)) return;
        const uint64_t slot = rank[i >> 5] + (uint32_t)__popc(w & low_mask(r));
        const ItemSpan sp = item_span(off, i, trim);
        store_triple(slot, i, sp.b, sp.e - sp.b, row, piece_len, piece_src, too_long);
    });
}

// SELECT FOR CORPUS LINES.  Lane g owns the lines that START in stripe g - lines lo .. past - 1, from the corpus' stripe index as
// multi_contains_corpus_kernel takes them (the last stripe's `past` is the line count: no byte is read for it).  Its first slot and
// the number of its selected lines come from rank and two partial words; a lane without a selected line - the normal case of a
// sparse selection - returns before it reads a byte of text.  The others walk from the stripe's first byte, the text tested for '\n'
// a 32-bit word at a time (newline_flags), 16 bytes per load from 16-byte aligned addresses, a 128-byte line per burst while one
// lies inside the data (TextRound: named slots, nothing in scratch): a stripe that begins inside somebody else's line is skipped to
// behind its first '\n'; every '\n' ends the current line, and a selected one of mine is stored - its number, the offset of its
// first byte, its length without the '\n', plus 1 with keep_newline; the last selected line is followed past the stripe end to its
// '\n' or to the end of the data (then it has no '\n' to keep), and the lane stops reading behind it.  The bitmap word of the current
// line stays in a register.  No byte at or beyond nbytes is read.
constexpr int kFilterCorpusThreads = 256;
__global__ __launch_bounds__(kFilterCorpusThreads) void filter_corpus_kernel(const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                                             const uint64_t *__restrict__ stripe_base, size_t nstripes, size_t nlines,
                                                                             const uint32_t *__restrict__ bits, uint32_t inv, uint32_t keep_newline,
                                                                             const uint64_t *__restrict__ rank, uint64_t *__restrict__ row,
                                                                             uint32_t *__restrict__ piece_len, uint64_t *__restrict__ piece_src,
                                                                             uint32_t *__restrict__ too_long) {
    const size_t g = (size_t)blockIdx.x * kFilterCorpusThreads + threadIdx.x;
    if (g >= nstripes) return;
    const uint64_t b0 = stripe_base[g], b1 = stripe_base[g + 1];
    const bool fresh = (b0 & kFreshStripe) != 0;
    const uint64_t lo = line_of(b0) + (fresh ? 0u : 1u);                          // the lines that start in my stripe: lo .. past - 1
    const uint64_t past = g + 1 < nstripes ? line_of(b1) + ((b1 & kFreshStripe) ? 0u : 1u) : (uint64_t)nlines;
    if (past <= lo) return;
    uint64_t slot = selected_before(bits, inv, rank, lo);
    uint32_t left = (uint32_t)(selected_before(bits, inv, rank, past) - slot);    // my selected lines still to store (a stripe holds at most kMaxStripe lines)
    if (!left) return;

    uint64_t line = fresh ? lo : lo - 1;           // the line that holds the byte at hand (not fresh: somebody else's, lo >= 1)
    bool mine = fresh;
    size_t pos = g * (size_t)stripe;               // 16-byte aligned: the corpus' base is, and a stripe is a power of two >= 512
    uint64_t line_start = pos;
    uint64_t word_at = ~(uint64_t)0;
    uint32_t word = 0;
    // the line at hand ends in front of offset p, with a '\n' there (has_newline) or with the data
    auto end_line = [&](uint64_t p, uint32_t has_newline) {
        if (mine) {
            if ((line >> 5) != word_at) { word_at = line >> 5; word = bits[word_at] ^ inv; }
            if ((word >> ((uint32_t)line & 31u)) & 1u) {
                store_triple(slot, line, line_start, p - line_start + (has_newline & keep_newline), row, piece_len, piece_src, too_long);
                slot++;
                left--;
            }
        }
        line++;
        line_start = p + 1;
        mine = true;
    };
    auto four = [&](uint32_t w, size_t p) {
        uint32_t f = newline_flags(w);
        while (f && left) {
            end_line(p + ((uint32_t)(__ffs((int)f) - 1) >> 3), 1u);
            f &= f - 1;
        }
    };
    auto sixteen = [&](const uint4 &v) { four(v.x, pos); four(v.y, pos + 4); four(v.z, pos + 8); four(v.w, pos + 12); pos += 16; };

    while (left && pos + kRound <= nbytes) {
        TextRound<kRound / 16> buf;
        buf.load(reinterpret_cast<const uint4 *>(bytes + pos));
        buf.for_each_slot(sixteen);
    }
    while (left && pos + 16 <= nbytes) sixteen(load_text(reinterpret_cast<const uint4 *>(bytes + pos)));
    for (; left && pos < nbytes; pos++)
        if (bytes[pos] == '\n') end_line(pos, 1u);
    if (left) end_line(nbytes, 0u);                // the corpus ends without '\n': the end of the data ends my last line
}

}  // namespace

// rank: nwords + 1 entries, behind them the scan's chunk sums and the popcount words (16-byte aligned: the scan reads them as uint4)
size_t bitmap_rank_words(size_t nbits) {
    const size_t nwords = (nbits + 31) / 32;
    return nwords + 1 + scan_scratch_words(nwords) + (nwords + 1) / 2 + 1;
}
int bitmap_rank(const uint32_t *bits, size_t nbits, bool invert, uint64_t *rank, void *stream) {
    const size_t nwords = (nbits + 31) / 32;
    uint64_t *sums = rank + nwords + 1;
    uint32_t *counts = reinterpret_cast<uint32_t *>((reinterpret_cast<uintptr_t>(sums + scan_scratch_words(nwords)) + 15) & ~(uintptr_t)15);
    if (nwords) {
        size_t blocks = (nwords + 255) / 256;
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(filter_popcounts_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, bits, nbits, invert ? ~0u : 0u, counts);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    const int e = scan_counts(counts, rank, sums, nwords, stream);           // (no words: rank[0] = the total, 0)
    if (e || !nwords) return e;
    return (int)hipMemsetAsync(rank, 0, sizeof(uint64_t), (hipStream_t)stream);      // the scan marks entry 0 as a stripe start: not here
}

int filter_items(const uint64_t *off, size_t nitems, uint32_t trim, const uint32_t *bits, bool invert, const uint64_t *rank, uint64_t *row, uint32_t *piece_len,
                 uint64_t *piece_src, uint32_t *too_long, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<filter_items_kernel>(0, nitems, kFilterMaxBlocks, stream, off, nitems, trim, bits, invert ? ~0u : 0u, rank, row, piece_len, piece_src,
                                                  too_long);
}

int filter_corpus(const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes, size_t nlines, const uint32_t *bits,
                  bool invert, bool keep_newline, const uint64_t *rank, uint64_t *row, uint32_t *piece_len, uint64_t *piece_src, uint32_t *too_long,
                  void *stream) {
    if (!nstripes || !nbytes || !nlines) return 0;
    const size_t blocks = (nstripes + kFilterCorpusThreads - 1) / kFilterCorpusThreads;
    hipLaunchKernelGGL(filter_corpus_kernel, dim3((unsigned)blocks), dim3(kFilterCorpusThreads), 0, (hipStream_t)stream, bytes, nbytes, stripe, stripe_base,
                       nstripes, nlines, bits, invert ? ~0u : 0u, keep_newline ? 1u : 0u, rank, row, piece_len, piece_src, too_long);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
