// device.hpp — host-visible interface of the HIP kernels (kernels_*.hip).  gfx950 only.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rrx {
namespace dev {

// ---- shared geometry and structs --------------------------------------------------------------------------------
// Geometry of the batch kernel: lane g of the grid owns the lines that START in the contiguous stripe
// bytes [g*stripe, (g+1)*stripe) and follows its last line past the stripe end.  Every lane streams its
// stripe straight from HBM into registers, kRound bytes (8 x 16 B) per round.
#ifndef RRX_THREADS
#define RRX_THREADS 1024
#endif
constexpr int kThreads = RRX_THREADS;       // lanes per workgroup: one LDS copy of the tables serves them all
// Stripe = bytes per lane: a per-corpus power of two.  Measured on the final kernel: several generations of waves
// per CU beat one generation of long-lived waves (the early finishers' slots get refilled while the slowest waves
// drain), until the per-stripe work (following the straddling line, the final flush) shows: 4 KiB is best at 8 GiB,
// 2 KiB at 1 GiB.  Automatic choice: about two million lanes, between 2 KiB and 16 KiB; explicit: 1-16 KiB.
constexpr uint32_t kMinStripe = 512, kMaxStripe = 16384, kMinAutoStripe = 2048;
constexpr size_t kTargetLanes = (size_t)1 << 21;
// (r4) Up to 512 MiB: the smallest stripe (from 512 bytes) that still leaves no more than 2^18 lanes - one generation of 256 workgroups.  A lane
// steps its stripe pair after pair, a chain of dependent LDS lookups: a 2 KiB stripe takes 55 us however small the corpus, so with 2 KiB stripes
// from 64 KiB to 128 MiB a match took 60-115 us on a handful of CUs; 512-byte stripes: 24-44 us (tools/probe/small_corpus_stripes.py).
inline uint32_t pick_stripe(size_t nbytes) {
    uint32_t s = kMinStripe;
    while (s < kMinAutoStripe && nbytes / s > ((size_t)1 << 18)) s *= 2;
    while (s < kMaxStripe && nbytes / s > kTargetLanes) s *= 2;
    return s;
}
// The size-based stripe suits lines of a few dozen bytes.  Every lane walks half a line past its stripe, so long lines
// want longer stripes (a{1,300} config, 200 B per line, 1 GiB: 4 KiB stripes +14 % over 2 KiB): double the stripe while a
// line is more than 1/16 of it.  Short lines want shorter stripes: a workgroup's 1024 lanes hold 1024 * stripe / avg_line
// lines, and beyond the 131072 its LDS result window is sure to hold (16 KiB) the result words go to memory one atomic at
// a time (k<n> lines of 5.4 bytes, 8 GiB: 4 KiB stripes 3.69 TB/s, 1 KiB stripes 4.53; profiles/r02_short_line_stripes.txt).
inline uint32_t stripe_for_lines(size_t nbytes, size_t avg_line) {
    uint32_t want = pick_stripe(nbytes);
    // ... but never below 2^18 lanes: 256 workgroups of 1024 lanes, one per CU (r4: the floor was 2^17 and 1 GiB of 440-byte lines got 8 KiB
    // stripes, i.e. 128 workgroups on 256 CUs: 2.6 TB/s against 4.4 with 4 KiB stripes; tools/probe/long_line_stripes.sh)
    while (want < kMaxStripe && avg_line * 16 > want && nbytes / (2 * (size_t)want) >= ((size_t)1 << 18)) want *= 2;
    while (want > 1024 && (avg_line + 1) * 128 < want) want /= 2;      // (512-byte stripes are for explicit requests)
    return want;
}
constexpr int kRound = 128;                      // one whole cache line per lane per round
constexpr int kMaxNfaWords = 16;                 // 512 positions per lane-resident state set
constexpr uint32_t kWideColumns = 129;           // columns 0..127 = byte values, 128 = any byte >= 0x80
constexpr uint32_t kWideMaxStates = 127;         // row byte offsets must fit 16 bits
constexpr uint32_t kClassedMaxEntries = 16384;   // row byte offsets are 16-bit: 64 KiB of 4-byte entries

struct NfaMasks {                                // passed by value -> SGPRs
    uint32_t init[kMaxNfaWords], fin[kMaxNfaWords], chain[kMaxNfaWords], self[kMaxNfaWords], excm[kMaxNfaWords];
    uint32_t cgrp[kMaxNfaWords], ctgt[kMaxNfaWords];   // add-carry rules: runs and their targets
};

struct NfaDevice {                               // tables in HBM (copied to LDS by every workgroup)
    uint32_t W = 0, nbits = 0, any_exc = 0, any_carry = 0, any_self = 0;
    NfaMasks masks;
    const uint32_t *B = nullptr;                 // [256][W]
    const uint32_t *X = nullptr;                 // [nbits][W]
};

// Group-cooperative NFA (automata beyond kMaxNfaWords*32 positions): the state set is spread over G = 8, 16 or 32 neighbouring
// lanes of a wave, K = 2 ... 8 consecutive 32-bit words per lane (word w of the set: lane w / K of the group, slot w % K), up to
// 8192 positions; a wave steps 64 / G strings.  (r4: K was fixed at 2 and a string of 2049+ positions took a whole wave.)
constexpr uint32_t kGroupMaxBits = 8192;
struct GroupNfaDevice {
    uint32_t G = 0, K = 0, nbits = 0, n_exc = 0, ncls = 0;
    uint32_t exc_mode = 0;                       // 0: exception positions anywhere; 2: position 0 (live on the first byte of a line
                                                 //   only) is the only one
    uint32_t self_slots = 0;                     // bit k: slot k of some lane holds a self loop
    uint32_t b_slots = 0;                        // bit k: slot k of some lane has a B row that is not all ones for some class >= 1
                                                 //   (the other slots are stepped by the shift alone; a class-0 byte kills the line)
    uint32_t exc_slots = 0;                      // bit k: slot k of some lane holds an exception position
    const uint32_t *masks = nullptr;             // [3][G][K]: fin, self, excm
    const uint32_t *Bcls = nullptr;              // [ncls][G][K]: positions enterable on a byte class (class 0: none)
    const uint8_t *cls = nullptr;                // [256] byte -> class (0x00 and >= 0x80: class 0)
    const uint16_t *xidx = nullptr;              // [nbits] exception row of a position (0xffff: none)
    const uint32_t *X = nullptr;                 // [n_exc][G][K]
};
// the geometry for `nbits` positions: the fewest lanes whose words hold them (more strings per wave), false beyond kGroupMaxBits
inline bool group_geometry(uint32_t nbits, uint32_t *G, uint32_t *K) {
    static const uint32_t forms[][2] = {{8, 3}, {8, 4}, {16, 3}, {16, 4}, {32, 3}, {32, 4}, {32, 5}, {32, 8}};
    for (const auto &f : forms)
        if (nbits <= f[0] * f[1] * 32u) { *G = f[0]; *K = f[1]; return true; }
    return false;
}

// Wave-resident NFA (automata beyond kGroupMaxBits positions, kernels_wave.hip): ONE WAVE holds one state set, WL 32-bit
// words per lane (WL = 1 ... 32: up to 65536 positions); exception edges are CSR lists, not rows.
constexpr uint32_t kBlockMaxBits = 65536;
struct WaveNfaDevice {
    uint32_t WL = 0, nbits = 0;
    uint32_t self_words = 0, exc_words = 0;     // bit i: word index i of some lane holds a self-loop / an exception position
    const uint32_t *masks = nullptr;             // [3][64][WL]: fin, self, excm (word w of the set = lane w / WL, index w % WL)
    const uint32_t *Bbyte = nullptr;             // [257][64][WL]: positions enterable on byte value 0..255 ('\n' an ordinary byte),
                                                 //   row 256 = the line-mode '\n' row {position 0}
    const uint32_t *xoff = nullptr;              // [nbits + 1]
    const uint32_t *xtgt = nullptr;              // targets of position p: xtgt[xoff[p] .. xoff[p+1])
    uint32_t ncls = 0;                           // sparse form only: the same rows per byte CLASS (for LDS) ...
    const uint32_t *Bcls = nullptr;              //   [ncls][64 * WL], class 0 = no position
    const uint8_t *cls = nullptr;                //   [256] byte -> class ('\n' an ordinary byte)
};

// Plain DFA (extents kernel: '\n' is an ordinary byte).
struct DfaDevice {
    uint32_t nstates = 0, ncls = 0, start = 0;
    const uint8_t *cls = nullptr;                // [256]
    const uint16_t *next = nullptr;              // [nstates][ncls]
    const uint8_t *acc = nullptr;                // [nstates]
};

constexpr size_t kPlainDfaLdsBudget = 64 * 1024;   // larger plain tables are read from HBM/L2 by the extents kernel

// Line-mode DFA tables (batch kernel): the '\n' transition of every row goes to the start row and carries
// the verdict of the line that just ended.  Entry = next row byte offset (16 bits) | nl << 16 | accept << 24.
struct LineDfaDevice {
    uint32_t nrows = 0;                          // rows (row 0 = dead)
    uint32_t stride = 0;                         // entries per row
    uint32_t start_off = 0;                      // byte offset of the start row
    uint32_t wide = 0;                           // 1: columns are byte values (kWideColumns); 0: byte classes
    uint32_t rep_log2 = 0;                       // wide form: 2^rep_log2 copies of the table interleaved dword by dword
                                                 //   (entry of copy k for logical dword i at dword i*R + k); lane l
                                                 //   reads copy l % R, i.e. only LDS banks congruent to l mod R
    uint32_t in_global = 0;                      // 1: table too large for LDS, read from HBM/L2; entry = next row's
                                                 //    first-entry index (24 bits) | nl << 30 | accept << 31
    const uint32_t *table = nullptr;             // [nrows][stride]
    const uint8_t *cls = nullptr;                // [256] (classed form only)
};

// Stride-2 line-mode table: one dependent lookup per TWO bytes.  The column of a byte pair comes from the
// state-independent table P (resolved off the critical path); T2[row][column] = next row after both bytes, with
// the number of lines that ended inside the pair (0..2) and their verdicts (oldest highest).
//   P  : u16 [128][130], P[c1*130 + c2] = byte offset of the pair's column inside a T2 row (row stride 130 = 65
//        words: the LDS bank is (c1 + c2/2) mod 32, it depends on both bytes); only for corpora without bytes >= 0x80
//   T2 : u32 [nrows][stride], entry = LDS address of the next row (16 bits) | lines << 16 | verdicts << 24,
//        2^rep_log2 interleaved copies like the wide table
//   P8 : u8 [128][136], P8[c1*136 + c2] = the same byte offset, where the largest one - (ncols - 1) * 4 << rep_log2 - fits a byte
//        (null elsewhere).  Four entries per dword, and the index needs no doubling: the indexed match kernels read it in P's
//        place (dfa2_byte_pairs_fit; table_engines.hpp: Dfa2T<true>).  Every other stride-2 kernel reads P.
struct Dfa2Device {
    uint32_t nrows = 0, stride = 0, start_off = 0, rep_log2 = 0;
    const uint16_t *P = nullptr;
    const uint32_t *T2 = nullptr;
    const uint8_t *P8 = nullptr;
};
constexpr uint32_t kDfa2PStride = 130;                // u16 entries per P row
constexpr uint32_t kDfa2PBytes = 128 * kDfa2PStride * 2;
// Row stride of P8: 34 dwords.  Simulated on the URL corpus (tools/probe/lds_conflict_sim.py, profiles/p8_lds_conflict_simulation.txt)
// the strides 131 ... 152 that are not a multiple of 32 cost the same 3.33-3.35 cycles per half-wave; 136 keeps rows dword-aligned
// and the table a multiple of 16 bytes (copy_table_to_lds).
constexpr uint32_t kDfa2P8Stride = 136;
constexpr uint32_t kDfa2P8Bytes = 128 * kDfa2P8Stride;
// items form (trim 1): code 128 = END OF ITEM - one row more, and column 128 (one of the two pad columns of every row)
constexpr uint32_t kDfa2PItemsBytes = (129 * kDfa2PStride * 2 + 15) & ~15u;
// LDS of a stride-2 workgroup: P (32.5 KiB) + one 46 KiB region shared by T2 and the result window = 78.5 KiB, i.e. two
// 1024-lane workgroups per 160-KiB CU (63 KiB with the byte-wide P8 of 17 KiB: still two - the wave slots bound them - and what
// that frees is given to nothing).  Copies of T2 are only made while they leave the window its 16 KiB.
constexpr uint32_t kDfa2RegionBytes = 46 * 1024;
constexpr uint32_t kDfa2MaxTable = kDfa2RegionBytes - 4 * 1024;       // a table this large leaves a 4 KiB window
constexpr uint32_t kDfa2TableBudget = 30 * 1024;                      // T2 with its copies

// ---- launchers --------------------------------------------------------------------------------------------------
// All launchers are asynchronous on `stream` and return a hipError_t value (0 = success).
// accept_bits: bitmap, bit i = line i accepted; must be zeroed before the launch (the launchers do not)

// ---- table engines, batch match path: kernels_table.hip
int match_stripes_dfa(const LineDfaDevice &p, bool clamp_high, const uint8_t *bytes, size_t nbytes, uint32_t stripe,
                      const uint64_t *stripe_base, size_t nstripes, uint32_t *accept_bits, void *stream);
uint32_t flush_mask_for(size_t nbytes, size_t nlines);      // the stride-2 kernel's common flush period from the mean line length
// clean: the text may hold bytes >= 0x80: they are stepped as 0x00 (rrx_contains_corpus, where both are ordinary text of one class).
// flush_mask 31 runs the kernel with the period compiled in (dfa2_flush_at_compile_time), every other value the one that takes it
// per launch.  slots != nullptr: the launch needs NO cleared bitmap - every word of the first `nwords` of `accept` is stored, the
// words two workgroups share through `slots` (one u64 per workgroup and one more, all zero between launches, used by one launch
// at a time).  Only where no bitmap word lies in three workgroups' ranges and every range fits dfa2_window_words(p):
// own_words_check yields both figures for a corpus.
int match_stripes_dfa2(const Dfa2Device &p, bool clean, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                       size_t nstripes, uint32_t *accept, void *stream, uint32_t flush_mask = 31u, unsigned long long *slots = nullptr,
                       size_t nwords = 0);
uint32_t dfa2_window_words(const Dfa2Device &p);             // words of the workgroup's result window in LDS
bool dfa2_flush_at_compile_time(uint32_t flush_mask);
// The sampled-table engine: the stride-2 kernel on a table with an ESCAPE state writes two bits per line into
// `wide_bits` (2 x the accept bitmap, zeroed by the caller); split_two_bit takes them apart (every word of both outputs is
// written) and counts the escaped lines; recheck_escaped_nfa lets the exact NFA lane engine decide those and ORs its accepts in.
int match_stripes_dfa2_two_bit(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                               size_t nstripes, uint32_t *wide_bits, void *stream);
// (`list`: the numbers of the escaped lines, `cap` entries; *escaped_total counts them all.  Up to `cap` escaped lines are decided
// a lane per line, more by a walk over the stripes: both kernels are queued, each reads the count and the one that is not
// needed ends at once.)
int split_two_bit(const uint32_t *wide, size_t nlines, uint32_t *accept_bits, uint32_t *escaped_bits, unsigned long long *escaped_total, uint64_t *list,
                  size_t cap, void *stream);

// One-pass mode (no line index yet): the stride-2 kernel writes counts[g] ('\n' per stripe, with flags) and every lane's
// verdict stream into `slabs` (onepass_slab_words() words); after scan_counts, compact_streams moves the streams to their
// place in the (zeroed) accept bitmap; words beyond cap_words are dropped (the caller learns from the line count that
// its bitmap was too small).
size_t onepass_slab_words(size_t nstripes, uint32_t stripe);
int match_onepass_dfa2(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                       uint32_t *slabs, void *stream);
int match_onepass_dfa(const LineDfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                      uint32_t *slabs, void *stream);
int compact_streams(const uint32_t *counts, const uint64_t *stripe_base, size_t nstripes, uint32_t stripe, const uint32_t *slabs,
                    uint32_t *accept_bits, size_t cap_words, void *stream);
// only_if != nullptr: the kernel does nothing unless *only_if != 0 (the fallback queued behind the stripe-wise items kernel)
int match_extents_dfa(const DfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                      uint8_t *accept, void *stream, const uint32_t *only_if = nullptr);

// ---- corpus index and result bitmaps: kernels_index.hip
int count_newlines_per_stripe(const uint8_t *bytes, size_t nbytes, uint32_t stripe, uint32_t *counts, size_t nstripes, uint32_t *flags, void *stream);
int scan_counts(const uint32_t *counts, uint64_t *base, uint64_t *chunk_sums, size_t n, void *stream);   // base[n] = total
size_t scan_scratch_words(size_t n);                                                                       // u64 words of chunk_sums
int expand_bits(const uint32_t *bits, size_t nlines, uint8_t *out, void *stream);
// *count (zeroed here, on `stream`) = set bits among the first `nlines` bits of a result bitmap
int bitmap_count(const uint32_t *bits, size_t nlines, unsigned long long *count, void *stream);
// mail[0] = *total without the flag bit, mail[1] = flags ? *flags : 0, mail[2] = last_byte ? *last_byte : '\n', mail[3] and
// mail[4] = own ? own[0], own[1] : 0 (own_words_check): the few words a
// synchronous entry hands back, written into pinned device-mapped host memory by a one-lane kernel at the end of the call
int mail_results(const uint64_t *total, const uint32_t *flags, const uint8_t *last_byte, uint64_t *mail, void *stream, const uint32_t *own = nullptr);
// Once per corpus, for the launches that need no cleared bitmap: over the first bitmap words of the batch kernel's workgroups
// (workgroup b starts at stripe b * kThreads; the last one's range ends with the bitmap) - own[0] is set to 1 unless they are
// strictly increasing, own[1] is raised to the largest distance from a workgroup's first word to the last word of its range
// (`own`: two words zeroed by the caller; nstripes > 0).  mail_results then hands them back as mail[3] and mail[4].
int own_words_check(const uint64_t *stripe_base, size_t nstripes, const uint8_t *last_byte, uint32_t *own, void *stream);
// line_off[i] = offset of the first byte of line i (built once per corpus from the stripe index; only patterns that accept
// the empty string need it); nlines + 1 entries are the caller's to size, entry nlines is written only when the corpus ends in '\n'.
int build_line_offsets(const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes,
                       uint64_t *line_off, void *stream);
// all matches of a pattern that accepts "": [k, k) for k = 0 .. length of the line.  first == nullptr: count[i]; otherwise the
// slots first[i], first[i] + 1, ... are filled (slots >= cap are not written)
int empty_matches(const uint64_t *line_off, size_t nlines, uint32_t *count, const uint64_t *first, uint32_t *match_start, uint32_t *match_end,
                  void *stream, size_t cap = ~(size_t)0);

// ---- explicit items, stripe-wise: kernels_items.hip
// explicit items (an offsets array over one buffer) stripe-wise: see kernels_items.hip.  The table is the plain one in the
// wide line-table format with kItemColumns columns: byte values 0..127, 128 = any byte >= 0x80, kItemEndColumn = end of item
constexpr uint32_t kItemColumns = 131, kItemEndColumn = 129;      // (130 in use, 131 keeps the row stride odd)
size_t items_index_bytes(size_t nbytes, size_t nitems);  // item-end bitmap, flag, stripe base
size_t items_result_bytes(size_t nitems);                // result bitmap of one match
// resolve_base / resolve_off (one-call form, nothing known on the host): nbytes is an UPPER BOUND the index is laid out for;
// the kernels take the batch's start and length from the offsets; *flag != 0 afterwards = batch unfit for the stripe-wise
// kernel (items_match then does nothing when handed the flag as skip_if)
int items_index_build(size_t nbytes, const uint64_t *off, size_t nitems, uint32_t trim, void *index, uint32_t **flag, void *stream,
                      const uint8_t *resolve_base = nullptr, size_t min_bytes = 0);
// Where the verdicts of a stripe-wise launch go, out of its result bitmap: one byte per item into `bytes` (16-byte aligned;
// expand_bits), or the bitmap itself into `bits` - ceil(nitems / 32) words at any 4-byte alignment, the bits of the last word beyond
// nitems 0 (copy_result_bits); an unfit batch (*skip_if != 0) leaves zeros there.
struct ItemVerdicts {
    uint8_t *bytes = nullptr;
    uint32_t *bits = nullptr;
    ItemVerdicts(uint8_t *b) : bytes(b) {}
    ItemVerdicts(uint32_t *w) : bits(w) {}
};
// The stripe-wise kernels on an items table - of the match table or of the contains table: the kernels are the same.  items_match2:
// explicit items with separators (trim 1) on the stride-2 table of their own (lower_dfa2's items form; P of kDfa2PItemsBytes).
int items_match2(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, size_t nitems, const void *index, void *result, ItemVerdicts out, void *stream,
                 const uint64_t *resolve_off = nullptr, const uint32_t *skip_if = nullptr);
int items_match(const LineDfaDevice &p, const uint8_t *bytes, size_t nbytes, size_t nitems, uint32_t trim, const void *index, void *result,
                ItemVerdicts out, void *stream, const uint64_t *resolve_off = nullptr, const uint32_t *skip_if = nullptr);

// ---- contains for explicit items, a lane per item: kernels_contains_items.hip
// (What the five lane-per-item kernels - this one, match_extents_kernel, the three searches below - share, their walk included: item_lanes.hpp.)
// `p`: the contains table in its plain form ('\n', NUL and bytes >= 0x80 are ordinary bytes of their class; nothing kills).
// found: its one accepting state if that state is absorbing - a lane stops reading there -, ~0u: none.  in_global: leave the
// table in HBM/L2 whatever its size.  Whole words of `bits` are written with plain stores (ceil(nitems / 32) of them, the bits
// beyond nitems 0): nothing to clear beforehand.  only_if as for match_extents_dfa.
int contains_extents_dfa(const DfaDevice &p, bool in_global, uint32_t found, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                         uint32_t *bits, void *stream, const uint32_t *only_if = nullptr);
// the first ceil(nitems / 32) words of a stripe-wise result bitmap into `bits`, the last one masked to nitems
int copy_result_bits(const uint32_t *result, size_t nitems, uint32_t *bits, void *stream);

// ---- which patterns of a set each explicit item contains, a lane per item: kernels_multi_items.hip
// The product table of a group of members (lower.hpp: MultiProgram): rows below first_hit carry no mask, `full` is the OR of all masks.
struct MultiDevice {
    uint32_t nstates = 0, ncls = 0, start = 0, first_hit = 0, full = 0;
    const uint8_t *cls = nullptr;                // [256]
    const uint16_t *next = nullptr;              // [nstates][ncls]
    const uint32_t *mask = nullptr;              // [nstates]
};
// The table's LDS form: next, the class map, the masks, each from a 16-byte boundary (plan.cpp groups the members by it)
inline size_t multi_lds_bytes(uint32_t nstates, uint32_t ncls) {
    return (((size_t)nstates * ncls * 2 + 15) & ~(size_t)15) + 256 + (((size_t)nstates * 4 + 15) & ~(size_t)15);
}
// Item i = bytes[off[i] .. off[i+1] - trim): m = the OR of the masks of the start row and of every row the item's bytes lead
// through; a lane stops reading once m == p.full.  first: out[i] = m, else out[i] |= m - plain loads and stores of the lane's own
// word, every one of the nitems words written, nothing to clear beforehand.  in_global: leave the table in HBM/L2 (the class map in
// LDS) whatever its size; it stays there anyway beyond kPlainDfaLdsBudget.
int multi_contains_extents(const MultiDevice &p, bool in_global, bool first, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                           uint32_t *out, void *stream);
// counts[k] += the items among the first nitems whose mask has bit k, k = 0 .. 31 (the caller zeroes the 32 counters)
int multi_counts(const uint32_t *mask, size_t nitems, unsigned long long *counts, void *stream);
// bit `pattern` of every mask as a bitmap in contains_extents_dfa's layout: ceil(nitems / 32) whole words, plain stores
int multi_plane(const uint32_t *mask, size_t nitems, uint32_t pattern, uint32_t *bits, void *stream);

// ---- which patterns of a set each line of a '\n'-corpus contains, a lane per stripe: kernels_multi_corpus.hip
// The same table and the same answer per item, the items being the corpus' lines without their '\n' (a last fragment without one
// is a line; '\n' never reaches the table): out[i] = (first ? 0 : out[i]) | the mask of line i, for every line of the corpus and no
// word beyond - the lane that owns the stripe a line STARTS in owns its word: plain stores, nothing to clear beforehand.  bytes,
// nbytes, stripe, stripe_base[nstripes + 1], nstripes: the corpus and its index (count_newlines_per_stripe, scan_counts); bytes is
// 16-byte aligned, no byte at or beyond nbytes is read.  Placement (in_global) as for multi_contains_extents.
int multi_contains_corpus(const MultiDevice &p, bool in_global, bool first, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                          size_t nstripes, uint32_t *out, void *stream);

// ---- first match per explicit item, a lane per item: kernels_search_items.hip
// The two search tables in their plain form, one image: fwd = "any bytes, then the pattern" (accepting exactly where a match ends),
// rev = the pattern right to left (accepting, walking back from a match end, exactly where a match starts; row 0 dead and absorbing:
// pack_search_items checks it).  '\n', NUL and bytes >= 0x80 are ordinary bytes of their class in both.
struct SearchItemsDevice {
    DfaDevice fwd, rev;
};
// Item i = bytes[off[i] .. off[i+1] - trim): [match_start[i], match_end[i]) = the accepted substring with the smallest end, then
// the smallest start, relative to the item; ~0u in both where none is accepted.  Every one of the 2 x nitems words is written
// with plain stores.  in_global: leave both tables in HBM/L2 whatever their size (they stay there anyway when together they pass
// kPlainDfaLdsBudget).  Matches that end beyond offset 0xFFFFFFFE of an item are not reported.
int search_extents_dfa(const SearchItemsDevice &p, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                       uint32_t *match_start, uint32_t *match_end, void *stream);

// ---- all matches per explicit item, a lane per item: kernels_search_all_items.hip
// The matches of item i are those of search_extents_dfa applied again and again to the rest of the item behind the previous match
// (patterns that do not accept the empty string: every match has a byte).  first == nullptr: count[i] = their number, every one of
// the nitems words written with a plain store - the forward table alone is placed and stepped.  Otherwise (`first`: the caller's
// exclusive prefix of the counts) match k of item i goes to slot first[i] + k of match_start / match_end, relative to the item;
// slots >= cap are not written, nor any other slot.  Placement and long items as search_extents_dfa.
int search_all_extents_dfa(const SearchItemsDevice &p, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                           uint32_t *count, const uint64_t *first, uint32_t *match_start, uint32_t *match_end, size_t cap, void *stream);
// The same for a pattern that accepts the empty string: [k, k) for k = 0 .. the item's trimmed length (empty_matches for an offsets
// array with a trim) - no table, no text.
int empty_item_matches(const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *count, const uint64_t *first, uint32_t *match_start,
                       uint32_t *match_end, size_t cap, void *stream);

// ---- leftmost-longest match per explicit item, a lane per item: kernels_search_longest_items.hip
// Two plain tables, one image: starts = "any bytes, then the pattern right to left" (never dies; stepped from the item's last byte
// down, accepting after the byte at offset s exactly when some match starts at s), anchored = the pattern's own DFA (stepped
// forwards from a match start, accepting exactly where a match from there ends; row 0 dead and absorbing: pack_search_longest
// checks it).  '\n', NUL and bytes >= 0x80 are ordinary bytes of their class in both.
struct SearchLongestDevice {
    DfaDevice starts, anchored;
};
// Item i = bytes[off[i] .. off[i+1] - trim): match_start[i] = the smallest s at which an accepted substring starts, match_end[i] =
// the largest e with item[s, e) accepted, relative to the item; ~0u in both where none is accepted.  nullable (the pattern accepts
// the empty string): the starts table is not stepped, start = 0 and end = the longest accepted prefix (0 if none other).  Every
// one of the 2 x nitems words is written with plain stores.  in_global as for search_extents_dfa.  An item is searched as if it
// ended at its offset 0xFFFFFFFE.
int search_longest_extents_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                               uint32_t trim, uint32_t *match_start, uint32_t *match_end, void *stream);

// ---- leftmost-longest match per line of a '\n'-corpus, a lane per stripe: kernels_search_longest_corpus.hip
// The same two tables and the same answer per item, the items being the corpus' lines without their '\n' (a last fragment without
// one is a line; '\n' never reaches a table): match_start[i], match_end[i] for every line i of the corpus and no word beyond - the
// lane that owns the stripe a line ENDS in owns its two words: plain stores, nothing to clear beforehand (between the kernel's two
// phases a line's words hold its start and its length).  bytes, nbytes, stripe, stripe_base[nstripes + 1], nstripes: the corpus and
// its index as for multi_contains_corpus; bytes is 16-byte aligned, no byte below offset 0 or at or beyond nbytes is read.
// nullable, in_global and lines beyond 0xFFFFFFFE bytes as for search_longest_extents_dfa.
int search_longest_corpus_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, size_t nbytes, uint32_t stripe,
                              const uint64_t *stripe_base, size_t nstripes, uint32_t *match_start, uint32_t *match_end, void *stream);

// ---- all leftmost-longest matches per explicit item, a lane per item: kernels_search_all_longest_items.hip
// The matches of item i are those of search_longest_extents_dfa applied again and again to the rest of the item behind the previous
// match (one byte further after an empty match).  first == nullptr (COUNT): the backward walk on starts leaves a MARK bit in `marks`
// for every offset at which some match starts - the bit of byte g of item i is bit (g - off[0]) & 31 of word ((g - off[0]) >> 5) + i,
// every word of an item's range stored, no other - and the forward phase on the marks counts: count[i], every one of the nitems
// words written with a plain store.  Otherwise (`first`: the caller's exclusive prefix of the counts) the forward phase alone, on
// the marks a COUNT launch on the same batch left: match k of item i goes to slot first[i] + k of match_start / match_end, relative
// to the item; slots >= cap are not written, nor any other slot.  marks holds marks_words words, at least
// search_all_longest_marks_words(extent, nitems) for extent >= off[nitems] - off[0]; words at or beyond marks_words are not touched.
// nullable: every offset 0 .. length is a start, marks is not touched.  Placement and long items as search_longest_extents_dfa.
size_t search_all_longest_marks_words(size_t extent_bytes, size_t nitems);
int search_all_longest_extents_dfa(const SearchLongestDevice &p, bool in_global, bool nullable, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                                   uint32_t trim, uint32_t *marks, size_t marks_words, uint32_t *count, const uint64_t *first, uint32_t *match_start,
                                   uint32_t *match_end, size_t cap, void *stream);

// ---- the span of a top-level capture group inside a known match, a lane per item: kernels_group_items.hip
// The four plain tables of a pattern A(B)C split at its group (lower.hpp: lower_dfa, lower_dfa_reversed), one image: a = A and b = B
// anchored forwards, rev_bc = (B)C and rev_c = C right to left, anchored; in each row 0 is dead and absorbing and class 0 leads
// there (pack_group checks it).  The table of an absent part is empty (nstates = 0, null pointers) and never launched.
struct GroupDevice {
    DfaDevice a, rev_bc, b, rev_c;
};
// The longest split point: for item i = bytes[off[i] .. off[i+1] - trim) and the stretch [lo[i], hi[i]] of it (relative to the item,
// clamped into it: no byte outside the item is read whatever the arrays hold), out[i] = the LARGEST x in [lo, hi] with item[lo, x)
// accepted by `fwd` and item[x, hi), read right to left, accepted by `rev`; ~0u where there is none or lo[i] == ~0u, and then
// on_none[i] = ~0u too (on_none may be null; it is left alone otherwise).  Every one of the nitems words of `out` is written with a
// plain store.  lo, hi, out and on_none may be the same arrays: a lane reads its own entries before it writes them.  The backward
// pass leaves a MARK bit for every offset p of the stretch with item[p, hi) accepted by rev: the bit of absolute offset g is bit
// (g - off[0]) & 31 of word ((g - off[0]) >> 5) + i of `marks` - every word of an item's stretch stored, no other, none at or
// beyond marks_words; search_all_longest_marks_words(extent, nitems) words hold them.  Placement (in_global) and long items as
// search_longest_extents_dfa.
int longest_split_dfa(const DfaDevice &rev, const DfaDevice &fwd, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                      const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out, uint32_t *on_none, void *stream);

// The same for every match of a match list (first: nitems + 1 entries, match k of item i is slot first[i] + k; lo, hi, out and
// on_none are indexed by the slot itself): a lane per item walking its slots, exactly the slots first[0] .. first[nitems] written.
// The marks as above, except that the consecutive slots of an item store the words they share one after the other.
int longest_split_list_dfa(const DfaDevice &rev, const DfaDevice &fwd, bool in_global, const uint8_t *bytes, const uint64_t *off, size_t nitems,
                           uint32_t trim, const uint64_t *first, const uint32_t *lo, const uint32_t *hi, uint32_t *marks, size_t marks_words, uint32_t *out,
                           uint32_t *on_none, void *stream);
// The slots first[0] .. first[nitems] of dst_a and dst_b (either may be null: left out), copied from src_a / src_b or, where that is
// null, filled with ~0u: the slot range is known on the device only.
int slot_range_copy(const uint64_t *first, size_t nitems, const uint32_t *src_a, uint32_t *dst_a, const uint32_t *src_b, uint32_t *dst_b, void *stream);

// ---- regexp_replace on explicit items, from a match list: kernels_replace_items.hip
// Item i = bytes[off[i] .. off[i+1] - trim); its matches are the slots first[i] .. first[i + 1] of match_start / match_end (relative
// to the item, in order, not overlapping: what every search_all* launcher above leaves); R = `rep_len` literal bytes.  The output
// item is the item with every match replaced by R.  No table: the kernels do not know which search made the list.
// replace_sizes (a lane per item): len[i] = the output item's length, saturated at ~0u, every one of the nitems words written;
// pos[slot] = the offset inside the output item at which that match's R begins, exactly the slots first[0] .. first[nitems].
// too_long != nullptr: *too_long = 1 (a plain store) if some output item has 2^30 bytes or more - what scan_counts cannot carry.
// replace_fill (a wave per 64 items, driven by output bytes): exactly the bytes out[out_off[0] .. out_off[nitems]), for item i
// nothing outside [out_off[i], out_off[i + 1]) whatever the lists hold; no byte outside an item is read (a source offset at or
// beyond the item's end gives 0).  rep (device memory) may be null when rep_len == 0, out when nothing can be written; both and
// `bytes` may sit at any address.  Both launch at most kReplaceMaxBlocks workgroups of kThreads lanes, then the grid strides.
constexpr size_t kReplaceMaxBlocks = 512;        // one generation on the 256 CUs at two workgroups each
int replace_sizes(const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start, const uint32_t *match_end,
                  uint32_t rep_len, uint32_t *len, uint32_t *pos, uint32_t *too_long, void *stream);
int replace_fill(const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_end,
                 const uint32_t *pos, const uint8_t *rep, uint32_t rep_len, const uint64_t *out_off, uint8_t *out, void *stream);

// ---- regexp_replace with group references, from a match list and reference spans: kernels_replace_template_items.hip
// The replacement of slot q is the concatenation of the template's segments (template.hpp), at most kTemplateMaxSegments: the bytes
// of a literal, item[s', e') of the match itself (kind 1) or of plane r's span (kind 2 + r: words r * plane_stride + q of ref_start /
// ref_end), s' = min(s, L), e' = clamp(e, s', L), nothing for a start of ~0u.  The segment program is three words per segment (kind,
// the literal's offset into `lits`, its length) in device memory; the kernels keep it in LDS.
constexpr uint32_t kTemplateMaxSegments = 32;
struct TemplateDevice {
    const uint32_t *segs = nullptr;              // nseg x 3 words
    const uint8_t *lits = nullptr;               // the literals' bytes, one behind the other
    uint32_t nseg = 0;
};
// replace_template_sizes / _fill: replace_sizes / replace_fill with R_k, the replacement of slot k, in place of R.
int replace_template_sizes(const TemplateDevice &tpl, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start,
                           const uint32_t *match_end, const uint32_t *ref_start, const uint32_t *ref_end, uint64_t plane_stride, uint32_t *len, uint32_t *pos,
                           uint32_t *too_long, void *stream);
int replace_template_fill(const TemplateDevice &tpl, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first,
                          const uint32_t *match_start, const uint32_t *match_end, const uint32_t *pos, const uint32_t *ref_start, const uint32_t *ref_end,
                          uint64_t plane_stride, const uint64_t *out_off, uint8_t *out, void *stream);

// ---- regexp_extract_all / split on explicit items, from a match list: kernels_pieces_items.hip
// Items and lists as for replace_sizes.  The PIECES of item i are its matches (gaps == false: m of them) or what lies between them
// (gaps == true: m + 1, the stretch before the first match, between two matches, behind the last), every start and end clamped into
// the item and behind the previous match's end, so that a piece lies inside its item whatever the list holds.
// pieces_sizes (a lane per item): list_off[i] = the item's first piece (first[i] - first[0], + i with gaps), all nitems + 1 words;
// for every piece piece_len[p] = its length saturated at ~0u and piece_src[p] = off[i] + its start, exactly the slots 0 .. npieces - 1.
// too_long != nullptr: *too_long = 1 (a plain store) if some piece has 2^30 bytes or more - what scan_counts cannot carry.
// pieces_fill: out[piece_off[p] + r] = bytes[piece_src[p] + r], r < piece_off[p + 1] - piece_off[p]: exactly the bytes
// out[piece_off[0] .. piece_off[npieces]), no byte of `bytes` outside a piece read; `bytes` and `out` may sit at any address, out may
// be null when nothing can be written.  It knows neither items nor matches: any ascending piece_off and any piece_src will do.  The
// output range is cut into chunks of kPiecesChunk bytes (at dword-aligned addresses) that the waves of a FIXED grid of
// kPiecesMaxBlocks workgroups take grid-stride: the output's size is on the device.
constexpr uint32_t kPiecesChunk = 4096;          // bytes of output per wave and turn of its chunk loop: 16 sweeps of 256 bytes
constexpr size_t kPiecesMaxBlocks = kReplaceMaxBlocks;
int pieces_sizes(const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start, const uint32_t *match_end,
                 bool gaps, uint64_t *list_off, uint32_t *piece_len, uint64_t *piece_src, uint32_t *too_long, void *stream);
int pieces_fill(const uint8_t *bytes, const uint64_t *piece_src, const uint64_t *piece_off, size_t npieces, uint8_t *out, void *stream);

// ---- the rows a result bitmap selects, as a new column: kernels_filter.hip
// Any bitmap in the result layout (bit i & 31 of word i >> 5 = row i).  invert == false: a row is selected iff its bit is 1;
// true: iff it is 0; the bits of the last word beyond nbits are never selected.
// bitmap_rank: rank[w] = the selected rows in front of word w, w = 0 .. nwords (rank[nwords] = all of them), plain numbers; the array
// holds bitmap_rank_words(nbits) u64 words - behind the nwords + 1 entries the chunk sums of scan_counts and the popcount words it
// scans.  Launches only (and one 8-byte memset): capturable.  nbits == 0: rank[0] = 0.
// filter_items (a lane per row, at most kFilterMaxBlocks workgroups of kThreads lanes, then the grid strides) and filter_corpus (a
// lane per stripe of the corpus' index, nlines = its line count): for the k-th selected row - k its rank - row[k] = its number,
// piece_src[k] = the absolute offset of its first byte (off[i]; the line's start), piece_len[k] = its length saturated at ~0u (the
// item without `trim`, 0 where trim exceeds it; the line without its '\n', plus 1 with keep_newline where the line has one in the
// text): exactly the slots 0 .. rank[nwords] - 1, plain stores, nothing to clear; what pieces_fill takes once piece_len is prefixed.
// row may be null (not stored).  too_long as for pieces_sizes.  filter_corpus reads no byte at or beyond nbytes and, for a lane
// without a selected line, no byte at all.
constexpr size_t kFilterMaxBlocks = kReplaceMaxBlocks;
size_t bitmap_rank_words(size_t nbits);
int bitmap_rank(const uint32_t *bits, size_t nbits, bool invert, uint64_t *rank, void *stream);
int filter_items(const uint64_t *off, size_t nitems, uint32_t trim, const uint32_t *bits, bool invert, const uint64_t *rank, uint64_t *row, uint32_t *piece_len,
                 uint64_t *piece_src, uint32_t *too_long, void *stream);
int filter_corpus(const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes, size_t nlines, const uint32_t *bits,
                  bool invert, bool keep_newline, const uint64_t *rank, uint64_t *row, uint32_t *piece_len, uint64_t *piece_src, uint32_t *too_long,
                  void *stream);

// ---- one long string on the plain DFA: kernels_long.hip
// One long string (regex.h:156-159 consumes it byte by byte): the string is cut into chunks, every chunk is stepped
// from EVERY table state at once (lane = (chunk, start state); the lanes of a chunk read the same text), which yields
// one state -> state map per chunk; maps are then composed in groups until one is left.  `scratch` holds the maps.
constexpr uint32_t kLongMaxStates = 254;         // row offsets state * 129 stay 16-bit
constexpr uint32_t kLongGroup = 128;             // maps composed per workgroup and level
// short strings: 256-byte chunks (a string of a few KiB is a handful of short launches, not one long sequential lane);
// from 256 KiB on chunks of 1 KiB or more, at most 65536 of them
inline uint32_t long_chunk(size_t nbytes) {
    uint32_t chunk = 256;
    while (((nbytes + chunk - 1) / chunk) > (chunk < 1024 ? 1024u : 65536u)) chunk <<= 1;
    return chunk;
}
size_t long_scratch_bytes(uint32_t nstates, size_t nbytes, uint32_t *chunk);
int match_long_dfa(const DfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t chunk, void *scratch, uint8_t *accept,
                   void *stream);

// ---- a directional run over one long string on a plain DFA: kernels_long_search.hip
// The table p (at most kLongMaxStates states) stepped over bytes[0, nbytes), nbytes > 0, forwards (from byte 0 up) or backwards
// (from byte nbytes - 1 down), from the state held in the device word *start_state, in chunks of long_chunk(nbytes) bytes counted
// in WALKING order (chunk 0 is walked first; backwards the chunks are counted from the string's end):
//   1  the chunk maps in walking order (kernels_long.hpp: the four-step build, the backward walk where `backward`);
//   2  up-sweep: groups of kLongGroup maps composed level by level until a level has at most kLongGroup maps, EVERY level kept;
//   3  down-sweep (long_entries_kernel): from that level down to the chunks, a workgroup per group stages the group's maps in LDS
//      and walks them in order from the group's entry state: the state every child is entered in;
//   4  extreme offset (long_extreme_kernel): a lane per chunk walks its chunk again from its entry state and keeps the LAST offset
//      in walking order at which the table is in an accepting state after a byte, and the chunk's exit state; long_reduce_kernel
//      takes the extreme of the chunks and the last chunk's exit state.
// out->extreme: forwards the LARGEST p + 1 such that the table accepts after the byte at offset p, backwards the SMALLEST p such
// that it accepts after the byte at p; ~0ull where it never accepts.  out->exit_state: the state after the whole run.  (The start
// state itself is not an event: no byte has been taken.)  row0_dead: row 0 of p is dead and absorbing (the anchored table of
// pack_search_longest) - lanes entered in it, or arriving there, stop.  A single chunk skips steps 1 to 3.  bytes needs no
// alignment.  Everything is written with plain vector stores, nothing needs clearing beforehand; `scratch` holds
// long_run_scratch_bytes(p.nstates, N) bytes for any N >= nbytes; out and start_state are device memory outside it (they may
// be the same record of two consecutive runs' hand-over: start_state is read before out is written).
struct LongRunResult {
    uint64_t extreme;
    uint32_t exit_state, pad;
};
size_t long_run_scratch_bytes(uint32_t nstates, size_t nbytes);
int long_run_dfa(const DfaDevice &p, bool backward, bool row0_dead, const uint8_t *bytes, size_t nbytes, const uint32_t *start_state, void *scratch,
                 LongRunResult *out, void *stream);
// *word = value, on the stream (the start state of a first run)
int long_set_word(uint32_t *word, uint32_t value, void *stream);

// ---- search: kernels_search.hip
// Search (the reference has acceptance only).  Per line: the match [s, e) with the smallest e, then the smallest s.
// Host tables: fwd = "any bytes, then the pattern" (never dies; accepting where some match ends), rev = the pattern read right to
// left (accepting, walking back from a match end, where a match starts).
// Stripe-wise search (kernels_search.hip).  The forward table is the LINE MODE product table (lower_search_line: one row per
// reachable pair of states plus the SKIP row - the line's first match has been found: wait for '\n' -, one column per byte
// class plus the '\n' column) in its STRIDE-2 form (lower_search_line2): one dependent lookup consumes two bytes and yields
// the four event bits of the pair.  Two layouts:
//   LDS form    (in_global = 0): P8[128][kSearchP8Stride] = 2 * pair column (a byte), T2 / T2_all[nrows][row_bytes / 2] with
//               16-bit entries (base_row + next row) << 4 | events; the kernel puts P8 at LDS address 0 and the table at
//               base_row * row_bytes, so that an entry's row field times row_bytes IS the row's LDS address;
//   global form (in_global = 1): the table stays in HBM/L2 (any size up to 256 MiB), P16[128][kSearchP16Stride] = 4 * pair
//               column in LDS, G2 / G2_all[nrows][ncols2] with 32-bit entries byte offset of the next row | events << 28.
// events = (flags of the first byte) << 2 | flags of the second; flags: 1 '\n', 2 hit, 3 hit whose match starts at the restart point.
constexpr uint32_t kSearchP8Stride = 132, kSearchP8Bytes = 128 * kSearchP8Stride;          // (33 dwords per row: odd)
constexpr uint32_t kSearchP16Stride = 130, kSearchP16Bytes = 128 * kSearchP16Stride * 2;
struct SearchChunkDevice {
    uint32_t nrows = 0, ncols2 = 0, row_bytes = 0, base_row = 0, in_global = 0;
    uint32_t start_row = 0, skip_row = 0;        // row indices (without base_row)
    uint32_t nr = 0, ncls = 0, start_r = 0;
    const uint8_t *P8 = nullptr;
    const uint16_t *P16 = nullptr;
    const uint16_t *T2 = nullptr, *T2_all = nullptr;
    const uint32_t *G2 = nullptr, *G2_all = nullptr;
    const uint16_t *rev = nullptr;               // [nr][ncls] reverse table, bit 15 = leads to an accepting state
    const uint8_t *cls = nullptr;                // [256] byte -> class
};
constexpr size_t kSearchChunkLdsBudget = 160 * 1024;     // one workgroup of 16 waves per CU: the whole LDS
size_t search_chunk_bytes();                             // bytes of text per wave (the granularity of its newline index)
size_t search_chunks_lds_bytes(const SearchChunkDevice &p);
// chunk_base: per-chunk newline prefix in the stripe_base format (bit 63: the chunk begins at the start of a line)
// clean: the text may hold bytes >= 0x80 (they cannot index the pair table: stepped as 0x00, which no pattern takes either)
// nlines: lines of the corpus (picks the build for chunks that hold more lines than the staging array: 5-byte lines)
int search_chunks(const SearchChunkDevice &p, bool clean, const uint8_t *bytes, size_t nbytes, const uint64_t *chunk_base, size_t nchunks, size_t nlines,
                  uint32_t *match_start, uint32_t *match_end, void *stream);
// all matches: count[line], then (with the caller's exclusive prefix `first`) the matches of line i at first[i], first[i] + 1, ...
int search_chunks_count(const SearchChunkDevice &p, bool clean, const uint8_t *bytes, size_t nbytes, const uint64_t *chunk_base, size_t nchunks,
                        uint32_t *count, void *stream);
int search_chunks_fill(const SearchChunkDevice &p, bool clean, const uint8_t *bytes, size_t nbytes, const uint64_t *chunk_base, size_t nchunks,
                       const uint64_t *first, uint32_t *match_start, uint32_t *match_end, void *stream);
// count and fill in one launch: first[nlines + 1] (CSR offsets of the lines' matches) and the matches themselves, slots
// >= cap counted but not written; scratch = search_all_scratch_bytes(nchunks), zeroed before the launch, holds the
// per-chunk status words, then the total (u64), then {ticket, error flag} (u32 each)
size_t search_all_scratch_bytes(size_t nchunks);
int search_chunks_all(const SearchChunkDevice &p, bool clean, const uint8_t *bytes, size_t nbytes, const uint64_t *chunk_base, size_t nchunks, size_t nlines,
                      uint64_t *first, uint32_t *match_start, uint32_t *match_end, size_t cap, void *scratch, void *stream);

// ---- NFA lane engines: kernels_nfa.inc (built by width in kernels_nfa_w*.hip; the entry points are in kernels_coop.hip)
int match_stripes_nfa(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                      size_t nstripes, uint32_t *accept_bits, void *stream);
int match_onepass_nfa(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                      uint32_t *slabs, void *stream);
int recheck_escaped_nfa(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes,
                        const uint32_t *escaped_bits, size_t nlines, const uint64_t *list, const unsigned long long *escaped_total, size_t cap,
                        uint32_t *accept_bits, void *stream);
int match_extents_nfa(const NfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                      uint8_t *accept, void *stream);
// "Contains a match" on the lane program with the contains B rows (pack.hpp: contains_b_rows): the line engine with a sticky
// `found` over the stripes of a corpus (the bitmap cleared by the caller: words are merged with atomic OR), and a lane per item
// (every word of the bitmap written: nothing to clear).
int contains_stripes_nfa(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                         size_t nstripes, uint32_t *bits, void *stream);
int contains_extents_nfa(const NfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *bits,
                         void *stream);
// One long string on the NFA lane engines: per chunk the rows "positions reached from position p" (lane = (chunk, p)), then
// the relations applied in order to {initial}.  `scratch` holds the rows (long_nfa_scratch_bytes).
size_t long_nfa_scratch_bytes(const NfaDevice &p, size_t nbytes, uint32_t *chunk, uint32_t *nchunks);
int match_long_nfa(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t chunk, uint32_t nchunks, void *scratch, uint8_t *accept,
                   void *stream);

// ---- group-cooperative NFA: kernels_coop.hip
int match_stripes_group_nfa(const GroupNfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                            size_t nstripes, uint32_t *accept_bits, void *stream);
int match_extents_group_nfa(const GroupNfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                            uint8_t *accept, void *stream);

// ---- wave-resident NFA and its sparse form: kernels_wave.hip
uint32_t wave_words_per_lane(uint32_t words);    // the instantiated WL that holds `words` 32-bit words (0: too many)
// The SPARSE form of the same engine (kernels_wave.hip: SparseNfa): WL then counts ROWS of 2048 positions and masks / Bbyte are
// laid out by rows - [3][WL][64] and [257][WL][64]: word w of the set = row w / 64, lane w % 64.
uint32_t sparse_rows(uint32_t words);            // the instantiated row count that holds `words` 32-bit words (0: too many)
int match_stripes_sparse_nfa(const WaveNfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                             size_t nstripes, uint32_t *accept_bits, void *stream);
int match_extents_sparse_nfa(const WaveNfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                             uint8_t *accept, void *stream);
int match_stripes_wave_nfa(const WaveNfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                           size_t nstripes, uint32_t *accept_bits, void *stream);
int match_extents_wave_nfa(const WaveNfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                           uint8_t *accept, void *stream);

}  // namespace dev
}  // namespace rrx
