// kernels_items.hip — explicit items (an offsets array over one byte buffer) matched stripe-wise: the item-end bitmap and its
// index kernel, the byte-stride and stride-2 items kernels and their launchers (match: a byte per item; contains: a bitmap).
// Engines: table_engines.hpp.
#include "table_engines.hpp"

namespace rrx {
namespace dev {
namespace {

// ============================================================================================ explicit items, stripe-wise
// (r4) The item-end bitmap is stored TRANSPOSED inside groups of 64 stripes: the 16 bytes (128 marks) of stripe g's round r sit at
// ((g / 64) * rounds + r) * 1 KiB + (g % 64) * 16 - what the 64 lanes of a wave ask for in one round is one contiguous KiB.  In the
// plain order a lane's 16 bytes lay stripe / 8 bytes from its neighbour's, a cache line each, and by the lane's next round the
// line was gone again: the items kernels fetched 2.2 x the bytes of the text (FETCH_SIZE; 0.36 ms per GiB whatever the table).
// A permutation of 16-byte pieces inside a group's part of the bitmap: the index kernel writes every word once as before.
__device__ __forceinline__ size_t ends_slot(size_t word, uint32_t sw_log2) {           // sw_log2 = log2(stripe / 32): words per stripe
    const size_t g = word >> sw_log2;
    const uint32_t j = (uint32_t)word & ((1u << sw_log2) - 1u);
    return ((((g >> 6) << (sw_log2 - 2)) + (j >> 2)) << 8) + ((g & 63) << 2) + (j & 3);
}
// rrx_match_extents on a large batch (an offsets array over one byte buffer: an Arrow-style string column): the items are
// lines without a delimiter.  match_extents_kernel gives every lane an item (0.9-1.0 TB/s: consecutive lanes read text an
// item apart).  Here the buffer is cut into stripes exactly like a corpus, and the item ends come from a bitmap built from
// the offsets (1 bit per byte) instead of a byte value.  The table is the plain table in the wide line-table format with
// one more column (abi.cpp: items_table): byte values 0..127 - '\n' an ordinary byte -, 128 = any byte >= 0x80, 129 = END OF
// ITEM (the verdict of the row, back to the start row):
//   ENDS = 1 (trim 1: every item is followed by one separator byte): the marked byte is the separator, stepped as byte 129;
//   ENDS = 2 (trim 0): the marked byte is the item's last byte, a byte 129 is stepped after it.
// Bytes >= 0x80 of the text are stepped as 0x80.
template <int ENDS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void match_items_stripes_kernel(LineDfaDevice prog, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                        uint32_t stripe, const uint64_t *__restrict__ stripe_base,
                                                                        const uint32_t *__restrict__ ends, uint32_t *__restrict__ accept_bits,
                                                                        uint32_t stage_off, uint32_t stage_words,
                                                                        const uint64_t *__restrict__ off, size_t nitems,
                                                                        const uint32_t *__restrict__ skip_if) {
    typedef LineDfaEngine<true, false> Engine;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // One-call form (rrx_match_extents, asynchronous): the host knows neither where the batch starts nor how long it is -
    // both come from the offsets here - and the index pass may have found the batch unfit (*skip_if != 0: an item without
    // a byte for its mark, a misaligned start, too small): then the lane-per-item kernel queued behind this one runs instead.
    if (skip_if && *skip_if) return;
    if (off) { const uint64_t first = off[0]; bytes += first; nbytes = (size_t)(off[nitems] - first); }
    if ((size_t)blockIdx.x * kThreads * stripe >= nbytes) return;    // (the grid was sized from an upper bound)
    uint32_t *stage = reinterpret_cast<uint32_t *>(smem + stage_off);
    Engine eng;
    eng.load(prog, smem);
    for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) stage[i] = 0;
    __syncthreads();
    const size_t g0 = (size_t)blockIdx.x * kThreads;
    const uint64_t window_word = line_of(stripe_base[g0]) >> 5;
    const size_t g = g0 + threadIdx.x;
    const size_t start = g * (size_t)stripe;
    if (start < nbytes) {
        const size_t stripe_end = start + stripe;
        const size_t my_end = stripe_end < nbytes ? stripe_end : nbytes;
        const uint64_t my_base = stripe_base[g];
        const bool fresh = (my_base & kFreshStripe) != 0;
        ResultsT<true> res;
        res.begin_staged(line_of(my_base), window_word, !fresh, accept_bits, stage);
        res.stage_words = stage_words;
        typename Engine::State st = fresh ? eng.fresh() : eng.skipping();
        const uint32_t swl = (uint32_t)__builtin_ctz(stripe) - 5u;
        auto end_bit = [&](size_t pos) -> bool { return (ends[ends_slot(pos >> 5, swl)] >> (pos & 31)) & 1u; };
        // one byte with its end bit: -> (nl, acc) of the step that matters
        // (plain entries carry "the next row is accepting" in bit 7 of the byte that is the line count elsewhere: see word())
        auto step1 = [&](uint32_t c, uint32_t &nl, uint32_t &acc) { eng.step(st, c, nl, acc); nl &= 1u; };
        auto step_byte = [&](size_t pos, uint32_t &nl, uint32_t &acc) {
            uint32_t c = bytes[pos];
            const bool m = end_bit(pos);
            if (c >= 0x80u) c = 0x80u;
            if (ENDS == 1 && m) c = kItemEndColumn;
            step1(c, nl, acc);
            if (ENDS == 2 && m) step1(kItemEndColumn, nl, acc);
        };
        // a text word (no byte >= 0x81 in it) with the end bits m4 of its four bytes
        auto word = [&](uint32_t w, uint32_t m4) {
            if constexpr (ENDS == 1) {
                {   // (no test for "some lane has a separator in this word": with 64 lanes it is nearly always so)
                    // bit k of m4 -> byte k (24-bit multiply: v_mul_lo_u32 runs at a quarter of the rate)
                    const uint32_t t = __umul24(m4, 0x00204081u) & 0x01010101u;
                    const uint32_t bm = (t << 8) - t;
                    w = (w & ~bm) | (0x81818181u & bm);
                }
                eng.consume_word(st, w, res.bits);
            } else {
                // trim 0: an item that ends ON this byte reports the verdict of the row the byte leads to and goes back to the start row
                // - the END column's entry, whose verdict the plain entry carries in bit 23.  So the marked lanes take (start row | one
                // line | that verdict) in place of what they read: three VALU more per byte, no second lookup, no branch.  (Round 2 and
                // the first half of round 3 stepped the END column under a wave-wide test per byte: with 64 lanes some lane nearly always
                // has a mark, so nearly every byte paid two dependent lookups - 12.7 VALU, 5.4 SALU and 1.8 LDS reads per byte.)
                const uint32_t end_entry = eng.start_off | 1u << 16;
                uint32_t mk, x, t0, t1;
#define RRX_ITEM_BYTE(SEL, KBIT)                                                                                                          \
                asm volatile("v_lshlrev_b32_sdwa %[c4], %[two], %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t" \
                             "v_add_u32_sdwa %[ad], %[e], %[c4] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t"       \
                             "ds_read_b32 %[e], %[ad]\n\t"                                                                                  \
                             "v_bfe_i32 %[mk], %[m4], " KBIT ", 1\n\t"                                                                       \
                             "s_waitcnt lgkmcnt(0)\n\t"                                                                                     \
                             "v_and_b32 %[x], 0x800000, %[e]\n\t"                                                                           \
                             "v_lshl_or_b32 %[x], %[x], 1, %[ee]\n\t"                                                                       \
                             "v_bfi_b32 %[e], %[mk], %[x], %[e]\n\t"                                                                        \
                             "v_lshlrev_b32_sdwa %[b], %[e], %[b] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD\n\t"     \
                             "v_or_b32_sdwa %[b], %[e], %[b] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD"              \
                             : [e] "+v"(st.e), [b] "+v"(res.bits), [c4] "=&v"(t0), [ad] "=&v"(t1), [mk] "=&v"(mk), [x] "=&v"(x)               \
                             : [w] "v"(w), [two] "v"(eng.col_shift), [m4] "v"(m4), [ee] "v"(end_entry)                                       \
                             : "memory")
                RRX_ITEM_BYTE("BYTE_0", "0"); RRX_ITEM_BYTE("BYTE_1", "1"); RRX_ITEM_BYTE("BYTE_2", "2"); RRX_ITEM_BYTE("BYTE_3", "3");
#undef RRX_ITEM_BYTE
            }
        };
        auto clamp = [](uint32_t w) -> uint32_t { const uint32_t hi = w & 0x80808080u; return w & ~(hi - (hi >> 7)); };      // >= 0x80 -> 0x80
        size_t pos = start;
        const uint4 *src = reinterpret_cast<const uint4 *>(bytes + start);
        const uint4 *esrc = reinterpret_cast<const uint4 *>(ends + ends_slot(start >> 5, swl));      // 128 bits per 128-byte round, rounds 1 KiB apart
        constexpr int kSlots = kRound / 16;
        const int rounds = (int)((my_end - start) / kRound);
        TextRound<kSlots> buf;
        uint4 eb = make_uint4(0, 0, 0, 0);
        if (rounds > 0) { buf.load(src); eb = esrc[0]; }
        for (int r = 0; r < rounds; r++) {
            const uint32_t ew[4] = {eb.x, eb.y, eb.z, eb.w};
            int slot = 0;
            buf.for_each_slot([&](const uint4 &v) {
                const uint32_t sb = (ew[slot >> 1] >> (16 * (slot & 1))) & 0xffffu;           // (slot: a constant after inlining)
                if (__builtin_amdgcn_ballot_w64(((v.x | v.y | v.z | v.w) & 0x80808080u) != 0)) {     // rare on text: one test per 16 bytes
                    word(clamp(v.x), sb & 15u); word(clamp(v.y), (sb >> 4) & 15u); word(clamp(v.z), (sb >> 8) & 15u); word(clamp(v.w), sb >> 12);
                } else {
                    word(v.x, sb & 15u); word(v.y, (sb >> 4) & 15u); word(v.z, (sb >> 8) & 15u); word(v.w, sb >> 12);
                }
                if (res.bits >> 15) res.flush();
                slot++;
            });
            if ((r & 3) == 3) res.flush();
            if (r + 1 < rounds) { buf.load(src + (size_t)(r + 1) * kSlots); eb = esrc[(size_t)(r + 1) * 64]; }
        }
        pos += (size_t)rounds * kRound;
        for (; pos < my_end; pos++) {                                 // tail of the buffer inside my stripe
            uint32_t nl, acc;
            step_byte(pos, nl, acc);
            res.push(nl, acc);
            if (res.bits >> 30) res.flush();
        }
        res.flush();
        // the item that straddles my stripe end is mine if it started here: follow it to its end
        const bool started = fresh || res.seen > 0;
        if (started && !end_bit(my_end - 1)) {
            uint32_t nl = 0, acc = 0;
            // 16 bytes and their 16 end bits per turn (pos is 16-byte aligned: stripes are multiples of 128; one byte and one
            // bitmap word per turn was a chain of 150 memory round trips for the slowest lane of a wave on 95-byte items)
            while (pos + 16 <= nbytes && !nl) {
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
                const uint32_t e16 = (ends[ends_slot(pos >> 5, swl)] >> (pos & 31)) & 0xffffu;
                const uint32_t w[4] = {clamp(v.x), clamp(v.y), clamp(v.z), clamp(v.w)};
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    if (!nl) {
                        uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
                        const bool m = (e16 >> k) & 1u;
                        if (ENDS == 1 && m) c = kItemEndColumn;
                        step1(c, nl, acc);
                        if (ENDS == 2 && m) step1(kItemEndColumn, nl, acc);
                    }
                }
                pos += 16;
            }
            for (; pos < nbytes && !nl; pos++) step_byte(pos, nl, acc);
            if (!nl) step1(kItemEndColumn, nl, acc);                   // (cannot happen: the last item ends where the buffer ends)
            res.push(nl, acc);
        }
        res.finish();
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) {
        const uint32_t v = stage[i];
        if (v) atomicOr(&accept_bits[window_word + i], v);
    }
}
// (r4) The same batch with a separator byte behind every item (trim 1) on the STRIDE-2 table of its own (lower_dfa2's items form):
// codes 0 ... 127 are the byte values - '\n' an ordinary byte -, code 128 is END OF ITEM, and the kernel puts it in the place of
// every marked byte (one v_perm_b32 per text word, its selector made from the word's four mark bits); bytes >= 0x80 are stepped
// as 0x00, which no pattern takes either.  From there on it is the batch kernel's step - two bytes per dependent lookup - with the
// items kernel's stripes, marks and result window.  (trim 0 stays on the byte-stride kernel above: an item that ends ON a byte
// needs that byte and the end in one symbol, and a pair with a mark on its first byte a second dependent lookup.)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void match_items_stripes2_kernel(Dfa2Device prog, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                         uint32_t stripe, const uint64_t *__restrict__ stripe_base,
                                                                         const uint32_t *__restrict__ ends, uint32_t *__restrict__ accept_bits,
                                                                         const uint64_t *__restrict__ off, size_t nitems,
                                                                         const uint32_t *__restrict__ skip_if) {
    __shared__ __attribute__((aligned(16))) struct {
        uint8_t t2_and_stage[kDfa2RegionBytes];
        uint16_t p[kDfa2PItemsBytes / 2];
    } lds;
    if (skip_if && *skip_if) return;                                 // (see match_items_stripes_kernel)
    if (off) { const uint64_t first = off[0]; bytes += first; nbytes = (size_t)(off[nitems] - first); }
    if ((size_t)blockIdx.x * kThreads * stripe >= nbytes) return;
    Dfa2 eng;
    eng.load(prog, lds.p, lds.t2_and_stage, kDfa2PItemsBytes);
    const uint32_t stage_off = (uint32_t)((Dfa2::lds_bytes(prog) + 15) & ~(size_t)15);
    uint32_t *const stage = reinterpret_cast<uint32_t *>(lds.t2_and_stage + stage_off);
    const uint32_t stage_words = (kDfa2RegionBytes - stage_off) / 4;
    for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) stage[i] = 0;
    __syncthreads();
    const size_t g0 = (size_t)blockIdx.x * kThreads;
    const uint64_t window_word = line_of(stripe_base[g0]) >> 5;
    const size_t g = g0 + threadIdx.x;
    const size_t start = g * (size_t)stripe;
    if (start < nbytes) {
        const size_t stripe_end = start + stripe;
        const size_t my_end = stripe_end < nbytes ? stripe_end : nbytes;
        const uint64_t my_base = stripe_base[g];
        const bool fresh = (my_base & kFreshStripe) != 0;
        ResultsT<true> res;
        res.begin_staged(line_of(my_base), window_word, !fresh, accept_bits, stage);
        res.stage_words = stage_words;
        Dfa2::State st = fresh ? eng.fresh() : eng.skipping();
        const uint32_t swl = (uint32_t)__builtin_ctz(stripe) - 5u;
        auto end_bit = [&](size_t pos) -> bool { return (ends[ends_slot(pos >> 5, swl)] >> (pos & 31)) & 1u; };
        auto code_at = [&](size_t pos) -> uint32_t { const uint32_t c = bytes[pos]; return end_bit(pos) ? 128u : c >= 0x80u ? 0u : c; };
        auto clean = [](uint32_t w) -> uint32_t { const uint32_t hi = (w & 0x80808080u) >> 7; return w & ~(hi * 0xffu); };       // >= 0x80 -> 0x00
        // the four bytes of a text word (none >= 0x80) with their mark bits m4: marked bytes become code 128
        auto word = [&](uint32_t w, uint32_t m4) {
            // bit k of m4 -> bit 2 of byte k: selector k + 4 (a byte of the constant) where marked, k (the text byte) elsewhere
            const uint32_t sel = (__umul24(m4, 0x00810204u) & 0x04040404u) | 0x03020100u;
            eng.consume_dword_items(st, __builtin_amdgcn_perm(0x80808080u, w, sel), res.bits);
        };
        size_t pos = start;
        const uint4 *src = reinterpret_cast<const uint4 *>(bytes + start);
        const uint4 *esrc = reinterpret_cast<const uint4 *>(ends + ends_slot(start >> 5, swl));      // 128 bits per 128-byte round, rounds 1 KiB apart
        constexpr int kSlots = kRound / 16;
        const int rounds = (int)((my_end - start) / kRound);
        TextRound<kSlots> buf;
        uint4 eb = make_uint4(0, 0, 0, 0);
        if (rounds > 0) { buf.load(src); eb = esrc[0]; }
        for (int r = 0; r < rounds; r++) {
            const uint32_t ew[4] = {eb.x, eb.y, eb.z, eb.w};
            int slot = 0;
            buf.for_each_slot([&](const uint4 &v) {
                const uint32_t sb = (ew[slot >> 1] >> (16 * (slot & 1))) & 0xffffu;           // (slot: a constant after inlining)
                if (__builtin_amdgcn_ballot_w64(((v.x | v.y | v.z | v.w) & 0x80808080u) != 0)) {     // rare on text: one test per 16 bytes
                    word(clean(v.x), sb & 15u); word(clean(v.y), (sb >> 4) & 15u); word(clean(v.z), (sb >> 8) & 15u); word(clean(v.w), sb >> 12);
                } else {
                    word(v.x, sb & 15u); word(v.y, (sb >> 4) & 15u); word(v.z, (sb >> 8) & 15u); word(v.w, sb >> 12);
                }
                if (res.bits >> 15) res.flush();
                slot++;
            });
            if ((r & 3) == 3) res.flush();
            if (r + 1 < rounds) { buf.load(src + (size_t)(r + 1) * kSlots); eb = esrc[(size_t)(r + 1) * 64]; }
        }
        pos += (size_t)rounds * kRound;
        // tail of the buffer inside my stripe (only the last stripe has one): whole pairs, then an odd last byte paired with a
        // virtual END.  The batch's last byte is its last item's separator: marked, so the odd byte reports two ends of which only
        // the first exists.
        for (; pos + 2 <= my_end; pos += 2) {
            uint32_t lines, verdicts;
            eng.step2(st, code_at(pos), code_at(pos + 1), lines, verdicts);
            res.bits = (res.bits << lines) | verdicts;
            if (res.bits >> 29) res.flush();
        }
        bool closed_by_end_of_data = false;
        if (pos < my_end) {
            const uint32_t c = code_at(pos);
            uint32_t lines, verdicts;
            eng.step2(st, c, 128u, lines, verdicts);
            if (c == 128u) res.push(1, verdicts >> 1);
            else { res.push(1, verdicts); closed_by_end_of_data = true; }       // (cannot happen: see above)
            pos++;
        }
        res.flush();
        // the item that straddles my stripe end is mine if it started here: follow it to its end, pair by pair (stripes are even-sized)
        const bool started = fresh || res.seen > 0;
        if (!closed_by_end_of_data && started && !end_bit(my_end - 1)) {
            uint32_t lines = 0, verdicts = 0;
            while (pos + 16 <= nbytes && !lines) {
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
                const uint32_t e16 = (ends[ends_slot(pos >> 5, swl)] >> (pos & 31)) & 0xffffu;
                const uint32_t w[4] = {clean(v.x), clean(v.y), clean(v.z), clean(v.w)};
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (!lines) {
                        const uint32_t c1 = (e16 >> (2 * k)) & 1u ? 128u : (w[k >> 1] >> (16 * (k & 1))) & 0xffu;
                        const uint32_t c2 = (e16 >> (2 * k + 1)) & 1u ? 128u : (w[k >> 1] >> (16 * (k & 1) + 8)) & 0xffu;
                        eng.step2(st, c1, c2, lines, verdicts);
                    }
                }
                pos += 16;
            }
            for (; pos + 2 <= nbytes && !lines; pos += 2) eng.step2(st, code_at(pos), code_at(pos + 1), lines, verdicts);
            if (!lines) eng.step2(st, pos < nbytes ? code_at(pos) : 128u, 128u, lines, verdicts);
            res.push(1, lines == 2 ? verdicts >> 1 : verdicts);               // only the first end of the pair is mine
        }
        res.finish();
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) {
        const uint32_t v = stage[i];
        if (v) atomicOr(&accept_bits[window_word + i], v);
    }
}
// The index of a batch of items from its offsets, in ONE pass over them (round 3; round 2: a memset of the bitmap, a kernel for
// the item ends with atomics on the words two workgroups share, and a binary search per stripe):
//  * ends: bitmap of the item ends (positions relative to off[0]); *flag |= 1 if an item has no byte to carry its mark.  The
//    ends are sorted: the 1024 items of a workgroup mark a contiguous range of bitmap words, and the workgroup OWNS the words
//    [word of its first mark, word of the next workgroup's first mark) - it leaves its own last marks that fall into the next
//    owner's first word to that owner, and picks up the marks the items in front of its own left in its first word (at most 32:
//    every item has a byte of its own).  The range is assembled in LDS, tile by tile, and written out whole with plain stores,
//    zero words included: every word of the bitmap is written exactly once, nothing is cleared beforehand, nothing is atomic.
//    (One atomic per item: 0.12 ms for 22 M items of 95 bytes, 1.0 ms for 55 M of 19; one 4-byte store per marked word:
//    0.34 / 0.83 ms - scattered partial writes into 128 MB.)
//  * stripe_base[g] = items that end before stripe g | kFreshStripe if the byte in front of it is marked; entry nstripes = all.
//    The item that holds a stripe's first byte knows its own number: it writes the entry (no search, no scan); the stripes behind
//    the batch's last byte (the index is laid out for an upper bound of its extent) are filled in by everybody.
constexpr uint32_t kEndsTile = 4096, kEndsPerLane = 4, kEndsItems = 256 * kEndsPerLane;      // items per workgroup
__global__ __launch_bounds__(256) void item_index_kernel(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim, uint32_t *__restrict__ ends,
                                                         uint32_t *__restrict__ flag, uint64_t limit_words, const uint8_t *__restrict__ bytes_base,
                                                         uint64_t min_bytes, uint32_t stripe_log2, size_t nstripes, uint64_t *__restrict__ stripe_base) {
    __shared__ uint32_t tile[kEndsTile];
    const uint64_t base = off[0], extent = off[nitems] > base ? off[nitems] - base : 0;
    // one-call form: the batch's extent is only known here.  Unfit (flag bit 1) if it is shorter than the stripe-wise path
    // pays for, longer than the bitmap was sized for, or does not start on a 16-byte boundary.
    if (bytes_base && blockIdx.x == 0 && threadIdx.x == 0) {
        if (!extent || extent < min_bytes || ((extent + 31) >> 5) > limit_words || (reinterpret_cast<uintptr_t>(bytes_base + base) & 15)) atomicOr(flag, 2u);
    }
    const size_t i0 = (size_t)blockIdx.x * kEndsItems;
    const size_t i1 = i0 + kEndsItems < nitems ? i0 + kEndsItems : nitems;     // first item of the next workgroup (nitems: none)
    auto mark_of = [&](size_t k) -> uint64_t {                      // position of item k's mark (a degenerate item: of its start)
        const uint64_t e = off[k + 1];
        return (e > base ? e - 1 : base) - base;
    };
    uint64_t word[kEndsPerLane];
    uint32_t mask[kEndsPerLane];
    uint64_t ob[kEndsPerLane], oe[kEndsPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kEndsPerLane; k++) {                   // (all loads first: four round trips in flight)
        const size_t i = i0 + (size_t)k * 256 + threadIdx.x;
        ob[k] = i < nitems ? off[i] : 0;
        oe[k] = i < nitems ? off[i + 1] : 0;
    }
    bool degenerate = false;
    const uint64_t stripe_mask = ((uint64_t)1 << stripe_log2) - 1;
#pragma unroll
    for (uint32_t k = 0; k < kEndsPerLane; k++) {
        const size_t i = i0 + (size_t)k * 256 + threadIdx.x;
        word[k] = ~0ull; mask[k] = 0;
        if (i < nitems) {
            if (oe[k] <= ob[k] || oe[k] - ob[k] < trim) degenerate = true;     // trim 1: at least the separator; trim 0: at least one byte
            else { const uint64_t pos = oe[k] - 1 - base; word[k] = pos >> 5; mask[k] = 1u << (pos & 31); }
            if (oe[k] > ob[k] && ob[k] >= base) {                   // the stripes whose first byte is one of mine
                const uint64_t s0 = ob[k] - base, e0 = oe[k] - base;
                uint64_t g = (s0 + stripe_mask) >> stripe_log2;
                const uint64_t g1 = (e0 + stripe_mask) >> stripe_log2;
                for (; g < g1 && g < nstripes; g++)
                    stripe_base[g] = (uint64_t)i | ((g == 0 || (g << stripe_log2) == s0) ? kFreshStripe : 0);
            }
        }
    }
    if (degenerate) atomicOr(flag, 1u);
    {   // stripes that begin at or behind the batch's last byte, and the closing entry
        const uint64_t gend = (extent + stripe_mask) >> stripe_log2;
        for (uint64_t g = gend + (uint64_t)blockIdx.x * 256 + threadIdx.x; g <= nstripes; g += (uint64_t)gridDim.x * 256)
            stripe_base[g] = (uint64_t)nitems | ((g < nstripes && (g == 0 || (g << stripe_log2) == extent)) ? kFreshStripe : 0);
    }
    const uint64_t F = blockIdx.x == 0 ? 0 : mark_of(i0) >> 5;      // my words: [F, X)
    uint64_t X = i1 < nitems ? mark_of(i1) >> 5 : ((extent + 31) >> 5) + 4;
    if (X > limit_words) X = limit_words;
    for (uint64_t T = F; T < X; T += kEndsTile) {
        const uint64_t n = X - T < kEndsTile ? X - T : kEndsTile;   // words of this tile
        for (uint32_t j = threadIdx.x; j < n; j += 256) tile[j] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kEndsPerLane; k++)
            if (word[k] >= T && word[k] < T + n) atomicOr(&tile[(uint32_t)(word[k] - T)], mask[k]);
        if (T == F && threadIdx.x < 32 && i0 >= 1 + (size_t)threadIdx.x) {      // what the items in front of mine left in my first word
            const size_t ip = i0 - 1 - threadIdx.x;
            const uint64_t b = off[ip], e = off[ip + 1];
            if (e > b && e - b >= trim && e > base && ((e - 1 - base) >> 5) == F) atomicOr(&tile[0], 1u << ((e - 1 - base) & 31));
        }
        __syncthreads();
        {   // write-out in the order of the TRANSPOSED layout (ends_slot): the words of the tile's stripes round by round, so that
            // consecutive lanes write consecutive 16-byte pieces (in the tile's own order every piece lands a KiB from the last:
            // 111 us instead of 71 for the index of a GiB)
            const uint32_t swl = stripe_log2 - 5u, sw = 1u << swl;
            const uint64_t gA = T >> swl;
            const uint32_t nst = (uint32_t)(((T + n - 1) >> swl) - gA) + 1u;
            const uint32_t total = nst << swl;
            for (uint32_t idx = threadIdx.x; idx < total; idx += 256) {
                const uint32_t q = idx >> 2, r = q / nst, s_ = q - r * nst;
                const uint64_t src = ((gA + s_) << swl) + 4u * r + (idx & 3u);
                if (src >= T && src < T + n) ends[ends_slot(src, swl)] = tile[(uint32_t)(src - T)];
            }
            (void)sw;
        }
        __syncthreads();
    }
}

}  // namespace

// The index of a batch of items (kept by an rrx_items handle, or built in scratch by rrx_match_extents):
//   [ends bitmap, 1 bit per byte | flag u32 (an item without a byte for its mark) | stripe base u64 (nstripes + 1)]
// and, per match, a result bitmap of nitems bits.
static size_t items_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t items_ends_bytes(size_t nbytes, uint32_t stripe) {           // whole groups of 64 stripes (ends_slot permutes inside a group)
    const size_t group_words = 2 * (size_t)stripe, words = (nbytes + 31) / 32 + 4;
    return (words + group_words - 1) / group_words * group_words * 4;
}
// the stripe an items batch wants: by its size and its mean item length, like a corpus (stripe_for_lines)
static uint32_t items_stripe(size_t nbytes, size_t nitems) { return stripe_for_lines(nbytes, nitems ? nbytes / nitems : nbytes); }
size_t items_index_bytes(size_t nbytes, size_t nitems) {
    const size_t nstripes = (nbytes + items_stripe(nbytes, nitems) - 1) / items_stripe(nbytes, nitems);
    return items_ends_bytes(nbytes, items_stripe(nbytes, nitems)) + 256 + items_align((nstripes + 1) * 8);
}
size_t items_result_bytes(size_t nitems) { return items_align(((nitems + 31) / 32 + 4) * 4); }
// trim 0 or 1; the buffer starts at off[0] and holds nbytes = off[nitems] - off[0] bytes.  -> *flag: device u32 inside the
// index, != 0 after the stream is done if some item has no byte for its mark (then the index is not usable).
int items_index_build(size_t nbytes, const uint64_t *off, size_t nitems, uint32_t trim, void *index, uint32_t **flag, void *stream,
                      const uint8_t *resolve_base, size_t min_bytes) {
    if (trim > 1 || !nitems || !nbytes) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t stripe = items_stripe(nbytes, nitems);
    const size_t nstripes = (nbytes + stripe - 1) / stripe;
    uint32_t *ends = static_cast<uint32_t *>(index);
    uint32_t *fl = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(index) + items_ends_bytes(nbytes, stripe));
    uint64_t *base = reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(fl) + 256);
    *flag = fl;
    if (stripe & (stripe - 1)) return (int)hipErrorInvalidValue;      // (stripes are powers of two)
    hipError_t e = hipMemsetAsync(fl, 0, 256, st);                    // the flag; the bitmap is written whole by the kernel
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(item_index_kernel, dim3((unsigned)((nitems + kEndsItems - 1) / kEndsItems)), dim3(256), 0, st, off, nitems, trim, ends, fl,
                       (uint64_t)(items_ends_bytes(nbytes, stripe) / 4), resolve_base, (uint64_t)min_bytes, (uint32_t)__builtin_ctz(stripe), nstripes, base);
    return (int)hipGetLastError();
}
// The stripe-wise kernels into `result` = items_result_bytes(nitems) of scratch: a bitmap of the items' verdicts, padded, bit nitems
// possibly set by the batch's closing end.  resolve_off != nullptr: the one-call form - `bytes` is the buffer the offsets index,
// `nbytes` the upper bound the index was laid out for, the kernel takes the batch's start and length from the offsets and does
// nothing if *skip_if != 0 (the bitmap stays zero).
static int items_run2(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, size_t nitems, const void *index, void *result, void *stream,
                      const uint64_t *resolve_off, const uint32_t *skip_if) {
    if (!p.P || !p.T2 || Dfa2::lds_bytes(p) > kDfa2MaxTable || !nitems || !nbytes) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t stripe = items_stripe(nbytes, nitems);
    const size_t nstripes = (nbytes + stripe - 1) / stripe;
    const uint32_t *ends = static_cast<const uint32_t *>(index);
    const uint64_t *base = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(index) + items_ends_bytes(nbytes, stripe) + 256);
    uint32_t *bits = static_cast<uint32_t *>(result);
    hipError_t e = hipMemsetAsync(bits, 0, ((nitems + 31) / 32 + 4) * 4, st);
    if (e != hipSuccess) return (int)e;
    const size_t blocks = (nstripes + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(match_items_stripes2_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, p, bytes, nbytes, stripe, base, ends, bits, resolve_off, nitems, skip_if);
    return (int)hipGetLastError();
}
static int items_run(const LineDfaDevice &p, const uint8_t *bytes, size_t nbytes, size_t nitems, uint32_t trim, const void *index, void *result,
                     void *stream, const uint64_t *resolve_off, const uint32_t *skip_if) {
    if (!p.wide || p.in_global || p.stride != (kItemColumns << p.rep_log2) || trim > 1 || !nitems || !nbytes) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t stripe = items_stripe(nbytes, nitems);
    const size_t nstripes = (nbytes + stripe - 1) / stripe;
    const uint32_t *ends = static_cast<const uint32_t *>(index);
    const uint64_t *base = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(index) + items_ends_bytes(nbytes, stripe) + 256);
    uint32_t *bits = static_cast<uint32_t *>(result);
    hipError_t e = hipMemsetAsync(bits, 0, ((nitems + 31) / 32 + 4) * 4, st);
    if (e != hipSuccess) return (int)e;
    const size_t table_bytes = LineDfaEngine<true, false>::lds_bytes(p);
    const uint32_t stage_off = (uint32_t)((table_bytes + 15) & ~(size_t)15);
    const size_t half_cu = 80 * 1024;
    const uint32_t stage_words = stage_off + kStageWords * sizeof(uint32_t) >= half_cu ? kStageWords : (uint32_t)((half_cu - stage_off) / 4);
    const size_t lds = stage_off + (size_t)stage_words * sizeof(uint32_t);
    const size_t blocks = (nstripes + kThreads - 1) / kThreads;
    if (trim == 1) {
        static LdsAttr attr;
        e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(match_items_stripes_kernel<1>), lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(match_items_stripes_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), lds, st, p, bytes, nbytes, stripe, base, ends, bits, stage_off, stage_words,
                           resolve_off, nitems, skip_if);
    } else {
        static LdsAttr attr;
        e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(match_items_stripes_kernel<2>), lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(match_items_stripes_kernel<2>, dim3((unsigned)blocks), dim3(kThreads), lds, st, p, bytes, nbytes, stripe, base, ends, bits, stage_off, stage_words,
                           resolve_off, nitems, skip_if);
    }
    return (int)hipGetLastError();
}
// ... and the verdicts out of `result` to where the caller wants them (device.hpp: ItemVerdicts)
static int items_deliver(const void *result, size_t nitems, ItemVerdicts out, void *stream) {
    const uint32_t *bits = static_cast<const uint32_t *>(result);
    return out.bits ? copy_result_bits(bits, nitems, out.bits, stream) : expand_bits(bits, nitems, out.bytes, stream);
}
int items_match2(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, size_t nitems, const void *index, void *result, ItemVerdicts out, void *stream,
                 const uint64_t *resolve_off, const uint32_t *skip_if) {
    const int rc = items_run2(p, bytes, nbytes, nitems, index, result, stream, resolve_off, skip_if);
    return rc ? rc : items_deliver(result, nitems, out, stream);
}
int items_match(const LineDfaDevice &p, const uint8_t *bytes, size_t nbytes, size_t nitems, uint32_t trim, const void *index, void *result,
                ItemVerdicts out, void *stream, const uint64_t *resolve_off, const uint32_t *skip_if) {
    const int rc = items_run(p, bytes, nbytes, nitems, trim, index, result, stream, resolve_off, skip_if);
    return rc ? rc : items_deliver(result, nitems, out, stream);
}

}  // namespace dev
}  // namespace rrx
