// kernels_table.hip — the batch match path of the table engines: the stride-2 stripe kernels, the launchers of the byte-stride
// ones, the stream compaction of the one-shot entry and the two-bit split of the sampled-table engine.  Engines:
// table_engines.hpp; shared device code: kernels_common.hpp.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// Same stripe geometry, feed and result path as match_stripes_kernel; pairs are aligned to even byte positions
// (stripes are even-sized), a line end may fall on either byte of a pair.
// ONEPASS (rrx_match_device): no line index yet.  Every lane starts in the start state (a lane that begins inside a line
// produces a verdict for the fragment, which the compaction drops), counts its '\n' on the side, and keeps its verdict
// stream in the workgroup's slab (LocalResults).  Bytes >= 0x80 cannot index the pair table: a text word that holds one is
// rewritten with 0x00 in their place (which rejects the line just the same) under a wave-uniform branch.
// `phase` is an instrumentation hook: the shipping kernels pass NoPhaseHook (nothing is emitted); tools/probe/stamps builds
// a kernel around this body whose hook writes a timestamp per workgroup and phase (where a launch's fixed cost goes).
struct NoPhaseHook { __device__ __forceinline__ void operator()(int) const {} __device__ __forceinline__ void round(int) const {} };
enum { kPhaseEntry = 0, kPhaseTablesLoaded, kPhaseFirstRound, kPhaseMainDone, kPhaseFollowDone, kPhaseWindowOut, kPhases };
// A round's text as ONE burst of eight loads (they merge into one request per 128-byte line).  The address is kept alive past
// the burst by an empty asm statement: where it dies with the last load, the register allocator may put it into that load's
// destination - a wait state inside the burst, whose loads then no longer merge (the unit kernel of round 4: -13 %).
__device__ __forceinline__ void feed_load(uint4 (&buf)[kRound / 16], const uint4 *p) {
#pragma unroll
    for (int i = 0; i < kRound / 16; i++) buf[i] = load_text(p + i);
    asm volatile("" : : "v"(p));
}
// One stripe of one lane: lane-local state only (what the caller keeps across stripes is the engine, the window and `g`).
// KB: result bits per line - 1 (accepted), or 2 (accepted, ESCAPED: the sampled-table engine, whose table does not know every
// transition; the table's line ends then shift two bits in, and everything that counts results counts bits).
// CLEAN: the text may hold bytes >= 0x80 (the one-pass entry, which has no index that could tell; rrx_contains_corpus on a corpus
// that holds some).  They are stepped as 0x00 - the same byte class on every table - under the wave-uniform test below.
// FLUSH_SLOTS: the common flush period in 16-byte slots.  A power of two: known at compile time - the test folds per unrolled slot,
// and from a whole round on (32: `(r & 3) == 3`) it is one test per round; 0: the period is `flush_mask + 1`, decided per launch.
// Engine: Dfa2, or Dfa2T<true> on the byte-wide pair table.
template <bool ONEPASS, class PhaseHook, int FLUSH_SLOTS, int KB = 1, bool CLEAN = ONEPASS, class Engine = Dfa2>
__device__ __forceinline__ void dfa2_stripe(const Engine &eng, const size_t g, const uint64_t window_word, uint32_t *const stage, const uint32_t stage_words,
                                            const uint8_t *__restrict__ bytes, const size_t nbytes, const uint32_t stripe,
                                            const uint64_t *__restrict__ stripe_base, uint32_t *__restrict__ accept_bits,
                                            uint32_t *__restrict__ counts, uint32_t *__restrict__ slabs, const uint32_t slab_row, PhaseHook &phase,
                                            const uint32_t flush_mask) {
    static_assert(FLUSH_SLOTS >= 0 && (FLUSH_SLOTS & (FLUSH_SLOTS - 1)) == 0, "0 or a power of two");
    const size_t start = g * (size_t)stripe;
    if (start < nbytes) {                                            // (no early return: the write-out below is collective)
    const size_t stripe_end = start + stripe;
    const size_t my_end = stripe_end < nbytes ? stripe_end : nbytes;
    bool fresh = true;
    typename std::conditional<ONEPASS, LocalResults, ResultsT<true>>::type res;
    if constexpr (ONEPASS) {
        res.begin(slabs + g, slab_row);
    } else {
        const uint64_t my_base = stripe_base[g];
        fresh = (my_base & kFreshStripe) != 0;
        res.begin_staged(line_of(my_base) * KB, window_word, !fresh, accept_bits, stage);
        res.stage_words = stage_words;
        res.drop_mask = (1u << KB) - 1u;
    }
    typename Engine::State st = fresh ? eng.fresh() : eng.skipping();
    auto clean = [](uint32_t w) -> uint32_t {                       // CLEAN: bytes >= 0x80 -> 0x00
        if (CLEAN && __builtin_amdgcn_ballot_w64((w & 0x80808080u) != 0)) {
            const uint32_t hi = (w & 0x80808080u) >> 7;             // 1 in every byte to clear
            w &= ~(hi * 0xffu);
        }
        return w;
    };

    size_t pos = start;
    const uint4 *src = reinterpret_cast<const uint4 *>(bytes + start);
    constexpr int kSlots = kRound / 16;
    const int rounds = (int)((my_end - start) / kRound);
    uint4 buf[kSlots];
    if (rounds > 0) feed_load(buf, src);
    // The line that straddles my stripe end is followed into the next stripe's text (below).  Its first 128 bytes are
    // requested while the last round is still being stepped: loaded on demand, 16 bytes at a time, they were a chain of
    // L2 round trips at the end of every wave's life, and the waves of a workgroup - of the whole chip, launched together
    // and fed at the same rate - reach that point at the same time.
    uint32_t last_word = 0;                                       // the last text word of my stripe (whole rounds only)
    bool ahead = false;                                           // buf holds the 128 bytes behind my stripe
    for (int r = 0; r < rounds; r++) {
        if (r == 1) phase(kPhaseFirstRound);
        phase.round(r);
#pragma unroll
        for (int i = 0; i < kSlots; i++) {
            if (CLEAN && __builtin_expect(__builtin_amdgcn_ballot_w64(((buf[i].x | buf[i].y | buf[i].z | buf[i].w) & 0x80808080u) != 0) != 0, 0)) {
                // some lane of the wave holds a byte >= 0x80 in this slot (one test per 16 bytes; rare on text)
                eng.consume_dword(st, clean(buf[i].x), res.bits);
                eng.consume_dword(st, clean(buf[i].y), res.bits);
                eng.consume_dword(st, clean(buf[i].z), res.bits);
                eng.consume_dword(st, clean(buf[i].w), res.bits);
            } else {
                eng.consume_dword(st, buf[i].x, res.bits);
                eng.consume_dword(st, buf[i].y, res.bits);
                if (KB == 2 && (res.bits >> 15)) res.flush();    // (two bits per line end: eight bytes can bring sixteen)
                eng.consume_dword(st, buf[i].z, res.bits);
                eng.consume_dword(st, buf[i].w, res.bits);
            }
            // All lanes flush TOGETHER every FLUSH_SLOTS (0: flush_mask + 1) slots - a period the host picks from the corpus' mean
            // line length so that about eight results gather in it (short lines: every other slot; 512 bytes for long ones).  The
            // overflow check behind it is for the lanes that meet far more: left to it alone, lanes overflow at different times and
            // the wave walks the flush path at nearly every slot (5-byte lines: +1.25 VALU per byte).
            bool together;
            if constexpr (FLUSH_SLOTS == 0) together = (((uint32_t)r * kSlots + (uint32_t)i) & flush_mask) == flush_mask;
            else if constexpr (FLUSH_SLOTS >= kSlots) together = i == kSlots - 1 && (r & (FLUSH_SLOTS / kSlots - 1)) == FLUSH_SLOTS / kSlots - 1;
            else together = (i & (FLUSH_SLOTS - 1)) == FLUSH_SLOTS - 1;
            if (together) res.flush();
            else if (res.bits >> 15) res.flush();            // <= 16 more results fit before the next check
        }
        if (r + 1 < rounds) {
            feed_load(buf, src + (r + 1) * kSlots);
        } else {
            last_word = buf[kSlots - 1].w;
            if (start + (size_t)(rounds + 1) * kRound <= nbytes) {
                feed_load(buf, src + (r + 1) * kSlots);
                ahead = true;
            }
        }
    }
    pos += (size_t)rounds * kRound;
    phase(kPhaseMainDone);
    auto byte_at = [&](size_t q) -> uint32_t { const uint32_t b = bytes[q]; return (CLEAN && b >= 0x80u) ? 0u : b; };

    // ---- tail of the corpus inside my stripe (only the last stripe has one): whole pairs, then an odd last byte.
    // The odd byte is paired with a virtual '\n': if it is a '\n' itself the pair reports two line ends, of which
    // only the first exists; otherwise the virtual '\n' is the end of data ending the last line, and the walk
    // below must not end it again.
    bool closed_by_end_of_data = false;
    for (; pos + 2 <= my_end; pos += 2) {
        uint32_t lines, verdicts;
        eng.step2(st, byte_at(pos), byte_at(pos + 1), lines, verdicts);
        res.bits = (res.bits << lines) | verdicts;
        if (res.bits >> (31 - 2 * KB)) res.flush();
    }
    if (pos < my_end) {
        const uint32_t b = byte_at(pos);
        uint32_t lines, verdicts;
        eng.step2(st, b, '\n', lines, verdicts);
        if (b == '\n') res.push(KB, verdicts >> KB);
        else { res.push(KB, verdicts); closed_by_end_of_data = true; }
        pos++;
    }
    res.flush();
    const uint32_t newlines = res.seen - (closed_by_end_of_data ? 1u : 0u);      // real '\n' inside my stripe

    // ---- follow my last line past the stripe end (same ownership rule as the byte kernel), pair by pair
    if (ONEPASS && res.seen == 0) fresh = g == 0 || bytes[start - 1] == '\n';   // a stripe without any '\n': whose line is it?
    const bool started = fresh || res.seen > 0;
    bool followed = false;
    const bool whole_rounds = rounds > 0 && start + (size_t)rounds * kRound == my_end;
    const uint32_t last_byte = whole_rounds ? last_word >> 24 : (uint32_t)bytes[my_end - 1];
    if (!closed_by_end_of_data && started && last_byte != '\n') {
        uint32_t lines = 0, verdicts = 0;
        if (ahead && pos == start + (size_t)(rounds + 1) * kRound - kRound) {      // (pos == my_end: the requested bytes are the next ones)
    #pragma unroll
            for (int i = 0; i < kSlots; i++) {
                if (!lines) {
                    const uint32_t w[4] = {clean(buf[i].x), clean(buf[i].y), clean(buf[i].z), clean(buf[i].w)};
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (!lines) eng.step2(st, (w[k >> 1] >> (16 * (k & 1))) & 0xffu, (w[k >> 1] >> (16 * (k & 1) + 8)) & 0xffu, lines, verdicts);
                    pos += 16;
                }
            }
        }
        while (pos + 16 <= nbytes && !lines) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
            const uint32_t w[4] = {clean(v.x), clean(v.y), clean(v.z), clean(v.w)};
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (!lines) eng.step2(st, (w[k >> 1] >> (16 * (k & 1))) & 0xffu, (w[k >> 1] >> (16 * (k & 1) + 8)) & 0xffu, lines, verdicts);
            pos += 16;
        }
        for (; pos + 2 <= nbytes && !lines; pos += 2) eng.step2(st, byte_at(pos), byte_at(pos + 1), lines, verdicts);
        if (!lines) eng.step2(st, pos < nbytes ? byte_at(pos) : '\n', '\n', lines, verdicts);   // end of data ends the line
        res.push(KB, lines == 2 * KB ? verdicts >> KB : verdicts);     // only the first line end of the pair is mine
        followed = true;
    }
    res.finish();
    phase(kPhaseFollowDone);
    if (ONEPASS)
        counts[g] = newlines | ((followed || closed_by_end_of_data) ? kExtraResult : 0u) | (last_byte == '\n' ? kEndsOnNewline : 0u);
    }
}

// A bitmap word that two neighbouring workgroups share, settled without a cleared bitmap: both exchange their bits into the
// boundary's 64-bit slot (zero between launches).  Whoever finds it empty has left its bits there and is done; the other one
// finds them, stores the whole word and empties the slot again.  Nobody waits for anybody.
__device__ __forceinline__ void settle_shared_word(unsigned long long *slot, uint32_t *word, uint32_t mine) {
    const unsigned long long old = atomicExch(slot, (1ull << 63) | mine);
    if (old) {
        *word = (uint32_t)old | mine;
        *slot = 0;
    }
}
// OWN_WORDS (one result bit per line, indexed): the bitmap need not be cleared before the launch.  The workgroup's lines lie
// in the words [window_word, next workgroup's first word]; the words strictly between are its own and leave the window as
// plain stores, zeros included; the two at the ends go through the exchange slots (`slots[b]`: the boundary in front of
// workgroup b).  The first workgroup owns its first word, the last one every word up to `nwords`, the size of the bitmap.
// The host launches this form only where the first words of the workgroups are strictly increasing - no word with three
// writers - and every workgroup's range fits the window (rrx_corpus_one_launch; abi.cpp: own_words_for).
// PAIRS8: the engine on the byte-wide pair table (prog.P8; the host picks these kernels exactly where the image holds one); P's
// static array shrinks from 32.5 KiB to 17 KiB, the region T2 and the window share stays what it is.
template <bool ONEPASS, int FLUSH_SLOTS, class PhaseHook = NoPhaseHook, int KB = 1, bool CLEAN = ONEPASS, bool OWN_WORDS = false, bool PAIRS8 = false>
__device__ __forceinline__ void dfa2_body(const Dfa2Device &prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                          const uint64_t *__restrict__ stripe_base, uint32_t *__restrict__ accept_bits,
                                          uint32_t *__restrict__ counts, uint32_t *__restrict__ slabs, PhaseHook phase = PhaseHook(),
                                          uint32_t flush_mask = 31u, unsigned long long *__restrict__ slots = nullptr, uint64_t nwords = 0) {
    static_assert(!OWN_WORDS || (!ONEPASS && KB == 1), "the exchange slots serve the indexed kernels with one bit per line");
    phase(kPhaseEntry);
    // T2 first: its entries hold 16-bit LDS addresses; the result window takes what T2 leaves of its region (16 KiB and
    // more for tables up to 30 KiB, 4 KiB at least).  The arrays are static, so P's base is a link-time constant.
    __shared__ __attribute__((aligned(16))) struct {
        uint8_t t2_and_stage[kDfa2RegionBytes];
        uint8_t p[Dfa2T<PAIRS8>::kPBytes];
    } lds;
    Dfa2T<PAIRS8> eng;
    eng.load(prog, lds.p, lds.t2_and_stage);
    const uint32_t stage_off = (uint32_t)((Dfa2::lds_bytes(prog) + 15) & ~(size_t)15);
    uint32_t *const stage = reinterpret_cast<uint32_t *>(lds.t2_and_stage + stage_off);
    const uint32_t stage_words = (kDfa2RegionBytes - stage_off) / 4;
    if (!ONEPASS)
        for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) stage[i] = 0;
    __syncthreads();
    phase(kPhaseTablesLoaded);

    const size_t g0 = (size_t)blockIdx.x * kThreads;
    uint64_t window_word = 0;
    if (!ONEPASS) window_word = (line_of(stripe_base[g0]) * KB) >> 5;       // the workgroup's first stripe exists: uniform load
    dfa2_stripe<ONEPASS, PhaseHook, FLUSH_SLOTS, KB, CLEAN, Dfa2T<PAIRS8>>(eng, g0 + threadIdx.x, window_word, stage, stage_words, bytes, nbytes, stripe, stripe_base, accept_bits,
                                                            counts, slabs, gridDim.x * kThreads, phase, flush_mask);
    if constexpr (OWN_WORDS) {
        __syncthreads();
        const bool last = blockIdx.x + 1 == gridDim.x;
        const uint64_t next_word = last ? nwords : line_of(stripe_base[g0 + kThreads]) >> 5;      // (stripe_base has an entry behind the last stripe)
        uint64_t span = next_word - window_word;                     // >= 1; the host has seen to it that the range fits the window
        if (span > stage_words) span = stage_words;                  // (never: and then no store would leave the bitmap either)
        for (uint32_t i = threadIdx.x + 1; i < (uint32_t)span; i += kThreads) accept_bits[window_word + i] = stage[i];
        if (threadIdx.x == 0) {
            if (blockIdx.x == 0) accept_bits[window_word] = stage[0];
            else settle_shared_word(&slots[blockIdx.x], &accept_bits[window_word], stage[0]);
        }
        if (threadIdx.x == 64 && !last && span < stage_words) settle_shared_word(&slots[blockIdx.x + 1], &accept_bits[next_word], stage[(uint32_t)span]);
    } else if (!ONEPASS) {
        // ---- write the window out: consecutive lanes, consecutive words (the atomics merge into whole lines in L2;
        // the first and the last word of the window are shared with the neighbouring workgroups)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < stage_words; i += kThreads) {
            const uint32_t v = stage[i];
            if (v) atomicOr(&accept_bits[window_word + i], v);
        }
    }
    phase(kPhaseWindowOut);
}
// (the unit hand-out inside the workgroup, round 4's option, never won and is gone: profiles/r04_unit_handout_ab.txt)
template <int FLUSH_SLOTS, bool OWN_WORDS, bool PAIRS8>
__global__ __launch_bounds__(kThreads) void match_stripes2_kernel(Dfa2Device prog, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                   uint32_t stripe, const uint64_t *__restrict__ stripe_base,
                                                                   uint32_t *__restrict__ accept_bits, uint32_t flush_mask,
                                                                   unsigned long long *__restrict__ slots, uint64_t nwords) {
    dfa2_body<false, FLUSH_SLOTS, NoPhaseHook, 1, false, OWN_WORDS, PAIRS8>(prog, bytes, nbytes, stripe, stripe_base, accept_bits, nullptr, nullptr, NoPhaseHook(), flush_mask,
                                                                    slots, nwords);
}
// the same over text that may hold bytes >= 0x80, stepped as 0x00 (rrx_contains_corpus: such bytes are ordinary text there, of the
// class of NUL, and UTF-8 text stays on the two-bytes-per-lookup kernel)
template <int FLUSH_SLOTS, bool OWN_WORDS, bool PAIRS8>
__global__ __launch_bounds__(kThreads) void match_stripes2_clean_kernel(
    Dfa2Device prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe, const uint64_t *__restrict__ stripe_base,
    uint32_t *__restrict__ accept_bits, uint32_t flush_mask, unsigned long long *__restrict__ slots, uint64_t nwords) {
    dfa2_body<false, FLUSH_SLOTS, NoPhaseHook, 1, true, OWN_WORDS, PAIRS8>(prog, bytes, nbytes, stripe, stripe_base, accept_bits, nullptr, nullptr, NoPhaseHook(), flush_mask,
                                                                   slots, nwords);
}
// two result bits per line (accepted, escaped) into a bitmap of twice the size: the sampled-table engine's first pass
__global__ __launch_bounds__(kThreads) void match_stripes2_two_bit_kernel(Dfa2Device prog, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                           uint32_t stripe, const uint64_t *__restrict__ stripe_base,
                                                                           uint32_t *__restrict__ wide_bits) {
    dfa2_body<false, 32, NoPhaseHook, 2>(prog, bytes, nbytes, stripe, stripe_base, wide_bits, nullptr, nullptr);
}
__global__ __launch_bounds__(kThreads) void match_stripes2_onepass_kernel(Dfa2Device prog, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                           uint32_t stripe, uint32_t *__restrict__ counts,
                                                                           uint32_t *__restrict__ slabs) {
    dfa2_body<true, 32>(prog, bytes, nbytes, stripe, nullptr, nullptr, counts, slabs);
}

// One-pass mode, last step: lane = stripe.  The stream of stripe g (counts[g] results, the first of them dropped if the
// stripe starts inside a line) goes to bits [base, base + n) of the accept bitmap, base = '\n' before the stripe.  The
// streams of a workgroup's 256 stripes cover one contiguous bit range: they are merged in an LDS window first and leave as
// whole words, consecutive lanes writing consecutive words (atomics only because the first and the last word are shared
// with the neighbouring workgroups; words beyond the window go to memory directly).
constexpr uint32_t kCompactWindowWords = 8192;
__global__ __launch_bounds__(256) void compact_streams_kernel(const uint32_t *__restrict__ counts, const uint64_t *__restrict__ stripe_base,
                                                               size_t nstripes, uint32_t stripe, const uint32_t *__restrict__ slabs,
                                                               uint32_t *__restrict__ accept_bits, size_t cap_words) {
    __shared__ uint32_t window[kCompactWindowWords];
    const size_t g0 = (size_t)blockIdx.x * 256;
    const size_t g1 = g0 + 256 < nstripes ? g0 + 256 : nstripes;
    const uint64_t window_word = line_of(stripe_base[g0]) >> 5;          // g0 < nstripes: the grid is sized that way
    // the words this workgroup's streams can reach: up to the line the next workgroup starts in, one more for the
    // extra result of the last stripe (stripe_base has nstripes + 1 entries); only those are cleared and written out
    const uint64_t span = (line_of(stripe_base[g1]) >> 5) - window_word + 2;
    const uint32_t used = span < kCompactWindowWords ? (uint32_t)span : kCompactWindowWords;
    for (uint32_t i = threadIdx.x; i < used; i += 256) window[i] = 0;
    __syncthreads();
    const size_t g = g0 + threadIdx.x;
    if (g < nstripes) {
        const uint32_t c = counts[g];
        const uint32_t n = (c & kCountMask) + ((c & kExtraResult) ? 1u : 0u);
        const uint64_t b = stripe_base[g];
        const uint64_t base = line_of(b);
        const bool fresh = (b & kFreshStripe) != 0;
        const size_t row = (nstripes + kThreads - 1) / kThreads * kThreads;     // slab[k][stripe], rows padded to whole workgroups
        const uint32_t *src = slabs + g;
        auto put = [&](uint64_t word, uint32_t v) {
            if (!v) return;
            if (word >= cap_words) return;                          // the caller's bitmap is too small: reported from the line count
            const uint64_t rel = word - window_word;
            if (rel < used) atomicOr(&window[(uint32_t)rel], v);
            else atomicOr(&accept_bits[word], v);
        };
        for (uint32_t k = 0; k * 32 < n; k++) {
            uint32_t v = src[(size_t)k * row];
            if (n - k * 32 < 32) v &= (1u << (n - k * 32)) - 1u;
            if (k == 0 && !fresh) v &= ~1u;                          // that line belongs to the lane before me
            const uint64_t bit = base + (uint64_t)k * 32;
            const uint32_t sh = (uint32_t)bit & 31u;
            put(bit >> 5, v << sh);
            if (sh) put((bit >> 5) + 1, v >> (32u - sh));
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < used; i += 256) {
        const uint32_t v = window[i];
        if (v && window_word + i < cap_words) atomicOr(&accept_bits[window_word + i], v);
    }
}

}  // namespace

int match_stripes_dfa(const LineDfaDevice &p, bool clamp_high, const uint8_t *bytes, size_t nbytes, uint32_t stripe,
                      const uint64_t *stripe_base, size_t nstripes, uint32_t *accept, void *stream) {
#define GO(WIDE, CLAMP) launch_stripes<LineDfaEngine<WIDE, CLAMP>, LineDfaDevice>(p, LineDfaEngine<WIDE, CLAMP>::lds_bytes(p), bytes, nbytes, stripe, stripe_base, nstripes, accept, stream)
    if (p.in_global) return launch_stripes<LineDfaGlobalEngine, LineDfaDevice>(p, 256, bytes, nbytes, stripe, stripe_base, nstripes, accept, stream);
    if (p.wide) return clamp_high ? GO(true, true) : GO(true, false);
    return GO(false, false);
#undef GO
}
// slots (16 bytes of a lane's text) between two flushes of ALL lanes, minus one: about sixteen line ends per period
uint32_t flush_mask_for(size_t nbytes, size_t nlines) {
    const size_t avg = nlines ? nbytes / nlines : nbytes;
    uint32_t slots = 1;
    while (slots < 32 && (size_t)slots * 2 * 16 <= avg * 16) slots *= 2;      // (measured: profiles/r04_flush_period_ab.txt)
    return slots - 1;
}
// The launch of every stride-2 stripe kernel: `kernel(p, bytes, nbytes, stripe, rest...)` on workgroups of kThreads lanes that take
// `stripes_per_wg` stripes each; a table beyond the kernels' LDS region is refused.
template <class... Params, class... Rest>
static int launch_dfa2(void (*kernel)(Params...), const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes,
                       size_t stripes_per_wg, void *stream, Rest... rest) {
    if (!nstripes) return 0;
    if (Dfa2::lds_bytes(p) > kDfa2MaxTable) return (int)hipErrorInvalidValue;
    const size_t blocks = (nstripes + stripes_per_wg - 1) / stripes_per_wg;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, p, bytes, nbytes, stripe, rest...);
    return (int)hipGetLastError();
}
uint32_t dfa2_window_words(const Dfa2Device &p) {
    const size_t stage_off = (Dfa2::lds_bytes(p) + 15) & ~(size_t)15;
    return stage_off < kDfa2RegionBytes ? (uint32_t)((kDfa2RegionBytes - stage_off) / 4) : 0u;
}
bool dfa2_flush_at_compile_time(uint32_t flush_mask) { return flush_mask == 31u; }
// The period the automatic choice gives text of 33 bytes per line and more - URL, kwlog, a{1,300}, both long-line workloads - is
// compiled in; every other one is a launch parameter.  `slots` != nullptr: the form that needs no cleared bitmap.  An image that
// holds the byte-wide pair table (p.P8: the host's decision, LineTables::byte_pairs) runs the kernels built on it.
template <bool PAIRS8>
static int launch_match_stripes2(const Dfa2Device &p, bool clean, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                                 size_t nstripes, uint32_t *accept, void *stream, uint32_t flush_mask, unsigned long long *slots, size_t nwords) {
    const bool fixed = dfa2_flush_at_compile_time(flush_mask);
#define GO(K) launch_dfa2(K, p, bytes, nbytes, stripe, nstripes, kThreads, stream, stripe_base, accept, flush_mask, slots, (uint64_t)nwords)
    if (clean) {
        if (slots) return fixed ? GO((match_stripes2_clean_kernel<32, true, PAIRS8>)) : GO((match_stripes2_clean_kernel<0, true, PAIRS8>));
        return fixed ? GO((match_stripes2_clean_kernel<32, false, PAIRS8>)) : GO((match_stripes2_clean_kernel<0, false, PAIRS8>));
    }
    if (slots) return fixed ? GO((match_stripes2_kernel<32, true, PAIRS8>)) : GO((match_stripes2_kernel<0, true, PAIRS8>));
    return fixed ? GO((match_stripes2_kernel<32, false, PAIRS8>)) : GO((match_stripes2_kernel<0, false, PAIRS8>));
#undef GO
}
int match_stripes_dfa2(const Dfa2Device &p, bool clean, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                       size_t nstripes, uint32_t *accept, void *stream, uint32_t flush_mask, unsigned long long *slots, size_t nwords) {
    return p.P8 ? launch_match_stripes2<true>(p, clean, bytes, nbytes, stripe, stripe_base, nstripes, accept, stream, flush_mask, slots, nwords)
                : launch_match_stripes2<false>(p, clean, bytes, nbytes, stripe, stripe_base, nstripes, accept, stream, flush_mask, slots, nwords);
}
// ---- the sampled-table engine's second step: the two-bit bitmap (bit 2i = line i accepted, bit 2i + 1 = line i ended in the
// ESCAPE state) taken apart into the accept bitmap - every word written, nothing to clear beforehand - and the bitmap of the
// escaped lines, which the exact engine then decides (recheck_escaped: kernels_nfa.inc); their number is added up on the side.
// `list` receives the numbers of the escaped lines (in no order; `cap` entries: what does not fit is counted all the same, and
// recheck_escaped then walks the stripes instead).  A workgroup collects its lines in LDS and reserves room in the list a
// thousand at a time: one atomic per escaped line - or per wave that met one - on the one counter cost a millisecond at
// 400 000 escaped lines.
__global__ __launch_bounds__(256) void split_two_bit_kernel(const uint32_t *__restrict__ wide, size_t words, uint32_t *__restrict__ accept_bits,
                                                             uint32_t *__restrict__ escaped_bits, unsigned long long *__restrict__ escaped_total,
                                                             uint64_t *__restrict__ list, size_t cap) {
    constexpr uint32_t kLocal = 4096, kFlushAt = kLocal - 256 * 8;      // (a turn adds at most 256 x 32 lines: see the two-step append below)
    __shared__ uint64_t local[kLocal];
    __shared__ uint32_t nlocal;
    __shared__ unsigned long long flush_base;
    if (threadIdx.x == 0) nlocal = 0;
    __syncthreads();
    auto even_bits = [](uint32_t x) -> uint32_t {                   // bits 0, 2, 4, ... packed into the low half
        x &= 0x55555555u;
        x = (x | x >> 1) & 0x33333333u;
        x = (x | x >> 2) & 0x0f0f0f0fu;
        x = (x | x >> 4) & 0x00ff00ffu;
        return (x | x >> 8) & 0xffffu;
    };
    auto flush = [&]() {                                             // whole workgroup; nlocal is stable here
        __syncthreads();
        const uint32_t n = nlocal;
        if (n) {
            if (threadIdx.x == 0) flush_base = atomicAdd(escaped_total, (unsigned long long)n);
            __syncthreads();
            const unsigned long long base = flush_base;
            for (uint32_t i = threadIdx.x; i < n; i += 256) if (base + i < cap) list[base + i] = local[i];
            __syncthreads();
            if (threadIdx.x == 0) nlocal = 0;
        }
        __syncthreads();
    };
    const size_t turns = (words + (size_t)gridDim.x * 256 - 1) / ((size_t)gridDim.x * 256);       // the same for every lane: the flushes are collective
    for (size_t it = 0; it < turns; it++) {
        const size_t w = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        uint32_t esc = 0;
        if (w < words) {
            const uint2 v = reinterpret_cast<const uint2 *>(wide)[w];
            accept_bits[w] = even_bits(v.x) | even_bits(v.y) << 16;
            esc = even_bits(v.x >> 1) | even_bits(v.y >> 1) << 16;
            escaped_bits[w] = esc;
        }
        // append my escaped lines, eight at a time (so that a turn never overruns the local buffer between two flushes)
        while (__syncthreads_or(esc != 0)) {
            uint32_t take = 0;
            for (uint32_t k = 0, m = esc; k < 8 && m; k++) { take |= m & (0u - m); m &= m - 1; }
            const uint32_t c = (uint32_t)__popc(take);
            if (c) {
                uint32_t at = atomicAdd(&nlocal, c);
                for (uint32_t m = take; m; m &= m - 1) local[at++] = (uint64_t)w * 32 + (uint32_t)(__ffs((int)m) - 1);
            }
            esc &= ~take;
            __syncthreads();
            if (nlocal > kFlushAt) flush();
        }
    }
    flush();
}
int match_stripes_dfa2_two_bit(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                               size_t nstripes, uint32_t *wide_bits, void *stream) {
    return launch_dfa2(match_stripes2_two_bit_kernel, p, bytes, nbytes, stripe, nstripes, kThreads, stream, stripe_base, wide_bits);
}
int split_two_bit(const uint32_t *wide, size_t nlines, uint32_t *accept_bits, uint32_t *escaped_bits, unsigned long long *escaped_total, uint64_t *list,
                  size_t cap, void *stream) {
    const size_t words = (nlines + 31) / 32;
    if (!words) return 0;
    size_t blocks = (words + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(split_two_bit_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, wide, words, accept_bits, escaped_bits, escaped_total,
                       list, cap);
    return (int)hipGetLastError();
}
// byte-stride table engines in one-pass mode (bytes >= 0x80 are always clamped: nobody has looked at the corpus yet)
int match_onepass_dfa(const LineDfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                      uint32_t *slabs, void *stream) {
    if (p.in_global) return launch_onepass<LineDfaGlobalEngine, LineDfaDevice>(p, 256, bytes, nbytes, stripe, nstripes, counts, slabs, stream);
    if (p.wide) return launch_onepass<LineDfaEngine<true, true>, LineDfaDevice>(p, LineDfaEngine<true, true>::lds_bytes(p), bytes, nbytes, stripe, nstripes, counts, slabs, stream);
    return launch_onepass<LineDfaEngine<false, false>, LineDfaDevice>(p, LineDfaEngine<false, false>::lds_bytes(p), bytes, nbytes, stripe, nstripes, counts, slabs, stream);
}
size_t onepass_slab_words(size_t nstripes, uint32_t stripe) {
    return ((nstripes + kThreads - 1) / kThreads) * slab_words_per_lane(stripe) * kThreads;
}
int match_onepass_dfa2(const Dfa2Device &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                       uint32_t *slabs, void *stream) {
    return launch_dfa2(match_stripes2_onepass_kernel, p, bytes, nbytes, stripe, nstripes, kThreads, stream, counts, slabs);
}
int compact_streams(const uint32_t *counts, const uint64_t *stripe_base, size_t nstripes, uint32_t stripe, const uint32_t *slabs,
                    uint32_t *accept_bits, size_t cap_words, void *stream) {
    if (!nstripes) return 0;
    hipLaunchKernelGGL(compact_streams_kernel, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, counts, stripe_base, nstripes,
                       stripe, slabs, accept_bits, cap_words);
    return (int)hipGetLastError();
}
int match_extents_dfa(const DfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint8_t *accept,
                      void *stream, const uint32_t *only_if) {
    // tables beyond the LDS budget (the batch kernel's "global" form) stay in HBM/L2 here too
    if (PlainDfaEngine::lds_bytes(p) > kPlainDfaLdsBudget)
        return launch_extents<PlainDfaGlobalEngine, DfaDevice>(p, PlainDfaGlobalEngine::lds_bytes(p), bytes, off, nitems, trim, accept, stream, only_if);
    return launch_extents<PlainDfaEngine, DfaDevice>(p, PlainDfaEngine::lds_bytes(p), bytes, off, nitems, trim, accept, stream, only_if);
}

}  // namespace dev
}  // namespace rrx
