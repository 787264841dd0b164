// kernels_nfa.inc — the shift-and NFA lane engines (state set in registers, bitmaps in LDS).  Shared device code:
// kernels_common.hpp.  Compiled four times, once per group of widths (kernels_nfa_w1.hip ... _w16.hip define
// RRX_NFA_PART): the instantiations of one group are a minute of hipcc, the groups build in parallel.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// ---- shift-and NFA: state set in W registers --------------------------------------------------------
template <int W>
struct NfaCore {
    struct State { uint32_t s[W]; };
    const uint32_t *B;      // LDS [256][W]
    const uint32_t *X;      // LDS [nbits][W]
    NfaMasks m;
    bool any_exc, any_carry;

    static size_t lds_bytes(const NfaDevice &p) { return ((size_t)256 * W + (size_t)p.nbits * W) * 4; }
    __device__ void load(const NfaDevice &p, uint8_t *lds) {
        uint32_t *b = reinterpret_cast<uint32_t *>(lds);
        uint32_t *x = b + 256 * W;
        copy_table_to_lds(b, p.B, 256u * W * 4u);
        copy_table_to_lds(x, p.X, p.nbits * W * 4u);
        B = b; X = x; m = p.masks; any_exc = p.any_exc != 0; any_carry = p.any_carry != 0;
    }
    __device__ __forceinline__ bool accepting(const State &st) const {
        uint32_t a = 0;
#pragma unroll
        for (int i = 0; i < W; i++) a |= st.s[i] & m.fin[i];
        return a != 0;
    }
    // next = ( ((S << 1) & CHAIN) | (S & SELF) | (((S & CGRP) + CGRP) & CTGT) | OR_{e in S & EXC} X[e] ) & B[c]
    __device__ __forceinline__ void advance(State &st, uint32_t c) const {
        uint32_t t[W];
        uint32_t exc = 0;
#pragma unroll
        for (int i = 0; i < W; i++) {
            uint32_t lo = i ? st.s[i - 1] : 0u;
            uint32_t sh = __builtin_amdgcn_alignbit(st.s[i], lo, 31);
            t[i] = (sh & m.chain[i]) | (st.s[i] & m.self[i]);
            exc |= st.s[i] & m.excm[i];
        }
        if (any_carry) {                                     // ((S & CGRP) + CGRP) & CTGT as one multiword add
            uint32_t cy = 0;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const uint64_t sum = (uint64_t)(st.s[i] & m.cgrp[i]) + m.cgrp[i] + cy;
                t[i] |= (uint32_t)sum & m.ctgt[i];
                cy = (uint32_t)(sum >> 32);
            }
        }
        if (any_exc && exc) {
#pragma unroll
            for (int i = 0; i < W; i++) {
                uint32_t e = st.s[i] & m.excm[i];
                while (e) {
                    int b = __ffs(e) - 1;
                    e &= e - 1;
                    const uint32_t *row = X + (size_t)(32 * i + b) * W;
#pragma unroll
                    for (int j = 0; j < W; j++) t[j] |= row[j];
                }
            }
        }
        const uint32_t *bc = B + c * W;
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = t[i] & bc[i];
    }
};

// ---- line-mode shift-and NFA (the batch kernel's NFA engine): NFA.cc:86-100 restated for one string per lane with the
// state set in W registers and the per-character bitmaps B[c] in LDS.  Everything the line protocol needs is folded
// into the automaton, so that a byte costs no compare and no re-initialisation:
//   * position 0 is the initial state.  The shift injects a 1 into it on EVERY byte, t0 = (S0 << 1) | 1, and only
//     B['\n'] contains position 0: after a '\n' the set is exactly {initial}, after any other byte position 0 is
//     clear.  Bytes 0x00 and >= 0x80 have empty rows: the set dies and stays dead until the next '\n'.
//   * the lowering leaves a never-entered gap position in front of every path of the path cover (lower_nfa, gaps),
//     so the bit shifted out of a path's end dies in the gap: no CHAIN mask.
//   * the verdict (S & FIN != 0, NFA.cc:103-107) is only evaluated in byte steps where SOME lane of the wave sits on a
//     '\n' (one SDWA compare + a scalar branch otherwise).
// Per byte and word: 1 shift (v_alignbit / v_lshl_or) + 1 AND with the B word, + 1 v_and_or for the self loops when
// the automaton has any (SELF); CARRY adds the add-carry groups (3 per word); RULES adds the exception rows of NfaCore
// (a divergent loop over the live exception positions) and takes the carry groups under a run-time flag.
template <int W, bool SELF, bool RULES, bool CARRY = false>
struct LineNfaEngine : NfaCore<W> {
    // Measured on the builds with rules (profiles/r02_nfa_variants.txt): the LDS result window and the four-rows-ahead
    // fetch each cost them 4-20 % (registers; their time goes to the exception loop), the plain builds gain from both.
    static constexpr bool kStaged = !RULES;
    static constexpr bool kLdsAtZero = true;                   // row_of(): byte * row bytes IS the LDS address of a B row
    static constexpr bool kEightWaves = W <= 2 && !RULES;      // 64 registers = two workgroups per CU
    static constexpr int kRoundBytes = W <= 4 ? kRound : kRound / 2;
    using State = typename NfaCore<W>::State;
    __device__ void load(const NfaDevice &p, uint8_t *lds) {
        NfaCore<W>::load(p, lds);
        // The byte step uses byte * row bytes as the LDS address of a B row: B must sit at LDS address 0, which it does
        // as long as the kernel has no static LDS in front of its dynamic LDS - the launchers check that on the host
        // (kLdsAtZero -> ensure_dynamic_lds).  (Adding the base would be a sixth VALU instruction per byte: the base is a
        // relocation, not an immediate.)
        __syncthreads();
        uint32_t *b = reinterpret_cast<uint32_t *>(lds);
        if (threadIdx.x < W) b[(size_t)'\n' * W + threadIdx.x] = threadIdx.x == 0 ? 1u : 0u;      // B['\n'] = {initial}
    }
    __device__ __forceinline__ State fresh() const {
        State st;
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = i == 0 ? 1u : 0u;
        return st;
    }
    __device__ __forceinline__ State skipping() const {
        State st;
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = 0;
        return st;
    }
    __device__ __forceinline__ void advance_line(State &st, uint32_t c) const { advance_row(st, this->B + c * W); }
    __device__ __forceinline__ void advance_row(State &st, const uint32_t *bc) const {
        uint32_t t[W];
        t[0] = (st.s[0] << 1) | 1u;
#pragma unroll
        for (int i = 1; i < W; i++) t[i] = __builtin_amdgcn_alignbit(st.s[i], st.s[i - 1], 31);
        if (SELF) {
#pragma unroll
            for (int i = 0; i < W; i++) t[i] |= st.s[i] & this->m.self[i];
        }
        if (RULES || CARRY) {
            if (CARRY || this->any_carry) {                      // ((S & CGRP) + CGRP) & CTGT as one multiword add
                uint32_t cy = 0;
#pragma unroll
                for (int i = 0; i < W; i++) {
                    const uint64_t sum = (uint64_t)(st.s[i] & this->m.cgrp[i]) + this->m.cgrp[i] + cy;
                    t[i] |= (uint32_t)sum & this->m.ctgt[i];
                    cy = (uint32_t)(sum >> 32);
                }
            }
            if (RULES && this->any_exc) {
                uint32_t exc = 0;
#pragma unroll
                for (int i = 0; i < W; i++) exc |= st.s[i] & this->m.excm[i];
                if (exc) {
#pragma unroll
                    for (int i = 0; i < W; i++) {
                        uint32_t e = st.s[i] & this->m.excm[i];
                        while (e) {
                            const int b = __ffs(e) - 1;
                            e &= e - 1;
                            const uint32_t *row = this->X + (size_t)(32 * i + b) * W;
#pragma unroll
                            for (int j = 0; j < W; j++) t[j] |= row[j];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = t[i] & bc[i];
    }
    // Byte K of text word w.  Two SDWA instructions read the byte straight out of the text register: the LDS address of
    // its B row (byte * row bytes; B is the first thing in LDS) and the lane mask "this byte is '\n'".  hipcc's own
    // code for the plain C form was 13 VALU per byte at W = 1 (field extraction, and the verdict if-converted into every
    // step).  The four B rows of a text word are requested before the first of the four dependent steps.
    typedef const __attribute__((address_space(3))) uint32_t *lds_u32_ptr;
    struct Row { uint32_t b[W]; };
    template <int K>
    __device__ __forceinline__ Row row_of(uint32_t w) const {
        uint32_t off;
        const uint32_t row_bytes = W * 4;
#define RRX_NFA_ROW(SEL) asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" SEL " src1_sel:DWORD" : "=v"(off) : "v"(w), "v"(row_bytes))
        if constexpr (K == 0) RRX_NFA_ROW("BYTE_0");
        if constexpr (K == 1) RRX_NFA_ROW("BYTE_1");
        if constexpr (K == 2) RRX_NFA_ROW("BYTE_2");
        if constexpr (K == 3) RRX_NFA_ROW("BYTE_3");
#undef RRX_NFA_ROW
        const lds_u32_ptr p = reinterpret_cast<lds_u32_ptr>(off);    // B sits at LDS address 0 (checked in load)
        Row r;
#pragma unroll
        for (int i = 0; i < W; i++) r.b[i] = p[i];
        return r;
    }
    template <int K>
    __device__ __forceinline__ void verdict(const State &st, uint32_t w, uint32_t &bits) const {
        uint64_t nlmask;
        const uint32_t ten = '\n';
#define RRX_NFA_NL(SEL) asm("v_cmp_eq_u32_sdwa %0, %1, %2 src0_sel:" SEL " src1_sel:DWORD" : "=s"(nlmask) : "v"(w), "v"(ten))
        if constexpr (K == 0) RRX_NFA_NL("BYTE_0");
        if constexpr (K == 1) RRX_NFA_NL("BYTE_1");
        if constexpr (K == 2) RRX_NFA_NL("BYTE_2");
        if constexpr (K == 3) RRX_NFA_NL("BYTE_3");
#undef RRX_NFA_NL
        if (nlmask) {                                             // wave-uniform: some lane ends a line on this byte
            uint32_t a = 0, tmp;
#pragma unroll
            for (int i = 0; i < W; i++) a |= st.s[i] & this->m.fin[i];
            // bits = (bits << 1) | verdict on the lanes of nlmask: the verdict enters as the carry of bits + bits
            asm volatile("v_cmp_ne_u32_e32 vcc, 0, %2\n\t"
                         "v_addc_co_u32_e32 %1, vcc, %0, %0, vcc\n\t"
                         "v_cndmask_b32_e64 %0, %0, %1, %3"
                         : "+v"(bits), "=&v"(tmp) : "v"(a), "s"(nlmask) : "vcc");
        }
    }
    __device__ __forceinline__ void consume_word(State &st, uint32_t w, uint32_t &bits) const {
        if constexpr (W <= 4 && !RULES) {
            const Row r0 = row_of<0>(w), r1 = row_of<1>(w), r2 = row_of<2>(w), r3 = row_of<3>(w);
            verdict<0>(st, w, bits); advance_row(st, r0.b);
            verdict<1>(st, w, bits); advance_row(st, r1.b);
            verdict<2>(st, w, bits); advance_row(st, r2.b);
            verdict<3>(st, w, bits); advance_row(st, r3.b);
        } else {                                                  // wide sets: one row in flight ahead of the step
            Row r = row_of<0>(w), n = row_of<1>(w);
            verdict<0>(st, w, bits); advance_row(st, r.b);
            r = row_of<2>(w);
            verdict<1>(st, w, bits); advance_row(st, n.b);
            n = row_of<3>(w);
            verdict<2>(st, w, bits); advance_row(st, r.b);
            verdict<3>(st, w, bits); advance_row(st, n.b);
        }
    }
    __device__ __forceinline__ void step(State &st, uint32_t c, uint32_t &nl, uint32_t &acc) const {
        const bool isnl = c == '\n';
        nl = isnl ? 1u : 0u;
        acc = (isnl && this->accepting(st)) ? 1u : 0u;
        advance_line(st, c);
    }
};

// ---- "which lines contain a match" on the line engine (rrx_contains_corpus under RRX_OPT_CONTAINS_NFA).  The program is the
// lane program with the contains B rows (pack.cpp: contains_b_rows): position 0 is in EVERY row, so the 1 that the shift injects
// survives every byte - a match may start anywhere -, and the rows of NUL and of bytes >= 0x80 are exactly {position 0}: such a
// byte ends every attempt under way and starts the next one.  The step is LineNfaEngine's; behind it one register, `found`,
// gathers S & FIN (one v_and_or_b32 per word), and under the wave-uniform '\n' branch the verdict is found != 0, after which the
// '\n' lanes clear it.  A lane that starts inside somebody else's line steps from the empty set and matches on from there: its
// first result is dropped by ResultsT, and its '\n' clears `found`.
// Two builds per width: RULES = false has self loops and carry groups compiled in (the one-pass kernels' policy), RULES = true
// has the exception rows and takes the carry groups under the run-time flag.
template <int W, bool RULES>
struct ContainsLineNfaEngine : LineNfaEngine<W, true, RULES, !RULES> {
    using Line = LineNfaEngine<W, true, RULES, !RULES>;
    static constexpr bool kStaged = Line::kStaged;
    static constexpr bool kLdsAtZero = true;
    static constexpr bool kEightWaves = W == 1 && !RULES;      // 58 registers; at W = 2 `found` is the 65th: the cap of two workgroups
                                                               //   per CU spilt 12 bytes per lane (profiles/contains_nfa_isa_check.txt)
    static constexpr int kRoundBytes = Line::kRoundBytes;
    struct State : NfaCore<W>::State { uint32_t found; };
    __device__ __forceinline__ State fresh() const {
        State st;
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = i == 0 ? 1u : 0u;
        st.found = 0;
        return st;
    }
    __device__ __forceinline__ State skipping() const {
        State st;
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = 0;
        st.found = 0;
        return st;
    }
    __device__ __forceinline__ void advance_found(State &st, const uint32_t *bc) const {
        this->advance_row(st, bc);
#pragma unroll
        for (int i = 0; i < W; i++) st.found = (st.s[i] & this->m.fin[i]) | st.found;
    }
    template <int K>
    __device__ __forceinline__ void verdict(State &st, uint32_t w, uint32_t &bits) const {
        uint64_t nlmask;
        const uint32_t ten = '\n';
#define RRX_NFA_NL(SEL) asm("v_cmp_eq_u32_sdwa %0, %1, %2 src0_sel:" SEL " src1_sel:DWORD" : "=s"(nlmask) : "v"(w), "v"(ten))
        if constexpr (K == 0) RRX_NFA_NL("BYTE_0");
        if constexpr (K == 1) RRX_NFA_NL("BYTE_1");
        if constexpr (K == 2) RRX_NFA_NL("BYTE_2");
        if constexpr (K == 3) RRX_NFA_NL("BYTE_3");
#undef RRX_NFA_NL
        if (nlmask) {                                             // wave-uniform: some lane ends a line on this byte
            uint32_t tmp;
            // bits = (bits << 1) | (found != 0) on the lanes of nlmask - the verdict enters as the carry of bits + bits -, and
            // those lanes start their next line with found = 0
            asm volatile("v_cmp_ne_u32_e32 vcc, 0, %1\n\t"
                         "v_addc_co_u32_e32 %2, vcc, %0, %0, vcc\n\t"
                         "v_cndmask_b32_e64 %0, %0, %2, %3\n\t"
                         "v_cndmask_b32_e64 %1, %1, 0, %3"
                         : "+v"(bits), "+v"(st.found), "=&v"(tmp) : "s"(nlmask) : "vcc");
        }
    }
    __device__ __forceinline__ void consume_word(State &st, uint32_t w, uint32_t &bits) const {
        using Row = typename Line::Row;
        if constexpr (W <= 4 && !RULES) {
            const Row r0 = this->template row_of<0>(w), r1 = this->template row_of<1>(w), r2 = this->template row_of<2>(w), r3 = this->template row_of<3>(w);
            verdict<0>(st, w, bits); advance_found(st, r0.b);
            verdict<1>(st, w, bits); advance_found(st, r1.b);
            verdict<2>(st, w, bits); advance_found(st, r2.b);
            verdict<3>(st, w, bits); advance_found(st, r3.b);
        } else {                                                  // wide sets: one row in flight ahead of the step
            Row r = this->template row_of<0>(w), n = this->template row_of<1>(w);
            verdict<0>(st, w, bits); advance_found(st, r.b);
            r = this->template row_of<2>(w);
            verdict<1>(st, w, bits); advance_found(st, n.b);
            n = this->template row_of<3>(w);
            verdict<2>(st, w, bits); advance_found(st, r.b);
            verdict<3>(st, w, bits); advance_found(st, n.b);
        }
    }
    __device__ __forceinline__ void step(State &st, uint32_t c, uint32_t &nl, uint32_t &acc) const {
        const bool isnl = c == '\n';
        nl = isnl ? 1u : 0u;
        acc = (isnl && st.found) ? 1u : 0u;
        if (isnl) st.found = 0;
        advance_found(st, this->B + c * W);
    }
};

// ---- plain engines for the extents kernel ('\n' is an ordinary byte) --------------------------------
template <int W>
struct PlainNfaEngine : NfaCore<W> {
    using State = typename NfaCore<W>::State;
    __device__ __forceinline__ void reset(State &st) const {
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = this->m.init[i];
    }
    __device__ __forceinline__ void kill(State &st) const {
#pragma unroll
        for (int i = 0; i < W; i++) st.s[i] = 0;
    }
    __device__ __forceinline__ void step(State &st, uint32_t c) const { this->advance(st, c); }
};

// ---- "which items contain a match" on the NFA (rrx_contains_extents / rrx_contains_items under RRX_OPT_CONTAINS_NFA): one lane per
// item on the program with the contains B rows, the walk of contains_extents_kernel written out (item_lanes.hpp: aligned on the
// offset, a 16-byte load only where all its bytes lie inside the item).  The step is NfaCore's with the CHAIN mask, then S |= init:
// a match may start behind every byte, '\n' is an ordinary byte, and NUL and bytes >= 0x80 need no compare - their rows are
// {position 0}, which the step never enters, so they leave exactly the initial set.  A lane leaves at its first S & FIN.  One
// ballot per 64 consecutive items, two plain word stores by lane 0: no atomics, nothing to clear (contains_extents_kernel).
template <int W>
__global__ __launch_bounds__(kThreads) void contains_extents_nfa_kernel(NfaDevice prog, const uint8_t *__restrict__ bytes,
                                                                         const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                         uint32_t *__restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    NfaCore<W> eng;
    eng.load(prog, smem);
    __syncthreads();
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        bool hit = false;
        if (i < nitems) {
            const auto [b, e] = item_span(off, i, trim);
            typename NfaCore<W>::State st;
#pragma unroll
            for (int k = 0; k < W; k++) st.s[k] = eng.m.init[k];
            hit = eng.accepting(st);
            size_t p = b;
            auto one = [&](uint32_t c) {
                eng.advance(st, c);
#pragma unroll
                for (int k = 0; k < W; k++) st.s[k] |= eng.m.init[k];
                hit = eng.accepting(st);
            };
            for (; p < e && (p & 15) && !hit; p++) one(bytes[p]);                  // up to 16-byte alignment
            for (; p + 16 <= e && !hit; p += 16) {                                 // 16 bytes per load
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (!hit) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
            }
            for (; p < e && !hit; p++) one(bytes[p]);
        }
        const uint64_t verdicts = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) {
            bits[first >> 5] = (uint32_t)verdicts;
            if (first + 32 < nitems) bits[(first >> 5) + 1] = (uint32_t)(verdicts >> 32);
        }
    });
}

// ---- one long string on an NFA engine (regex.h:156-159 consumes it byte by byte; one lane doing the same manages a few
// MB/s).  The string is cut into chunks and every chunk is stepped from EVERY position at once - lane = (chunk, start
// position p), the set starts as {p} - which yields, per chunk, the row "positions reached from p": the chunk's
// transition RELATION.  The relations are then composed pairwise, level by level (lane = (pair, position)), and the
// whole string's relation is applied to {initial}.  Work is bytes x positions lane steps (lanes whose set has died stop early), so this is for automata of
// a few dozen to a few hundred positions; '\n' is an ordinary byte, 0x00 and >= 0x80 kill every row.
template <int W>
__global__ __launch_bounds__(256) void long_rows_nfa_kernel(NfaDevice prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t chunk,
                                                             uint32_t nchunks, uint32_t *__restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    PlainNfaEngine<W> eng;
    eng.load(prog, smem);
    __syncthreads();
    const uint32_t N = prog.nbits;
    const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;      // (chunk, start position)
    if (item >= (size_t)nchunks * N) return;
    const size_t k = item / N;
    const uint32_t p = (uint32_t)(item % N);
    const size_t a = k * (size_t)chunk, b = a + chunk < nbytes ? a + chunk : nbytes;
    typename PlainNfaEngine<W>::State st;
#pragma unroll
    for (int i = 0; i < W; i++) st.s[i] = (uint32_t)i == (p >> 5) ? 1u << (p & 31) : 0u;
    auto alive = [&]() { uint32_t o = 0; for (int i = 0; i < W; i++) o |= st.s[i]; return o != 0; };
    size_t pos = a;
    // chunk starts are multiples of 16 from the base, and the base may sit at any address (rrx.h asks for no alignment):
    // sixteen bytes per load only where the chunk starts on a 16-byte boundary, as long_walk does; else byte by byte
    if ((reinterpret_cast<uintptr_t>(bytes + pos) & 15) == 0) {
        for (; pos + 16 <= b && alive(); pos += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + pos);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
                if (c == 0 || c >= 0x80) eng.kill(st); else eng.step(st, c);
            }
        }
    }
    for (; pos < b && alive(); pos++) { const uint32_t c = bytes[pos]; if (c == 0 || c >= 0x80) eng.kill(st); else eng.step(st, c); }
#pragma unroll
    for (int i = 0; i < W; i++) rows[item * W + i] = st.s[i];
}
// out[k] = in[2k+1] o in[2k]: the row of position p in the composed relation is the OR of the rows (in chunk 2k+1) of
// the positions its row in chunk 2k holds.  Lane = (k, p).  A last odd relation is copied.
template <int W>
__global__ __launch_bounds__(256) void long_compose_nfa_kernel(const uint32_t *__restrict__ in, uint32_t nin, uint32_t N, uint32_t *__restrict__ out) {
    const size_t item = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t nout = (nin + 1) / 2;
    if (item >= (size_t)nout * N) return;
    const size_t k = item / N;
    const uint32_t *a = in + ((size_t)2 * k * N + item % N) * W;     // my row in the left relation
    uint32_t acc[W];
    if (2 * k + 1 >= nin) {
#pragma unroll
        for (int i = 0; i < W; i++) acc[i] = a[i];
    } else {
        const uint32_t *bm = in + (size_t)(2 * k + 1) * N * W;       // the right relation
#pragma unroll
        for (int i = 0; i < W; i++) acc[i] = 0;
#pragma unroll
        for (int i = 0; i < W; i++) {
            uint32_t e = a[i];
            while (e) {
                const uint32_t q = 32u * i + (uint32_t)__ffs(e) - 1u;
                e &= e - 1;
                const uint32_t *row = bm + (size_t)q * W;
#pragma unroll
                for (int j = 0; j < W; j++) acc[j] |= row[j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < W; i++) out[item * W + i] = acc[i];
}
// the whole string's relation applied to {initial}: accept iff a final position is reached
template <int W>
__global__ void long_finish_nfa_kernel(NfaDevice prog, const uint32_t *__restrict__ rel, uint8_t *__restrict__ accept) {
    if (threadIdx.x || blockIdx.x) return;
    uint32_t a = 0;
    for (int i = 0; i < W; i++) {
        uint32_t e = prog.masks.init[i];
        while (e) {
            const uint32_t q = 32u * i + (uint32_t)__ffs(e) - 1u;
            e &= e - 1;
            for (int j = 0; j < W; j++) a |= rel[(size_t)q * W + j] & prog.masks.fin[j];
        }
    }
    accept[0] = a ? 1 : 0;
}

// ---- the sampled-table engine's third step: the lines its table could not decide (they ended in the ESCAPE state), stepped by
// the exact engine.  Lane = stripe, as in the batch kernel: a lane owns the lines that START in its stripe, looks at their bits
// of the escaped-lines bitmap - nearly all lanes find none and leave: a table that fits its text escapes on a handful of lines -
// and otherwise walks its stripe, sixteen bytes per load: lines that did not escape are skipped to their '\n', the others are
// stepped through the NFA.  A line ends at its '\n' or at the end of the data; 0x00 and bytes >= 0x80 reject it.  (The first
// form gave a lane a word of the bitmap and had it FIND its lines through the index: a binary search and a byte-by-byte scan
// of up to a stripe per word, 17 ms for 0.2 % escaped lines of 8 GiB.)
template <int W>
__global__ __launch_bounds__(256) void recheck_escaped_kernel(NfaDevice prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                               const uint64_t *__restrict__ stripe_base, size_t nstripes,
                                                               const uint32_t *__restrict__ escaped_bits, uint32_t *__restrict__ accept_bits,
                                                               const unsigned long long *__restrict__ escaped_total, size_t cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (*escaped_total <= cap) return;                    // the list holds every escaped line: recheck_lines_kernel decides them
    PlainNfaEngine<W> eng;
    eng.load(prog, smem);
    __syncthreads();
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nstripes) return;
    const uint64_t b0 = stripe_base[g], b1 = stripe_base[g + 1];
    const bool next_fresh = g + 1 < nstripes ? (b1 & kFreshStripe) != 0 : bytes[nbytes - 1] == '\n';
    const uint64_t lo = line_of(b0) + ((b0 & kFreshStripe) ? 0u : 1u);            // the lines that start in my stripe: lo .. hi
    const uint64_t past = line_of(b1) + (next_fresh ? 0u : 1u);                   // (hi + 1)
    if (past <= lo) return;
    auto escaped = [&](uint64_t line) -> bool { return (escaped_bits[line >> 5] >> (line & 31u)) & 1u; };
    uint64_t last = past;                                                         // my last escaped line (past: none)
    for (uint64_t w = lo >> 5; w <= (past - 1) >> 5; w++) {
        uint32_t m = escaped_bits[w];
        if (w == lo >> 5) m &= ~0u << (lo & 31u);
        if (w == (past - 1) >> 5 && ((past - 1) & 31u) != 31u) m &= (2u << ((past - 1) & 31u)) - 1u;
        if (m) last = w * 32 + (31u - (uint32_t)__clz((int)m));
    }
    if (last == past) return;
    // ---- walk my stripe from its first byte; the text comes sixteen bytes at a time (pos is kept 16-byte aligned + an offset)
    size_t pos = g * (size_t)stripe;
    uint4 buf = make_uint4(0, 0, 0, 0);
    size_t buf_at = ~(size_t)0;
    auto byte_at = [&](size_t q) -> uint32_t {                                   // q < nbytes
        const size_t a = q & ~(size_t)15;
        if (a != buf_at) {
            buf_at = a;
            if (a + 16 <= nbytes) buf = *reinterpret_cast<const uint4 *>(bytes + a);
            else {
                uint32_t w4[4] = {0, 0, 0, 0};
                for (size_t k = a; k < nbytes; k++) w4[(k - a) >> 2] |= (uint32_t)bytes[k] << (8 * ((k - a) & 3));
                buf = make_uint4(w4[0], w4[1], w4[2], w4[3]);
            }
        }
        const uint32_t k = (uint32_t)(q & 15);
        const uint32_t word = k < 4 ? buf.x : k < 8 ? buf.y : k < 12 ? buf.z : buf.w;
        return (word >> (8 * (k & 3))) & 0xffu;
    };
    auto skip_line = [&]() { while (pos < nbytes && byte_at(pos++) != '\n') {} };   // pos -> behind the next '\n' (or the end of the data)
    uint64_t line = lo;
    if (!(b0 & kFreshStripe)) skip_line();                                        // my first byte lies inside somebody else's line
    for (; line <= last && pos <= nbytes; line++) {
        if (!escaped(line)) { skip_line(); continue; }
        typename PlainNfaEngine<W>::State st;
        eng.reset(st);
        bool dead = false;
        while (pos < nbytes) {
            const uint32_t c = byte_at(pos++);
            if (c == '\n') break;
            if (dead) continue;
            if (c == 0 || c >= 0x80) { eng.kill(st); dead = true; } else eng.step(st, c);
        }
        if (!dead && eng.accepting(st)) atomicOr(&accept_bits[line >> 5], 1u << (line & 31u));
    }
}

// The common case: the escaped lines are few and the split kernel has listed them.  Lane = listed line.  Nobody keeps line
// offsets: the line's first byte is found through the stripe index - a binary search for the stripe that holds the line's
// preceding '\n', then that stripe's text sixteen bytes per load, its '\n' counted a word at a time - and the line is stepped
// through the NFA.  Work proportional to the escaped lines, not to the corpus.
template <int W>
__global__ __launch_bounds__(256) void recheck_lines_kernel(NfaDevice prog, const uint8_t *__restrict__ bytes, size_t nbytes, uint32_t stripe,
                                                             const uint64_t *__restrict__ stripe_base, size_t nstripes, const uint64_t *__restrict__ list,
                                                             const unsigned long long *__restrict__ escaped_total, size_t cap, uint32_t *__restrict__ accept_bits) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const unsigned long long total = *escaped_total;
    if (!total || total > cap) return;
    PlainNfaEngine<W> eng;
    eng.load(prog, smem);
    __syncthreads();
    uint4 buf = make_uint4(0, 0, 0, 0);
    size_t buf_at = ~(size_t)0;
    auto chunk_at = [&](size_t a) -> uint4 {                                      // a: 16-byte aligned, < nbytes
        if (a + 16 <= nbytes) return *reinterpret_cast<const uint4 *>(bytes + a);
        uint32_t w4[4] = {0, 0, 0, 0};
        for (size_t k = a; k < nbytes; k++) w4[(k - a) >> 2] |= (uint32_t)bytes[k] << (8 * ((k - a) & 3));
        return make_uint4(w4[0], w4[1], w4[2], w4[3]);
    };
    auto byte_at = [&](size_t q) -> uint32_t {
        const size_t a = q & ~(size_t)15;
        if (a != buf_at) { buf_at = a; buf = chunk_at(a); }
        const uint32_t k = (uint32_t)(q & 15);
        const uint32_t word = k < 4 ? buf.x : k < 8 ? buf.y : k < 12 ? buf.z : buf.w;
        return (word >> (8 * (k & 3))) & 0xffu;
    };
    auto newlines_in = [](uint32_t w) -> uint32_t {                               // exact: a 0x80 flag per byte equal to '\n'
        const uint32_t t = w ^ 0x0a0a0a0au;
        return ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
    };
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (size_t)gridDim.x * 256) {
        const uint64_t line = list[j];
        size_t pos = 0;
        if (line) {
            size_t lo = 0, hi = nstripes;                             // the last stripe with fewer than `line` newlines in front of it
            while (hi - lo > 1) {
                const size_t mid = lo + (hi - lo) / 2;
                if (line_of(stripe_base[mid]) < line) lo = mid; else hi = mid;
            }
            uint32_t need = (uint32_t)(line - line_of(stripe_base[lo]));          // the need-th '\n' from the stripe's first byte on
            pos = lo * (size_t)stripe;
            // (sixty-four bytes requested together while whole blocks lie in the data: one memory round trip per chunk made a lane
            // whose line starts two KiB into its stripe wait a hundred and twenty-eight of them)
            while (pos + 64 <= nbytes) {
                const uint4 *q4 = reinterpret_cast<const uint4 *>(bytes + pos);
                const uint4 v0 = q4[0], v1 = q4[1], v2 = q4[2], v3 = q4[3];
                const uint32_t c = (uint32_t)(__popc(newlines_in(v0.x)) + __popc(newlines_in(v0.y)) + __popc(newlines_in(v0.z)) + __popc(newlines_in(v0.w)) +
                                              __popc(newlines_in(v1.x)) + __popc(newlines_in(v1.y)) + __popc(newlines_in(v1.z)) + __popc(newlines_in(v1.w)) +
                                              __popc(newlines_in(v2.x)) + __popc(newlines_in(v2.y)) + __popc(newlines_in(v2.z)) + __popc(newlines_in(v2.w)) +
                                              __popc(newlines_in(v3.x)) + __popc(newlines_in(v3.y)) + __popc(newlines_in(v3.z)) + __popc(newlines_in(v3.w)));
                if (c >= need) break;
                need -= c;
                pos += 64;
            }
            while (pos < nbytes) {
                const uint4 v = chunk_at(pos);
                const uint32_t f[4] = {newlines_in(v.x), newlines_in(v.y), newlines_in(v.z), newlines_in(v.w)};
                const uint32_t c = (uint32_t)(__popc(f[0]) + __popc(f[1]) + __popc(f[2]) + __popc(f[3]));
                if (c < need) { need -= c; pos += 16; continue; }
                for (int q = 0; q < 4; q++) {                                     // it is in this chunk: which byte
                    uint32_t m = f[q];
                    while (m) {
                        const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                        m &= m - 1;
                        if (--need == 0) { pos += 4u * q + (bit >> 3) + 1u; q = 4; break; }
                    }
                }
                break;
            }
        }
        typename PlainNfaEngine<W>::State st;
        eng.reset(st);
        bool dead = false;
        while (pos < nbytes) {
            const uint32_t c = byte_at(pos++);
            if (c == '\n') break;
            if (dead) break;
            if (c == 0 || c >= 0x80) { eng.kill(st); dead = true; } else eng.step(st, c);
        }
        if (!dead && eng.accepting(st)) atomicOr(&accept_bits[line >> 5], 1u << (line & 31u));
    }
}

}  // namespace

// Widths of this part.  The device tables are padded to the instantiated width by the caller (NfaDevice::W is the padded width).
#if RRX_NFA_PART == 0
#define RRX_NFA_DISPATCH(CALL) switch (p.W) { case 1: return CALL(1); case 2: return CALL(2); default: return (int)hipErrorInvalidValue; }
#define RRX_NFA_NAME(base) base##_part0
#elif RRX_NFA_PART == 1
#define RRX_NFA_DISPATCH(CALL) switch (p.W) { case 3: return CALL(3); case 4: return CALL(4); default: return (int)hipErrorInvalidValue; }
#define RRX_NFA_NAME(base) base##_part1
#elif RRX_NFA_PART == 2
#define RRX_NFA_DISPATCH(CALL) switch (p.W) { case 5: case 6: return CALL(6); case 7: case 8: return CALL(8); default: return (int)hipErrorInvalidValue; }
#define RRX_NFA_NAME(base) base##_part2
#else
#define RRX_NFA_DISPATCH(CALL) switch (p.W) { case 9: case 10: case 11: case 12: return CALL(12); case 13: case 14: case 15: case 16: return CALL(16); default: return (int)hipErrorInvalidValue; }
#define RRX_NFA_NAME(base) base##_part3
#endif

int RRX_NFA_NAME(match_stripes_nfa)(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                                    size_t nstripes, uint32_t *accept, void *stream) {
    // four builds per width: the bare chain, + self loops, + add-carry groups, + exception rows
#define GO(WW, S, R, C) launch_stripes<LineNfaEngine<WW, S, R, C>, NfaDevice>(p, LineNfaEngine<WW, S, R, C>::lds_bytes(p), bytes, nbytes, stripe, stripe_base, nstripes, accept, stream)
#define CALL(WW) (p.any_exc ? GO(WW, true, true, false) : p.any_carry ? GO(WW, true, false, true) : p.any_self ? GO(WW, true, false, false) : GO(WW, false, false, false))
    RRX_NFA_DISPATCH(CALL)
#undef CALL
#undef GO
}
// one-pass mode: three builds per width (exception rows / self loops and carry groups / the bare chain)
int RRX_NFA_NAME(match_onepass_nfa)(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, size_t nstripes, uint32_t *counts,
                                    uint32_t *slabs, void *stream) {
#define GO(WW, S, R, C) launch_onepass<LineNfaEngine<WW, S, R, C>, NfaDevice>(p, LineNfaEngine<WW, S, R, C>::lds_bytes(p), bytes, nbytes, stripe, nstripes, counts, slabs, stream)
#define CALL(WW) (p.any_exc ? GO(WW, true, true, false) : (p.any_self || p.any_carry) ? GO(WW, true, false, true) : GO(WW, false, false, false))
    RRX_NFA_DISPATCH(CALL)
#undef CALL
#undef GO
}
int RRX_NFA_NAME(match_long_nfa)(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t chunk, uint32_t nchunks, void *scratch,
                                 uint8_t *accept, void *stream) {
#define CALL(WW) [&]() -> int {                                                                                                  \
        const size_t lds = PlainNfaEngine<WW>::lds_bytes(p);                                                                       \
        static LdsAttr attr;                                                                                                        \
        hipError_t e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(long_rows_nfa_kernel<WW>), lds);                   \
        if (e != hipSuccess) return (int)e;                                                                                         \
        const size_t items = (size_t)nchunks * p.nbits;                                                                             \
        hipLaunchKernelGGL(long_rows_nfa_kernel<WW>, dim3((unsigned)((items + 255) / 256)), dim3(256), lds, (hipStream_t)stream, p, bytes, nbytes, chunk, \
                           nchunks, static_cast<uint32_t *>(scratch));                                                             \
        uint32_t *cur = static_cast<uint32_t *>(scratch), *other = cur + items * WW;      /* levels ping-pong between two areas */ \
        for (uint32_t n = nchunks; n > 1; n = (n + 1) / 2) {                                                                       \
            const size_t out_items = (size_t)((n + 1) / 2) * p.nbits;                                                              \
            hipLaunchKernelGGL(long_compose_nfa_kernel<WW>, dim3((unsigned)((out_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cur, n, p.nbits, other); \
            uint32_t *tmp = cur; cur = other; other = tmp;                                                                          \
        }                                                                                                                           \
        hipLaunchKernelGGL(long_finish_nfa_kernel<WW>, dim3(1), dim3(64), 0, (hipStream_t)stream, p, cur, accept);               \
        return (int)hipGetLastError();                                                                                              \
    }()
    RRX_NFA_DISPATCH(CALL)
#undef CALL
}
int RRX_NFA_NAME(recheck_escaped_nfa)(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base, size_t nstripes,
                                      const uint32_t *escaped_bits, size_t nlines, const uint64_t *list, const unsigned long long *escaped_total, size_t cap,
                                      uint32_t *accept_bits, void *stream) {
#define CALL(WW) [&]() -> int {                                                                                                  \
        const size_t lds = PlainNfaEngine<WW>::lds_bytes(p);                                                                       \
        if (!nstripes || !nlines) return 0;                                                                                         \
        static LdsAttr attr, attr2;                                                                                                 \
        hipError_t e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(recheck_lines_kernel<WW>), lds);                   \
        if (e == hipSuccess) e = ensure_dynamic_lds(attr2, reinterpret_cast<const void *>(recheck_escaped_kernel<WW>), lds);      \
        if (e != hipSuccess) return (int)e;                                                                                         \
        /* the listed lines (nothing to do without any, or when the list ran over) ... */                                           \
        hipLaunchKernelGGL(recheck_lines_kernel<WW>, dim3(1024), dim3(256), lds, (hipStream_t)stream, p, bytes, nbytes, stripe, stripe_base, nstripes, list,   \
                           escaped_total, cap, accept_bits);                                                                       \
        /* ... and the walk over the stripes for a corpus that escapes on more lines than the list holds */                         \
        hipLaunchKernelGGL(recheck_escaped_kernel<WW>, dim3((unsigned)((nstripes + 255) / 256)), dim3(256), lds, (hipStream_t)stream, p, bytes, nbytes, stripe, \
                           stripe_base, nstripes, escaped_bits, accept_bits, escaped_total, cap);                                  \
        return (int)hipGetLastError();                                                                                              \
    }()
    RRX_NFA_DISPATCH(CALL)
#undef CALL
}
int RRX_NFA_NAME(match_extents_nfa)(const NfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint8_t *accept,
                                    void *stream) {
#define CALL(WW) launch_extents<PlainNfaEngine<WW>, NfaDevice>(p, PlainNfaEngine<WW>::lds_bytes(p), bytes, off, nitems, trim, accept, stream)
    RRX_NFA_DISPATCH(CALL)
#undef CALL
}
// contains on the program with the contains B rows: two builds per width (exception rows / self loops and carry groups) ...
int RRX_NFA_NAME(contains_stripes_nfa)(const NfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t stripe, const uint64_t *stripe_base,
                                       size_t nstripes, uint32_t *bits, void *stream) {
#define GO(WW, R) launch_stripes<ContainsLineNfaEngine<WW, R>, NfaDevice>(p, ContainsLineNfaEngine<WW, R>::lds_bytes(p), bytes, nbytes, stripe, stripe_base, nstripes, bits, stream)
#define CALL(WW) (p.any_exc ? GO(WW, true) : GO(WW, false))
    RRX_NFA_DISPATCH(CALL)
#undef CALL
#undef GO
}
// ... and a lane per item: every workgroup copies the program into LDS (up to 48 KiB), so the grid is bounded and strides
int RRX_NFA_NAME(contains_extents_nfa)(const NfaDevice &p, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, uint32_t *bits,
                                       void *stream) {
    if (!nitems) return 0;
#define CALL(WW) launch_item_lanes<contains_extents_nfa_kernel<WW>>(NfaCore<WW>::lds_bytes(p), nitems, kItemLanesMaxBlocks, stream, p, bytes, off, nitems, trim, bits)
    RRX_NFA_DISPATCH(CALL)
#undef CALL
}
}  // namespace dev
}  // namespace rrx
