// table_engines.hpp — the table engine structs: the byte-stride line and plain DFA engines (tables in LDS or in HBM/L2)
// and the stride-2 engine Dfa2.  No kernels and no launchers.  Included by kernels_items.hip and, through item_lanes.hpp (what the
// lane-per-item kernels share), by the units that hold such a kernel.
#pragma once
#include "kernels_common.hpp"

namespace rrx {
namespace dev {
namespace {

// ============================================================================================ engines
// Line-mode engines expose
//     void load(program, lds)               cooperative table copy into LDS
//     State fresh() / State skipping()      start of a line / inside a line owned by somebody else
//     void step(State&, c, nl, acc)         consume one byte; nl = 1 iff it was '\n', acc = verdict of the
//                                           line it ended (valid when nl)

// ---- wide / classed table DFA: '\n' handling folded into the table -------------------------------
template <bool WIDE, bool CLAMP>
struct LineDfaEngine {
    static constexpr bool kStaged = true;      // results go through the workgroup's LDS window (ResultsT<true>)
    static constexpr bool kEightWaves = false;
    static constexpr int kRoundBytes = kRound;
    // Table entry: bits 0..15 = byte offset of the next row, byte 2 = 1 iff the consumed byte was '\n',
    // byte 3 = verdict of the line it ended.  (16-bit entries read with ds_read_u16 measured 3-4 % slower.)
    struct State { uint32_t e; };
    const uint8_t *tab;                    // LDS, byte-addressed
    const uint8_t *cls;                    // LDS [256] (classed form)
    uint32_t start_off, dead_off;
    uint32_t col_shift;                    // log2(bytes between neighbouring columns) = 2 + log2(copies)

    static size_t lds_bytes(const LineDfaDevice &p) { return (size_t)p.nrows * p.stride * 4 + (WIDE ? 0 : 256); }
    typedef const __attribute__((address_space(3))) uint32_t *lds_u32_ptr;
    __device__ void load(const LineDfaDevice &p, uint8_t *lds) {
        uint32_t *t = reinterpret_cast<uint32_t *>(lds);
        const int n = (int)(p.nrows * p.stride);
        // In the SDWA form the low half of an entry is the ABSOLUTE LDS address of the next row, so that
        // e.word[0] + 4*c is the address to read, with no base to add per byte.
        const uint32_t base = (WIDE && !CLAMP) ? (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)lds : 0u;
        copy_table_to_lds(t, p.table, (uint32_t)n * 4u, base);
        if (!WIDE) {
            uint8_t *c = lds + (size_t)n * 4;
            for (int i = threadIdx.x; i < 256; i += blockDim.x) c[i] = p.cls[i];
            cls = c;
        }
        tab = lds;
        // R interleaved copies (wide form): lane l lives in copy l % R, whose dwords sit in banks = l (mod R)
        const uint32_t copy = WIDE ? (threadIdx.x & ((1u << p.rep_log2) - 1u)) * 4u : 0u;
        col_shift = 2u + (WIDE ? p.rep_log2 : 0u);
        start_off = p.start_off + base + copy;
        dead_off = base + copy;
    }
    __device__ __forceinline__ State fresh() const { return State{start_off}; }
    __device__ __forceinline__ State skipping() const { return State{dead_off}; }   // dead row: waits for '\n'
    // Byte K of text word w, fused with the result accumulation bits = (bits << nl) | acc.  A wave64 integer
    // VALU op costs 4 cycles on a CDNA4 SIMD, so the step is written as 4 VALU + 1 LDS per byte with the
    // field extractions folded into SDWA operand selects (hipcc emits 6-7 for the plain C form below):
    //     c4   = w.byte[K] << 2                 v_lshlrev_b32_sdwa   src1_sel:BYTE_K
    //     addr = e.word[0] + c4                 v_add_u32_sdwa       src0_sel:WORD_0
    //     e    = LDS[addr]                      ds_read_b32
    //     bits = bits << e.byte[2]              v_lshlrev_b32_sdwa   src0_sel:BYTE_2
    //     bits = bits |  e.byte[3]              v_or_b32_sdwa        src0_sel:BYTE_3
    template <int K>
    __device__ __forceinline__ void consume(State &st, uint32_t w, uint32_t &bits) const {
        if constexpr (WIDE && !CLAMP) {
            // One asm block per byte (separate statements made hipcc pad every byte with an s_nop).  The block
            // waits for its own LDS read; the only other memory traffic of the wave are global loads (vmcnt).
            uint32_t t0, t1;
#define RRX_STEP(SEL)                                                                                                        \
            asm volatile("v_lshlrev_b32_sdwa %[c4], %[two], %[w] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:" SEL "\n\t" \
                         "v_add_u32_sdwa %[ad], %[e], %[c4] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t"       \
                         "ds_read_b32 %[e], %[ad]\n\t"                                                                                  \
                         "s_waitcnt lgkmcnt(0)\n\t"                                                                                     \
                         "v_lshlrev_b32_sdwa %[b], %[e], %[b] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD\n\t"     \
                         "v_or_b32_sdwa %[b], %[e], %[b] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD"              \
                         : [e] "+v"(st.e), [b] "+v"(bits), [c4] "=&v"(t0), [ad] "=&v"(t1)                                               \
                         : [w] "v"(w), [two] "v"(col_shift)                                                                             \
                         : "memory")
            if constexpr (K == 0) RRX_STEP("BYTE_0");
            if constexpr (K == 1) RRX_STEP("BYTE_1");
            if constexpr (K == 2) RRX_STEP("BYTE_2");
            if constexpr (K == 3) RRX_STEP("BYTE_3");
#undef RRX_STEP
        } else {
            uint32_t nl, acc;
            step(st, (w >> (8 * K)) & 0xffu, nl, acc);
            bits = (bits << nl) | acc;
        }
    }
    __device__ __forceinline__ void consume_word(State &st, uint32_t w, uint32_t &bits) const {
        consume<0>(st, w, bits); consume<1>(st, w, bits); consume<2>(st, w, bits); consume<3>(st, w, bits);
    }
    __device__ __forceinline__ void step(State &st, uint32_t c, uint32_t &nl, uint32_t &acc) const {
        uint32_t col;
        if (WIDE) col = CLAMP ? (c < 128u ? c : 128u) : c;      // !CLAMP: the corpus holds no byte >= 0x80
        else col = cls[c];
        const uint32_t off = (st.e & 0xffffu) + (col << col_shift);      // (absolute LDS address in the SDWA form)
        st.e = (WIDE && !CLAMP) ? *reinterpret_cast<lds_u32_ptr>(off) : *reinterpret_cast<const uint32_t *>(tab + off);
        nl = (st.e >> 16) & 0xffu;
        acc = st.e >> 24;
    }
};

// ---- table DFA whose table stays in global memory (L2-resident): any automaton up to 65535 interned sets ----
struct LineDfaGlobalEngine {
    static constexpr bool kStaged = true;
    static constexpr bool kEightWaves = false;
    static constexpr int kRoundBytes = kRound;
    struct State { uint32_t e; };          // low 24 bits = index of the current row's first entry
    const uint32_t *__restrict__ tab;      // HBM / L2
    const uint8_t *cls;                    // LDS [256]
    uint32_t start_off;

    static size_t lds_bytes(const LineDfaDevice &) { return 256; }
    __device__ void load(const LineDfaDevice &p, uint8_t *lds) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lds[i] = p.cls[i];
        cls = lds; tab = p.table; start_off = p.start_off;
    }
    __device__ __forceinline__ State fresh() const { return State{start_off}; }
    __device__ __forceinline__ State skipping() const { return State{0}; }
    __device__ __forceinline__ void step(State &st, uint32_t c, uint32_t &nl, uint32_t &acc) const {
        st.e = tab[(st.e & 0xffffffu) + cls[c]];
        nl = (st.e >> 30) & 1u;
        acc = st.e >> 31;
    }
    template <int K>
    __device__ __forceinline__ void consume(State &st, uint32_t w, uint32_t &bits) const {
        uint32_t nl, acc;
        step(st, (w >> (8 * K)) & 0xffu, nl, acc);
        bits = (bits << nl) | acc;
    }
    __device__ __forceinline__ void consume_word(State &st, uint32_t w, uint32_t &bits) const {
        consume<0>(st, w, bits); consume<1>(st, w, bits); consume<2>(st, w, bits); consume<3>(st, w, bits);
    }
};

struct PlainDfaEngine {
    struct State { uint32_t s; };
    const uint8_t *cls;     // LDS [256]
    const uint16_t *next;   // LDS [nstates][ncls]
    const uint8_t *acc;     // LDS [nstates]
    uint32_t ncls, start;

    static size_t lds_bytes(const DfaDevice &p) {
        size_t t = ((size_t)p.nstates * p.ncls * 2 + 15) & ~(size_t)15;
        return t + 256 + ((p.nstates + 15) & ~15u);
    }
    __device__ void load(const DfaDevice &p, uint8_t *lds) {
        size_t tb = ((size_t)p.nstates * p.ncls * 2 + 15) & ~(size_t)15;
        uint16_t *n = reinterpret_cast<uint16_t *>(lds);
        uint8_t *c = lds + tb;
        uint8_t *a = c + 256;
        for (int i = threadIdx.x; i < (int)(p.nstates * p.ncls); i += blockDim.x) n[i] = p.next[i];
        for (int i = threadIdx.x; i < 256; i += blockDim.x) c[i] = p.cls[i];
        for (int i = threadIdx.x; i < (int)p.nstates; i += blockDim.x) a[i] = p.acc[i];
        next = n; cls = c; acc = a; ncls = p.ncls; start = p.start;
    }
    __device__ __forceinline__ void reset(State &st) const { st.s = start; }
    __device__ __forceinline__ void kill(State &st) const { st.s = 0; }
    __device__ __forceinline__ bool accepting(const State &st) const { return acc[st.s] != 0; }
    __device__ __forceinline__ void step(State &st, uint32_t c) const { st.s = next[st.s * ncls + cls[c]]; }
};

// The same automaton with its table left in HBM/L2 (tables beyond the LDS budget: the batch kernel's "global" form,
// here for explicit items and single strings).  One dependent L2 read per byte.
struct PlainDfaGlobalEngine {
    struct State { uint32_t s; };
    const uint8_t *cls;                   // LDS [256]
    const uint16_t *__restrict__ next;    // HBM / L2 [nstates][ncls]
    const uint8_t *__restrict__ acc;      // HBM / L2 [nstates]
    uint32_t ncls, start;

    static size_t lds_bytes(const DfaDevice &) { return 256; }
    __device__ void load(const DfaDevice &p, uint8_t *lds) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lds[i] = p.cls[i];
        cls = lds; next = p.next; acc = p.acc; ncls = p.ncls; start = p.start;
    }
    __device__ __forceinline__ void reset(State &st) const { st.s = start; }
    __device__ __forceinline__ void kill(State &st) const { st.s = 0; }
    __device__ __forceinline__ bool accepting(const State &st) const { return acc[st.s] != 0; }
    __device__ __forceinline__ void step(State &st, uint32_t c) const { st.s = next[(size_t)st.s * ncls + cls[c]]; }
};

// ============================================================================================ stride-2 table kernel
// The per-byte table step is bounded by the latency of its dependent LDS round trip (add -> ds_read -> wait, ~210
// cycles at 8 chains per SIMD).  Here ONE dependent lookup consumes TWO bytes: the pair's column comes from the
// state-independent table P (its read does not wait for the state), then e = T2[row(e)][column].  U2: 46 distinct
// pair columns of 289 class pairs, T2 = 16 KiB.  Per pair: 5 VALU + 2 LDS reads, and one shift per text dword where P holds
// 16-bit entries: 2.75 VALU per byte on the u16 table, 2.5 on the byte-wide one.
// PAIRS8: the pair table is the byte-wide P8[128][kDfa2P8Stride] (device.hpp) - four entries per LDS dword where the u16 table
// has two, and an index made of the raw text bytes.  The entries are the same byte offsets; only the line form has it.
template <bool PAIRS8>
struct Dfa2T {
    typedef const __attribute__((address_space(3))) uint32_t *lds_u32_ptr;
    struct State { uint32_t e; };          // low 16 bits = LDS address of the current row (of this lane's copy)
    const uint8_t *P;                      // LDS (a static array at a link-time address: no base to add per pair)
    uint32_t start_off, dead_off;
    static constexpr uint32_t kPBytes = PAIRS8 ? kDfa2P8Bytes : kDfa2PBytes;

    __host__ __device__ static size_t lds_bytes(const Dfa2Device &p) { return (size_t)p.nrows * p.stride * 4; }     // dynamic part: T2
    __device__ void load(const Dfa2Device &p, void *p_lds, uint8_t *t_lds, uint32_t p_bytes = kPBytes) {
        const uint32_t tbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)t_lds;
        copy_table_to_lds(p_lds, PAIRS8 ? static_cast<const void *>(p.P8) : static_cast<const void *>(p.P), p_bytes);
        copy_table_to_lds(t_lds, p.T2, p.nrows * p.stride * 4, tbase);
        const uint32_t copy = (threadIdx.x & ((1u << p.rep_log2) - 1u)) * 4u;
        P = static_cast<const uint8_t *>(p_lds);
        start_off = p.start_off + tbase + copy;
        dead_off = tbase + copy;
    }
    __device__ __forceinline__ State fresh() const { return State{start_off}; }
    __device__ __forceinline__ State skipping() const { return State{dead_off}; }
#define RRX_LDS_U8(x) (*(P + (x)))
#define RRX_LDS_U16(x) (*reinterpret_cast<const uint16_t *>(P + (x)))
#define RRX_LDS_U32(x) (*reinterpret_cast<lds_u32_ptr>(x))
    // generic pair step (tails and the walk past the stripe end)
    __device__ __forceinline__ void step2(State &st, uint32_t c1, uint32_t c2, uint32_t &lines, uint32_t &verdicts) const {
        const uint32_t col = PAIRS8 ? (uint32_t)RRX_LDS_U8(c1 * kDfa2P8Stride + c2) : (uint32_t)RRX_LDS_U16((c1 * kDfa2PStride + c2) * 2);
        st.e = *reinterpret_cast<lds_u32_ptr>((st.e & 0xffffu) + col);
        lines = (st.e >> 16) & 0xffu;
        verdicts = st.e >> 24;
    }
    // the four bytes of text word w (two pairs), fused with bits = (bits << lines) | verdicts.  Per pair, on the u16 table
    // (w2 = w << 1, once per text word: every byte < 0x80, doubling stays inside the byte):
    //     t    = (2 c1) * 130                v_mul_u32_u24_sdwa   src0_sel:BYTE_even
    //     idx  = t + 2 c2                    v_add_u32_sdwa       src1_sel:BYTE_odd        (byte offset into P)
    //     col  = P[idx]                      ds_read_u16                                   (does not wait for the state)
    //     addr = e.word[0] + col             v_add_u32_sdwa       src0_sel:WORD_0
    //     e    = LDS[addr]                   ds_read_b32
    //     bits = (bits << e.byte[2]) | e.byte[3]                 2 x SDWA
    // and on the byte-wide one, on w itself: t = c1 * 136, idx = t + c2, col = P8[idx] (ds_read_u8), then the same.
    __device__ __forceinline__ void consume_dword(State &st, uint32_t w, uint32_t &bits) const {
        const uint32_t w2 = PAIRS8 ? w : w << 1;
        const uint32_t stride = PAIRS8 ? kDfa2P8Stride : kDfa2PStride;
        uint32_t ta, ia, tb, ib;
        asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(ta) : "v"(w2), "v"(stride));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(ia) : "v"(ta), "v"(w2));
        asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(tb) : "v"(w2), "v"(stride));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(ib) : "v"(tb), "v"(w2));
        const uint32_t ca = PAIRS8 ? (uint32_t)RRX_LDS_U8(ia) : (uint32_t)RRX_LDS_U16(ia);
        const uint32_t cb = PAIRS8 ? (uint32_t)RRX_LDS_U8(ib) : (uint32_t)RRX_LDS_U16(ib);
        uint32_t addr;
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(addr) : "v"(st.e), "v"(ca));
        st.e = RRX_LDS_U32(addr);
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(addr) : "v"(st.e), "v"(cb));
        st.e = RRX_LDS_U32(addr);
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
    }
    // The items form (codes 0 ... 128, 128 = END OF ITEM): a byte can no longer be doubled inside the text word, so the entry index
    // c1 * 130 + c2 is made first and doubled afterwards - one VALU more per pair.  (u16 table only: 129 codes have no byte-wide form.)
    __device__ __forceinline__ void consume_dword_items(State &st, uint32_t w, uint32_t &bits) const {
        static_assert(!PAIRS8, "the items form indexes the u16 pair table");
        const uint32_t stride = kDfa2PStride;
        uint32_t ta, ia, tb, ib;
        asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(ta) : "v"(w), "v"(stride));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(ia) : "v"(ta), "v"(w));
        asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(tb) : "v"(w), "v"(stride));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(ib) : "v"(tb), "v"(w));
        const uint32_t ca = RRX_LDS_U16(ia << 1);
        const uint32_t cb = RRX_LDS_U16(ib << 1);
        uint32_t addr;
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(addr) : "v"(st.e), "v"(ca));
        st.e = RRX_LDS_U32(addr);
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(addr) : "v"(st.e), "v"(cb));
        st.e = RRX_LDS_U32(addr);
        asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
        asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(bits) : "v"(st.e), "v"(bits));
    }
};
typedef Dfa2T<false> Dfa2;

}  // namespace
}  // namespace dev
}  // namespace rrx
