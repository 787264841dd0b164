// item_lanes.hpp — what the lane-per-item kernels share: the span of an item, the wave-per-64-items grid-stride loop,
// match_extents_kernel itself, and the host half of their launchers.  Included by the units that hold such a kernel only:
// kernels_table.hip and kernels_nfa.inc (match_extents_kernel), kernels_contains_items.hip, kernels_search_items.hip,
// kernels_search_all_items.hip, kernels_search_longest_items.hip, kernels_search_all_longest_items.hip, kernels_replace_items.hip and
// kernels_replace_template_items.hip (through replace_sweep.hpp), kernels_pieces_items.hip (no walk in these three: their kernels take the span, the loop and the
// launcher), kernels_group_items.hip and kernels_multi_items.hip (contains_extents_kernel's walk on a product table) - and by
// kernels_search_longest_corpus.hip, a lane-per-STRIPE kernel, for the launcher, the result constants and the placement rule of the
// two plain tables alone.
//
// THE WALK, described here once.  A lane reads its item [b, e) straight from HBM/L2, forwards or backwards, in three stretches:
// single bytes up to a 16-byte boundary, one uint4 per 16 bytes (forwards the low byte first, backwards the high byte), single
// bytes again.  No byte outside the stretch is ever read: a wide load is used only where all its 16 bytes lie inside it.  Before
// EVERY byte the walk tests the kernel's exit flag (a dead or absorbing state, a hit).  The three search kernels align on the
// ADDRESS ((p + skew) & 15, skew = the buffer's address mod 16); match_extents_kernel and contains_extents_kernel align on the
// OFFSET (p & 15), as they always have - on a buffer that is not 16-byte aligned their wide loads are unaligned ones.  Both rules
// are kept on purpose: changing which loads the two older kernels issue is a change of their speed, to be measured on its own.
// The loops are still WRITTEN OUT in every kernel: as shared functions taking the exit test and the per-byte step they cost 8 to
// 32 SGPRs per kernel and match_extents_kernel<PlainNfaEngine<6>> one wave per SIMD (profiles/item_lanes_isa_check.txt).
#pragma once
#include "table_engines.hpp"

namespace rrx {
namespace dev {
namespace {

constexpr uint32_t kNoMatch = 0xffffffffu;               // match_start / match_end of an item without a match
constexpr size_t kMaxItemOffset = 0xfffffffeu;           // result offsets are 32-bit and ~0u says "none": the search kernels treat an item as if it ended here

// Item i of an offsets array: bytes [b, e), the last `trim` bytes (the separator) left out, at most `cap` bytes long.
struct ItemSpan { size_t b, e; };
__device__ __forceinline__ ItemSpan item_span(const uint64_t *__restrict__ off, size_t i, uint32_t trim, size_t cap = ~(size_t)0) {
    const size_t b = off[i];
    size_t e = off[i + 1];
    e = e - b >= trim ? e - trim : b;
    if (e - b > cap) e = b + cap;
    return {b, e};
}

// The grid-stride loop of the kernels whose results are rows: a pass gives every wave 64 CONSECUTIVE items starting at `first`, a
// multiple of 64, so that a wave's result stores are contiguous 256-byte rows (contains: two words of the bitmap that the wave
// owns).  The loop runs on the wave's first item: every lane of a wave makes every turn, also a lane whose own item, first + lane,
// lies behind the last one.  What such a lane does is the body's business - the search kernels return at once, contains votes 0 in its ballot.
template <class Pass>
__device__ __forceinline__ void for_each_wave_pass(size_t nitems, Pass &&pass) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t per_pass = (size_t)gridDim.x * kThreads;
    for (size_t first = (size_t)blockIdx.x * kThreads + (threadIdx.x - lane); first < nitems; first += per_pass) pass(first, lane);
}

// ============================================================================================ extents kernel
// One lane per item on the regex' own engine.  Used for explicit (offset,len) batches, for the iterator facade's single strings,
// and wherever '\n' is an ordinary character.  NUL and bytes >= 0x80 kill.
template <class Engine, class Program>
__global__ __launch_bounds__(kThreads) void match_extents_kernel(Program prog, const uint8_t *__restrict__ bytes,
                                                                  const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                  uint8_t *__restrict__ accept, const uint32_t *__restrict__ only_if) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (only_if && !*only_if) return;            // queued behind the stripe-wise kernel as its fallback: the batch was fit, nothing to do
    Engine eng;
    eng.load(prog, smem);
    __syncthreads();
    // (one item per lane when the grid covers the batch; the predicated fallback is launched with a bounded grid and strides)
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < nitems; i += (size_t)gridDim.x * kThreads) {
        const auto [b, e] = item_span(off, i, trim);
        typename Engine::State st;
        eng.reset(st);
        bool dead = false;
        size_t p = b;
        auto one = [&](uint32_t c) {
            if (c == 0 || c >= 0x80) { eng.kill(st); dead = true; }
            else eng.step(st, c);
        };
        for (; p < e && (p & 15) && !dead; p++) one(bytes[p]);                 // up to 16-byte alignment
        for (; p + 16 <= e && !dead; p += 16) {                                // 16 bytes per load
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (!dead) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        }
        for (; p < e && !dead; p++) one(bytes[p]);
        accept[i] = eng.accepting(st) ? 1 : 0;
    }
}

// ============================================================================================ host half
constexpr size_t kItemLanesMaxBlocks = 1024;     // two generations on the 256 CUs at two workgroups each; beyond 2^20 items the grid strides

// kThreads lanes per workgroup, `lds_bytes` of dynamic LDS, a workgroup per kThreads items but at most max_blocks (0: no cap).
// The kernel is a template argument - the pointer, not its type, which kernels of one signature share: `attr` is one static per kernel
// as long as a kernel has ONE call site (a second one passing other argument types would be a second instantiation).
template <auto kernel, class... Args>
int launch_item_lanes(size_t lds_bytes, size_t nitems, size_t max_blocks, void *stream, Args... args) {
    static LdsAttr attr;
    const hipError_t e = ensure_dynamic_lds(attr, reinterpret_cast<const void *>(kernel), lds_bytes);
    if (e != hipSuccess) return (int)e;
    size_t blocks = (nitems + kThreads - 1) / kThreads;
    if (max_blocks && blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds_bytes, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}

template <class Engine, class Program>
int launch_extents(const Program &p, size_t table_bytes, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                   uint8_t *accept, void *stream, const uint32_t *only_if = nullptr) {
    if (!nitems) return 0;
    // the fallback behind the stripe-wise kernel mostly has nothing to do: a grid that ends at once (86 k workgroups: 33 us)
    return launch_item_lanes<match_extents_kernel<Engine, Program>>(table_bytes, nitems, only_if ? kItemLanesMaxBlocks : 0, stream, p, bytes, off, nitems,
                                                                    trim, accept, only_if);
}

inline bool plain_table_ok(const DfaDevice &t) { return t.nstates && t.next && t.cls && t.acc; }
// Two plain tables of one kernel go into LDS, one behind the other, while together they fit the budget; else - and for a regex
// that asked for the global form - both stay in HBM/L2 (their class maps in LDS).
inline bool two_tables_in_lds(const DfaDevice &a, const DfaDevice &b, bool in_global) {
    return !in_global && PlainDfaEngine::lds_bytes(a) + PlainDfaEngine::lds_bytes(b) <= kPlainDfaLdsBudget;
}

}  // namespace
}  // namespace dev
}  // namespace rrx
