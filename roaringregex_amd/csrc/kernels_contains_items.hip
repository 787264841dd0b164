// kernels_contains_items.hip — "which items contain a match" (rrx_contains_extents / rrx_contains_items): the lane-per-item
// kernel on the plain contains table and the copy of a stripe-wise result out of its scratch bitmap.  The stripe-wise forms are
// the items kernels themselves on the contains items tables (kernels_items.hip: items_match / items_match2).
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// One lane per item on the contains table (lower.hpp: contains_dfa) in its plain form: the walk of item_lanes.hpp, aligned on the
// offset as in match_extents_kernel, with three differences from that kernel:
//  * no byte kills: NUL and bytes >= 0x80 are class 0 in the table's own byte -> class map, and class 0 is a live column here;
//  * a lane stops reading once its state cannot change any more: `found`, the one accepting state, is absorbing, and so is row 0
//    (SKIP - the start row of the empty language, unreachable otherwise).  found = ~0u: the host found no such state, no early exit;
//  * the result is a bitmap.  One ballot gathers the verdicts of a pass' 64 consecutive items, lane 0 writes them as two plain 32-bit
//    stores.  The wave owns both words - no atomics, and nothing to clear beforehand; lanes behind the last item vote 0, a second
//    word wholly behind the last item is not written.
template <class Engine, class Program>
__global__ __launch_bounds__(kThreads) void contains_extents_kernel(Program prog, uint32_t found, const uint8_t *__restrict__ bytes,
                                                                     const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                     uint32_t *__restrict__ bits, const uint32_t *__restrict__ only_if) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (only_if && !*only_if) return;            // queued behind the stripe-wise kernel as its fallback: the batch was fit, nothing to do
    Engine eng;
    eng.load(prog, smem);
    __syncthreads();
    for_each_wave_pass(nitems, [&](size_t first, uint32_t lane) {
        const size_t i = first + lane;
        bool hit = false;
        if (i < nitems) {
            const auto [b, e] = item_span(off, i, trim);
            typename Engine::State st;
            eng.reset(st);
            bool done = st.s == found || st.s == 0;
            size_t p = b;
            auto one = [&](uint32_t c) {
                eng.step(st, c);
                done = st.s == found || st.s == 0;
            };
            for (; p < e && (p & 15) && !done; p++) one(bytes[p]);                 // up to 16-byte alignment
            for (; p + 16 <= e && !done; p += 16) {                                // 16 bytes per load
                const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (!done) one((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
            }
            for (; p < e && !done; p++) one(bytes[p]);
            hit = eng.accepting(st);
        }
        const uint64_t verdicts = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) {
            bits[first >> 5] = (uint32_t)verdicts;
            if (first + 32 < nitems) bits[(first >> 5) + 1] = (uint32_t)(verdicts >> 32);
        }
    });
}

// The first `words` words of a stripe-wise result (scratch: padded, and bit nitems may be set by the batch's closing end) into the
// caller's bitmap, the last word masked.
__global__ __launch_bounds__(256) void copy_result_bits_kernel(const uint32_t *__restrict__ src, size_t words, uint32_t last_mask,
                                                               uint32_t *__restrict__ dst) {
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256)
        dst[w] = w + 1 == words ? src[w] & last_mask : src[w];
}

}  // namespace

int contains_extents_dfa(const DfaDevice &p, bool in_global, uint32_t found, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim,
                         uint32_t *bits, void *stream, const uint32_t *only_if) {
    if (!nitems) return 0;
    if (!plain_table_ok(p)) return (int)hipErrorInvalidValue;
    const size_t max_blocks = only_if ? kItemLanesMaxBlocks : 0;      // (the fallback mostly has nothing to do: see launch_extents)
    // tables beyond the LDS budget, and the tables of a regex that asked for the global form, stay in HBM/L2
    if (in_global || PlainDfaEngine::lds_bytes(p) > kPlainDfaLdsBudget)
        return launch_item_lanes<contains_extents_kernel<PlainDfaGlobalEngine, DfaDevice>>(PlainDfaGlobalEngine::lds_bytes(p), nitems, max_blocks, stream, p, found,
                                                                                          bytes, off, nitems, trim, bits, only_if);
    return launch_item_lanes<contains_extents_kernel<PlainDfaEngine, DfaDevice>>(PlainDfaEngine::lds_bytes(p), nitems, max_blocks, stream, p, found, bytes, off,
                                                                                nitems, trim, bits, only_if);
}

int copy_result_bits(const uint32_t *result, size_t nitems, uint32_t *bits, void *stream) {
    const size_t words = (nitems + 31) / 32;
    if (!words) return 0;
    const uint32_t last_mask = (nitems & 31) ? (1u << (nitems & 31)) - 1u : 0xffffffffu;
    size_t blocks = (words + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(copy_result_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, result, words, last_mask, bits);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
