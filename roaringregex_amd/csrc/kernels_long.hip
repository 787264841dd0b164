// kernels_long.hip — one long string on the plain DFA: chunk maps from every state, their composition in groups, and the
// launcher match_long_dfa.  The maps and their composition: kernels_long.hpp (shared with kernels_long_search.hip).
#include "kernels_long.hpp"

namespace rrx {
namespace dev {
namespace {

__global__ void long_finish_kernel(const uint16_t *__restrict__ map, DfaDevice p, uint8_t *__restrict__ accept) {
    if (threadIdx.x == 0 && blockIdx.x == 0) accept[0] = p.acc[map[p.start]];
}

}  // namespace

size_t long_scratch_bytes(uint32_t nstates, size_t nbytes, uint32_t *chunk) {
    *chunk = long_chunk(nbytes);
    const size_t k0 = (nbytes + *chunk - 1) / *chunk, k1 = (k0 + kLongGroup - 1) / kLongGroup;
    // level 0, then the levels ping-pong between two areas; then per chunk kLongSlots distinct prefix states and their
    // results (u16 each) and a flag byte
    return (k0 + k1 + 2) * nstates * sizeof(uint16_t) + k0 * (kLongSlots * 2 * sizeof(uint16_t) + 1) + 16;
}
int match_long_dfa(const DfaDevice &p, const uint8_t *bytes, size_t nbytes, uint32_t chunk, void *scratch, uint8_t *accept,
                   void *stream) {
    const uint32_t D = p.nstates;
    if (!D || D > kLongMaxStates || !nbytes) return (int)hipErrorInvalidValue;
    const hipError_t e = long_maps_lds<false>(D);
    if (e != hipSuccess) return (int)e;
    uint32_t n = (uint32_t)((nbytes + chunk - 1) / chunk);
    uint16_t *cur = static_cast<uint16_t *>(scratch), *other = cur + (size_t)n * D;
    const size_t k1 = ((size_t)n + kLongGroup - 1) / kLongGroup;
    uint16_t *dist = cur + ((size_t)n + k1 + 2) * D, *res = dist + (size_t)n * kLongSlots;
    uint8_t *flags = reinterpret_cast<uint8_t *>(res + (size_t)n * kLongSlots);
    long_build_maps<false>(p, bytes, nbytes, chunk, n, cur, dist, res, flags, (hipStream_t)stream);
    uint16_t *area[2] = {other, cur};                          // level 1 writes behind level 0, level 2 over level 0, ...
    for (int lvl = 0; n > 1; lvl++) {
        const uint32_t m = (n + kLongGroup - 1) / kLongGroup;
        uint16_t *dst = area[lvl & 1];
        hipLaunchKernelGGL(long_compose_kernel, dim3(m), dim3(kLongThreads), (size_t)kLongGroup * D * sizeof(uint16_t), (hipStream_t)stream, cur, n, D, kLongGroup, dst);
        cur = dst;
        n = m;
    }
    hipLaunchKernelGGL(long_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cur, p, accept);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
