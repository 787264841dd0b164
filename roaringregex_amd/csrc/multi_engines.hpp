// multi_engines.hpp — the two placements of a group's product table (device.hpp: MultiDevice), shared by the kernels that step it:
// kernels_multi_items.hip (a lane per item) and kernels_multi_corpus.hip (a lane per stripe of a '\n'-corpus).
#pragma once
#include "kernels_common.hpp"

namespace rrx {
namespace dev {
namespace {

// The product table in LDS: the plain DFA engine's layout with a 32-bit mask per row in the place of its accept byte.
struct MultiLdsEngine {
    const uint8_t *cls;      // LDS [256]
    const uint16_t *next;    // LDS [nstates][ncls]
    const uint32_t *mask;    // LDS [nstates]
    uint32_t ncls;

    static size_t lds_bytes(const MultiDevice &p) { return multi_lds_bytes(p.nstates, p.ncls); }
    __device__ void load(const MultiDevice &p, uint8_t *lds) {
        const size_t tb = ((size_t)p.nstates * p.ncls * 2 + 15) & ~(size_t)15;
        uint16_t *n = reinterpret_cast<uint16_t *>(lds);
        uint8_t *c = lds + tb;
        uint32_t *m = reinterpret_cast<uint32_t *>(c + 256);
        for (int i = threadIdx.x; i < (int)(p.nstates * p.ncls); i += blockDim.x) n[i] = p.next[i];
        for (int i = threadIdx.x; i < 256; i += blockDim.x) c[i] = p.cls[i];
        for (int i = threadIdx.x; i < (int)p.nstates; i += blockDim.x) m[i] = p.mask[i];
        next = n; cls = c; mask = m; ncls = p.ncls;
    }
    __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t c) const { return next[s * ncls + cls[c]]; }
};
// The same table left in HBM/L2 (a group beyond the LDS budget, a set compiled for the global form): the class map in LDS.
struct MultiGlobalEngine {
    const uint8_t *cls;                   // LDS [256]
    const uint16_t *__restrict__ next;    // HBM / L2
    const uint32_t *__restrict__ mask;    // HBM / L2
    uint32_t ncls;

    static size_t lds_bytes(const MultiDevice &) { return 256; }
    __device__ void load(const MultiDevice &p, uint8_t *lds) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lds[i] = p.cls[i];
        cls = lds; next = p.next; mask = p.mask; ncls = p.ncls;
    }
    __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t c) const { return next[(size_t)s * ncls + cls[c]]; }
};

}  // namespace
}  // namespace dev
}  // namespace rrx
