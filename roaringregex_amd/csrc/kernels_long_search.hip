// kernels_long_search.hip — a directional run over one long string on a plain DFA (rrx_search_longest_string, rrx_contains_string):
// the chunk maps of kernels_long.hpp in walking order, every level of their composition kept, the down-sweep that turns the levels
// into the state every chunk is ENTERED in, and the second walk per chunk that reports where the table accepts.  device.hpp has the
// contract (long_run_dfa).
#include "kernels_long.hpp"

namespace rrx {
namespace dev {
namespace {

__global__ void long_set_word_kernel(uint32_t *__restrict__ word, uint32_t value) {
    if (threadIdx.x == 0 && blockIdx.x == 0) word[0] = value;
}

// Down-sweep of one level: workgroup g owns the maps in[g*group .. g*group + group) of the level and the state parent[g] their
// group is entered in; entry[g*group + i] = the state member i is entered in.  The maps are staged in LDS as long_compose_kernel
// stages them; one lane walks them (a chain of `group` dependent LDS reads), the entries leave coalesced.
__global__ __launch_bounds__(kLongThreads) void long_entries_kernel(const uint16_t *__restrict__ in, uint32_t nin, uint32_t D, uint32_t group,
                                                                    const uint32_t *__restrict__ parent, uint32_t *__restrict__ entry) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *sm = reinterpret_cast<uint16_t *>(smem);
    uint32_t *ent = reinterpret_cast<uint32_t *>(smem + (((size_t)group * D * sizeof(uint16_t) + 15) & ~(size_t)15));
    const size_t lo = (size_t)blockIdx.x * group, hi = lo + group < nin ? lo + group : nin;
    const uint32_t cnt = (uint32_t)(hi - lo);
    for (uint32_t i = threadIdx.x; i < cnt * D; i += kLongThreads) sm[i] = in[lo * D + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = parent[blockIdx.x];
        for (uint32_t k = 0; k < cnt; k++) { ent[k] = s; s = sm[k * D + s]; }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < cnt; k += kLongThreads) entry[lo + k] = ent[k];
}

// The widened table with bit 15 of an entry = "the target row accepts": 254 * 129 < 32768, and the step stays one LDS read
constexpr uint32_t kLongAccepts = 0x8000u, kLongRowMask = 0x7fffu;
__device__ __forceinline__ void long_load_wide_marked(const DfaDevice &p, uint16_t *wide) {
    const uint32_t D = p.nstates;
    for (uint32_t i = threadIdx.x; i < D * kWideColumns; i += blockDim.x) {
        const uint32_t s = i / kWideColumns, c = i % kWideColumns;
        const uint32_t t = p.next[s * p.ncls + p.cls[c]];
        wide[i] = (uint16_t)(t * kWideColumns | (p.acc[t] ? kLongAccepts : 0u));
    }
}

// Step 4.  ext[k] = the last offset in walking order at which the table accepts after a byte of chunk k (forwards the offset
// BEHIND that byte, backwards the byte's own), ~0ull where it does not; exit_state[k] = the state the chunk is left in.  With one
// chunk `entry` is the run's start word itself.
template <bool BACK>
__global__ __launch_bounds__(kLongThreads) void long_extreme_kernel(DfaDevice p, uint32_t row0_dead, const uint8_t *__restrict__ bytes, size_t nbytes,
                                                                    uint32_t chunk, uint32_t nchunks, const uint32_t *__restrict__ entry,
                                                                    uint64_t *__restrict__ ext, uint32_t *__restrict__ exit_state) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *wide = reinterpret_cast<uint16_t *>(smem);
    long_load_wide_marked(p, wide);
    __syncthreads();
    const size_t k = (size_t)blockIdx.x * kLongThreads + threadIdx.x;
    if (k >= nchunks) return;
    size_t a, b;
    long_chunk_span<BACK>(k, chunk, nbytes, a, b);
    uint32_t row = entry[k] * kWideColumns;
    uint64_t last = ~0ull;
    auto one = [&](uint32_t c, size_t at) {
        const uint32_t e = wide[row + (c < 128 ? c : 128)];
        row = e & kLongRowMask;
        if (e & kLongAccepts) last = at;
    };
    auto stopped = [&] { return row0_dead && row == 0; };
    if constexpr (BACK) {
        size_t q = b;                                    // bytes [q, b) have been walked
        for (; q > a && (reinterpret_cast<uintptr_t>(bytes + q) & 15) && !stopped(); q--) one(bytes[q - 1], q - 1);
        for (; q >= a + 16 && !stopped(); q -= 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q - 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 15; i >= 0; i--) one((w[i >> 2] >> (8 * (i & 3))) & 0xffu, q - 16 + i);
        }
        for (; q > a && !stopped(); q--) one(bytes[q - 1], q - 1);
    } else {
        size_t q = a;                                    // bytes [a, q) have been walked
        for (; q < b && (reinterpret_cast<uintptr_t>(bytes + q) & 15) && !stopped(); q++) one(bytes[q], q + 1);
        for (; q + 16 <= b && !stopped(); q += 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + q);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 16; i++) one((w[i >> 2] >> (8 * (i & 3))) & 0xffu, q + i + 1);
        }
        for (; q < b && !stopped(); q++) one(bytes[q], q + 1);
    }
    ext[k] = last;
    exit_state[k] = row / kWideColumns;
}

// The extreme of the chunks - their minimum backwards, their maximum forwards, ~0ull where no chunk has one - and the exit state
// of the chunk walked last.  One workgroup.
template <bool BACK>
__global__ __launch_bounds__(kLongThreads) void long_reduce_kernel(const uint64_t *__restrict__ ext, const uint32_t *__restrict__ exit_state, uint32_t n,
                                                                   LongRunResult *__restrict__ out) {
    __shared__ uint64_t best[kLongThreads];
    auto better = [](uint64_t x, uint64_t y) {           // ~0ull loses against every offset either way
        if constexpr (BACK) return x < y ? x : y;
        else return (int64_t)x > (int64_t)y ? x : y;
    };
    uint64_t mine = ~0ull;
    for (uint32_t k = threadIdx.x; k < n; k += kLongThreads) mine = better(mine, ext[k]);
    best[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t half = kLongThreads / 2; half; half >>= 1) {
        if (threadIdx.x < half) best[threadIdx.x] = better(best[threadIdx.x], best[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out->extreme = best[0];
        out->exit_state = exit_state[n - 1];
        out->pad = 0;
    }
}

// The scratch of a run over n chunks of a table of D states: per chunk the extreme (u64), the exit state and the entry state
// (u32), then the entries and the maps of the upper levels, then what the four-step build takes per chunk.
struct LongRunLayout {
    static constexpr int kMaxLevels = 4;                 // 65536 chunks: 65536, 512, 4
    uint32_t nlevels = 0, count[kMaxLevels] = {};
    size_t first[kMaxLevels] = {};                       // first node of a level among all nodes
    size_t ext = 0, exit_state = 0, entry = 0, maps = 0, dist = 0, res = 0, flags = 0, bytes = 0;
    LongRunLayout(uint32_t D, size_t n) {
        size_t nodes = 0;
        for (size_t c = n;; c = (c + kLongGroup - 1) / kLongGroup) {
            count[nlevels] = (uint32_t)c;
            first[nlevels++] = nodes;
            nodes += c;
            if (c <= kLongGroup || nlevels == kMaxLevels) break;
        }
        auto take = [&](size_t size) { const size_t at = bytes; bytes += (size + 15) & ~(size_t)15; return at; };
        ext = take(n * sizeof(uint64_t));
        exit_state = take(n * sizeof(uint32_t));
        entry = take(nodes * sizeof(uint32_t));
        maps = take(nodes * D * sizeof(uint16_t));
        dist = take(n * kLongSlots * sizeof(uint16_t));
        res = take(n * kLongSlots * sizeof(uint16_t));
        flags = take(n);
    }
};
// chunks of a run over nbytes bytes, and the most any run over at most nbytes bytes has (chunks are 256 bytes or more)
size_t long_run_chunks(size_t nbytes) { return (nbytes + long_chunk(nbytes) - 1) / long_chunk(nbytes); }
size_t long_run_max_chunks(size_t nbytes) { const size_t n = (nbytes + 255) / 256; return n < 65536 ? (n ? n : 1) : 65536; }

// long_entries_kernel serves both directions: one slot (kernels_long.hpp: long_compose_lds)
hipError_t long_entries_lds(size_t bytes) {
    static LdsAttr attr;
    return ensure_dynamic_lds(attr, reinterpret_cast<const void *>(long_entries_kernel), bytes);
}

template <bool BACK>
int long_run(const DfaDevice &p, bool row0_dead, const uint8_t *bytes, size_t nbytes, const uint32_t *start_state, uint8_t *scratch, LongRunResult *out,
             hipStream_t st) {
    const uint32_t D = p.nstates, chunk = long_chunk(nbytes), n = (uint32_t)long_run_chunks(nbytes);
    const LongRunLayout lay(D, n);
    if (lay.count[lay.nlevels - 1] > kLongGroup) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)D * kWideColumns * sizeof(uint16_t);
    const size_t entries_lds = (((size_t)kLongGroup * D * sizeof(uint16_t) + 15) & ~(size_t)15) + kLongGroup * sizeof(uint32_t);
    static LdsAttr attr_extreme;                         // (long_extreme_kernel<BACK>: a kernel per direction, a slot per direction)
    hipError_t e = long_maps_lds<BACK>(D);
    if (e == hipSuccess) e = long_entries_lds(entries_lds);
    if (e == hipSuccess) e = ensure_dynamic_lds(attr_extreme, reinterpret_cast<const void *>(long_extreme_kernel<BACK>), lds);
    if (e != hipSuccess) return (int)e;
    uint64_t *ext = reinterpret_cast<uint64_t *>(scratch + lay.ext);
    uint32_t *exit_state = reinterpret_cast<uint32_t *>(scratch + lay.exit_state), *entry = reinterpret_cast<uint32_t *>(scratch + lay.entry);
    uint16_t *maps = reinterpret_cast<uint16_t *>(scratch + lay.maps);
    const uint32_t *chunk_entry = start_state;
    if (n > 1) {
        long_build_maps<BACK>(p, bytes, nbytes, chunk, n, maps, reinterpret_cast<uint16_t *>(scratch + lay.dist), reinterpret_cast<uint16_t *>(scratch + lay.res),
                              scratch + lay.flags, st);
        for (uint32_t l = 0; l + 1 < lay.nlevels; l++)                       // up-sweep: level l + 1 from level l
            hipLaunchKernelGGL(long_compose_kernel, dim3(lay.count[l + 1]), dim3(kLongThreads), (size_t)kLongGroup * D * sizeof(uint16_t), st,
                               maps + lay.first[l] * D, lay.count[l], D, kLongGroup, maps + lay.first[l + 1] * D);
        for (uint32_t l = lay.nlevels; l-- > 0;) {                           // down-sweep: the top level is one group, entered in the start state
            const uint32_t groups = (lay.count[l] + kLongGroup - 1) / kLongGroup;
            const uint32_t *parent = l + 1 == lay.nlevels ? start_state : entry + lay.first[l + 1];
            hipLaunchKernelGGL(long_entries_kernel, dim3(groups), dim3(kLongThreads), entries_lds, st, maps + lay.first[l] * D, lay.count[l], D, kLongGroup,
                               parent, entry + lay.first[l]);
        }
        chunk_entry = entry;
    }
    hipLaunchKernelGGL(long_extreme_kernel<BACK>, dim3((n + kLongThreads - 1) / kLongThreads), dim3(kLongThreads), lds, st, p, row0_dead ? 1u : 0u, bytes, nbytes,
                       chunk, n, chunk_entry, ext, exit_state);
    hipLaunchKernelGGL(long_reduce_kernel<BACK>, dim3(1), dim3(kLongThreads), 0, st, ext, exit_state, n, out);
    return (int)hipGetLastError();
}

}  // namespace

size_t long_run_scratch_bytes(uint32_t nstates, size_t nbytes) { return LongRunLayout(nstates, long_run_max_chunks(nbytes)).bytes; }

int long_run_dfa(const DfaDevice &p, bool backward, bool row0_dead, const uint8_t *bytes, size_t nbytes, const uint32_t *start_state, void *scratch,
                 LongRunResult *out, void *stream) {
    if (!p.nstates || p.nstates > kLongMaxStates || !nbytes) return (int)hipErrorInvalidValue;
    return backward ? long_run<true>(p, row0_dead, bytes, nbytes, start_state, static_cast<uint8_t *>(scratch), out, (hipStream_t)stream)
                    : long_run<false>(p, row0_dead, bytes, nbytes, start_state, static_cast<uint8_t *>(scratch), out, (hipStream_t)stream);
}

int long_set_word(uint32_t *word, uint32_t value, void *stream) {
    hipLaunchKernelGGL(long_set_word_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, word, value);
    return (int)hipGetLastError();
}

}  // namespace dev
}  // namespace rrx
