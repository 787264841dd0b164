// kernels_replace_items.hip — regexp_replace on explicit items, WRITTEN on the device (rrx_replace_matches_sizes / _fill,
// rrx_replace_all_longest_*): from a column (bytes, offsets, trim), a match list per item (the CSR arrays every rrx_search_all* entry
// returns) and a literal replacement R of rep_len bytes to the new column.  No table, no regex: the kernels do not know where a list
// came from.  Output item i = t[0:s_0] + R + t[e_0:s_1] + R + ... + R + t[e_{m-1}:], t = the item without its separator.
// Two kernels, the two passes of every CSR result: SIZES (a lane per item) and FILL (a wave per 64 items, driven by OUTPUT bytes);
// both are described in replace_sweep.hpp, which the template unit shares.
#include "replace_sweep.hpp"

namespace rrx {
namespace dev {
namespace {

// The literal replacement: the same rep_len bytes behind every match.
struct LiteralReplacement {
    const uint8_t *__restrict__ rep;
    uint32_t rep_len;
    __device__ __forceinline__ bool holds(uint64_t, uint64_t at, uint64_t q, uint64_t, bool &in_rep, uint64_t &origin, uint64_t &lim, uint64_t &len) const {
        len = rep_len;
        if (q - at >= rep_len) return false;
        in_rep = true;
        origin = at;
        if (at + rep_len < lim) lim = at + rep_len;
        return true;
    }
    __device__ __forceinline__ uint32_t byte(uint64_t at) const { return rep[at]; }
};

// SIZES (replace_sweep.hpp: replace_sizes_walk): pos[slot] = s_k - (what the matches before it removed) + k * rep_len.
__global__ __launch_bounds__(kThreads) void replace_sizes_kernel(const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                 const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_start,
                                                                 const uint32_t *__restrict__ match_end, uint32_t rep_len, uint32_t *__restrict__ len,
                                                                 uint32_t *__restrict__ pos, uint32_t *__restrict__ too_long) {
    replace_sizes_walk(off, nitems, trim, first, match_start, match_end, len, pos, too_long, [=](uint64_t, uint64_t) { return (uint64_t)rep_len; });
}

// FILL (replace_sweep.hpp: replace_fill_sweep): d = r - pos[j]: R[d] if d < rep_len, else byte match_end[j] + d - rep_len of the item.
__global__ __launch_bounds__(kThreads, 8) void replace_fill_kernel(const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off, size_t nitems,
                                                                uint32_t trim, const uint64_t *__restrict__ first,
                                                                const uint32_t *__restrict__ match_end, const uint32_t *__restrict__ pos,
                                                                const uint8_t *__restrict__ rep, uint32_t rep_len,
                                                                const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    __shared__ uint64_t staged[kWavesPerBlock][65];
    replace_fill_sweep(staged[threadIdx.x >> 6], bytes, off, nitems, trim, first, match_end, pos, LiteralReplacement{rep, rep_len}, out_off, out);
}

}  // namespace

int replace_sizes(const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start, const uint32_t *match_end,
                  uint32_t rep_len, uint32_t *len, uint32_t *pos, uint32_t *too_long, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<replace_sizes_kernel>(0, nitems, kReplaceMaxBlocks, stream, off, nitems, trim, first, match_start, match_end, rep_len, len, pos,
                                                   too_long);
}

int replace_fill(const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_end,
                 const uint32_t *pos, const uint8_t *rep, uint32_t rep_len, const uint64_t *out_off, uint8_t *out, void *stream) {
    if (!nitems) return 0;
    return launch_item_lanes<replace_fill_kernel>(0, nitems, kReplaceMaxBlocks, stream, bytes, off, nitems, trim, first, match_end, pos, rep, rep_len,
                                                  out_off, out);
}

}  // namespace dev
}  // namespace rrx
