// kernels_replace_template_items.hip — regexp_replace with GROUP REFERENCES on explicit items, written on the device
// (rrx_replace_template_sizes / _fill, rrx_replace_groups_longest_*): kernels_replace_items.hip with a replacement per match.  From a
// column, a match list per item, the spans of the referenced groups per match (one PLANE of two words per slot and group) and a
// template - a short program of segments, each a literal, the match itself or a plane's span - to the new column.  Output item i =
// t[0:s_0] + R_0 + t[e_0:s_1] + R_1 + ... + R_{m-1} + t[e_{m-1}:], R_k = the segments of match k one behind the other.  No table, no
// regex: the kernels do not know where the lists and the spans came from.  The literal pair of kernels is left as it is: a template
// costs a walk over its segments per match (sizes) and per located byte (fill) that a fixed R does not need.
#include "item_lanes.hpp"

namespace rrx {
namespace dev {
namespace {

// THE SEGMENT PROGRAM.  Three words per segment in device memory (kind, literal offset, literal length; kind 0 = literal, 1 = the
// match, 2 + r = plane r), copied into LDS by every workgroup: it is the same for every lane, and a walk reads it once per segment.
struct TemplateLds {
    const uint32_t *seg;                         // (LDS) nseg x 3 words
    uint32_t nseg;
};
__device__ __forceinline__ void load_template(const TemplateDevice &tpl, uint32_t *seg) {
    if (threadIdx.x < tpl.nseg * 3) seg[threadIdx.x] = tpl.segs[threadIdx.x];
    __syncthreads();
}

// What walk_template found: the segment that holds byte d of the replacement - it ends before byte `end` of it - and its source:
// byte d - delta of the literals, or of the item (delta = where the segment begins in the replacement - where its source begins).
struct TemplateHit {
    bool found = false, literal = false;
    uint64_t end = 0, delta = 0;
};
// THE ONE WALK over the replacement of `slot` in an item of L bytes: the segments in order with a running length.  Returns the
// replacement's length if no segment holds byte d (d = ~0: the sizes pass; the fill pass: d lies behind the replacement); stops at
// the segment that holds d otherwise (*hit; what it returns then is not the length).  Both passes go through here, so that they
// cannot disagree about a length.  A span (s, e) contributes item[s', e'), s' = min(s, L), e' = clamp(e, s', L), nothing where s is
// ~0u: no offset outside the item comes out of here, whatever the arrays hold.
__device__ __forceinline__ uint64_t walk_template(const TemplateLds &t, uint64_t slot, uint64_t L, const uint32_t *__restrict__ match_start,
                                                  const uint32_t *__restrict__ match_end, const uint32_t *__restrict__ ref_start,
                                                  const uint32_t *__restrict__ ref_end, uint64_t plane_stride, uint64_t d, TemplateHit *hit) {
    uint64_t run = 0;
    for (uint32_t k = 0; k < t.nseg; k++) {
        const uint32_t kind = t.seg[3 * k];
        uint64_t src, n;
        if (kind == 0) {
            src = t.seg[3 * k + 1];
            n = t.seg[3 * k + 2];
        } else {
            uint32_t s, e;
            if (kind == 1) { s = match_start[slot]; e = match_end[slot]; }
            else { const uint64_t w = (uint64_t)(kind - 2) * plane_stride + slot; s = ref_start[w]; e = ref_end[w]; }
            if (s == kNoMatch) continue;
            const uint64_t s1 = s < L ? s : L, e1 = e < s1 ? s1 : e < L ? e : L;
            src = s1;
            n = e1 - s1;
        }
        if (hit && d - run < n) {
            hit->found = true;
            hit->literal = kind == 0;
            hit->end = run + n;
            hit->delta = run - src;
            return run;
        }
        run += n;
    }
    return run;
}

// SIZES.  replace_sizes_kernel with the length of R_k from the walk: pos[slot] = where R_k begins inside the OUTPUT item, len[i] =
// the output item's length, saturated at ~0u; `shift` is (the replacements so far - what the matches removed) mod 2^64.  Every one of
// the nitems words of `len` and exactly the slots first[i] .. first[i + 1] of `pos` are written with plain stores.  too_long as there.
__global__ __launch_bounds__(kThreads) void replace_template_sizes_kernel(TemplateDevice tpl, const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                          const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_start,
                                                                          const uint32_t *__restrict__ match_end, const uint32_t *__restrict__ ref_start,
                                                                          const uint32_t *__restrict__ ref_end, uint64_t plane_stride,
                                                                          uint32_t *__restrict__ len, uint32_t *__restrict__ pos,
                                                                          uint32_t *__restrict__ too_long) {
    __shared__ uint32_t seg[3 * kTemplateMaxSegments];
    load_template(tpl, seg);
    const TemplateLds t = {seg, tpl.nseg};
    for_each_wave_pass(nitems, [&](size_t first_item, uint32_t lane) {
        const size_t i = first_item + lane;
        if (i >= nitems) return;
        const auto [b, e] = item_span(off, i, trim);
        const uint64_t f0 = first[i], f1 = first[i + 1];
        uint64_t shift = 0;
        for (uint64_t slot = f0; slot < f1; slot++) {
            const uint64_t s = match_start[slot], en = match_end[slot];
            pos[slot] = (uint32_t)(s + shift);
            shift += walk_template(t, slot, e - b, match_start, match_end, ref_start, ref_end, plane_stride, ~(uint64_t)0, nullptr) - (en - s);
        }
        uint64_t total = (uint64_t)(e - b) + shift;
        if ((int64_t)total < 0) total = 0;                   // (a list that removes more than the item holds: not a list of this item)
        len[i] = total > 0xffffffffu ? 0xffffffffu : (uint32_t)total;
        if (too_long && total >= ((uint64_t)1 << 30)) *too_long = 1;
    });
}

// FILL.  replace_fill_kernel's shape - a wave per 64 items, their output range swept 256 contiguous bytes per turn, dwords aligned
// by address, the partial first and last dwords byte by byte; the staged offsets, the item search and the pos search are those of
// kernels_replace_items.hip, described there.  locate has ONE LEVEL MORE: once the slot j with the last pos <= r is known and
// d = r - pos[j], the walk over R_j's segments finds the one that holds byte d: the source is a byte of the literals or of the item,
// `lim` that segment's end; if none holds it, the byte lies behind R_j and comes from the item at match_end[j] + d - |R_j| (the raw
// end, as in the literal kernel).  A source offset at or beyond the item's end gives 0 there; a segment's source lies inside the item
// by the walk's clamping.  Nothing outside [lo, hi) is written.
constexpr uint32_t kWavesPerBlock = kThreads / 64;
__device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
__global__ __launch_bounds__(kThreads, 8) void replace_template_fill_kernel(TemplateDevice tpl, const uint8_t *__restrict__ bytes,
                                                                            const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                            const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_start,
                                                                            const uint32_t *__restrict__ match_end, const uint32_t *__restrict__ pos,
                                                                            const uint32_t *__restrict__ ref_start, const uint32_t *__restrict__ ref_end,
                                                                            uint64_t plane_stride, const uint64_t *__restrict__ out_off,
                                                                            uint8_t *__restrict__ out) {
    __shared__ uint64_t staged[kWavesPerBlock][65];
    __shared__ uint32_t seg[3 * kTemplateMaxSegments];
    load_template(tpl, seg);
    const TemplateLds t = {seg, tpl.nseg};
    const uint8_t *__restrict__ lits = tpl.lits;
    uint64_t *row = staged[threadIdx.x >> 6];
    for_each_wave_pass(nitems, [&](size_t first_of_lane, uint32_t lane) {
        const size_t first_item = wave_uniform(first_of_lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (the previous pass has read the row)
        __builtin_amdgcn_wave_barrier();
        row[lane] = out_off[first_item + lane < nitems ? first_item + lane : nitems];
        if (lane == 0) row[64] = out_off[first_item + 64 < nitems ? first_item + 64 : nitems];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t lo = wave_uniform(row[0]), hi = wave_uniform(row[64]);
        if (hi <= lo) return;
        const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(out) + lo) & 3u);
        const uint64_t span = (hi - lo) + mis;                      // the sweep: bytes [0, span) from the aligned dword of out + lo on
        for (uint64_t rel = (uint64_t)lane * 4; rel < span; rel += 256) {
            const uint32_t c0 = rel < mis ? mis - (uint32_t)rel : 0u;                         // (rel < mis: rel == 0)
            const uint32_t c1 = span - rel < 4 ? (uint32_t)(span - rel) : 4u;
            // the segment that holds the byte located last: output bytes below lim; lits[q - origin] or byte q - origin of the item at b
            uint64_t lim = 0, origin = 0, b = 0, item_len = 0;
            bool in_lit = false;
            auto locate = [&](uint64_t q) {
                uint32_t idx = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if (row[idx + step] <= q) idx += step;
                const uint64_t o0 = row[idx], o1 = row[idx + 1], r = q - o0;
                const auto [ib, ie] = item_span(off, first_item + idx, trim);
                b = ib;
                item_len = ie - ib;
                const uint64_t f0 = first[first_item + idx], f1 = first[first_item + idx + 1];
                uint64_t below = f0, above = f1 > f0 ? f1 : f0;     // slots below `below` have pos <= r, those from `above` on pos > r
                while (below < above) {
                    const uint64_t mid = below + ((above - below) >> 1);
                    if (pos[mid] <= r) below = mid + 1;
                    else above = mid;
                }
                lim = o1;
                if (below < f1) { const uint64_t next = o0 + pos[below]; if (next < lim) lim = next; }
                in_lit = false;
                origin = o0;
                if (below > f0) {
                    const uint64_t j = below - 1, at = o0 + pos[j];  // where R_j begins in the output
                    TemplateHit hit;
                    const uint64_t rep_len = walk_template(t, j, item_len, match_start, match_end, ref_start, ref_end, plane_stride, q - at, &hit);
                    if (hit.found) {
                        in_lit = hit.literal;
                        origin = at + hit.delta;
                        if (at + hit.end < lim) lim = at + hit.end;
                    } else origin = at + rep_len - match_end[j];
                }
            };
            uint32_t word = 0;
            for (uint32_t c = c0; c < c1; c++) {
                const uint64_t q = lo + (rel + c - mis);
                if (c == c0 || q >= lim) locate(q);
                const uint64_t at = q - origin;
                const uint32_t v = in_lit ? lits[at] : at < item_len ? bytes[b + at] : 0u;
                word |= v << (8 * c);
            }
            uint8_t *dst = out + lo + (rel - mis);                   // (4-byte aligned; below out + lo only where c0 > 0: not stored to)
            if (c0 == 0 && c1 == 4) *reinterpret_cast<uint32_t *>(dst) = word;
            else for (uint32_t c = c0; c < c1; c++) dst[c] = (uint8_t)(word >> (8 * c));
        }
    });
}

}  // namespace

int replace_template_sizes(const TemplateDevice &tpl, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first, const uint32_t *match_start,
                           const uint32_t *match_end, const uint32_t *ref_start, const uint32_t *ref_end, uint64_t plane_stride, uint32_t *len, uint32_t *pos,
                           uint32_t *too_long, void *stream) {
    if (!nitems) return 0;
    if (tpl.nseg > kTemplateMaxSegments) return (int)hipErrorInvalidValue;
    return launch_item_lanes<replace_template_sizes_kernel>(0, nitems, kReplaceMaxBlocks, stream, tpl, off, nitems, trim, first, match_start, match_end,
                                                            ref_start, ref_end, plane_stride, len, pos, too_long);
}

int replace_template_fill(const TemplateDevice &tpl, const uint8_t *bytes, const uint64_t *off, size_t nitems, uint32_t trim, const uint64_t *first,
                          const uint32_t *match_start, const uint32_t *match_end, const uint32_t *pos, const uint32_t *ref_start, const uint32_t *ref_end,
                          uint64_t plane_stride, const uint64_t *out_off, uint8_t *out, void *stream) {
    if (!nitems) return 0;
    if (tpl.nseg > kTemplateMaxSegments) return (int)hipErrorInvalidValue;
    return launch_item_lanes<replace_template_fill_kernel>(0, nitems, kReplaceMaxBlocks, stream, tpl, bytes, off, nitems, trim, first, match_start, match_end,
                                                           pos, ref_start, ref_end, plane_stride, out_off, out);
}

}  // namespace dev
}  // namespace rrx
