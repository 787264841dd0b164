// kernels_replace_template_items.hip — regexp_replace with GROUP REFERENCES on explicit items, written on the device
// (rrx_replace_template_sizes / _fill, rrx_replace_groups_longest_*): kernels_replace_items.hip with a replacement per match.  From a
// column, a match list per item, the spans of the referenced groups per match (one PLANE of two words per slot and group) and a
// template - a short program of segments, each a literal, the match itself or a plane's span - to the new column.  Output item i =
// t[0:s_0] + R_0 + t[e_0:s_1] + R_1 + ... + R_{m-1} + t[e_{m-1}:], R_k = the segments of match k one behind the other.  No table, no
// regex: the kernels do not know where the lists and the spans came from.  The sizes walk and the fill sweep are those of the literal
// pair (replace_sweep.hpp); a template costs a walk over its segments per match (sizes) and per located byte (fill) that a fixed R
// does not need, so the literal pair keeps kernels of its own.
#include "replace_sweep.hpp"

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

// The replacement of a template: R_j from the walk.  A segment that holds the byte is a literal (a byte of `lits`) or a span of the
// item; `lim` is that segment's end.
struct TemplateReplacement {
    TemplateLds t;
    const uint8_t *__restrict__ lits;
    const uint32_t *__restrict__ match_start, *__restrict__ match_end, *__restrict__ ref_start, *__restrict__ ref_end;
    uint64_t plane_stride;
    __device__ __forceinline__ bool holds(uint64_t j, uint64_t at, uint64_t q, uint64_t item_len, bool &in_lit, uint64_t &origin, uint64_t &lim,
                                          uint64_t &len) const {
        TemplateHit hit;
        len = walk_template(t, j, item_len, match_start, match_end, ref_start, ref_end, plane_stride, q - at, &hit);
        if (!hit.found) return false;
        in_lit = hit.literal;
        origin = at + hit.delta;
        if (at + hit.end < lim) lim = at + hit.end;
        return true;
    }
    __device__ __forceinline__ uint32_t byte(uint64_t at) const { return lits[at]; }
};

// SIZES (replace_sweep.hpp: replace_sizes_walk) with the length of R_k from the walk.
__global__ __launch_bounds__(kThreads) void replace_template_sizes_kernel(TemplateDevice tpl, const uint64_t *__restrict__ off, size_t nitems, uint32_t trim,
                                                                          const uint64_t *__restrict__ first, const uint32_t *__restrict__ match_start,
                                                                          const uint32_t *__restrict__ match_end, const uint32_t *__restrict__ ref_start,
                                                                          const uint32_t *__restrict__ ref_end, uint64_t plane_stride,
                                                                          uint32_t *__restrict__ len, uint32_t *__restrict__ pos,
                                                                          uint32_t *__restrict__ too_long) {
    __shared__ uint32_t seg[3 * kTemplateMaxSegments];
    load_template(tpl, seg);
    const TemplateLds t = {seg, tpl.nseg};
    replace_sizes_walk(off, nitems, trim, first, match_start, match_end, len, pos, too_long, [&](uint64_t slot, uint64_t L) {
        return walk_template(t, slot, L, match_start, match_end, ref_start, ref_end, plane_stride, ~(uint64_t)0, nullptr);
    });
}

// FILL (replace_sweep.hpp: replace_fill_sweep).  locate has ONE LEVEL MORE than with a literal: once the slot j with the last
// pos <= r is known and d = r - pos[j], the walk over R_j's segments finds the one that holds byte d: the source is a byte of the
// literals or of the item, `lim` that segment's end; if none holds it, the byte lies behind R_j and comes from the item at
// match_end[j] + d - |R_j| (the raw end, as with a literal).  A source offset at or beyond the item's end gives 0 there; a segment's
// source lies inside the item by the walk's clamping.
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
    const TemplateReplacement R = {{seg, tpl.nseg}, tpl.lits, match_start, match_end, ref_start, ref_end, plane_stride};
    replace_fill_sweep(staged[threadIdx.x >> 6], bytes, off, nitems, trim, first, match_end, pos, R, out_off, out);
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
