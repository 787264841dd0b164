// item_columns.cpp — new columns from the matches of explicit items: regexp_replace (rrx_replace_matches_* from any match list,
// rrx_replace_all_longest_* in one call) and the list<binary> columns of regexp_extract_all and split (rrx_pieces_* from any match
// list, rrx_extract_all_longest_* / rrx_split_longest_* in one call).  A one-call entry is the leftmost-longest match list of the
// call's own (items.hpp: LongestMatchList), then the tail every sized column shares (items.hpp: SizedColumn - sizes, a second scan,
// the cap rule and the fill) around the two launches that are the column's.
#include <cstring>

#include "items.hpp"

using namespace rrx;

// The template on `device`, uploaded once (a synchronous copy: after it the two passes queue launches only), `device` made current.
// Three words per segment - kind (0 a literal, 1 the match, 2 + r plane r), the literal's offset and length - then the literals.
static_assert(kTemplateSegments == dev::kTemplateMaxSegments, "the parser's limit is what the kernels' LDS copy holds");
int rrx_template::on(int device, dev::TemplateDevice *out) const {
    std::lock_guard<std::mutex> lock(mu);
    auto it = on_device.find(device);
    if (it == on_device.end()) {
        OnDevice<dev::TemplateDevice> d;
        std::vector<uint32_t> words;
        for (const TemplateSegment &s : t.segs) {
            words.push_back(s.ref < 0 ? 0u : s.ref == 0 ? 1u : 2u + (uint32_t)t.plane_of(s.ref));
            words.push_back(s.lit_off);
            words.push_back(s.lit_len);
        }
        const size_t seg_bytes = words.size() * sizeof(uint32_t);
        hipError_t e = d.mem.alloc(device, seg_bytes + t.lits.size() + 16);
        if (e == hipSuccess && seg_bytes) e = hipMemcpy(d.mem.p, words.data(), seg_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && !t.lits.empty()) e = hipMemcpy(static_cast<uint8_t *>(d.mem.p) + seg_bytes, t.lits.data(), t.lits.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "replacement template upload");
        d.d.segs = static_cast<const uint32_t *>(d.mem.p);
        d.d.lits = static_cast<const uint8_t *>(d.mem.p) + seg_bytes;
        d.d.nseg = (uint32_t)t.segs.size();
        it = on_device.emplace(device, std::move(d)).first;
    }
    *out = it->second.d;
    HIP_TRY(hipSetDevice(device));
    return RRX_OK;
}

extern "C" {

// regexp_replace from a match list (kernels_replace_items.hip): the two passes of every CSR result.  No regex, no table, nothing
// known on the host and nothing read back.
int rrx_replace_matches_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                              const uint32_t *d_end, uint32_t rep_len, uint32_t *d_len, uint32_t *d_pos, void *stream) {
    if (nitems && (!d_off || !d_first || !d_start || !d_end || !d_len || !d_pos)) return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::replace_sizes(d_off, nitems, trim, d_first, d_start, d_end, rep_len, d_len, d_pos, nullptr, stream), "replace_sizes launch");
}
int rrx_replace_matches_fill(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first,
                             const uint32_t *d_end, const uint32_t *d_pos, const void *d_rep, uint32_t rep_len, const uint64_t *d_out_off, void *d_out,
                             void *stream) {
    if (nitems && (!d_off || !d_first || !d_end || !d_pos || !d_out_off || (rep_len && !d_rep))) return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::replace_fill(static_cast<const uint8_t *>(d_bytes), d_off, nitems, trim, d_first, d_end, d_pos, static_cast<const uint8_t *>(d_rep),
                                      rep_len, d_out_off, static_cast<uint8_t *>(d_out), stream),
                    "replace_fill launch");
}
// Every leftmost-longest match replaced, in one call: the match list, then the column's tail (items.hpp: SizedColumn) - the output
// items' lengths, their scan into d_out_off and, if the column fits `cap`, the bytes.
static int replace_all_longest_one_call(const rrx_regex *re, const ItemBatch &b, const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out,
                                        size_t cap, size_t *total, void *stream) {
    const int device = b.device;
    const size_t nitems = b.nitems;
    if (!batch_args_ok(re, b, {}) || !total || !d_out_off || (rep_len && !rep) || (nitems && cap && !d_out)) return fail(RRX_ERR_ARG, "null argument");
    *total = 0;
    int rc = search_longest_tables_on(re, device);
    if (rc) return rc;
    if (!nitems) return empty_batch({d_out_off}, stream);
    LongestMatchList m;
    rc = m.count(re, b, "hipMalloc(replace prefix)", stream);
    if (rc) return rc;
    // (one word more than the lists need: the generic kernels are never handed a null array)
    SizedColumn col("replace", "an output item of 2^30 bytes or more: use rrx_search_all_longest_extents and the two passes rrx_replace_matches_sizes / _fill");
    DeviceArray<uint32_t> d_pos;
    DeviceArray<uint8_t> d_rep;
    hipError_t he = m.alloc_lists(device);
    if (he == hipSuccess) he = d_pos.alloc(device, (m.nmatches + 1) * sizeof(uint32_t));
    if (he == hipSuccess) he = col.alloc(device, nitems, d_out_off, true, m.c.sums);          // (the first scan's scratch: the stream orders the two)
    if (he == hipSuccess && rep_len) he = d_rep.alloc(device, rep_len);
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(replace lists)");
    // (the call does not return before a synchronise: `rep` stays valid)
    if (rep_len) HIP_TRY(hipMemcpyAsync(d_rep, rep, rep_len, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = m.fill(re, b, stream);
    if (rc) return rc;
    rc = col.sizes([&](uint32_t *d_len, uint32_t *d_flag) {
        return launched(dev::replace_sizes(b.off, nitems, b.trim, m.first, m.start, m.end, rep_len, d_len, d_pos, d_flag, stream), "replace sizes and scan launch");
    }, total, stream);
    if (rc) return rc;
    return col.fill(cap, [&] {
        return launched(dev::replace_fill(b.bytes, b.off, nitems, b.trim, m.first, m.end, d_pos, d_rep, rep_len, d_out_off, static_cast<uint8_t *>(d_out), stream),
                        "replace_fill launch");
    }, stream);
}
int rrx_replace_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out, size_t cap, size_t *total, void *stream) {
    return replace_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), rep, rep_len, d_out_off, d_out, cap, total, stream);
}
int rrx_replace_all_longest_items(const rrx_regex *re, const rrx_items *it, const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out,
                                  size_t cap, size_t *total, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return replace_all_longest_one_call(re, batch_of(it), rep, rep_len, d_out_off, d_out, cap, total, stream);
}

// Replacement templates (template.cpp parses; the handle keeps what the kernels take, per device).
int rrx_template_compile(const void *rep, size_t rep_len, rrx_template **out) {
    if (!out || (rep_len && !rep)) return fail(RRX_ERR_ARG, "null argument");
    *out = nullptr;
    std::unique_ptr<rrx_template> tpl(new rrx_template());
    size_t at = 0;
    switch (parse_template(static_cast<const uint8_t *>(rep), rep_len, tpl->t, &at)) {
    case TemplateError::syntax:
        return fail(RRX_ERR_PATTERN, "replacement template: '\\' at offset " + std::to_string(at) + " is followed by neither a digit nor '\\'");
    case TemplateError::too_many_segments:
        return fail(RRX_ERR_UNSUPPORTED, "replacement template: more than " + std::to_string(kTemplateSegments) + " segments");
    case TemplateError::none:
        break;
    }
    *out = tpl.release();
    return RRX_OK;
}
void rrx_template_free(rrx_template *tpl) { delete tpl; }
size_t rrx_template_refs(const rrx_template *tpl, int *groups, size_t cap) {
    if (!tpl) return 0;
    for (size_t k = 0; groups && k < tpl->t.refs.size() && k < cap; k++) groups[k] = tpl->t.refs[k];
    return tpl->t.refs.size();
}
size_t rrx_template_segments(const rrx_template *tpl, int *refs, uint32_t *lit_lens, size_t cap, void *lits, size_t lits_cap) {
    if (!tpl) return 0;
    const auto &t = tpl->t;
    for (size_t k = 0; k < t.segs.size() && k < cap; k++) {
        if (refs) refs[k] = t.segs[k].ref;
        if (lit_lens) lit_lens[k] = t.segs[k].lit_len;
    }
    if (lits && lits_cap) std::memcpy(lits, t.lits.data(), t.lits.size() < lits_cap ? t.lits.size() : lits_cap);
    return t.segs.size();
}

// regexp_replace with group references from a match list and the references' spans (kernels_replace_template_items.hip): the two
// passes of rrx_replace_matches_*, the replacement of a match put together from the template's segments.  Asynchronous but for the
// template's first use on a device (its upload).
static bool template_refs_ok(const rrx_template *tpl, size_t nitems, const uint32_t *d_ref_start, const uint32_t *d_ref_end) {
    return tpl && (!nitems || tpl->t.refs.empty() || (d_ref_start && d_ref_end));
}
int rrx_replace_template_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                               const uint32_t *d_end, const rrx_template *tpl, const uint32_t *d_ref_start, const uint32_t *d_ref_end, size_t plane_stride,
                               uint32_t *d_len, uint32_t *d_pos, void *stream) {
    if (!template_refs_ok(tpl, nitems, d_ref_start, d_ref_end) || (nitems && (!d_off || !d_first || !d_start || !d_end || !d_len || !d_pos)))
        return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    dev::TemplateDevice t;
    const int rc = tpl->on(device, &t);
    if (rc) return rc;
    return launched(dev::replace_template_sizes(t, d_off, nitems, trim, d_first, d_start, d_end, d_ref_start, d_ref_end, plane_stride, d_len, d_pos, nullptr,
                                                stream),
                    "replace_template_sizes launch");
}
int rrx_replace_template_fill(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first,
                              const uint32_t *d_start, const uint32_t *d_end, const uint32_t *d_pos, const rrx_template *tpl, const uint32_t *d_ref_start,
                              const uint32_t *d_ref_end, size_t plane_stride, const uint64_t *d_out_off, void *d_out, void *stream) {
    if (!template_refs_ok(tpl, nitems, d_ref_start, d_ref_end) || (nitems && (!d_off || !d_first || !d_start || !d_end || !d_pos || !d_out_off)))
        return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    dev::TemplateDevice t;
    const int rc = tpl->on(device, &t);
    if (rc) return rc;
    return launched(dev::replace_template_fill(t, static_cast<const uint8_t *>(d_bytes), d_off, nitems, trim, d_first, d_start, d_end, d_pos, d_ref_start,
                                               d_ref_end, plane_stride, d_out_off, static_cast<uint8_t *>(d_out), stream),
                    "replace_template_fill launch");
}

// regexp_extract_all / split from a match list (kernels_pieces_items.hip): the pieces of every item as a list<binary> column.  The
// generic pair takes no regex, knows nothing on the host and reads nothing back.
int rrx_pieces_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint64_t *d_first, const uint32_t *d_start,
                     const uint32_t *d_end, int mode, uint64_t *d_list_off, uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream) {
    if (mode != RRX_PIECES_MATCHES && mode != RRX_PIECES_GAPS) return fail(RRX_ERR_ARG, "mode is neither RRX_PIECES_MATCHES nor RRX_PIECES_GAPS");
    if (nitems && (!d_off || !d_first || !d_start || !d_end || !d_list_off || !d_piece_len || !d_piece_src)) return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::pieces_sizes(d_off, nitems, trim, d_first, d_start, d_end, mode == RRX_PIECES_GAPS, d_list_off, d_piece_len, d_piece_src, nullptr,
                                      stream),
                    "pieces_sizes launch");
}
int rrx_pieces_fill(int device, const void *d_bytes, const uint64_t *d_piece_src, const uint64_t *d_piece_off, size_t npieces, void *d_out, void *stream) {
    if (npieces && (!d_piece_src || !d_piece_off)) return fail(RRX_ERR_ARG, "null argument");
    if (!npieces) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::pieces_fill(static_cast<const uint8_t *>(d_bytes), d_piece_src, d_piece_off, npieces, static_cast<uint8_t *>(d_out), stream),
                    "pieces_fill launch");
}
// The pieces of every leftmost-longest match list, in one call: the match list, then the column's tail (items.hpp: SizedColumn) -
// the piece lengths, their scan into the piece offsets and, if both caps hold, the bytes.  The number of pieces follows from the
// number of matches on the host.
static int pieces_all_longest_one_call(const rrx_regex *re, const ItemBatch &b, bool gaps, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap,
                                       void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream) {
    const int device = b.device;
    const size_t nitems = b.nitems;
    if (!batch_args_ok(re, b, {}) || !npieces || !total || !d_list_off || !d_piece_off || (nitems && cap && !d_out)) return fail(RRX_ERR_ARG, "null argument");
    *npieces = *total = 0;
    int rc = search_longest_tables_on(re, device);
    if (rc) return rc;
    if (!nitems) return empty_batch({d_list_off, d_piece_off}, stream);
    LongestMatchList m;
    rc = m.count(re, b, "hipMalloc(pieces prefix)", stream);
    if (rc) return rc;
    const size_t np = m.nmatches + (gaps ? nitems : 0);
    *npieces = np;
    // (one word more than the lists need: the generic kernels are never handed a null array)
    SizedColumn col("pieces", "a piece of 2^30 bytes or more: use rrx_search_all_longest_extents and the two passes rrx_pieces_sizes / _fill");
    DeviceArray<uint64_t> d_src;
    hipError_t he = m.alloc_lists(device);
    if (he == hipSuccess) he = col.alloc(device, np, d_piece_off, np <= pieces_cap);
    if (he == hipSuccess) he = d_src.alloc(device, (np + 1) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(pieces lists)");
    rc = m.fill(re, b, stream);
    if (rc) return rc;
    rc = col.sizes([&](uint32_t *d_len, uint32_t *d_flag) {
        return launched(dev::pieces_sizes(b.off, nitems, b.trim, m.first, m.start, m.end, gaps, d_list_off, d_len, d_src, d_flag, stream), "pieces sizes and scan launch");
    }, total, stream);
    if (rc) return rc;
    return col.fill(cap, [&] { return launched(dev::pieces_fill(b.bytes, d_src, col.off, np, static_cast<uint8_t *>(d_out), stream), "pieces_fill launch"); }, stream);
}
int rrx_extract_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces, size_t *total,
                                    void *stream) {
    return pieces_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), false, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total,
                                       stream);
}
int rrx_extract_all_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out,
                                  size_t cap, size_t *npieces, size_t *total, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(it), false, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total, stream);
}
int rrx_split_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, uint64_t *d_list_off,
                              uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream) {
    return pieces_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), true, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total,
                                       stream);
}
int rrx_split_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap,
                            size_t *npieces, size_t *total, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(it), true, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total, stream);
}

}  // extern "C"
