// group.cpp — rrx_group: a pattern A(B)C split at one top-level capture group (frontend.hpp: split_group), its four anchored tables,
// and the entries that turn the leftmost-longest match of every item into the group's span (rrx_group_spans_* /
// rrx_extract_group_longest_*): the longest split point (kernels_group_items.hip), launched once per part that is there.  Also
// the same for every match of a match list (rrx_group_spans_list_*) and regexp_replace with group references in one call
// (rrx_replace_groups_longest_*), which needs the handles' insides.
#include <cstring>

#include "items.hpp"

using namespace rrx;

// The whole pattern as an ordinary regex, the parts' source text, and the tables: a and rev_bc where A is there, rev_c where C is, b
// always (an absent part's launch is skipped, its tables stay empty).  Everything a device entry could refuse for is settled at compile.
struct rrx_group {
    rrx_regex *whole = nullptr;
    std::string text[3];                                 // A, B, C
    bool has_a = false, has_c = false;
    bool empty = false;                                  // the empty language: no match anywhere, no table
    DfaProgram a, rev_bc, b, rev_c;
    mutable std::mutex mu;
    mutable std::map<int, OnDevice<dev::GroupDevice>> on_device;      // (under `mu`)
    ~rrx_group() { delete whole; }
    bool in_global() const { return whole->requested == RRX_ENGINE_DFA_GLOBAL; }
    // The tables on `device`, uploaded once
    int tables(int device, const dev::GroupDevice **out) const {
        std::lock_guard<std::mutex> lock(mu);
        auto it = on_device.find(device);
        if (it == on_device.end()) {
            Image img;
            OnDevice<dev::GroupDevice> t;
            if (!pack_group(a, rev_bc, b, rev_c, img, t.d)) return fail(RRX_ERR_UNSUPPORTED, "group tables: row 0 of a table is not its dead row");
            const hipError_t e = upload(device, img, t.mem);
            if (e != hipSuccess) return hip_fail(e, "device table upload");
            it = on_device.emplace(device, std::move(t)).first;
        }
        *out = &it->second.d;
        return RRX_OK;
    }
};

namespace {

const char *const kGroupArgError = "null argument, or marks_words below nitems + 1";
// d_marks may be null only where no launch needs it: both A and C absent
bool group_args_ok(const rrx_group *g, const ItemBatch &b, ItemMarks m, const uint32_t *d_start, const uint32_t *d_end) {
    return batch_args_ok(g, b, {d_start, d_end}) && ((!g->has_a && !g->has_c) || marks_ok(b.nitems, m));
}

// From the spans in (in_start, in_end) to the group's spans in (d_start, d_end); the two pairs may be the same arrays.
//   A there:  launch 1 on (reverse (B)C, A) over [s, e] -> i into d_start            A absent:  i = s, a copy
//   C there:  launch 2 on (reverse C, B) over [i, e]    -> j into d_end              C absent:  j = e, a copy
// An item without a split gets ~0u in the launch's own array and, through on_none, in the other one; launch 2 passes an item on
// whose start is ~0u.  The copies come first: launch 1 reads e from in_end and may write ~0u into d_end.
int group_spans(const rrx_group *g, const ItemBatch &b, const uint32_t *in_start, const uint32_t *in_end, ItemMarks m, uint32_t *d_start, uint32_t *d_end,
                void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    hipStream_t st = (hipStream_t)stream;
    if (!nitems) return RRX_OK;                          // (nothing to refuse an empty batch for: compile has settled the tables)
    const dev::GroupDevice *t = nullptr;
    if (!g->empty) {
        const int rc = g->tables(device, &t);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(device));
    if (g->empty) {
        HIP_TRY(hipMemsetAsync(d_start, 0xff, nitems * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(d_end, 0xff, nitems * sizeof(uint32_t), st));
        return RRX_OK;
    }
    if (!g->has_a && d_start != in_start) HIP_TRY(hipMemcpyAsync(d_start, in_start, nitems * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (!g->has_c && d_end != in_end) HIP_TRY(hipMemcpyAsync(d_end, in_end, nitems * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (g->has_a) {
        const int rc = launched(dev::longest_split_dfa(t->rev_bc, t->a, g->in_global(), bytes, off, nitems, trim, in_start, in_end, m.words, m.nwords, d_start,
                                                       d_end, stream),
                                "group split (A | BC) launch");
        if (rc) return rc;
    }
    if (g->has_c) {
        const uint32_t *lo = g->has_a ? d_start : in_start;
        const int rc = launched(dev::longest_split_dfa(t->rev_c, t->b, g->in_global(), bytes, off, nitems, trim, lo, in_end, m.words, m.nwords, d_end, d_start,
                                                       stream),
                                "group split (B | C) launch");
        if (rc) return rc;
    }
    return RRX_OK;
}

// group_spans for every match of a match list: the arrays are indexed by the slot, the slot range d_first[0] .. d_first[nitems] is
// known on the device only - an absent part's copy and the empty language's fill are a small kernel over it, not a memcpy.
int group_spans_list(const rrx_group *g, const ItemBatch &b, const uint64_t *d_first, const uint32_t *in_start, const uint32_t *in_end, ItemMarks m,
                     uint32_t *d_start, uint32_t *d_end, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    if (!nitems) return RRX_OK;
    const dev::GroupDevice *t = nullptr;
    if (!g->empty) {
        const int rc = g->tables(device, &t);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(device));
    if (g->empty) return launched(dev::slot_range_copy(d_first, nitems, nullptr, d_start, nullptr, d_end, stream), "group list fill launch");
    {
        uint32_t *copy_start = !g->has_a && d_start != in_start ? d_start : nullptr, *copy_end = !g->has_c && d_end != in_end ? d_end : nullptr;
        const int rc = launched(dev::slot_range_copy(d_first, nitems, in_start, copy_start, in_end, copy_end, stream), "group list copy launch");
        if (rc) return rc;
    }
    if (g->has_a) {
        const int rc = launched(dev::longest_split_list_dfa(t->rev_bc, t->a, g->in_global(), bytes, off, nitems, trim, d_first, in_start, in_end, m.words,
                                                            m.nwords, d_start, d_end, stream),
                                "group list split (A | BC) launch");
        if (rc) return rc;
    }
    if (g->has_c) {
        const uint32_t *lo = g->has_a ? d_start : in_start;
        const int rc = launched(dev::longest_split_list_dfa(t->rev_c, t->b, g->in_global(), bytes, off, nitems, trim, d_first, lo, in_end, m.words, m.nwords,
                                                            d_end, d_start, stream),
                                "group list split (B | C) launch");
        if (rc) return rc;
    }
    return RRX_OK;
}

// rrx_search_longest_* on the whole pattern into the group arrays, then the launches in place
int group_extract(const rrx_group *g, const ItemBatch &b, ItemMarks m, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!b.nitems) return RRX_OK;
    const int rc = rrx_search_longest_extents(g->whole, b.device, b.bytes, b.off, b.nitems, b.trim, d_start, d_end, stream);
    if (rc || g->empty) return rc;          // (the empty language: the search has filled both arrays)
    return group_spans(g, b, d_start, d_end, m, d_start, d_end, stream);
}


// regexp_replace with group references in one call: rrx_replace_all_longest_*'s steps with the spans of the referenced groups between
// the match list and the column's tail (items.hpp: SizedColumn) - one plane per referenced group, each from its own handle - and the
// template's two passes in place of the literal ones.  groups[g - 1]: the handle of group g of ONE pattern; the first one there is searches.
int replace_groups_one_call(const rrx_group *const *groups, size_t ngroups, const rrx_template *tpl, const ItemBatch &b, uint64_t *d_out_off, void *d_out,
                            size_t cap, size_t *total, void *stream) {
    const int device = b.device;
    const size_t nitems = b.nitems;
    if (!groups || !tpl || !total || !d_out_off || (nitems && (!b.off || (cap && !d_out)))) return fail(RRX_ERR_ARG, "null argument");
    const rrx_group *lead = nullptr;
    for (size_t k = 0; k < ngroups; k++) {
        if (!groups[k]) continue;
        if (!lead) lead = groups[k];
        else if (groups[k]->whole->pattern != lead->whole->pattern) return fail(RRX_ERR_ARG, "the group handles are not of one pattern");
    }
    if (!lead) return fail(RRX_ERR_ARG, "no group handle");
    for (int ref : tpl->t.refs)
        if ((size_t)ref > ngroups || !groups[ref - 1]) return fail(RRX_ERR_ARG, "the template references group " + std::to_string(ref) + ", which has no handle");
    const rrx_regex *re = lead->whole;
    *total = 0;
    int rc = search_longest_tables_on(re, device);
    if (rc) return rc;
    if (!nitems) return empty_batch({d_out_off}, stream);
    dev::TemplateDevice t;
    rc = tpl->on(device, &t);
    if (rc) return rc;
    LongestMatchList m;
    rc = m.count(re, b, "hipMalloc(replace prefix)", stream);
    if (rc) return rc;
    // (one word more than the lists need: the generic kernels are never handed a null array)
    const size_t nplanes = tpl->t.refs.size(), stride = m.nmatches;
    SizedColumn col("replace", "an output item of 2^30 bytes or more: use rrx_search_all_longest_extents, rrx_group_spans_list_extents and the two passes rrx_replace_template_sizes / _fill");
    DeviceArray<uint32_t> d_pos, d_ref_start, d_ref_end;
    hipError_t he = m.alloc_lists(device);
    if (he == hipSuccess) he = d_pos.alloc(device, (m.nmatches + 1) * sizeof(uint32_t));
    if (he == hipSuccess) he = col.alloc(device, nitems, d_out_off, true, m.c.sums);          // (the first scan's scratch: the stream orders the two)
    if (he == hipSuccess) he = d_ref_start.alloc(device, (nplanes * stride + 1) * sizeof(uint32_t));
    if (he == hipSuccess) he = d_ref_end.alloc(device, (nplanes * stride + 1) * sizeof(uint32_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(replace lists)");
    rc = m.fill(re, b, stream);
    if (rc) return rc;
    // the marks of the count pass have served the fill: the planes' launches take the buffer over, one after the other on the stream
    for (size_t r = 0; r < nplanes && m.nmatches; r++) {
        rc = group_spans_list(groups[tpl->t.refs[r] - 1], b, m.first, m.start, m.end, {m.c.marks, m.c.nwords}, d_ref_start + r * stride, d_ref_end + r * stride,
                              stream);
        if (rc) return rc;
    }
    rc = col.sizes([&](uint32_t *d_len, uint32_t *d_flag) {
        return launched(dev::replace_template_sizes(t, b.off, nitems, b.trim, m.first, m.start, m.end, d_ref_start, d_ref_end, stride, d_len, d_pos, d_flag, stream),
                        "replace sizes and scan launch");
    }, total, stream);
    if (rc) return rc;
    return col.fill(cap, [&] {
        return launched(dev::replace_template_fill(t, b.bytes, b.off, nitems, b.trim, m.first, m.start, m.end, d_pos, d_ref_start, d_ref_end, stride, d_out_off,
                                                   static_cast<uint8_t *>(d_out), stream),
                        "replace_template_fill launch");
    }, stream);
}

}  // namespace

extern "C" {

int rrx_group_compile_ex(const char *pattern, int group, int engine, rrx_group **out) {
    if (!pattern || !out) return fail(RRX_ERR_ARG, "null argument");
    *out = nullptr;
    if (group <= 0) return fail(RRX_ERR_ARG, "group numbers start at 1");
    rrx_regex *whole = nullptr;
    const int rc = rrx_compile_ex(pattern, engine, &whole);                   // (RRX_ERR_PATTERN, an unknown engine, an automaton no engine takes)
    if (rc) return rc;
    std::unique_ptr<rrx_group> g(new rrx_group());
    g->whole = whole;
    try {
        GroupSplit s = split_group(whole->pattern, group);
        for (int k = 0; k < 3; k++) g->text[k] = s.text[k];
        g->has_a = s.has_a;
        g->has_c = s.has_c;
        {
            std::lock_guard<std::mutex> lock(whole->mu);
            const int lrc = whole->build_search_longest();
            if (lrc) return lrc;
            g->empty = whole->search_longest.empty;
        }
        auto reduced = [](const RefAutomaton &a) { return reduce(trim(a)); };
        bool ok = true;
        if (s.has_a) ok = lower_dfa(reduced(s.a), kMaxSubsetStates, g->a) && lower_dfa_reversed(reduced(s.bc), kMaxSubsetStates, g->rev_bc);
        if (ok && s.has_c) ok = lower_dfa(reduced(s.b), kMaxSubsetStates, g->b) && lower_dfa_reversed(reduced(s.c), kMaxSubsetStates, g->rev_c);
        if (ok && !s.has_c) ok = lower_dfa(reduced(s.b), kMaxSubsetStates, g->b);      // (not launched: kept for rrx_group_program_words' B)
        if (!ok) return fail(RRX_ERR_UNSUPPORTED, "a table of the split pattern (A, B, or the reverse of (B)C or C) does not determinise within the state budget");
    } catch (const GroupArgError &e) {
        return fail(RRX_ERR_ARG, e.what());
    } catch (const GroupUnsupported &e) {
        return fail(RRX_ERR_UNSUPPORTED, e.what());
    } catch (const PatternError &e) {
        return fail(RRX_ERR_PATTERN, e.what());
    } catch (const BudgetError &e) {
        return fail(RRX_ERR_UNSUPPORTED, e.what());
    } catch (const std::exception &e) {
        return fail(RRX_ERR_PATTERN, std::string("internal: ") + e.what());
    }
    *out = g.release();
    return RRX_OK;
}
int rrx_group_compile(const char *pattern, int group, rrx_group **out) { return rrx_group_compile_ex(pattern, group, RRX_ENGINE_AUTO, out); }
void rrx_group_free(rrx_group *grp) { delete grp; }
const rrx_regex *rrx_group_regex(const rrx_group *grp) { return grp ? grp->whole : nullptr; }

size_t rrx_group_part(const rrx_group *grp, int which, char *buf, size_t cap) {
    if (!grp || which < 0 || which > 2) return 0;
    const std::string &s = grp->text[which];
    if (buf && cap) std::memcpy(buf, s.data(), s.size() < cap ? s.size() : cap);
    return s.size();
}
size_t rrx_group_program_words(const rrx_group *grp, int which, uint32_t *out, size_t cap) {
    if (!grp) return 0;
    const DfaProgram *p = which == RRX_PROGRAM_GROUP_A ? &grp->a : which == RRX_PROGRAM_GROUP_REV_BC ? &grp->rev_bc
                          : which == RRX_PROGRAM_GROUP_B ? &grp->b : which == RRX_PROGRAM_GROUP_REV_C ? &grp->rev_c : nullptr;
    std::vector<uint32_t> w;
    if (p && p->nstates) append_words(w, *p);
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    return w.size();
}

int rrx_group_spans_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                            const uint32_t *d_match_start, const uint32_t *d_match_end, uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start,
                            uint32_t *d_group_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!group_args_ok(grp, b, {d_marks, marks_words}, d_group_start, d_group_end) || !batch_args_ok(grp, b, {d_match_start, d_match_end}))
        return fail(RRX_ERR_ARG, kGroupArgError);
    return group_spans(grp, b, d_match_start, d_match_end, {d_marks, marks_words}, d_group_start, d_group_end, stream);
}
int rrx_group_spans_items(const rrx_group *grp, const rrx_items *it, const uint32_t *d_match_start, const uint32_t *d_match_end, uint32_t *d_marks,
                          size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, kGroupArgError);
    return rrx_group_spans_extents(grp, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_match_start, d_match_end, d_marks, marks_words, d_group_start,
                                   d_group_end, stream);
}
int rrx_group_spans_list_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                 const uint64_t *d_first, const uint32_t *d_match_start, const uint32_t *d_match_end, uint32_t *d_marks, size_t marks_words,
                                 uint32_t *d_group_start, uint32_t *d_group_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!group_args_ok(grp, b, {d_marks, marks_words}, d_group_start, d_group_end) || !batch_args_ok(grp, b, {d_first, d_match_start, d_match_end}))
        return fail(RRX_ERR_ARG, kGroupArgError);
    return group_spans_list(grp, b, d_first, d_match_start, d_match_end, {d_marks, marks_words}, d_group_start, d_group_end, stream);
}
int rrx_group_spans_list_items(const rrx_group *grp, const rrx_items *it, const uint64_t *d_first, const uint32_t *d_match_start,
                               const uint32_t *d_match_end, uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end,
                               void *stream) {
    if (!it) return fail(RRX_ERR_ARG, kGroupArgError);
    return rrx_group_spans_list_extents(grp, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_first, d_match_start, d_match_end, d_marks,
                                        marks_words, d_group_start, d_group_end, stream);
}
int rrx_replace_groups_longest_extents(const rrx_group *const *groups, size_t ngroups, const rrx_template *tpl, int device, const void *d_bytes,
                                       const uint64_t *d_off, size_t nitems, uint32_t trim, uint64_t *d_out_off, void *d_out, size_t cap, size_t *total,
                                       void *stream) {
    return replace_groups_one_call(groups, ngroups, tpl, batch_of(device, d_bytes, d_off, nitems, trim), d_out_off, d_out, cap, total, stream);
}
int rrx_replace_groups_longest_items(const rrx_group *const *groups, size_t ngroups, const rrx_template *tpl, const rrx_items *it, uint64_t *d_out_off,
                                     void *d_out, size_t cap, size_t *total, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return replace_groups_one_call(groups, ngroups, tpl, batch_of(it), d_out_off, d_out, cap, total, stream);
}
int rrx_extract_group_longest_extents(const rrx_group *grp, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                      uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start, uint32_t *d_group_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!group_args_ok(grp, b, {d_marks, marks_words}, d_group_start, d_group_end)) return fail(RRX_ERR_ARG, kGroupArgError);
    return group_extract(grp, b, {d_marks, marks_words}, d_group_start, d_group_end, stream);
}
int rrx_extract_group_longest_items(const rrx_group *grp, const rrx_items *it, uint32_t *d_marks, size_t marks_words, uint32_t *d_group_start,
                                    uint32_t *d_group_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, kGroupArgError);
    return rrx_extract_group_longest_extents(grp, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_marks, marks_words, d_group_start, d_group_end,
                                             stream);
}

}  // extern "C"
