// item_search.cpp — WHERE the matches of explicit items are, a lane per item: the first match (rrx_search_extents / _items), the
// leftmost-longest one (rrx_search_longest_*), all matches (rrx_search_all_extents* / _items*) and all leftmost-longest matches
// (rrx_search_all_longest_*), the last two as a _count / _fill pair and as one call.  Nothing is known on the host and - but for the
// one-call entries - nothing read back: the kernels take every extent from the offsets.
#include "items.hpp"

using namespace rrx;

int search_longest_tables_on(const rrx_regex *re, int device) {
    const dev::SearchLongestDevice *t;
    return tables_on(re, device, &rrx_regex::search_longest_tables, &t);
}

namespace {

const char *const kMarksError = "null argument, or marks_words below nitems + 1";

// The first match of every item (rrx_search_corpus for explicit items), on the two plain search tables.  A pattern that accepts the
// empty string matches [0, 0) in every item: two fills, no table.  An empty batch still reports a regex without search tables.
int search_lanes(const rrx_regex *re, const ItemBatch &b, uint32_t *d_start, uint32_t *d_end, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchItemsDevice *t;
    const int rc = tables_on(re, device, &rrx_regex::search_item_tables, &t);
    if (rc || !nitems) return rc;
    if (!t) {
        HIP_TRY(hipMemsetAsync(d_start, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, bytes, off, nitems, trim, d_start, d_end, stream),
                    "search_extents launch");
}

// The LEFTMOST-LONGEST match of every item, on the starts table (backwards over the whole item: the smallest start) and the
// anchored table (forwards from there: the largest end).  The empty language matches nowhere: two fills, no table.  A pattern that
// accepts the empty string starts at 0 everywhere and runs the forward pass alone.  (No tables: they do not determinise.)
int search_longest_lanes(const rrx_regex *re, const ItemBatch &b, uint32_t *d_start, uint32_t *d_end, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchLongestDevice *t;
    const int rc = tables_on(re, device, &rrx_regex::search_longest_tables, &t);
    if (rc || !nitems) return rc;
    if (!t) {
        HIP_TRY(hipMemsetAsync(d_start, 0xff, nitems * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0xff, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_longest_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, re->search_longest.nullable, bytes, off, nitems, trim,
                                                    d_start, d_end, stream),
                    "search_longest_extents launch");
}

// EVERY match of every item (rrx_search_all* for explicit items): search_lanes' tables and kernel shape, the search applied again
// to the rest of the item behind each match.  d_first == nullptr: the counts; otherwise the matches into the slots behind
// d_first[i], those below `cap`.  A pattern that accepts the empty string has the matches [k, k) for k = 0 .. length: no table, no
// text.  (No marks: the argument is there for the one-call body, which takes either family's lanes.)
int search_all_lanes(const rrx_regex *re, const ItemBatch &b, ItemMarks, uint32_t *d_count, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                     size_t cap, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchItemsDevice *t;
    const int rc = tables_on(re, device, &rrx_regex::search_item_tables, &t);
    if (rc || !nitems) return rc;
    if (!t) return launched(dev::empty_item_matches(off, nitems, trim, d_count, d_first, d_start, d_end, cap, stream), "empty_item_matches launch");
    return launched(dev::search_all_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, bytes, off, nitems, trim, d_count, d_first, d_start, d_end,
                                                cap, stream),
                    "search_all_extents launch");
}

// EVERY LEFTMOST-LONGEST match of every item: search_longest_lanes' tables, the search applied again to the rest of the item behind
// each match.  d_first == nullptr: the marks and the counts; otherwise the matches into the slots behind d_first[i], those below
// `cap`, on the marks the count pass left.  The empty language matches nowhere: the counts are a fill, there is no table and no
// text pass.  (No tables: they do not determinise.)
int search_all_longest_lanes(const rrx_regex *re, const ItemBatch &b, ItemMarks marks, uint32_t *d_count, const uint64_t *d_first, uint32_t *d_start,
                             uint32_t *d_end, size_t cap, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchLongestDevice *t;
    const int rc = tables_on(re, device, &rrx_regex::search_longest_tables, &t);
    if (rc || !nitems) return rc;
    if (!t) {
        if (!d_first) HIP_TRY(hipMemsetAsync(d_count, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_all_longest_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, re->search_longest.nullable, bytes, off, nitems, trim,
                                                        marks.words, marks.nwords, d_count, d_first, d_start, d_end, cap, stream),
                    "search_all_longest_extents launch");
}

// The two families of "all matches": their lanes, their tables step, whether they keep marks, their word in the error texts
struct AllMatches {
    const char *word;
    bool marks;
    int (*tables)(const rrx_regex *, int device);
    int (*lanes)(const rrx_regex *, const ItemBatch &, ItemMarks, uint32_t *, const uint64_t *, uint32_t *, uint32_t *, size_t, void *);
};
int search_tables_on(const rrx_regex *re, int device) {
    const dev::SearchItemsDevice *t;
    return tables_on(re, device, &rrx_regex::search_item_tables, &t);
}
const AllMatches kAll = {"search_all", false, search_tables_on, search_all_lanes};
const AllMatches kAllLongest = {"search_all_longest", true, search_longest_tables_on, search_all_longest_lanes};

// count + scan of one call.  A family with marks sizes them from the batch's real extent: off[0] and off[nitems] are read back.
// Leaves d_first complete (nitems + 1 entries, entry 0 = 0) and *total = d_first[nitems]; nitems > 0, the tables checked by the
// caller.
int count_scan(const AllMatches &f, const rrx_regex *re, const ItemBatch &b, MatchCounts &c, uint64_t *d_first, size_t *total, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const std::string word = f.word;
    if (f.marks) {
        static const char *const what[3] = {"hipMemcpyAsync(&lo, off, sizeof lo, hipMemcpyDeviceToHost, st)",
                                            "hipMemcpyAsync(&hi, off + nitems, sizeof hi, hipMemcpyDeviceToHost, st)", "hipStreamSynchronize(st)"};
        uint64_t lo = 0, hi = 0;
        const int rc = read_offset_ends(off, nitems, stream, what, &lo, &hi);
        if (rc) return rc;
        c.nwords = rrx_search_all_longest_marks_words(hi > lo ? (size_t)(hi - lo) : 0, nitems);
    }
    hipError_t he = c.count.alloc(device, nitems * sizeof(uint32_t));
    if (he == hipSuccess && f.marks) he = c.marks.alloc(device, c.nwords * sizeof(uint32_t));
    if (he == hipSuccess) he = c.sums.alloc(device, dev::scan_scratch_words(nitems) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, ("hipMalloc(" + word + (f.marks ? " counts and marks)" : " counts)")).c_str());
    const int rc = f.lanes(re, b, {c.marks, c.nwords}, c.count, nullptr, nullptr, nullptr, 0, stream);
    if (rc) return rc;
    uint64_t tot = 0;
    const int src = scan_total(c.count, d_first, c.sums, nitems, stream, (word + " scan launch").c_str(), (word + " scan").c_str(), &tot);
    if (!src) *total = (size_t)tot;
    return src;
}

// count + scan + fill in one call
int all_one_call(const AllMatches &f, const rrx_regex *re, const ItemBatch &b, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total,
                 void *stream) {
    *total = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = f.tables(re, b.device);
    if (rc) return rc;
    if (!b.nitems) return empty_batch({d_first}, stream);
    MatchCounts c;
    rc = count_scan(f, re, b, c, d_first, total, stream);
    if (rc) return rc;
    if (*total && cap) {                                                         // matches in slots >= cap are counted, not written
        rc = f.lanes(re, b, {c.marks, c.nwords}, nullptr, d_first, d_start, d_end, cap, stream);
        if (!rc) { const hipError_t he = hipStreamSynchronize(st); if (he != hipSuccess) rc = hip_fail(he, (std::string(f.word) + " fill").c_str()); }
    }
    return rc;
}
bool one_call_args_ok(const rrx_regex *re, const ItemBatch &b, const uint64_t *d_first, const uint32_t *d_start, const uint32_t *d_end, size_t cap,
                      const size_t *total) {
    return re && total && d_first && !(b.nitems && (!b.off || (cap && (!d_start || !d_end))));
}

}  // namespace

int LongestMatchList::count(const rrx_regex *re, const ItemBatch &b, const char *prefix_alloc_text, void *stream) {
    const hipError_t he = first.alloc(b.device, (b.nitems + 1) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, prefix_alloc_text);
    return count_scan(kAllLongest, re, b, c, first, &nmatches, stream);
}
hipError_t LongestMatchList::alloc_lists(int device) {
    const hipError_t he = start.alloc(device, (nmatches + 1) * sizeof(uint32_t));
    return he == hipSuccess ? end.alloc(device, (nmatches + 1) * sizeof(uint32_t)) : he;
}
int LongestMatchList::fill(const rrx_regex *re, const ItemBatch &b, void *stream) {
    return nmatches ? search_all_longest_lanes(re, b, {c.marks, c.nwords}, nullptr, first, start, end, nmatches, stream) : RRX_OK;
}

extern "C" {

int rrx_search_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                       uint32_t *d_start, uint32_t *d_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(re, b, {d_start, d_end})) return fail(RRX_ERR_ARG, "null argument");
    return search_lanes(re, b, d_start, d_end, stream);
}
int rrx_search_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_extents(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_start, d_end, stream);
}

int rrx_search_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                               uint32_t *d_start, uint32_t *d_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(re, b, {d_start, d_end})) return fail(RRX_ERR_ARG, "null argument");
    return search_longest_lanes(re, b, d_start, d_end, stream);
}
int rrx_search_longest_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_longest_extents(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_start, d_end, stream);
}

int rrx_search_all_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                 uint32_t *d_count, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(re, b, {d_count})) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, b, {}, d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_items_count(const rrx_regex *re, const rrx_items *it, uint32_t *d_count, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_all_extents_count(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_count, stream);
}
int rrx_search_all_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(re, b, {d_first, d_start, d_end})) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, b, {}, nullptr, d_first, d_start, d_end, ~(size_t)0, stream);
}
int rrx_search_all_items_fill(const rrx_regex *re, const rrx_items *it, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_all_extents_fill(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_first, d_start, d_end, stream);
}
int rrx_search_all_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                           uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!one_call_args_ok(re, b, d_first, d_start, d_end, cap, total)) return fail(RRX_ERR_ARG, "null argument");
    return all_one_call(kAll, re, b, d_first, d_start, d_end, cap, total, stream);
}
int rrx_search_all_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total,
                         void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_all_extents(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_first, d_start, d_end, cap, total, stream);
}

size_t rrx_search_all_longest_marks_words(size_t extent_bytes, size_t nitems) { return dev::search_all_longest_marks_words(extent_bytes, nitems); }
int rrx_search_all_longest_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                         uint32_t *d_marks, size_t marks_words, uint32_t *d_count, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!batch_args_ok(re, b, {d_count}) || !marks_ok(nitems, {d_marks, marks_words})) return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, b, {d_marks, marks_words}, d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_longest_items_count(const rrx_regex *re, const rrx_items *it, uint32_t *d_marks, size_t marks_words, uint32_t *d_count, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, kMarksError);
    return rrx_search_all_longest_extents_count(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_marks, marks_words, d_count, stream);
}
int rrx_search_all_longest_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                        const uint32_t *d_marks, size_t marks_words, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                                        void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    const ItemMarks marks = {const_cast<uint32_t *>(d_marks), marks_words};      // (the fill kernel only reads the marks)
    if (!batch_args_ok(re, b, {d_first, d_start, d_end}) || !marks_ok(nitems, marks)) return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, b, marks, nullptr, d_first, d_start, d_end, ~(size_t)0, stream);
}
int rrx_search_all_longest_items_fill(const rrx_regex *re, const rrx_items *it, const uint32_t *d_marks, size_t marks_words, const uint64_t *d_first,
                                      uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, kMarksError);
    return rrx_search_all_longest_extents_fill(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_marks, marks_words, d_first, d_start, d_end,
                                               stream);
}
int rrx_search_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                   uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    if (!one_call_args_ok(re, b, d_first, d_start, d_end, cap, total)) return fail(RRX_ERR_ARG, "null argument");
    return all_one_call(kAllLongest, re, b, d_first, d_start, d_end, cap, total, stream);
}
int rrx_search_all_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                                 size_t *total, void *stream) {
    if (!it) return fail(RRX_ERR_ARG, "null argument");
    return rrx_search_all_longest_extents(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_first, d_start, d_end, cap, total, stream);
}

}  // extern "C"
