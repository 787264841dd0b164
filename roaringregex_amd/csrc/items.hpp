// items.hpp — what the units of the explicit-items entries share (items.cpp, item_search.cpp, item_columns.cpp, group.cpp; the scan
// step also search.cpp): the batch as every lane-per-item path takes it, the argument check of an entry on a batch, the two
// read-backs of the one-call entries, the tables step, and the leftmost-longest match list of a call's own.
#pragma once
#include <initializer_list>

#include "handles.hpp"

// A batch of items as the lane-per-item paths take it: the raw arguments of an _extents entry, or an rrx_items without its index.
struct ItemBatch { int device; const uint8_t *bytes; const uint64_t *off; size_t nitems; uint32_t trim; };
inline ItemBatch batch_of(int device, const void *d_bytes, const uint64_t *d_off, size_t n, uint32_t trim) { return {device, static_cast<const uint8_t *>(d_bytes), d_off, n, trim}; }
inline ItemBatch batch_of(const rrx_items *it) { return {it->device, it->d_bytes, it->d_off, it->nitems, it->trim}; }
// The mark words of the leftmost-longest kernels (device.hpp: search_all_longest_marks_words)
struct ItemMarks { uint32_t *words; size_t nwords; };
// The marks of a batch of nitems items take a word per item at the very least, whatever the extent: a shorter buffer cannot be meant
inline bool marks_ok(size_t nitems, ItemMarks m) { return !nitems || (m.words && m.nwords >= nitems + 1); }

// What an entry asks of its arguments before anything else: its handle and, for a batch that has items, the offsets and every array
// of `arrays`.  (An _items entry checks `it` first: rrx_items_create has refused a batch with items and no offsets.)
inline bool batch_args_ok(const void *handle, const ItemBatch &b, std::initializer_list<const void *> arrays) {
    if (!handle || (b.nitems && !b.off)) return false;
    for (const void *p : arrays) if (b.nitems && !p) return false;
    return true;
}

// off[0] and off[nitems] of a batch read back on `stream`: one synchronise.  `what`: the error texts of the two copies and the wait.
inline int read_offset_ends(const uint64_t *d_off, size_t nitems, void *stream, const char *const (&what)[3], uint64_t *first, uint64_t *last) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(first, d_off, sizeof *first, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(e, what[0]);
    e = hipMemcpyAsync(last, d_off + nitems, sizeof *last, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(e, what[1]);
    e = hipStreamSynchronize(st);
    return e == hipSuccess ? RRX_OK : hip_fail(e, what[2]);
}

// The scan step of a one-call entry: the exclusive prefix of n counts into d_prefix (n + 1 entries, d_prefix[n] = the total) on the
// scratch d_sums (scan_scratch_words(n)), entry 0 zeroed, the total read back - together with the device word d_flag where there is
// one - and ONE synchronise.  `launch_text`, `text`: the error texts of the launch and of what follows it.
inline int scan_total(const uint32_t *d_count, uint64_t *d_prefix, uint64_t *d_sums, size_t n, void *stream, const char *launch_text, const char *text,
                      uint64_t *total, const uint32_t *d_flag = nullptr, uint32_t *flag = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    const int le = rrx::dev::scan_counts(d_count, d_prefix, d_sums, n, stream);
    if (le) return hip_fail((hipError_t)le, launch_text);
    hipError_t he = hipMemsetAsync(d_prefix, 0, sizeof(uint64_t), st);          // the scan marks entry 0 as a stripe start: not here
    if (he == hipSuccess) he = hipMemcpyAsync(total, d_prefix + n, sizeof *total, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && d_flag) he = hipMemcpyAsync(flag, d_flag, sizeof *flag, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    return he == hipSuccess ? RRX_OK : hip_fail(he, text);
}

// The tables of one of a regex' searches on `device` (`tables`: rrx_regex::search_item_tables, ::search_longest_tables ...), uploaded
// at their first use, and `device` made current: what every entry of that search begins with, on an empty batch too - a regex
// without the tables is reported for it as well.  *t = nullptr: the search needs no table for this pattern.
template <class T> int tables_on(const rrx_regex *re, int device, int (rrx_regex::*tables)(int, const T **) const, const T **t) {
    const int rc = (re->*tables)(device, t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return RRX_OK;
}

// ---- item_search.cpp, for the columns built on leftmost-longest match lists (item_columns.cpp)
// The tables step of the leftmost-longest search
int search_longest_tables_on(const rrx_regex *re, int device);
// The counts of a one-call entry, the marks of the count pass and the scan's scratch, in device memory of the call's own (freed
// when it leaves: hipFree waits for what is queued; calls share nothing)
struct MatchCounts {
    DeviceArray<uint32_t> count, marks;
    DeviceArray<uint64_t> sums;                  // scan_scratch_words(nitems): free again once the call has synchronised
    size_t nwords = 0;
};
// The leftmost-longest match list of a batch in memory of the call's own.  count(): the prefix (nitems + 1 entries), the counts,
// the marks - sized from the batch's real extent: off[0] and off[nitems] are read back - and the scan; leaves nmatches, one
// synchronise (nitems > 0, the tables checked by the caller).  alloc_lists(): start and end, one word more than the list needs -
// the generic kernels are never handed a null array.  fill(): the matches on the marks that count() left, no launch where there
// is none.
struct LongestMatchList {
    MatchCounts c;
    DeviceArray<uint64_t> first;
    DeviceArray<uint32_t> start, end;
    size_t nmatches = 0;
    int count(const rrx_regex *re, const ItemBatch &b, const char *prefix_alloc_text, void *stream);
    hipError_t alloc_lists(int device);
    int fill(const rrx_regex *re, const ItemBatch &b, void *stream);
};
