// items.hpp — what the units of the explicit-items entries share (items.cpp, item_search.cpp, item_columns.cpp, group.cpp, filter.cpp;
// the scan step and the empty-batch answer also search.cpp): the batch as every lane-per-item path takes it, the argument check of an
// entry on a batch, the two read-backs of the one-call entries, the tail of the one-call entries that write a sized column
// (SizedColumn: sizes, scan, cap rule, fill), the tables step, and the leftmost-longest match list of a call's own.
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

// What a one-call entry answers for a batch without items: entry 0 of every offsets array it returns, zero.  One synchronise.
inline int empty_batch(std::initializer_list<uint64_t *> offsets, void *stream) {
    for (uint64_t *d_off : offsets) HIP_TRY(hipMemsetAsync(d_off, 0, sizeof(uint64_t), (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return RRX_OK;
}

// The tail of a one-call entry that writes a variable-size column of n entries: their lengths, the scan of the lengths into the
// offsets, the cap rule and the fill.  THE CAP RULE: the total is exact whatever the caps; a column beyond a cap - its n entries
// beyond the caller's offsets array (`fits` false), or its bytes beyond `cap` - is not written, not a byte of it.
//   alloc()  the lengths (n words, one at the very least: the generic kernels are never handed a null array) with the flag word
//            behind them; the scan's scratch unless the caller has one of scan_scratch_words(n) to lend (d_sums); offsets of the
//            call's own (n + 1 entries) where the caller's do not hold the column.  The caller reports a failure with its own lists.
//   sizes()  the flag zeroed, the caller's launch - it fills the lengths and raises the flag where an entry has 2^30 bytes or more:
//            the scan carries 30 bits -, scan_total with the flag; a raised flag is refused with `too_long`.  Leaves *total.
//   fill()   the caller's launch and its one synchronise, only where every cap holds and there is a byte to write.
// Both launches return what the entry is to return (launched(...)).  `word`: "replace", "pieces", "filter" in the error texts.
struct SizedColumn {
    const char *const word, *const too_long;
    SizedColumn(const char *word_, const char *too_long_) : word(word_), too_long(too_long_) {}
    size_t n = 0, total = 0;
    bool fits = true;
    DeviceArray<uint32_t> len;
    DeviceArray<uint64_t> own_sums, own_off;
    uint64_t *sums = nullptr, *off = nullptr;
    hipError_t alloc(int device, size_t n_, uint64_t *d_off, bool fits_, uint64_t *d_sums = nullptr) {
        n = n_, fits = fits_, off = d_off, sums = d_sums;
        hipError_t he = len.alloc(device, ((n ? n : 1) + 1) * sizeof(uint32_t));
        if (he == hipSuccess && !sums) { he = own_sums.alloc(device, rrx::dev::scan_scratch_words(n) * sizeof(uint64_t)); sums = own_sums; }
        if (he == hipSuccess && !fits) { he = own_off.alloc(device, (n + 1) * sizeof(uint64_t)); off = own_off; }
        return he;
    }
    template <class Launch> int sizes(Launch &&launch, size_t *total_out, void *stream) {
        const std::string w = word;
        uint32_t *d_flag = len + (n ? n : 1), flag = 0;
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), (hipStream_t)stream));
        int rc = launch(static_cast<uint32_t *>(len), d_flag);
        if (rc) return rc;
        uint64_t tot = 0;
        rc = scan_total(len, off, sums, n, stream, (w + " sizes and scan launch").c_str(), (w + " scan").c_str(), &tot, d_flag, &flag);
        if (rc) return rc;
        if (flag) return fail(RRX_ERR_UNSUPPORTED, too_long);
        *total_out = total = (size_t)tot;
        return RRX_OK;
    }
    template <class Launch> int fill(size_t cap, Launch &&launch, void *stream) {
        if (!fits || !total || total > cap) return RRX_OK;
        const int rc = launch();
        if (rc) return rc;
        const hipError_t he = hipStreamSynchronize((hipStream_t)stream);
        return he == hipSuccess ? RRX_OK : hip_fail(he, (std::string(word) + " fill").c_str());
    }
};

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
