// items.cpp — explicit items (an offsets array: rrx_match_extents / rrx_contains_extents / rrx_search_extents / rrx_search_all_extents* /
// rrx_search_longest_extents / rrx_search_all_longest_extents* / rrx_replace_* / rrx_pieces_*, and rrx_items, the batch indexed once)
// and single strings (rrx_match_string, rrx_match_cstr).
#include <algorithm>
#include <cstring>

#include "handles.hpp"

using namespace rrx;

static constexpr size_t kLongStringBytes = 32 * 1024;   // shorter single strings stay on one lane (NFA engines)
// Table engines: the chunk maps by convergence cost a handful of short launches (60-80 us), a sequential lane 94 ns per byte
// (tools/probe/facade_latency.py: 1.9 ms for 20 KB against 59 us; 130 us for 1 KB): from 1 KiB on the chunks win.
static constexpr size_t kLongStringBytesTable = 1024;
static constexpr uint32_t kLongNfaMaxBits = 256;        // NFA engines: chunk relations cost bytes x positions lane steps

extern "C" {

// below these a batch stays on the lane-per-item kernel (the index costs more than it saves)
static constexpr size_t kItemsStripesMin = (size_t)1 << 16;
static constexpr size_t kItemsStripesMinBytes = (size_t)8 << 20;
// A batch of items as the lane-per-item paths take it: the raw arguments of an _extents entry, or an rrx_items without its index.
struct ItemBatch { int device; const uint8_t *bytes; const uint64_t *off; size_t nitems; uint32_t trim; };
static ItemBatch batch_of(int device, const void *d_bytes, const uint64_t *d_off, size_t n, uint32_t trim) { return {device, static_cast<const uint8_t *>(d_bytes), d_off, n, trim}; }
static ItemBatch batch_of(const rrx_items *it) { return {it->device, it->d_bytes, it->d_off, it->nitems, it->trim}; }
// A lane (lane group, workgroup) per item: the match set on the regex' engine, one byte per item; the contains set on the plain
// arrays of its table, the bitmap itself.
static int extents_lanes(const rrx_regex *re, const TableSet &set, const DeviceTables *t, const uint8_t *b, const uint64_t *d_off, size_t nitems,
                         uint32_t trim, dev::ItemVerdicts out, void *stream, const uint32_t *only_if = nullptr) {
    int e = 0;
    if (&set == &re->contains_set) e = dev::contains_extents_dfa(t->dfa, set.lt.global, set.found, b, d_off, nitems, trim, out.bits, stream, only_if);
    else switch (re->engine) {
    case RRX_ENGINE_NFA_SPARSE: e = dev::match_extents_sparse_nfa(t->block, b, d_off, nitems, trim, out.bytes, stream); break;
    case RRX_ENGINE_NFA_BLOCK: e = dev::match_extents_wave_nfa(t->block, b, d_off, nitems, trim, out.bytes, stream); break;
    case RRX_ENGINE_NFA_WAVE: e = dev::match_extents_group_nfa(t->group, b, d_off, nitems, trim, out.bytes, stream); break;
    case RRX_ENGINE_NFA: e = dev::match_extents_nfa(t->nfa, b, d_off, nitems, trim, out.bytes, stream); break;
    default: e = dev::match_extents_dfa(t->dfa, b, d_off, nitems, trim, out.bytes, stream, only_if);
    }
    return e ? hip_fail((hipError_t)e, (std::string(set.word) + "_extents launch").c_str()) : RRX_OK;
}
// The table of the stripe-wise items kernels on `device`: the stride-2 items table for trim 1 (unless RRX_OPT_ITEMS_STRIDE2 is 0),
// else - or where that one does not fit - the byte-stride items table; both nullptr: the set has none (the lane-per-item kernel).
struct ItemsTable { const dev::LineDfaDevice *items1 = nullptr; const dev::Dfa2Device *items2 = nullptr; };
static ItemsTable pick_items_table(const rrx_regex *re, TableSet &set, int device, uint32_t trim) {
    ItemsTable t;
    if (trim == 1 && re->items_stride2.load()) t.items2 = re->items2_table(set, device);
    if (!t.items2) t.items1 = re->items_table(set, device);
    return t;
}
// The most a one-call batch of items at `d_bytes` can span (the index, the stripe and the grids are sized for it; the kernels take
// the real extent from the offsets): what is left of the allocation that holds d_bytes.
// The tail of the allocation is only a BOUND: a batch carved out of a memory pool (a caching allocator's block, a slice of a
// column store) would size the index, the stripe and the grids for all of the pool behind it - a 24 MiB batch 6 GiB into a
// 10 GiB pool: 512 MiB of scratch and two workgroups' worth of stripes.  So the bound is trusted only while it is plausible
// for the batch: at most 128 bytes per item (string columns; 16 MiB at least).  Beyond that - and for memory whose range
// the runtime does not report (pools, managed and virtual memory: bound 0) - the batch's real extent is read back, one
// synchronisation on `stream`, as round 2 did for every batch.
static int items_extent_bound(const void *d_bytes, const uint64_t *d_off, size_t nitems, void *stream, size_t *out) {
    size_t bound = 0;
    hipDeviceptr_t abase = nullptr;
    size_t asize = 0;
    if (hipMemGetAddressRange(&abase, &asize, const_cast<void *>(d_bytes)) == hipSuccess && abase)
        bound = (size_t)(static_cast<const uint8_t *>(abase) + asize - static_cast<const uint8_t *>(d_bytes));
    else (void)hipGetLastError();
    const size_t plausible = std::max<size_t>(nitems * 128, (size_t)16 << 20);
    if (!bound || bound > plausible) {
        uint64_t first = 0, last = 0;
        HIP_TRY(hipMemcpyAsync(&first, d_off, sizeof first, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipMemcpyAsync(&last, d_off + nitems, sizeof last, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        const size_t extent = last > first ? (size_t)last : 0;
        bound = bound ? std::min(bound, extent) : extent;
    }
    *out = bound;
    return RRX_OK;
}
// A one-call batch of items on `set` (`t`: its tables on `device`), the verdicts into `out`.
// A large batch on a table with an items form runs stripe-wise over the byte buffer, the item ends taken from a bitmap built from
// the offsets (kernels_items.hip: match_items_stripes_kernel) and the table a copy of the plain one with an END OF ITEM column.
// Needs: the entry's own conditions (stripes_ok), trim 0 or 1, at most 126 table states, no item without a byte to carry its mark.
// ASYNCHRONOUS: nothing is read back.  The host knows neither off[0] nor off[nitems]; it sizes the index for the most the batch can
// span - what is left of the allocation that holds d_bytes - and the kernels take the real extent from the offsets.  Whether the
// batch is fit (alignment, no degenerate item, large enough) is decided on the device: both kernels are queued, each predicated on
// the index pass's fit flag - the stripe-wise kernel does nothing on an unfit batch (a bitmap copied out of its scratch: zeros) and
// the lane-per-item kernel behind it, which writes every byte or word, nothing on a fit one.
// (r4) trim 1 on a table with a stride-2 form: the stride-2 items table (it also serves automata whose byte-stride items table is
// beyond the LDS - a{1,300}: 302 rows of 130 columns)
static int extents_batch(const rrx_regex *re, TableSet &set, const DeviceTables *t, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems,
                         uint32_t trim, bool stripes_ok, dev::ItemVerdicts out, void *stream) {
    const uint8_t *b = static_cast<const uint8_t *>(d_bytes);
    ItemsTable it;
    if (stripes_ok && trim <= 1 && nitems >= kItemsStripesMin) it = pick_items_table(re, set, device, trim);
    const bool items = it.items1 || it.items2;
    size_t bound = 0;
    if (items) {
        const int rc = items_extent_bound(d_bytes, d_off, nitems, stream, &bound);
        if (rc) return rc;
    }
    if (!items || bound < kItemsStripesMinBytes) return extents_lanes(re, set, t, b, d_off, nitems, trim, out, stream);
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(re->onepass_mu);
    void *buf = nullptr;
    const size_t ib = dev::items_index_bytes(bound, nitems);
    int rc = re->onepass_for(device, ib + dev::items_result_bytes(nitems), &buf, st);      // (ordered behind the scratch's last user)
    if (rc) return rc;
    uint32_t *d_flag = nullptr;
    int le = dev::items_index_build(bound, d_off, nitems, trim, buf, &d_flag, stream, b, kItemsStripesMinBytes);
    if (!le) le = it.items2 ? dev::items_match2(*it.items2, b, bound, nitems, buf, static_cast<uint8_t *>(buf) + ib, out, stream, d_off, d_flag)
                            : dev::items_match(*it.items1, b, bound, nitems, trim, buf, static_cast<uint8_t *>(buf) + ib, out, stream, d_off, d_flag);
    if (!le) rc = extents_lanes(re, set, t, b, d_off, nitems, trim, out, stream, d_flag);
    const int rc2 = re->onepass_done(device, st);                // (whatever was queued: the next user waits for it)
    if (le) return hip_fail((hipError_t)le, (std::string(set.word) + "_items_stripes launch").c_str());
    return rc ? rc : rc2;
}
// The match entries go stripe-wise only on the table engine and into a 16-byte aligned byte array (expand_bits)
static bool match_stripes_ok(const rrx_regex *re, const uint8_t *d_accept) { return re->engine == RRX_ENGINE_DFA && !(reinterpret_cast<uintptr_t>(d_accept) & 15); }
int rrx_match_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                      uint8_t *d_accept, void *stream) {
    if (!re || (nitems && (!d_off || !d_accept))) return fail(RRX_ERR_ARG, "null argument");
    const DeviceTables *t;
    int rc = re->tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return extents_batch(re, re->match_set, t, device, d_bytes, d_off, nitems, trim, match_stripes_ok(re, d_accept), d_accept, stream);      // (no items: an empty launch)
}

int rrx_items_create(int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, void *stream, rrx_items **out) {
    if (!out || (nitems && (!d_bytes || !d_off))) return fail(RRX_ERR_ARG, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rrx_items> it(new rrx_items());      // (its device memory goes with it on every early return)
    it->device = device; it->d_bytes = static_cast<const uint8_t *>(d_bytes); it->d_off = d_off; it->nitems = nitems; it->trim = trim;
    hipStream_t st = (hipStream_t)stream;
    if (nitems && trim <= 1) {
        uint64_t first = 0, last = 0;
        hipError_t e = hipMemcpyAsync(&first, d_off, sizeof first, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&last, d_off + nitems, sizeof last, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_fail(e, "items offsets readback");
        it->first = first;
        if (last > first && !(reinterpret_cast<uintptr_t>(it->d_bytes + first) & 15)) {
            it->nbytes = (size_t)(last - first);
            e = it->d_index.alloc(device, dev::items_index_bytes(it->nbytes, nitems));
            if (e == hipSuccess) e = it->d_result.alloc(device, dev::items_result_bytes(nitems));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(items index)");
            uint32_t *d_flag = nullptr;
            int le = dev::items_index_build(it->nbytes, d_off, nitems, trim, it->d_index.p, &d_flag, stream);
            uint32_t degenerate = 1;
            if (!le) { e = hipMemcpyAsync(&degenerate, d_flag, sizeof degenerate, hipMemcpyDeviceToHost, st); if (e == hipSuccess) e = hipStreamSynchronize(st); }
            if (le || e != hipSuccess) return le ? hip_fail((hipError_t)le, "items index launch") : hip_fail(e, "items index");
            it->stripes = degenerate == 0;
        }
    }
    *out = it.release();
    return RRX_OK;
}
size_t rrx_items_count(const rrx_items *it) { return it ? it->nitems : 0; }
int rrx_items_stripe_wise(const rrx_items *it) { return it && it->stripes ? 1 : 0; }
void rrx_items_free(rrx_items *it) { delete it; }

// An indexed batch on `set` (`t`: its tables on the batch's device): stripe-wise where the index admits it (it said so once: no
// second attempt), the entry's own conditions hold (stripes_ok) and the set has an items table; else a lane per item.
static int items_batch(const rrx_regex *re, TableSet &set, const DeviceTables *t, const rrx_items *it, bool stripes_ok, dev::ItemVerdicts out, void *stream) {
    const ItemsTable tab = it->stripes && stripes_ok ? pick_items_table(re, set, it->device, it->trim) : ItemsTable();
    if (!tab.items1 && !tab.items2) return extents_lanes(re, set, t, it->d_bytes, it->d_off, it->nitems, it->trim, out, stream);
    std::lock_guard<std::mutex> lock(it->mu);
    const int le = tab.items2 ? dev::items_match2(*tab.items2, it->d_bytes + it->first, it->nbytes, it->nitems, it->d_index.p, it->d_result.p, out, stream)
                              : dev::items_match(*tab.items1, it->d_bytes + it->first, it->nbytes, it->nitems, it->trim, it->d_index.p, it->d_result.p, out, stream);
    return le ? hip_fail((hipError_t)le, (std::string(set.word) + "_items launch").c_str()) : RRX_OK;
}
int rrx_match_items(const rrx_regex *re, const rrx_items *it, uint8_t *d_accept, void *stream) {
    if (!re || !it || (it->nitems && !d_accept)) return fail(RRX_ERR_ARG, "null argument");
    if (!it->nitems) return RRX_OK;
    const DeviceTables *t;
    int rc = re->tables(it->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(it->device));
    return items_batch(re, re->match_set, t, it, match_stripes_ok(re, d_accept), d_accept, stream);
}

// "Which items contain a match": the same two paths on the contains set - stripe-wise wherever the contains table has an items form,
// whatever the regex' MATCH engine is and at any alignment of the bitmap (the stripe-wise kernels write into scratch, the caller's
// bitmap receives a masked copy).  An empty batch still reports a regex without a contains table.
int rrx_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                         uint32_t *d_bits, void *stream) {
    if (!re || (nitems && (!d_off || !d_bits))) return fail(RRX_ERR_ARG, "null argument");
    const DeviceTables *t;
    int rc = re->contains_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    return extents_batch(re, re->contains_set, t, device, d_bytes, d_off, nitems, trim, /*stripes_ok=*/true, d_bits, stream);
}
int rrx_contains_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_bits, void *stream) {
    if (!re || !it || (it->nitems && !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    const DeviceTables *t;
    int rc = re->contains_tables(it->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(it->device));
    if (!it->nitems) return RRX_OK;
    return items_batch(re, re->contains_set, t, it, /*stripes_ok=*/true, d_bits, stream);
}

// WHERE the first match of every item is (rrx_search_corpus for explicit items): a lane per item on the two plain search tables.
// Nothing is known on the host and nothing read back: the kernel takes every extent from the offsets.  A pattern that accepts the
// empty string matches [0, 0) in every item: two fills, no table.  An empty batch still reports a regex without search tables.
static int search_lanes(const rrx_regex *re, const ItemBatch &b, uint32_t *d_start, uint32_t *d_end, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchItemsDevice *t;
    const int rc = re->search_item_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    if (!t) {
        HIP_TRY(hipMemsetAsync(d_start, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, bytes, off, nitems, trim, d_start, d_end, stream),
                    "search_extents launch");
}
int rrx_search_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                       uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || (nitems && (!d_off || !d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), d_start, d_end, stream);
}
int rrx_search_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !it || (it->nitems && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_lanes(re, batch_of(it), d_start, d_end, stream);
}

// The LEFTMOST-LONGEST match of every item, on the starts table (backwards over the whole item: the smallest start) and the
// anchored table (forwards from there: the largest end).  The empty language matches nowhere: two fills, no table.  A pattern that
// accepts the empty string starts at 0 everywhere and runs the forward pass alone.  (No tables: they do not determinise.)
static int search_longest_lanes(const rrx_regex *re, const ItemBatch &b, uint32_t *d_start, uint32_t *d_end, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchLongestDevice *t;
    const int rc = re->search_longest_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    if (!t) {
        HIP_TRY(hipMemsetAsync(d_start, 0xff, nitems * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0xff, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_longest_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, re->search_longest.nullable, bytes, off, nitems, trim,
                                                    d_start, d_end, stream),
                    "search_longest_extents launch");
}
int rrx_search_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                               uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || (nitems && (!d_off || !d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_longest_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), d_start, d_end, stream);
}
int rrx_search_longest_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !it || (it->nitems && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_longest_lanes(re, batch_of(it), d_start, d_end, stream);
}

// EVERY match of every item (rrx_search_all* for explicit items): search_lanes' tables and kernel shape, the search applied again
// to the rest of the item behind each match.  d_first == nullptr: the counts; otherwise the matches into the slots behind
// d_first[i], those below `cap`.  A pattern that accepts the empty string has the matches [k, k) for k = 0 .. length: no table, no
// text.
static int search_all_lanes(const rrx_regex *re, const ItemBatch &b, uint32_t *d_count, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                            void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchItemsDevice *t;
    const int rc = re->search_item_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    if (!t) return launched(dev::empty_item_matches(off, nitems, trim, d_count, d_first, d_start, d_end, cap, stream), "empty_item_matches launch");
    return launched(dev::search_all_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, bytes, off, nitems, trim, d_count, d_first, d_start, d_end,
                                                cap, stream),
                    "search_all_extents launch");
}
// count + scan + fill in one call, the counts and the scan's scratch in device memory of the call's own (freed when it leaves:
// hipFree waits for what is queued): calls share nothing.
static int search_all_one_call(const rrx_regex *re, const ItemBatch &b, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total,
                               void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    *total = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = search_all_lanes(re, batch_of(device, bytes, off, 0, trim), nullptr, nullptr, nullptr, nullptr, 0, stream);      // (the tables, the device)
    if (rc) return rc;
    if (!nitems) { HIP_TRY(hipMemsetAsync(d_first, 0, sizeof(uint64_t), st)); HIP_TRY(hipStreamSynchronize(st)); return RRX_OK; }
    DeviceArray<uint32_t> d_count;
    DeviceArray<uint64_t> d_sums;
    hipError_t he = d_count.alloc(device, nitems * sizeof(uint32_t));
    if (he == hipSuccess) he = d_sums.alloc(device, dev::scan_scratch_words(nitems) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(search_all counts)");
    rc = search_all_lanes(re, b, d_count, nullptr, nullptr, nullptr, 0, stream);
    if (rc) return rc;
    const int le = dev::scan_counts(d_count, d_first, d_sums, nitems, stream);  // d_first[nitems] = total
    if (le) return hip_fail((hipError_t)le, "search_all scan launch");
    he = hipMemsetAsync(d_first, 0, sizeof(uint64_t), st);                      // the scan marks entry 0 as a stripe start: not here
    uint64_t tot = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&tot, d_first + nitems, sizeof tot, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "search_all scan");
    *total = (size_t)tot;
    if (tot && cap) {                                                            // matches in slots >= cap are counted, not written
        rc = search_all_lanes(re, b, nullptr, d_first, d_start, d_end, cap, stream);
        if (!rc) { he = hipStreamSynchronize(st); if (he != hipSuccess) rc = hip_fail(he, "search_all fill"); }
    }
    return rc;
}
int rrx_search_all_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                 uint32_t *d_count, void *stream) {
    if (!re || (nitems && (!d_off || !d_count))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_items_count(const rrx_regex *re, const rrx_items *it, uint32_t *d_count, void *stream) {
    if (!re || !it || (it->nitems && !d_count)) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, batch_of(it), d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || (nitems && (!d_off || !d_first || !d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), nullptr, d_first, d_start, d_end, ~(size_t)0, stream);
}
int rrx_search_all_items_fill(const rrx_regex *re, const rrx_items *it, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !it || (it->nitems && (!d_first || !d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_lanes(re, batch_of(it), nullptr, d_first, d_start, d_end, ~(size_t)0, stream);
}
int rrx_search_all_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                           uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream) {
    if (!re || !total || !d_first || (nitems && (!d_off || (cap && (!d_start || !d_end))))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), d_first, d_start, d_end, cap, total, stream);
}
int rrx_search_all_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total,
                         void *stream) {
    if (!re || !it || !total || !d_first || (it->nitems && cap && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_one_call(re, batch_of(it), d_first, d_start, d_end, cap, total, stream);
}

// EVERY LEFTMOST-LONGEST match of every item: search_longest_lanes' tables, the search applied again to the rest of the item behind
// each match.  d_first == nullptr: the marks and the counts; otherwise the matches into the slots behind d_first[i], those below
// `cap`, on the marks the count pass left.  The empty language matches nowhere: the counts are a fill, there is no table and no
// text pass.  (No tables: they do not determinise.)
struct ItemMarks { uint32_t *words; size_t nwords; };
static int search_all_longest_lanes(const rrx_regex *re, const ItemBatch &b, ItemMarks marks, uint32_t *d_count, const uint64_t *d_first, uint32_t *d_start,
                                    uint32_t *d_end, size_t cap, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    const dev::SearchLongestDevice *t;
    const int rc = re->search_longest_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    if (!t) {
        if (!d_first) HIP_TRY(hipMemsetAsync(d_count, 0, nitems * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_all_longest_extents_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, re->search_longest.nullable, bytes, off, nitems, trim,
                                                        marks.words, marks.nwords, d_count, d_first, d_start, d_end, cap, stream),
                    "search_all_longest_extents launch");
}
// The marks of a batch of nitems items take a word per item at the very least, whatever the extent: a shorter buffer cannot be meant
static bool marks_ok(size_t nitems, const uint32_t *d_marks, size_t marks_words) { return !nitems || (d_marks && marks_words >= nitems + 1); }
static const char *const kMarksError = "null argument, or marks_words below nitems + 1";
// count + scan of one call (search_all_one_call's first half), the counts, the marks and the scan's scratch in device memory of the
// call's own, the marks sized from the batch's real extent: off[0] and off[nitems] are read back.  Leaves d_first complete
// (nitems + 1 entries, entry 0 = 0) and *total = d_first[nitems]; nitems > 0, the tables checked by the caller.
struct LongestCounts {
    DeviceArray<uint32_t> count, marks;
    DeviceArray<uint64_t> sums;                  // scan_scratch_words(nitems): free again once the call has synchronised
    size_t nwords = 0;
};
static int search_all_longest_count_scan(const rrx_regex *re, const ItemBatch &b, LongestCounts &c, uint64_t *d_first, size_t *total, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    hipStream_t st = (hipStream_t)stream;
    uint64_t lo = 0, hi = 0;
    HIP_TRY(hipMemcpyAsync(&lo, off, sizeof lo, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&hi, off + nitems, sizeof hi, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.nwords = rrx_search_all_longest_marks_words(hi > lo ? (size_t)(hi - lo) : 0, nitems);
    hipError_t he = c.count.alloc(device, nitems * sizeof(uint32_t));
    if (he == hipSuccess) he = c.marks.alloc(device, c.nwords * sizeof(uint32_t));
    if (he == hipSuccess) he = c.sums.alloc(device, dev::scan_scratch_words(nitems) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(search_all_longest counts and marks)");
    const int rc = search_all_longest_lanes(re, b, {c.marks, c.nwords}, c.count, nullptr, nullptr, nullptr, 0, stream);
    if (rc) return rc;
    const int le = dev::scan_counts(c.count, d_first, c.sums, nitems, stream);  // d_first[nitems] = total
    if (le) return hip_fail((hipError_t)le, "search_all_longest scan launch");
    he = hipMemsetAsync(d_first, 0, sizeof(uint64_t), st);                      // the scan marks entry 0 as a stripe start: not here
    uint64_t tot = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&tot, d_first + nitems, sizeof tot, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "search_all_longest scan");
    *total = (size_t)tot;
    return RRX_OK;
}
// count + scan + fill in one call (search_all_one_call)
static int search_all_longest_one_call(const rrx_regex *re, const ItemBatch &b, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                                       size_t *total, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    *total = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = search_all_longest_lanes(re, batch_of(device, bytes, off, 0, trim), {}, nullptr, nullptr, nullptr, nullptr, 0, stream);   // (the tables, the device)
    if (rc) return rc;
    if (!nitems) { HIP_TRY(hipMemsetAsync(d_first, 0, sizeof(uint64_t), st)); HIP_TRY(hipStreamSynchronize(st)); return RRX_OK; }
    LongestCounts c;
    rc = search_all_longest_count_scan(re, b, c, d_first, total, stream);
    if (rc) return rc;
    if (*total && cap) {                                                         // matches in slots >= cap are counted, not written
        rc = search_all_longest_lanes(re, b, {c.marks, c.nwords}, nullptr, d_first, d_start, d_end, cap, stream);
        if (!rc) { const hipError_t he = hipStreamSynchronize(st); if (he != hipSuccess) rc = hip_fail(he, "search_all_longest fill"); }
    }
    return rc;
}
size_t rrx_search_all_longest_marks_words(size_t extent_bytes, size_t nitems) { return dev::search_all_longest_marks_words(extent_bytes, nitems); }
int rrx_search_all_longest_extents_count(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                         uint32_t *d_marks, size_t marks_words, uint32_t *d_count, void *stream) {
    if (!re || (nitems && (!d_off || !d_count)) || !marks_ok(nitems, d_marks, marks_words)) return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), {d_marks, marks_words}, d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_longest_items_count(const rrx_regex *re, const rrx_items *it, uint32_t *d_marks, size_t marks_words, uint32_t *d_count, void *stream) {
    if (!re || !it || (it->nitems && !d_count) || !marks_ok(it->nitems, d_marks, marks_words)) return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, batch_of(it), {d_marks, marks_words}, d_count, nullptr, nullptr, nullptr, 0, stream);
}
int rrx_search_all_longest_extents_fill(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                        const uint32_t *d_marks, size_t marks_words, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end,
                                        void *stream) {
    if (!re || (nitems && (!d_off || !d_first || !d_start || !d_end)) || !marks_ok(nitems, d_marks, marks_words)) return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, batch_of(device, d_bytes, d_off, nitems, trim), {const_cast<uint32_t *>(d_marks), marks_words}, nullptr, d_first,
                                    d_start, d_end, ~(size_t)0, stream);       // (the fill kernel only reads the marks)
}
int rrx_search_all_longest_items_fill(const rrx_regex *re, const rrx_items *it, const uint32_t *d_marks, size_t marks_words, const uint64_t *d_first,
                                      uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !it || (it->nitems && (!d_first || !d_start || !d_end)) || !marks_ok(it->nitems, d_marks, marks_words))
        return fail(RRX_ERR_ARG, kMarksError);
    return search_all_longest_lanes(re, batch_of(it), {const_cast<uint32_t *>(d_marks), marks_words}, nullptr, d_first, d_start, d_end, ~(size_t)0, stream);
}
int rrx_search_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                   uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total, void *stream) {
    if (!re || !total || !d_first || (nitems && (!d_off || (cap && (!d_start || !d_end))))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), d_first, d_start, d_end, cap, total, stream);
}
int rrx_search_all_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap,
                                 size_t *total, void *stream) {
    if (!re || !it || !total || !d_first || (it->nitems && cap && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    return search_all_longest_one_call(re, batch_of(it), d_first, d_start, d_end, cap, total, stream);
}

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
// Every leftmost-longest match replaced, in one call: search_all_longest_one_call's count + scan and fill into match arrays of the
// call's own, then sizes, a second scan (the lengths into d_out_off) and - if the column fits `cap` - the bytes.  The sizes kernel
// raises a device word where an output item has 2^30 bytes or more (the scan carries 30 bits); it is read back with the total.
static int replace_all_longest_one_call(const rrx_regex *re, const ItemBatch &b, const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out,
                                        size_t cap, size_t *total, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    *total = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = search_all_longest_lanes(re, batch_of(device, bytes, off, 0, trim), {}, nullptr, nullptr, nullptr, nullptr, 0, stream);   // (the tables, the device)
    if (rc) return rc;
    if (!nitems) { HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), st)); HIP_TRY(hipStreamSynchronize(st)); return RRX_OK; }
    LongestCounts c;
    DeviceArray<uint64_t> d_first;
    hipError_t he = d_first.alloc(device, (nitems + 1) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(replace prefix)");
    size_t nmatches = 0;
    rc = search_all_longest_count_scan(re, b, c, d_first, &nmatches, stream);
    if (rc) return rc;
    // (one word more than the lists need: the generic kernels are never handed a null array; the last word of d_len is the flag)
    DeviceArray<uint32_t> d_start, d_end, d_pos, d_len;
    DeviceArray<uint8_t> d_rep;
    const size_t list_bytes = (nmatches + 1) * sizeof(uint32_t);
    he = d_start.alloc(device, list_bytes);
    if (he == hipSuccess) he = d_end.alloc(device, list_bytes);
    if (he == hipSuccess) he = d_pos.alloc(device, list_bytes);
    if (he == hipSuccess) he = d_len.alloc(device, (nitems + 1) * sizeof(uint32_t));
    if (he == hipSuccess && rep_len) he = d_rep.alloc(device, rep_len);
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(replace lists)");
    if (rep_len) HIP_TRY(hipMemcpyAsync(d_rep, rep, rep_len, hipMemcpyHostToDevice, st));      // (the call does not return before a synchronise: `rep` stays valid)
    if (nmatches) {
        rc = search_all_longest_lanes(re, b, {c.marks, c.nwords}, nullptr, d_first, d_start, d_end, nmatches, stream);
        if (rc) return rc;
    }
    uint32_t *d_flag = d_len + nitems;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), st));
    int le = dev::replace_sizes(off, nitems, trim, d_first, d_start, d_end, rep_len, d_len, d_pos, d_flag, stream);
    if (!le) le = dev::scan_counts(d_len, d_out_off, c.sums, nitems, stream);   // d_out_off[nitems] = total (the first scan's scratch: the stream orders them)
    if (le) return hip_fail((hipError_t)le, "replace sizes and scan launch");
    he = hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), st);                     // the scan marks entry 0 as a stripe start: not here
    uint64_t tot = 0;
    uint32_t flag = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&tot, d_out_off + nitems, sizeof tot, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "replace scan");
    if (flag) return fail(RRX_ERR_UNSUPPORTED, "an output item of 2^30 bytes or more: use rrx_search_all_longest_extents and the two passes rrx_replace_matches_sizes / _fill");
    *total = (size_t)tot;
    if (tot && tot <= cap) {                                                     // a column beyond cap: not a byte of it is written
        le = dev::replace_fill(bytes, off, nitems, trim, d_first, d_end, d_pos, d_rep, rep_len, d_out_off, static_cast<uint8_t *>(d_out), stream);
        if (le) return hip_fail((hipError_t)le, "replace_fill launch");
        he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "replace fill");
    }
    return RRX_OK;
}
int rrx_replace_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out, size_t cap, size_t *total, void *stream) {
    if (!re || !total || !d_out_off || (rep_len && !rep) || (nitems && (!d_off || (cap && !d_out)))) return fail(RRX_ERR_ARG, "null argument");
    return replace_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), rep, rep_len, d_out_off, d_out, cap, total, stream);
}
int rrx_replace_all_longest_items(const rrx_regex *re, const rrx_items *it, const void *rep, uint32_t rep_len, uint64_t *d_out_off, void *d_out,
                                  size_t cap, size_t *total, void *stream) {
    if (!re || !it || !total || !d_out_off || (rep_len && !rep) || (it->nitems && cap && !d_out)) return fail(RRX_ERR_ARG, "null argument");
    return replace_all_longest_one_call(re, batch_of(it), rep, rep_len, d_out_off, d_out, cap, total, stream);
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
// The pieces of every leftmost-longest match list, in one call (replace_all_longest_one_call's shape): count + scan and fill into
// match arrays of the call's own, then sizes, a second scan (the piece lengths into the piece offsets - the caller's array if it
// holds them, one of the call's own otherwise: the total is exact either way) and - if both caps hold - the bytes.  The number of
// pieces follows from the number of matches on the host.  The sizes kernel raises a device word where a piece has 2^30 bytes or more.
static int pieces_all_longest_one_call(const rrx_regex *re, const ItemBatch &b, bool gaps, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap,
                                       void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream) {
    const auto &[device, bytes, off, nitems, trim] = b;
    *npieces = *total = 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = search_all_longest_lanes(re, batch_of(device, bytes, off, 0, trim), {}, nullptr, nullptr, nullptr, nullptr, 0, stream);   // (the tables, the device)
    if (rc) return rc;
    if (!nitems) {
        HIP_TRY(hipMemsetAsync(d_list_off, 0, sizeof(uint64_t), st));
        HIP_TRY(hipMemsetAsync(d_piece_off, 0, sizeof(uint64_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        return RRX_OK;
    }
    LongestCounts c;
    DeviceArray<uint64_t> d_first;
    hipError_t he = d_first.alloc(device, (nitems + 1) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(pieces prefix)");
    size_t nmatches = 0;
    rc = search_all_longest_count_scan(re, b, c, d_first, &nmatches, stream);
    if (rc) return rc;
    const size_t np = nmatches + (gaps ? nitems : 0);
    *npieces = np;
    // (one word more than the lists need: the generic kernels are never handed a null array; the last word of d_len is the flag)
    DeviceArray<uint32_t> d_start, d_end, d_len;
    DeviceArray<uint64_t> d_src, d_sums, d_own_off;
    he = d_start.alloc(device, (nmatches + 1) * sizeof(uint32_t));
    if (he == hipSuccess) he = d_end.alloc(device, (nmatches + 1) * sizeof(uint32_t));
    if (he == hipSuccess) he = d_len.alloc(device, (np + 2) * sizeof(uint32_t));
    if (he == hipSuccess) he = d_src.alloc(device, (np + 1) * sizeof(uint64_t));
    if (he == hipSuccess) he = d_sums.alloc(device, dev::scan_scratch_words(np) * sizeof(uint64_t));
    if (he == hipSuccess && np > pieces_cap) he = d_own_off.alloc(device, (np + 1) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(pieces lists)");
    uint64_t *piece_off = np > pieces_cap ? (uint64_t *)d_own_off : d_piece_off;
    if (nmatches) {
        rc = search_all_longest_lanes(re, b, {c.marks, c.nwords}, nullptr, d_first, d_start, d_end, nmatches, stream);
        if (rc) return rc;
    }
    uint32_t *d_flag = d_len + np + 1;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), st));
    int le = dev::pieces_sizes(off, nitems, trim, d_first, d_start, d_end, gaps, d_list_off, d_len, d_src, d_flag, stream);
    if (!le) le = dev::scan_counts(d_len, piece_off, d_sums, np, stream);       // piece_off[np] = total
    if (le) return hip_fail((hipError_t)le, "pieces sizes and scan launch");
    he = hipMemsetAsync(piece_off, 0, sizeof(uint64_t), st);                     // the scan marks entry 0 as a stripe start: not here
    uint64_t tot = 0;
    uint32_t flag = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&tot, piece_off + np, sizeof tot, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "pieces scan");
    if (flag) return fail(RRX_ERR_UNSUPPORTED, "a piece of 2^30 bytes or more: use rrx_search_all_longest_extents and the two passes rrx_pieces_sizes / _fill");
    *total = (size_t)tot;
    if (np <= pieces_cap && tot && tot <= cap) {                                 // a column beyond either cap: not a byte of it is written
        le = dev::pieces_fill(bytes, d_src, piece_off, np, static_cast<uint8_t *>(d_out), stream);
        if (le) return hip_fail((hipError_t)le, "pieces_fill launch");
        he = hipStreamSynchronize(st);
        if (he != hipSuccess) return hip_fail(he, "pieces fill");
    }
    return RRX_OK;
}
static bool pieces_args_ok(const void *handle, const uint64_t *d_off, size_t nitems, const uint64_t *d_list_off, const uint64_t *d_piece_off, const void *d_out,
                           size_t cap, const size_t *npieces, const size_t *total) {
    return handle && npieces && total && d_list_off && d_piece_off && !(nitems && (!d_off || (cap && !d_out)));
}
int rrx_extract_all_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                                    uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces, size_t *total,
                                    void *stream) {
    if (!pieces_args_ok(re, d_off, nitems, d_list_off, d_piece_off, d_out, cap, npieces, total)) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), false, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total,
                                       stream);
}
int rrx_extract_all_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out,
                                  size_t cap, size_t *npieces, size_t *total, void *stream) {
    if (!it || !pieces_args_ok(re, it->d_off, it->nitems, d_list_off, d_piece_off, d_out, cap, npieces, total)) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(it), false, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total, stream);
}
int rrx_split_longest_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, uint64_t *d_list_off,
                              uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap, size_t *npieces, size_t *total, void *stream) {
    if (!pieces_args_ok(re, d_off, nitems, d_list_off, d_piece_off, d_out, cap, npieces, total)) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(device, d_bytes, d_off, nitems, trim), true, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total,
                                       stream);
}
int rrx_split_longest_items(const rrx_regex *re, const rrx_items *it, uint64_t *d_list_off, uint64_t *d_piece_off, size_t pieces_cap, void *d_out, size_t cap,
                            size_t *npieces, size_t *total, void *stream) {
    if (!it || !pieces_args_ok(re, it->d_off, it->nitems, d_list_off, d_piece_off, d_out, cap, npieces, total)) return fail(RRX_ERR_ARG, "null argument");
    return pieces_all_longest_one_call(re, batch_of(it), true, d_list_off, d_piece_off, pieces_cap, d_out, cap, npieces, total, stream);
}

// One device-resident string of any length.  Long strings take the chunk-map path when the automaton has a small
// table (every chunk stepped from every state, maps composed); the rest is one item of the extents kernel.
// long_string_plan decides which, once per call: the scratch is sized and the string matched by the same plan.
// `scratch`: caller-provided device memory of plan.scratch_bytes (rrx_match_cstr passes the tail of its own buffer).
struct LongStringPlan {
    enum Kind { kOneItem, kLongDfa, kLongNfa } kind = kOneItem;       // one item of the extents kernel, or the chunk maps of a table / NFA engine
    uint32_t chunk = 0, nchunks = 0;
    size_t scratch_bytes = 2 * sizeof(uint64_t);                      // (one item: its two offsets)
};
static LongStringPlan long_string_plan(const rrx_regex *re, const DeviceTables *t, size_t nbytes) {
    LongStringPlan p;
    if (re->engine == RRX_ENGINE_DFA && nbytes >= kLongStringBytesTable && t->dfa.nstates && t->dfa.nstates <= dev::kLongMaxStates) {
        p.kind = LongStringPlan::kLongDfa;
        p.scratch_bytes = dev::long_scratch_bytes(t->dfa.nstates, nbytes, &p.chunk);
    } else if (re->engine == RRX_ENGINE_NFA && nbytes >= kLongStringBytes && t->nfa.nbits <= kLongNfaMaxBits) {
        p.kind = LongStringPlan::kLongNfa;
        p.scratch_bytes = dev::long_nfa_scratch_bytes(t->nfa, nbytes, &p.chunk, &p.nchunks);
    }
    return p;
}
static int match_string_with(const rrx_regex *re, int device, const DeviceTables *t, const LongStringPlan &plan, const uint8_t *d_bytes, size_t nbytes,
                             uint8_t *d_accept, uint8_t *scratch, hipStream_t st) {
    if (plan.kind == LongStringPlan::kLongDfa) {
        return launched(dev::match_long_dfa(t->dfa, d_bytes, nbytes, plan.chunk, scratch, d_accept, st), "match_long launch");
    }
    if (plan.kind == LongStringPlan::kLongNfa) {
        return launched(dev::match_long_nfa(t->nfa, d_bytes, nbytes, plan.chunk, plan.nchunks, scratch, d_accept, st), "match_long_nfa launch");
    }
    const uint64_t off[2] = {0, nbytes};
    uint64_t *d_off = reinterpret_cast<uint64_t *>(scratch);
    hipError_t e = hipMemcpyAsync(d_off, off, sizeof off, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                    // `off` leaves scope
    if (e != hipSuccess) return hip_fail(e, "extent upload");
    return rrx_match_extents(re, device, d_bytes, d_off, 1, 0, d_accept, st);
}

int rrx_match_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint8_t *d_accept, void *stream) {
    if (!re || (nbytes && !d_bytes) || !d_accept) return fail(RRX_ERR_ARG, "null argument");
    const DeviceTables *t;
    int rc = re->tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    std::lock_guard<std::mutex> lock(re->scratch_mu);
    void *scratch = nullptr;
    const LongStringPlan plan = long_string_plan(re, t, nbytes);
    rc = re->scratch_for(device, plan.scratch_bytes, &scratch);
    if (rc) return rc;
    rc = match_string_with(re, device, t, plan, static_cast<const uint8_t *>(d_bytes), nbytes, d_accept, static_cast<uint8_t *>(scratch),
                           static_cast<hipStream_t>(stream));
    const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));      // the scratch is reused by the next call
    if (!rc && e != hipSuccess) rc = hip_fail(e, "match_string");
    return rc;
}

int rrx_match_cstr(const rrx_regex *re, int device, const char *text, int *accepted, size_t *len) {
    if (!re || !text || !accepted) return fail(RRX_ERR_ARG, "null argument");
    const size_t n = std::strlen(text);                       // regex.h:157: consume up to the terminator
    if (len) *len = n;
    const DeviceTables *t;
    int rc = re->tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    // one persistent device buffer: [text, padded to 16 | accept byte, padded to 16 | scratch of the match]
    std::lock_guard<std::mutex> lock(re->scratch_mu);
    const size_t acc_at = (n + 15) & ~(size_t)15, scratch_at = acc_at + 16;
    void *buf = nullptr;
    const LongStringPlan plan = long_string_plan(re, t, n);
    rc = re->scratch_for(device, scratch_at + plan.scratch_bytes, &buf);
    if (rc) return rc;
    uint8_t *d = static_cast<uint8_t *>(buf);
    hipError_t e = n ? hipMemcpy(d, text, n, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) return hip_fail(e, "text upload");
    rc = match_string_with(re, device, t, plan, d, n, d + acc_at, d + scratch_at, nullptr);
    uint8_t a = 0;
    if (!rc) { e = hipMemcpy(&a, d + acc_at, 1, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = hip_fail(e, "accept readback"); }
    *accepted = a;
    return rc;
}

}  // extern "C"
