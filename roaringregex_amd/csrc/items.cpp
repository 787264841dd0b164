// items.cpp — batches of explicit items (an offsets array), matched whole and asked whether they contain a match: rrx_items, the
// batch indexed once, rrx_match_extents / rrx_match_items and rrx_contains_extents / rrx_contains_items, stripe-wise where the batch
// and the table admit it, else a lane per item.
#include <algorithm>

#include "items.hpp"

using namespace rrx;

extern "C" {

// below these a batch stays on the lane-per-item kernel (the index costs more than it saves)
static constexpr size_t kItemsStripesMin = (size_t)1 << 16;
static constexpr size_t kItemsStripesMinBytes = (size_t)8 << 20;
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
        static const char *const what[3] = {"hipMemcpyAsync(&first, d_off, sizeof first, hipMemcpyDeviceToHost, (hipStream_t)stream)",
                                            "hipMemcpyAsync(&last, d_off + nitems, sizeof last, hipMemcpyDeviceToHost, (hipStream_t)stream)",
                                            "hipStreamSynchronize((hipStream_t)stream)"};
        uint64_t first = 0, last = 0;
        const int rc = read_offset_ends(d_off, nitems, stream, what, &first, &last);
        if (rc) return rc;
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
    if (!batch_args_ok(re, batch_of(device, d_bytes, d_off, nitems, trim), {d_accept})) return fail(RRX_ERR_ARG, "null argument");
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
        static const char *const what[3] = {"items offsets readback", "items offsets readback", "items offsets readback"};
        uint64_t first = 0, last = 0;
        const int rc = read_offset_ends(d_off, nitems, stream, what, &first, &last);
        if (rc) return rc;
        it->first = first;
        if (last > first && !(reinterpret_cast<uintptr_t>(it->d_bytes + first) & 15)) {
            it->nbytes = (size_t)(last - first);
            hipError_t e = it->d_index.alloc(device, dev::items_index_bytes(it->nbytes, nitems));
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
    if (!it || !batch_args_ok(re, batch_of(it), {d_accept})) return fail(RRX_ERR_ARG, "null argument");
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
// RRX_OPT_CONTAINS_NFA: the route of both entries.  *taken: the batch is answered here, on the NFA lane engine - always a lane per
// item (kernels_nfa.inc: contains_extents_nfa_kernel), which writes every word of the bitmap: no extent bound, nothing read back,
// no scratch, no event; a pattern that accepts the empty string and the empty language: a fill, no kernel.
static int contains_on_nfa(const rrx_regex *re, int device, const uint8_t *b, const uint64_t *d_off, size_t nitems, uint32_t trim, uint32_t *d_bits,
                           void *stream, bool *taken) {
    bool fill = false;
    const dev::NfaDevice *nfa = nullptr;
    const int rc = re->contains_nfa_tables(device, taken, &nfa, &fill);
    if (rc || !*taken) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    if (!nfa) return fill_bitmap(d_bits, nitems, fill, stream);
    return launched(dev::contains_extents_nfa(*nfa, b, d_off, nitems, trim, d_bits, stream), "contains_extents launch");
}
int rrx_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim,
                         uint32_t *d_bits, void *stream) {
    if (!batch_args_ok(re, batch_of(device, d_bytes, d_off, nitems, trim), {d_bits})) return fail(RRX_ERR_ARG, "null argument");
    bool on_nfa = false;
    int rc = contains_on_nfa(re, device, static_cast<const uint8_t *>(d_bytes), d_off, nitems, trim, d_bits, stream, &on_nfa);
    if (rc || on_nfa) return rc;
    const DeviceTables *t;
    rc = re->contains_tables(device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (!nitems) return RRX_OK;
    return extents_batch(re, re->contains_set, t, device, d_bytes, d_off, nitems, trim, /*stripes_ok=*/true, d_bits, stream);
}
int rrx_contains_items(const rrx_regex *re, const rrx_items *it, uint32_t *d_bits, void *stream) {
    if (!it || !batch_args_ok(re, batch_of(it), {d_bits})) return fail(RRX_ERR_ARG, "null argument");
    bool on_nfa = false;
    int rc = contains_on_nfa(re, it->device, it->d_bytes, it->d_off, it->nitems, it->trim, d_bits, stream, &on_nfa);
    if (rc || on_nfa) return rc;
    const DeviceTables *t;
    rc = re->contains_tables(it->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(it->device));
    if (!it->nitems) return RRX_OK;
    return items_batch(re, re->contains_set, t, it, /*stripes_ok=*/true, d_bits, stream);
}

}  // extern "C"
