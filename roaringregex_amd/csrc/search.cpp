// search.cpp — first match and all matches per line of a corpus (rrx_search_corpus, rrx_search_all*): the corpus' line offsets
// and chunk index, built at the first search, and the launches.
#include "items.hpp"

using namespace rrx;

extern "C" {

// per-line offsets of the corpus, built on the first search (cached in the corpus)
static int line_offsets(const rrx_corpus *c, void *stream) {
    {
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->d_line_off) {
            DeviceArray<uint64_t> off;                  // (the error text is the old call's, as HIP_TRY spelt it: texts do not change with the owners)
            if (hipError_t ae = off.alloc(c->device, (c->nlines + 1) * sizeof(uint64_t)))
                return hip_fail(ae, "hipMalloc(reinterpret_cast<void **>(&off), (c->nlines + 1) * sizeof(uint64_t))");
            // entry nlines: one past the last '\n' - the kernel writes it when the corpus ends in '\n'; otherwise the
            // last line ends at the end of the data, as if a '\n' followed it
            const uint64_t past = (uint64_t)c->nbytes + 1;
            hipError_t he = hipMemcpyAsync(off + c->nlines, &past, sizeof past, hipMemcpyHostToDevice, (hipStream_t)stream);
            if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream);          // `past` leaves scope
            int le = he == hipSuccess ? dev::build_line_offsets(c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, off, stream) : 0;
            if (he == hipSuccess && !le) he = hipStreamSynchronize((hipStream_t)stream);   // once per corpus: later searches may use other streams
            if (he != hipSuccess || le) return he != hipSuccess ? hip_fail(he, "line offsets") : hip_fail((hipError_t)le, "line_offsets launch");
            c->d_line_off = std::move(off);
        }
    }
    return RRX_OK;
}

// newline prefix per search chunk (the granularity of the stripe-wise search kernel), built on the first search
static int chunk_index(const rrx_corpus *c, void *stream) {
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->d_chunk_base) return RRX_OK;
    const size_t chunk = dev::search_chunk_bytes();
    c->nchunks = (c->nbytes + chunk - 1) / chunk;
    if (c->stripe == chunk) { c->d_chunk_base = c->d_base; return RRX_OK; }
    DeviceArray<uint32_t> counts;
    DeviceArray<uint64_t> base;
    hipError_t e = counts.alloc(c->device, (c->nchunks + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = base.alloc(c->device, (c->nchunks + 1 + dev::scan_scratch_words(c->nchunks)) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemsetAsync(counts + c->nchunks, 0, sizeof(uint32_t), (hipStream_t)stream);
    int le = 0;
    if (e == hipSuccess) le = dev::count_newlines_per_stripe(c->d_bytes, c->nbytes, (uint32_t)chunk, counts, c->nchunks, counts + c->nchunks, stream);
    if (e == hipSuccess && !le) le = dev::scan_counts(counts, base, base + c->nchunks + 1, c->nchunks, stream);
    if (e == hipSuccess && !le) e = hipStreamSynchronize((hipStream_t)stream);     // once per corpus: later searches may use other streams
    if (e != hipSuccess || le) return e != hipSuccess ? hip_fail(e, "search chunk index") : hip_fail((hipError_t)le, "search chunk index launch");
    c->d_chunk_own = std::move(base);
    c->d_chunk_base = c->d_chunk_own;
    return RRX_OK;
}

// What every search entry begins with, behind its null checks: the tables (*ct = nullptr: the pattern accepts the empty string),
// the device and - for a corpus with lines and a pattern with tables - the chunk index.
static int search_begin(const rrx_regex *re, const rrx_corpus *c, void *stream, const dev::SearchChunkDevice **ct) {
    const int rc = re->search_tables(c->device, ct);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return c->nlines && *ct ? chunk_index(c, stream) : RRX_OK;
}

int rrx_search_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !c || (c->nlines && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    const dev::SearchChunkDevice *ct;
    int rc = search_begin(re, c, stream, &ct);
    if (rc || !c->nlines) return rc;
    if (!ct) {
        // the pattern accepts the empty string: the accepted substring with the smallest end is [0, 0) in every string - no
        // table, no line offsets, two fills
        HIP_TRY(hipMemsetAsync(d_start, 0, c->nlines * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0, c->nlines * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_chunks(*ct, c->has_high, c->d_bytes, c->nbytes, c->d_chunk_base, c->nchunks, c->nlines, d_start, d_end, stream), "search_chunks launch");
}

// The LEFTMOST-LONGEST match of every line: rrx_search_longest_extents' tables, answer and shortcuts (item_search.cpp) with the
// corpus' lines as the items, a lane per stripe on the corpus' own stripe index - no line offsets, no chunk index, nothing read back.
int rrx_search_longest_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !c || !d_start || !d_end) return fail(RRX_ERR_ARG, "null argument");
    const dev::SearchLongestDevice *t;
    const int rc = tables_on(re, c->device, &rrx_regex::search_longest_tables, &t);
    if (rc || !c->nlines) return rc;
    if (!t) {                                                        // the empty language matches nowhere: two fills, no table, no text
        HIP_TRY(hipMemsetAsync(d_start, 0xff, c->nlines * sizeof(uint32_t), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(d_end, 0xff, c->nlines * sizeof(uint32_t), (hipStream_t)stream));
        return RRX_OK;
    }
    return launched(dev::search_longest_corpus_dfa(*t, re->requested == RRX_ENGINE_DFA_GLOBAL, re->search_longest.nullable, c->d_bytes, c->nbytes, c->stripe,
                                                   c->d_base, c->nstripes, d_start, d_end, stream),
                    "search_longest_corpus launch");
}

int rrx_search_all_count(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_count, void *stream) {
    if (!re || !c || (c->nlines && !d_count)) return fail(RRX_ERR_ARG, "null argument");
    const dev::SearchChunkDevice *ct;
    int rc = search_begin(re, c, stream, &ct);
    if (rc || !c->nlines) return rc;
    if (!ct) {                                                       // accepts "": a match at every offset of the line, its end included
        rc = line_offsets(c, stream);
        if (rc) return rc;
        return launched(dev::empty_matches(c->d_line_off, c->nlines, d_count, nullptr, nullptr, nullptr, stream), "empty_matches launch");
    }
    return launched(dev::search_chunks_count(*ct, c->has_high, c->d_bytes, c->nbytes, c->d_chunk_base, c->nchunks, d_count, stream), "search_chunks_count launch");
}

int rrx_search_all_fill(const rrx_regex *re, const rrx_corpus *c, const uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, void *stream) {
    if (!re || !c || (c->nlines && (!d_first || !d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    const dev::SearchChunkDevice *ct;
    int rc = search_begin(re, c, stream, &ct);
    if (rc || !c->nlines) return rc;
    if (!ct) {
        rc = line_offsets(c, stream);
        if (rc) return rc;
        return launched(dev::empty_matches(c->d_line_off, c->nlines, nullptr, d_first, d_start, d_end, stream), "empty_matches launch");
    }
    return launched(dev::search_chunks_fill(*ct, c->has_high, c->d_bytes, c->nbytes, c->d_chunk_base, c->nchunks, d_first, d_start, d_end, stream), "search_chunks_fill launch");
}

// count + fill in one call: one launch (decoupled look-back over the chunks' match counts).  A pattern that accepts the empty
// string: the line lengths, a device scan, a fill.
int rrx_search_all(const rrx_regex *re, const rrx_corpus *c, uint64_t *d_first, uint32_t *d_start, uint32_t *d_end, size_t cap, size_t *total,
                   void *stream) {
    if (!re || !c || !total || !d_first || (cap && (!d_start || !d_end))) return fail(RRX_ERR_ARG, "null argument");
    *total = 0;
    const dev::SearchChunkDevice *ct;
    int rc = search_begin(re, c, stream, &ct);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!c->nlines) return empty_batch({d_first}, stream);
    if (ct) {
        const size_t sb = dev::search_all_scratch_bytes(c->nchunks);
        {
            std::lock_guard<std::mutex> lock(c->mu);
            if (!c->d_all_scratch)
                if (hipError_t ae = c->d_all_scratch.alloc(c->device, sb)) return hip_fail(ae, "hipMalloc(&c->d_all_scratch, sb)");
        }
        HIP_TRY(hipMemsetAsync(c->d_all_scratch, 0, sb, st));
        int e = dev::search_chunks_all(*ct, c->has_high, c->d_bytes, c->nbytes, c->d_chunk_base, c->nchunks, c->nlines, d_first, d_start, d_end, cap,
                                       c->d_all_scratch, stream);
        if (e) return hip_fail((hipError_t)e, "search_chunks_all launch");
        uint64_t tail[2] = {0, 0};                                 // total, {ticket, error flag}
        HIP_TRY(hipMemcpyAsync(tail, static_cast<uint8_t *>(c->d_all_scratch) + c->nchunks * sizeof(uint64_t), sizeof tail, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (tail[1] >> 32) return fail(RRX_ERR_HIP, "search_all: a chunk's match count was never published (look-back gave up)");
        *total = (size_t)tail[0];
        return RRX_OK;
    }
    // accepts "": count (line length + 1), scan on the device, fill
    rc = line_offsets(c, stream);
    if (rc) return rc;
    DeviceArray<uint32_t> d_count;                                              // (both freed when the call leaves: hipFree waits for what is queued)
    DeviceArray<uint64_t> d_sums;
    if (hipError_t ae = d_count.alloc(c->device, (c->nlines + 1) * sizeof(uint32_t)))
        return hip_fail(ae, "hipMalloc(reinterpret_cast<void **>(&d_count), (c->nlines + 1) * sizeof(uint32_t))");
    hipError_t he = d_sums.alloc(c->device, dev::scan_scratch_words(c->nlines) * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc");
    int e = dev::empty_matches(c->d_line_off, c->nlines, d_count, nullptr, nullptr, nullptr, stream);
    if (e) return hip_fail((hipError_t)e, "empty_matches / scan launch");
    uint64_t tot = 0;
    rc = scan_total(d_count, d_first, d_sums, c->nlines, stream, "empty_matches / scan launch", "search_all scan", &tot);
    if (rc) return rc;
    *total = (size_t)tot;
    if (tot && cap) {                                                            // matches beyond `cap` are counted, not written (as rrx.h says)
        e = dev::empty_matches(c->d_line_off, c->nlines, nullptr, d_first, d_start, d_end, stream, cap);
        if (e) rc = hip_fail((hipError_t)e, "empty_matches launch");
        if (!rc) { he = hipStreamSynchronize(st); if (he != hipSuccess) rc = hip_fail(he, "search_all fill"); }
    }
    return rc;
}

}  // extern "C"
