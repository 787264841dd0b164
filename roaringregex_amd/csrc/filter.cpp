// filter.cpp — the rows a result bitmap selects, written as a new column: the generic entries on any bitmap (rrx_bitmap_rank,
// rrx_filter_sizes for an offsets column, rrx_filter_corpus_sizes for the lines of a corpus; the bytes are rrx_pieces_fill's) and the
// one-call "grep" forms rrx_filter_contains_* - the pattern's contains bitmap of the call's own, its rank, then the tail every sized
// column shares (items.hpp: SizedColumn) around the selected rows' triples and the fill (kernels_filter.hip, kernels_pieces_items.hip).
#include <functional>

#include "items.hpp"

using namespace rrx;

namespace {
// What the one-call forms differ in: how many rows there are, who answers contains, and who names the selected rows.
struct FilterSource {
    int device;
    const uint8_t *bytes;
    size_t nrows;
    std::function<int(uint32_t *d_bits, void *stream)> contains;
    std::function<int(const uint32_t *d_bits, const uint64_t *d_rank, uint64_t *d_row, uint32_t *d_len, uint64_t *d_src, uint32_t *d_flag, void *stream)> sizes;
};
struct FilterOut { uint64_t *d_row, *d_out_off; size_t rows_cap; void *d_out; size_t cap; size_t *nrows, *total; };

bool filter_out_ok(const FilterOut &o) { return o.d_out_off && o.nrows && o.total && (!o.rows_cap || o.d_row) && (!o.cap || o.d_out); }

// contains into a bitmap of the call's own, its rank, the number of selected rows read back; then the column's tail (items.hpp:
// SizedColumn): the selected rows' triples, the scan of their lengths and, if both caps hold, the bytes.
int filter_one_call(const FilterSource &s, bool invert, const FilterOut &o, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    *o.nrows = *o.total = 0;
    const size_t n = s.nrows, nwords = (n + 31) / 32;
    DeviceArray<uint32_t> d_bits;
    DeviceArray<uint64_t> d_rank;
    if (n) {
        hipError_t he = d_bits.alloc(s.device, nwords * sizeof(uint32_t));
        if (he == hipSuccess) he = d_rank.alloc(s.device, dev::bitmap_rank_words(n) * sizeof(uint64_t));
        if (he != hipSuccess) return hip_fail(he, "hipMalloc(filter bitmap)");
    }
    int rc = s.contains(d_bits, stream);           // (no rows: what the entry says about the pattern all the same)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(s.device));
    uint64_t nsel = 0;
    if (n) {
        const int le = dev::bitmap_rank(d_bits, n, invert, d_rank, stream);
        if (le) return hip_fail((hipError_t)le, "filter rank launch");
        HIP_TRY(hipMemcpyAsync(&nsel, d_rank + nwords, sizeof nsel, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *o.nrows = (size_t)nsel;
    if (!nsel) return empty_batch({o.d_out_off}, stream);
    const bool rows_fit = nsel <= o.rows_cap;
    SizedColumn col("filter", "a selected row of 2^30 bytes or more: use the contains entry and the generic entries rrx_bitmap_rank, rrx_filter_sizes / rrx_filter_corpus_sizes and rrx_pieces_fill");
    DeviceArray<uint64_t> d_src;
    hipError_t he = col.alloc(s.device, nsel, o.d_out_off, rows_fit);
    if (he == hipSuccess) he = d_src.alloc(s.device, nsel * sizeof(uint64_t));
    if (he != hipSuccess) return hip_fail(he, "hipMalloc(filter rows)");
    rc = col.sizes([&](uint32_t *d_len, uint32_t *d_flag) { return s.sizes(d_bits, d_rank, rows_fit ? o.d_row : nullptr, d_len, d_src, d_flag, stream); },
                   o.total, stream);
    if (rc) return rc;
    return col.fill(o.cap, [&] { return launched(dev::pieces_fill(s.bytes, d_src, col.off, nsel, static_cast<uint8_t *>(o.d_out), stream), "pieces_fill launch"); },
                    stream);
}
int filter_items_one_call(const ItemBatch &b, std::function<int(uint32_t *, void *)> contains, bool invert, const FilterOut &o, void *stream) {
    const FilterSource s{b.device, b.bytes, b.nitems, std::move(contains),
                         [&](const uint32_t *bits, const uint64_t *rank, uint64_t *row, uint32_t *len, uint64_t *src, uint32_t *flag, void *st) {
                             return launched(dev::filter_items(b.off, b.nitems, b.trim, bits, invert, rank, row, len, src, flag, st), "filter_items launch");
                         }};
    return filter_one_call(s, invert, o, stream);
}
}  // namespace

extern "C" {

size_t rrx_bitmap_rank_words(size_t nbits) { return dev::bitmap_rank_words(nbits); }

int rrx_bitmap_rank(int device, const uint32_t *d_bits, size_t nbits, int invert, uint64_t *d_rank, size_t rank_words, void *stream) {
    if (!d_rank || (nbits && !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    if (rank_words < dev::bitmap_rank_words(nbits)) return fail(RRX_ERR_ARG, "rank array shorter than rrx_bitmap_rank_words(nbits)");
    HIP_TRY(hipSetDevice(device));
    return launched(dev::bitmap_rank(d_bits, nbits, invert != 0, d_rank, stream), "bitmap_rank launch");
}

int rrx_filter_sizes(int device, const uint64_t *d_off, size_t nitems, uint32_t trim, const uint32_t *d_bits, int invert, const uint64_t *d_rank, uint64_t *d_row,
                     uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream) {
    if (nitems && (!d_off || !d_bits || !d_rank || !d_row || !d_piece_len || !d_piece_src)) return fail(RRX_ERR_ARG, "null argument");
    if (!nitems) return RRX_OK;
    HIP_TRY(hipSetDevice(device));
    return launched(dev::filter_items(d_off, nitems, trim, d_bits, invert != 0, d_rank, d_row, d_piece_len, d_piece_src, nullptr, stream), "filter_items launch");
}

int rrx_filter_corpus_sizes(const rrx_corpus *c, const uint32_t *d_bits, int invert, int keep_newline, const uint64_t *d_rank, uint64_t *d_row,
                            uint32_t *d_piece_len, uint64_t *d_piece_src, void *stream) {
    if (!c || !d_bits || !d_rank || !d_row || !d_piece_len || !d_piece_src) return fail(RRX_ERR_ARG, "null argument");
    if (!c->nlines) return RRX_OK;
    HIP_TRY(hipSetDevice(c->device));
    return launched(dev::filter_corpus(c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, c->nlines, d_bits, invert != 0, keep_newline != 0, d_rank, d_row,
                                       d_piece_len, d_piece_src, nullptr, stream),
                    "filter_corpus launch");
}

int rrx_filter_contains_extents(const rrx_regex *re, int device, const void *d_bytes, const uint64_t *d_off, size_t nitems, uint32_t trim, int invert,
                                uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap, void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream) {
    const ItemBatch b = batch_of(device, d_bytes, d_off, nitems, trim);
    const FilterOut o{d_row, d_out_off, rows_cap, d_out, cap, nrows, total};
    if (!batch_args_ok(re, b, {}) || !filter_out_ok(o)) return fail(RRX_ERR_ARG, "null argument");
    return filter_items_one_call(b, [&](uint32_t *bits, void *st) { return rrx_contains_extents(re, device, d_bytes, d_off, nitems, trim, bits, st); },
                                 invert != 0, o, stream);
}
int rrx_filter_contains_items(const rrx_regex *re, const rrx_items *it, int invert, uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap, void *d_out, size_t cap,
                              size_t *nrows, size_t *total, void *stream) {
    const FilterOut o{d_row, d_out_off, rows_cap, d_out, cap, nrows, total};
    if (!it || !batch_args_ok(re, batch_of(it), {}) || !filter_out_ok(o)) return fail(RRX_ERR_ARG, "null argument");
    return filter_items_one_call(batch_of(it), [&](uint32_t *bits, void *st) { return rrx_contains_items(re, it, bits, st); }, invert != 0, o, stream);
}
int rrx_filter_contains_corpus(const rrx_regex *re, const rrx_corpus *c, int invert, int keep_newline, uint64_t *d_row, uint64_t *d_out_off, size_t rows_cap,
                               void *d_out, size_t cap, size_t *nrows, size_t *total, void *stream) {
    const FilterOut o{d_row, d_out_off, rows_cap, d_out, cap, nrows, total};
    if (!re || !c || !filter_out_ok(o)) return fail(RRX_ERR_ARG, "null argument");
    FilterSource s{c->device, c->d_bytes, c->nlines, [&](uint32_t *bits, void *st) { return rrx_contains_corpus(re, c, bits, st); },
                   [&](const uint32_t *bits, const uint64_t *rank, uint64_t *row, uint32_t *len, uint64_t *src, uint32_t *flag, void *st) {
                       return launched(dev::filter_corpus(c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, c->nlines, bits, invert != 0, keep_newline != 0,
                                                          rank, row, len, src, flag, st),
                                       "filter_corpus launch");
                   }};
    return filter_one_call(s, invert != 0, o, stream);
}

}  // extern "C"
