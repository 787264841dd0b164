// strings.cpp — single strings: whole-string acceptance (rrx_match_string, rrx_match_cstr: one device-resident string of any
// length, on the chunk maps or as one item of rrx_match_extents) and the leftmost-longest match inside one
// (rrx_search_longest_string, rrx_contains_string: directional runs on the chunk maps, or one item of rrx_search_longest_extents).
#include <algorithm>
#include <cstring>

#include "items.hpp"

using namespace rrx;

static constexpr size_t kLongStringBytes = 32 * 1024;   // shorter single strings stay on one lane (NFA engines)
// Table engines: the chunk maps by convergence cost a handful of short launches (60-80 us), a sequential lane 94 ns per byte
// (tools/probe/facade_latency.py: 1.9 ms for 20 KB against 59 us; 130 us for 1 KB): from 1 KiB on the chunks win.
static constexpr size_t kLongStringBytesTable = 1024;
static constexpr uint32_t kLongNfaMaxBits = 256;        // NFA engines: chunk relations cost bytes x positions lane steps
// Leftmost-longest search in one string: shorter strings are one item of the lane-per-item kernel.  Measured on URL text
// (tools/probe/search_string_rate.py, profiles/search_longest_string_rate.txt; on a library built with 256 here - the Makefile's
// search-from256 - so that the chunk route is timed below the crossing too): the chunk route costs 220-245 us from 512 bytes to
// 64 KiB (its launches and read-backs), the single lane 27 us + 74 ns per byte; they cross near 2.6 KiB - 2 KiB is the nearest power
// of two (at 2 KiB the chunks lose, 224 us against 180; at 4 KiB they win, 228 against 324).
#ifndef RRX_LONG_SEARCH_STRING_BYTES
#define RRX_LONG_SEARCH_STRING_BYTES 2048
#endif
static constexpr size_t kLongSearchStringBytes = RRX_LONG_SEARCH_STRING_BYTES;
// The forward pass runs in windows, each entered in the state the one before was left in: the first ends at the last 16-byte
// aligned ADDRESS within kLongSearchFirstWindow bytes of the match start (one chunk, one lane; every later window then begins
// aligned), and each later one is kLongSearchWindowGrowth times everything walked so far - a short match costs a short walk, a
// match of L bytes walks less than 16 L, and 1 GiB is seven windows.
static constexpr size_t kLongSearchFirstWindow = 256, kLongSearchWindowGrowth = 15;

extern "C" {

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

// ---- the leftmost-longest match inside one long string
namespace {

constexpr uint64_t kNoSpan = ~0ull;
constexpr size_t kRunHeader = 64;      // in front of the runs' scratch: the start word of a first run, the result record behind it

// One item of rrx_search_longest_extents, its two words widened.  `scratch`: kRunHeader bytes.
int search_string_one_item(const rrx_regex *re, int device, const uint8_t *d_bytes, size_t nbytes, uint8_t *scratch, uint64_t span[2], hipStream_t st) {
    if (nbytes > 0xFFFFFFFEull)
        return fail(RRX_ERR_UNSUPPORTED, "search_longest_string: a string beyond 0xFFFFFFFE bytes on the one-item path (a table beyond 254 states, or "
                                         "RRX_ENGINE_DFA_GLOBAL) would be searched in part only");
    const uint64_t off[2] = {0, nbytes};
    uint64_t *d_off = reinterpret_cast<uint64_t *>(scratch);
    uint32_t *d_words = reinterpret_cast<uint32_t *>(scratch + sizeof off);
    hipError_t e = hipMemcpyAsync(d_off, off, sizeof off, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                    // `off` leaves scope
    if (e != hipSuccess) return hip_fail(e, "extent upload");
    const int rc = rrx_search_longest_extents(re, device, d_bytes, d_off, 1, 0, d_words, d_words + 1, st);
    if (rc) return rc;
    uint32_t words[2] = {0, 0};
    e = hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "search_longest_string readback");
    for (int i = 0; i < 2; i++) span[i] = words[0] == ~0u ? kNoSpan : words[i];
    return RRX_OK;
}

// One directional run and its record read back: one synchronise
int run_and_read(const dev::DfaDevice &p, bool backward, bool row0_dead, const uint8_t *d_bytes, size_t nbytes, const uint32_t *d_state, uint8_t *scratch,
                 dev::LongRunResult *d_rec, dev::LongRunResult *rec, hipStream_t st) {
    const int rc = launched(dev::long_run_dfa(p, backward, row0_dead, d_bytes, nbytes, d_state, scratch + kRunHeader, d_rec, st), "long_run launch");
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(rec, d_rec, sizeof *rec, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? RRX_OK : hip_fail(e, "long_run readback");
}

// The chunk route: span[0] = the start (backwards on starts), span[1] = the end (forwards on anchored, in windows); with
// `start_only` span[1] is the start too.  `scratch`: kRunHeader bytes and the runs' scratch behind them.
int search_string_chunks(const rrx_regex *re, const dev::SearchLongestDevice *t, const uint8_t *d_bytes, size_t nbytes, bool start_only, uint8_t *scratch,
                         uint64_t span[2], hipStream_t st) {
    int rc = RRX_OK;
    uint32_t *d_state = reinterpret_cast<uint32_t *>(scratch);
    dev::LongRunResult *d_rec = reinterpret_cast<dev::LongRunResult *>(scratch + 16), rec = {};
    // ---- backwards on starts over the whole string: the smallest start (a nullable pattern starts at 0)
    uint64_t start = 0;
    if (!re->search_longest.nullable) {
        rc = launched(dev::long_set_word(d_state, t->starts.start, st), "long_set_word launch");
        if (!rc) rc = run_and_read(t->starts, true, false, d_bytes, nbytes, d_state, scratch, d_rec, &rec, st);
        if (rc || rec.extreme == kNoSpan) return rc;
        start = rec.extreme;
    }
    span[0] = span[1] = start;
    if (start_only) return RRX_OK;
    // ---- forwards on anchored from the start, window after window, until row 0 (dead and absorbing) or the string's end
    rc = launched(dev::long_set_word(d_state, t->anchored.start, st), "long_set_word launch");
    size_t pos = (size_t)start;
    const uint32_t *d_entered = d_state;
    while (!rc && pos < nbytes) {
        const size_t walked = pos - (size_t)start;
        size_t len = walked ? walked * kLongSearchWindowGrowth : kLongSearchFirstWindow - (reinterpret_cast<uintptr_t>(d_bytes + pos) & 15);
        len = std::min(len, nbytes - pos);
        rc = run_and_read(t->anchored, false, true, d_bytes + pos, len, d_entered, scratch, d_rec, &rec, st);
        if (rc) break;
        if (rec.extreme != kNoSpan) span[1] = pos + rec.extreme;
        pos += len;
        d_entered = &d_rec->exit_state;                                      // (read by the next run before it writes its record)
        if (rec.exit_state == 0) break;
    }
    return rc;
}

// span = what rrx_search_longest_extents gives for the one item made of the whole string, widened (kNoSpan in both: no match); with
// `start_only` the start alone is asked for.
int search_string(const rrx_regex *re, int device, const uint8_t *d_bytes, size_t nbytes, bool start_only, uint64_t span[2], hipStream_t st) {
    span[0] = span[1] = kNoSpan;
    const dev::SearchLongestDevice *t;
    int rc = tables_on(re, device, &rrx_regex::search_longest_tables, &t);
    if (rc || !t) return rc;                                                 // (the empty language: no kernel)
    const bool chunks = nbytes >= kLongSearchStringBytes && re->requested != RRX_ENGINE_DFA_GLOBAL && t->starts.nstates <= dev::kLongMaxStates &&
                        t->anchored.nstates <= dev::kLongMaxStates;
    std::lock_guard<std::mutex> lock(re->scratch_mu);
    void *mem = nullptr;
    rc = re->scratch_for(device, kRunHeader + (chunks ? dev::long_run_scratch_bytes(std::max(t->starts.nstates, t->anchored.nstates), nbytes) : 0), &mem);
    if (rc) return rc;
    uint8_t *scratch = static_cast<uint8_t *>(mem);
    rc = chunks ? search_string_chunks(re, t, d_bytes, nbytes, start_only, scratch, span, st)
                : search_string_one_item(re, device, d_bytes, nbytes, scratch, span, st);
    if (rc) (void)hipStreamSynchronize(st);              // the scratch is reused by the next call: nothing of a failed one stays queued on it
    return rc;
}

int upload_and_wait(void *d_dst, const void *src, size_t n, hipStream_t st, const char *what) {
    hipError_t e = hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);                        // `src` leaves scope; the entry is synchronous
    return e == hipSuccess ? RRX_OK : hip_fail(e, what);
}

}  // namespace

extern "C" {

int rrx_search_longest_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint64_t *d_span, void *stream) {
    if (!re || (nbytes && !d_bytes) || !d_span) return fail(RRX_ERR_ARG, "null argument");
    uint64_t span[2];
    const int rc = search_string(re, device, static_cast<const uint8_t *>(d_bytes), nbytes, false, span, static_cast<hipStream_t>(stream));
    return rc ? rc : upload_and_wait(d_span, span, sizeof span, static_cast<hipStream_t>(stream), "search_longest_string");
}

int rrx_contains_string(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint8_t *d_found, void *stream) {
    if (!re || (nbytes && !d_bytes) || !d_found) return fail(RRX_ERR_ARG, "null argument");
    uint64_t span[2];
    const int rc = search_string(re, device, static_cast<const uint8_t *>(d_bytes), nbytes, true, span, static_cast<hipStream_t>(stream));
    if (rc) return rc;
    const uint8_t found = span[0] != kNoSpan;
    return upload_and_wait(d_found, &found, 1, static_cast<hipStream_t>(stream), "contains_string");
}

}  // extern "C"
