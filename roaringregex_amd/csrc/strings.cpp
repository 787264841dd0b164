// strings.cpp — single strings (rrx_match_string, rrx_match_cstr): one device-resident string of any length, on the chunk maps or as
// one item of rrx_match_extents.
#include <cstring>

#include "handles.hpp"

using namespace rrx;

static constexpr size_t kLongStringBytes = 32 * 1024;   // shorter single strings stay on one lane (NFA engines)
// Table engines: the chunk maps by convergence cost a handful of short launches (60-80 us), a sequential lane 94 ns per byte
// (tools/probe/facade_latency.py: 1.9 ms for 20 KB against 59 us; 130 us for 1 KB): from 1 KiB on the chunks win.
static constexpr size_t kLongStringBytesTable = 1024;
static constexpr uint32_t kLongNfaMaxBits = 256;        // NFA engines: chunk relations cost bytes x positions lane steps

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
