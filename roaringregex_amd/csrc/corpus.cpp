// corpus.cpp — rrx_corpus (the line index of a device-resident text) and what runs on it in batches: match, contains, the
// sampled-table launch; the bitmap helpers, the one-shot entry, the host pipeline; the mailbox (handles.hpp).
#include <algorithm>
#include <cstring>

#include "handles.hpp"

using namespace rrx;

namespace {
constexpr int kMailSlots = 64, kMailWords = 8;
struct MailPage { uint64_t *host = nullptr, *dev = nullptr; std::vector<int> free_slots; };
std::mutex g_mail_mu;
std::map<int, MailPage> g_mail;
}  // namespace
int mailbox_acquire(int device, Mailbox *out) {
    std::lock_guard<std::mutex> lock(g_mail_mu);
    MailPage &pg = g_mail[device];
    if (!pg.host) {
        PinnedAlloc h;
        void *d = nullptr;
        hipError_t e = h.alloc(kMailSlots * kMailWords * sizeof(uint64_t), hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h.p, 0);
        if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(mailbox)");
        pg.host = static_cast<uint64_t *>(h.release()); pg.dev = static_cast<uint64_t *>(d);
        for (int i = kMailSlots - 1; i >= 0; i--) pg.free_slots.push_back(i);
    }
    if (pg.free_slots.empty()) return fail(RRX_ERR_HIP, "more than 64 synchronous calls in flight on one device");
    out->slot = pg.free_slots.back(); pg.free_slots.pop_back();
    out->device = device;
    out->host = pg.host + (size_t)out->slot * kMailWords;
    out->dev = pg.dev + (size_t)out->slot * kMailWords;
    return RRX_OK;
}
void mailbox_release(const Mailbox &m) {
    if (m.slot < 0) return;
    std::lock_guard<std::mutex> lock(g_mail_mu);
    g_mail[m.device].free_slots.push_back(m.slot);
}

static constexpr uint32_t kSampleGroups = 8, kSampleBytes = 256;     // 8 x 32 lanes x 128 pair steps = 1024 half-waves, 64 KiB
static constexpr size_t kSampleMinCorpus = (size_t)64 << 20;         // smaller corpora: the order search (tens of ms) would not pay

extern "C" {

int rrx_corpus_create(int device, const void *d_bytes, size_t nbytes, void *stream, rrx_corpus **out) {
    return rrx_corpus_create_ex(device, d_bytes, nbytes, 0, stream, out);
}

int rrx_corpus_create_ex(int device, const void *d_bytes, size_t nbytes, uint32_t stripe_bytes, void *stream, rrx_corpus **out) {
    if (!out || (nbytes && !d_bytes)) return fail(RRX_ERR_ARG, "null argument");
    if (stripe_bytes && (stripe_bytes < dev::kMinStripe || stripe_bytes > dev::kMaxStripe || (stripe_bytes & (stripe_bytes - 1))))
        return fail(RRX_ERR_ARG, "stripe must be a power of two in [512, 16384]");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(RRX_ERR_ARG, "corpus base must be 16-byte aligned");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<rrx_corpus> c(new rrx_corpus());     // (its memory goes with it on every early return)
    c->device = device;
    c->d_bytes = static_cast<const uint8_t *>(d_bytes);
    c->nbytes = nbytes;
    c->stripe = stripe_bytes ? stripe_bytes : dev::pick_stripe(nbytes);
    // automatic choice on a large corpus: the line length is taken from its first 4 MiB first (two small launches), so
    // that a corpus of very short or very long lines is indexed once, not twice (the check below still stands)
    constexpr size_t kSample = (size_t)4 << 20;
    if (!stripe_bytes && nbytes >= 16 * kSample) {
        rrx_corpus *sample = nullptr;
        if (rrx_corpus_create_ex(device, d_bytes, kSample, dev::pick_stripe(kSample), stream, &sample) == RRX_OK && sample) {
            if (sample->nlines) c->stripe = dev::stripe_for_lines(nbytes, kSample / sample->nlines);
            rrx_corpus_free(sample);
        }
    }
    c->nstripes = (nbytes + c->stripe - 1) / c->stripe;
    hipError_t e = c->d_counts.alloc(device, (c->nstripes + 3) * sizeof(uint32_t));
    if (e == hipSuccess) e = c->d_base.alloc(device, (c->nstripes + 1 + dev::scan_scratch_words(c->nstripes)) * sizeof(uint64_t));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(line index)");
    uint32_t *d_flags = c->d_counts + c->nstripes;
    e = hipMemsetAsync(d_flags, 0, 3 * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(flags)");
    int rc = dev::count_newlines_per_stripe(c->d_bytes, nbytes, c->stripe, c->d_counts, c->nstripes, d_flags, stream);
    if (!rc) rc = dev::scan_counts(c->d_counts, c->d_base, c->d_base + c->nstripes + 1, c->nstripes, stream);
    if (!rc && c->nstripes) rc = dev::own_words_check(c->d_base, c->nstripes, c->d_bytes + nbytes - 1, d_flags + 1, stream);
    if (rc) return hip_fail((hipError_t)rc, "line index launch");
    MailboxGuard mail;
    if (int mrc = mailbox_acquire(device, &mail.m)) return mrc;
    if (nbytes >= kSampleMinCorpus && c->nstripes >= 64 * kSampleGroups &&
        c->h_sample.alloc((size_t)kSampleGroups * 32 * kSampleBytes) == hipSuccess) {
        c->sample_lanes = kSampleGroups * 32;
        for (uint32_t g = 0; g < kSampleGroups; g++) {            // group g: 32 consecutive stripes, the groups spread over the corpus
            const size_t first_stripe = (size_t)g * (c->nstripes / kSampleGroups);
            if (hipMemcpy2DAsync(c->h_sample + (size_t)g * 32 * kSampleBytes, kSampleBytes, c->d_bytes + first_stripe * c->stripe, c->stripe,
                                 kSampleBytes, 32, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize((hipStream_t)stream);      // the copies of the groups before this one may still be writing the buffer
                c->h_sample.reset(); c->sample_lanes = 0;
                break;
            }
        }
    }
    mail.stream = (hipStream_t)stream; mail.queued = true;
    rc = dev::mail_results(c->d_base + c->nstripes, d_flags, nbytes ? c->d_bytes + nbytes - 1 : nullptr, mail.m.dev, stream, d_flags + 1);
    if (rc) return hip_fail((hipError_t)rc, "line index launch");
    e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "line index readback");
    mail.drained = true;
    const uint64_t total = mail.m.host[0];
    const uint32_t flags = (uint32_t)mail.m.host[1];
    const uint8_t last = nbytes ? (uint8_t)mail.m.host[2] : (uint8_t)'\n';
    c->has_high = (flags & 1u) != 0;
    c->own_words = c->nstripes && mail.m.host[3] == 0;
    c->own_span = (uint32_t)mail.m.host[4];
    c->nlines = (size_t)total + ((nbytes && last != '\n') ? 1 : 0);
    // with the line count known: the stripe this corpus wants (stripe_for_lines); if it is another one, index once more
    if (!stripe_bytes && c->nlines) {
        const uint32_t want = dev::stripe_for_lines(nbytes, nbytes / c->nlines);
        if (want != c->stripe) {
            c.reset();                                   // (the first index goes before the second one is allocated)
            return rrx_corpus_create_ex(device, d_bytes, nbytes, want, stream, out);
        }
    }
    *out = c.release();
    return RRX_OK;
}
size_t rrx_corpus_num_lines(const rrx_corpus *c) { return c->nlines; }
size_t rrx_corpus_num_bytes(const rrx_corpus *c) { return c->nbytes; }
uint32_t rrx_corpus_stripe_bytes(const rrx_corpus *c) { return c->stripe; }
int rrx_corpus_one_launch(const rrx_corpus *c, uint32_t *span_words) {
    if (span_words) *span_words = c->own_words ? c->own_span : 0;
    return c->own_words ? 1 : 0;
}
void rrx_corpus_free(rrx_corpus *c) { delete c; }

size_t rrx_corpus_bitmap_words(const rrx_corpus *c) { return (c->nlines + 31) / 32; }

// The batch entry on the sampled table: the stride-2 kernel with two result bits per line (accepted, escaped), the two bitmaps
// taken apart, the escaped lines decided by the NFA lane engine.  Scratch (the wide bitmap, the escaped bitmap, the list) is the
// regex' event-ordered per-device buffer, the count of escaped lines its own 16 bytes per device (sampled_escapes: read by
// rrx_sampled_escapes); everything is queued on `stream`, nothing is read back.
static int match_corpus_sampled(const rrx_regex *re, const rrx_corpus *c, const DeviceTables *t, uint32_t *d_accept_bits, void *stream) {
    dev::Dfa2Device d2;
    int rc = re->sampled_tables(c->device, &d2);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t words = rrx_corpus_bitmap_words(c);
    const size_t wide_bytes = (2 * words * sizeof(uint32_t) + 15) & ~(size_t)15, esc_bytes = (words * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t cap = std::max<size_t>(words / 2, 1024);                        // listed escaped lines: 1.5 % of the lines (then: the walk over the stripes)
    std::lock_guard<std::mutex> lock(re->onepass_mu);
    void *buf = nullptr;
    rc = re->onepass_for(c->device, wide_bytes + esc_bytes + cap * sizeof(uint64_t), &buf, st);
    if (rc) return rc;
    uint32_t *wide = static_cast<uint32_t *>(buf);
    uint32_t *escaped = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(buf) + wide_bytes);
    uint64_t *list = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(buf) + wide_bytes + esc_bytes);
    DeviceAlloc &count = re->sampled_dev.escapes[c->device];
    if (!count.p) HIP_TRY(count.alloc(c->device, 16));
    unsigned long long *total = static_cast<unsigned long long *>(count.p);
    constexpr uint32_t kSlots = kSampledRelearns + 1;                            // a pinned counter per table generation
    PinnedArray<unsigned long long> &all_seen = re->sampled_dev.seen;
    if (!all_seen && all_seen.alloc(kSlots * sizeof(unsigned long long)) == hipSuccess)
        for (uint32_t k = 0; k < kSlots; k++) all_seen[k] = 0;
    unsigned long long *const seen = all_seen ? all_seen + re->sampled.seen_slot() : nullptr;
    // what the last FINISHED launch counted, against the size of the last launch queued (the same corpus in a scan loop; otherwise a hint)
    if (seen) re->sampled.judge(seen[0]);
    hipError_t he = hipMemsetAsync(wide, 0, wide_bytes, st);                     // (the kernel merges words with atomic OR)
    if (he == hipSuccess) he = hipMemsetAsync(total, 0, 16, st);
    int e = he != hipSuccess ? (int)he : dev::match_stripes_dfa2_two_bit(d2, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, wide, stream);
    if (!e) e = dev::split_two_bit(wide, c->nlines, d_accept_bits, escaped, total, list, cap, stream);
    if (!e) e = dev::recheck_escaped_nfa(t->nfa, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, escaped, c->nlines, list, total, cap, d_accept_bits, stream);
    if (!e && seen) {                                                            // behind the kernels: the count into pinned memory (nobody waits for it)
        if (hipMemcpyAsync(seen, total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) (void)hipGetLastError();
        re->sampled.queued(c->nlines);
    }
    const int rc2 = re->onepass_done(c->device, st);
    if (e) return hip_fail((hipError_t)e, "sampled-table launch");
    return rc2;
}

// The exchange slots of `c` for a launch on `stream` that needs no cleared bitmap, or nullptr: the launch clears.  That is the
// case where the corpus' index says so (three workgroups in one word), where a workgroup's range is longer than the window the
// regex' table leaves, and on a stream that is being captured: a graph may be replayed on any stream, beside launches that use
// the array of this one, and nothing is allocated during a capture.
static unsigned long long *own_words_for(const rrx_corpus *c, const dev::Dfa2Device &d2, hipStream_t stream) {
    if (!c->own_words || c->own_span >= dev::dfa2_window_words(d2)) return nullptr;
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (capture != hipStreamCaptureStatusNone) return nullptr;
    std::lock_guard<std::mutex> lock(c->mu);
    auto it = c->slot_arrays.find(stream);
    if (it != c->slot_arrays.end()) return it->second;
    if (c->slot_arrays.size() >= rrx_corpus::kMaxSlotArrays) return nullptr;
    const size_t bytes = ((c->nstripes + dev::kThreads - 1) / dev::kThreads + 1) * sizeof(unsigned long long);
    DeviceArray<unsigned long long> slots;
    if (slots.alloc(c->device, bytes) != hipSuccess || hipMemsetAsync(slots, 0, bytes, stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return c->slot_arrays.emplace(stream, std::move(slots)).first->second;
}
static uint32_t flush_mask_of(const rrx_regex *re, const rrx_corpus *c) {
    return re->opt_flush_slots.load() ? (uint32_t)re->opt_flush_slots.load() - 1u : dev::flush_mask_for(c->nbytes, c->nlines);
}
uint32_t rrx_match_flush_slots(const rrx_regex *re, const rrx_corpus *c, int *compiled_in) {
    const uint32_t mask = flush_mask_of(re, c);
    if (compiled_in) *compiled_in = dev::dfa2_flush_at_compile_time(mask) ? 1 : 0;
    return mask + 1;
}

// The table engine of a LineTables on a corpus: the stride-2 table where there is one - on a corpus with bytes >= 0x80 only if
// the caller allows the instantiation that steps them as 0x00 (stride2_over_high) -, else the line table.  The kernels merge
// words with atomic OR into a bitmap that is cleared here first - but for the stride-2 kernel where it can settle every word
// itself (own_words_for): that call is ONE launch.
static int launch_line_tables(const rrx_regex *re, const rrx_corpus *c, const LineTables &lt, const DeviceTables *t, bool stride2_over_high, uint32_t *bits,
                              void *stream) {
    const size_t words = rrx_corpus_bitmap_words(c);
    const bool stride2 = lt.has_dfa2 && (!c->has_high || stride2_over_high);
    dev::Dfa2Device d2;
    unsigned long long *slots = nullptr;
    if (stride2) { d2 = re->dfa2_device(t); slots = own_words_for(c, d2, (hipStream_t)stream); }
    if (!slots) HIP_TRY(hipMemsetAsync(bits, 0, words * sizeof(uint32_t), (hipStream_t)stream));
    if (!stride2) return launched(dev::match_stripes_dfa(t->line, c->has_high, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, bits, stream), "match_stripes launch");
    return launched(dev::match_stripes_dfa2(d2, c->has_high, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, bits, stream, flush_mask_of(re, c), slots, words),
                    "match_stripes launch");
}

int rrx_match_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_accept_bits, void *stream) {
    if (!re || !c || (c->nlines && !d_accept_bits)) return fail(RRX_ERR_ARG, "null argument");
    if (!re->t2_order.decided() && c->h_sample && !c->has_high) (void)re->decide_t2_order(c->h_sample, c->sample_lanes, kSampleBytes, /*now=*/false);
    const DeviceTables *t;
    int rc = re->tables(c->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->nlines) return RRX_OK;
    // the sampled table: its build starts at the first match against a corpus that carries a text sample (in the background;
    // this launch and the next ones run on the NFA engine until it is in), and serves corpora without bytes >= 0x80
    const bool sampled_on = re->opt_sampled_table.load() != 0;
    if (re->sampled.eligible() && sampled_on && !c->has_high) {
        const bool beside = re->opt_background_order.load() != 0;
        if (c->h_sample) (void)re->sampled.start_first(c->h_sample, c->sample_lanes, kSampleBytes, beside);      // (nothing if decided before)
        if (c->h_sample && re->sampled.ready() && re->sampled.retired())
            re->sampled.start_relearn(c->h_sample, c->sample_lanes, kSampleBytes, beside);     // (this launch and the next ones: the NFA engine, until the new table is in)
        if (re->sampled.in_use(sampled_on)) return match_corpus_sampled(re, c, t, d_accept_bits, stream);
    }
    // (a corpus with bytes >= 0x80 leaves the stride-2 table for the byte-stride one)
    if (re->engine == RRX_ENGINE_DFA)                                        // (every table engine: plan_engines)
        return launch_line_tables(re, c, re->match, t, /*stride2_over_high=*/false, d_accept_bits, stream);
    // the NFA kernels merge words with atomic OR: start from an all-zero bitmap
    HIP_TRY(hipMemsetAsync(d_accept_bits, 0, rrx_corpus_bitmap_words(c) * sizeof(uint32_t), (hipStream_t)stream));
    int e = 0;
    switch (re->engine) {
    case RRX_ENGINE_NFA_SPARSE: e = dev::match_stripes_sparse_nfa(t->block, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream); break;
    case RRX_ENGINE_NFA_BLOCK: e = dev::match_stripes_wave_nfa(t->block, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream); break;
    case RRX_ENGINE_NFA_WAVE: e = dev::match_stripes_group_nfa(t->group, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream); break;
    default: e = dev::match_stripes_nfa(t->nfa, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream);
    }
    return launched(e, "match_stripes launch");
}

// "Which lines contain a match": the batch kernels of rrx_match_corpus on the contains table (build_contains).  On a corpus with
// bytes >= 0x80 the stride-2 table keeps its kernel - the instantiation that steps such bytes as 0x00, which is their class.
int rrx_contains_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_bits, void *stream) {
    if (!re || !c || (c->nlines && !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    // RRX_OPT_CONTAINS_NFA: the line engine with a sticky `found` on the program with the contains B rows - a clear and one kernel
    bool on_nfa = false, fill = false;
    const dev::NfaDevice *nfa = nullptr;
    int rc = re->contains_nfa_tables(c->device, &on_nfa, &nfa, &fill);
    if (rc) return rc;
    if (on_nfa) {
        HIP_TRY(hipSetDevice(c->device));
        if (!c->nlines) return RRX_OK;
        rc = fill_bitmap(d_bits, c->nlines, fill, stream);                  // (the kernels merge words with atomic OR)
        if (rc || !nfa) return rc;
        return launched(dev::contains_stripes_nfa(*nfa, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_bits, stream), "contains_stripes launch");
    }
    const DeviceTables *t;
    rc = re->contains_tables(c->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->nlines) return RRX_OK;
    return launch_line_tables(re, c, re->contains_set.lt, t, /*stride2_over_high=*/true, d_bits, stream);
}
int rrx_bitmap_count(int device, const uint32_t *d_bits, size_t nlines, uint64_t *d_count, void *stream) {
    if (!d_count || (nlines && !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit atomics");
    return launched(dev::bitmap_count(d_bits, nlines, reinterpret_cast<unsigned long long *>(d_count), stream), "bitmap_count launch");
}

// One-shot entry: a device-resident buffer that nobody has indexed.  With the lane engines (tables and NFA) the text is
// read ONCE: the match kernel counts the '\n' of every stripe on the side and leaves every lane's verdicts as a stream of
// its own; a scan of the counts and a small compaction kernel then put the streams at their line numbers.  The
// cooperative engines build the index first (two passes).  Synchronous: *nlines is read back.
int rrx_match_device(const rrx_regex *re, int device, const void *d_bytes, size_t nbytes, uint32_t *d_accept_bits, size_t cap_words,
                     size_t *nlines, void *stream) {
    if (!re || (nbytes && !d_bytes) || !nlines || (cap_words && !d_accept_bits)) return fail(RRX_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(RRX_ERR_ARG, "corpus base must be 16-byte aligned");
    *nlines = 0;
    HIP_TRY(hipSetDevice(device));
    if (!nbytes) return RRX_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // cooperative engines: two passes (index, then match) - and so does a regex that runs on its sampled table: the index pass and the
    // table kernel (1.4 + 2.1 ms per 8 GiB of URL text) are a fifth of the NFA lane engine's one pass (16.7 ms)
    const bool sampled = re->sampled.in_use(re->opt_sampled_table.load() != 0);
    if ((re->engine != RRX_ENGINE_DFA && re->engine != RRX_ENGINE_NFA) || sampled) {
        rrx_corpus *c = nullptr;
        int rc = rrx_corpus_create(device, d_bytes, nbytes, stream, &c);
        if (rc) return rc;
        *nlines = c->nlines;
        if (rrx_corpus_bitmap_words(c) > cap_words) rc = fail(RRX_ERR_ARG, "accept bitmap too small for the number of strings");
        if (!rc) rc = rrx_match_corpus(re, c, d_accept_bits, stream);
        const hipError_t e = hipStreamSynchronize(st);                      // the index arrays of `c` are freed next
        if (!rc && e != hipSuccess) rc = hip_fail(e, "match_device");
        rrx_corpus_free(c);
        return rc;
    }
    const DeviceTables *t;
    int rc = re->tables(device, &t);
    if (rc) return rc;
    const uint8_t *bytes = static_cast<const uint8_t *>(d_bytes);
    const uint32_t stripe = dev::pick_stripe(nbytes);
    const size_t nstripes = (nbytes + stripe - 1) / stripe;
    // scratch: [counts u32 (nstripes) | flag u32 | pad] [base u64 (nstripes + 1) + scan scratch] [slabs u32]
    const size_t counts_bytes = ((nstripes + 2) * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t base_bytes = (nstripes + 1 + dev::scan_scratch_words(nstripes)) * sizeof(uint64_t);
    const size_t slab_bytes = dev::onepass_slab_words(nstripes, stripe) * sizeof(uint32_t);
    std::lock_guard<std::mutex> lock(re->onepass_mu);
    void *buf = nullptr;
    rc = re->onepass_for(device, counts_bytes + base_bytes + slab_bytes, &buf, st);
    if (rc) return rc;
    uint32_t *d_counts = static_cast<uint32_t *>(buf);
    uint64_t *d_base = reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(buf) + counts_bytes);
    uint32_t *d_slabs = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(buf) + counts_bytes + base_bytes);
    MailboxGuard mail;
    rc = mailbox_acquire(device, &mail.m);
    if (rc) return rc;
    if (cap_words) HIP_TRY(hipMemsetAsync(d_accept_bits, 0, cap_words * sizeof(uint32_t), st));
    int e = re->engine == RRX_ENGINE_NFA ? dev::match_onepass_nfa(t->nfa, bytes, nbytes, stripe, nstripes, d_counts, d_slabs, stream)
            : re->match.has_dfa2         ? dev::match_onepass_dfa2(re->dfa2_device(t), bytes, nbytes, stripe, nstripes, d_counts, d_slabs, stream)
                                         : dev::match_onepass_dfa(t->line, bytes, nbytes, stripe, nstripes, d_counts, d_slabs, stream);
    if (!e) e = dev::scan_counts(d_counts, d_base, d_base + nstripes + 1, nstripes, stream);
    // (words beyond the caller's bitmap are dropped by the compaction; whether there were any follows from the line count)
    if (!e) e = dev::compact_streams(d_counts, d_base, nstripes, stripe, d_slabs, d_accept_bits, cap_words, stream);
    mail.stream = st; mail.queued = true;
    if (!e) e = dev::mail_results(d_base + nstripes, nullptr, bytes + nbytes - 1, mail.m.dev, stream);
    if (e) return hip_fail((hipError_t)e, "one-pass launch");
    const hipError_t he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "one-pass readback");
    mail.drained = true;
    *nlines = (size_t)mail.m.host[0] + ((uint8_t)mail.m.host[2] != '\n' ? 1 : 0);
    if ((*nlines + 31) / 32 > cap_words) return fail(RRX_ERR_ARG, "accept bitmap too small for the number of strings");
    return RRX_OK;
}

int rrx_bitmap_to_bytes(int device, const uint32_t *d_bits, size_t nlines, uint8_t *d_accept, void *stream) {
    if (nlines && (!d_bits || !d_accept)) return fail(RRX_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(d_accept) & 15) return fail(RRX_ERR_ARG, "byte buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    return launched(dev::expand_bits(d_bits, nlines, d_accept, stream), "expand_bits launch");
}

// Host buffer in, one byte per string out.  Large inputs are cut into line-aligned chunks; the upload of chunk i+1 is
// queued before index + match + download of chunk i (two device buffers).  PCIe inclusive; never the benchmarked rate.
static int match_host_chunk(const rrx_regex *re, int device, uint8_t *d_text, size_t len, hipStream_t st, uint32_t *d_bits,
                            uint8_t *d_acc, uint8_t *accept, size_t cap, size_t line_off, size_t *nlines_out) {
    rrx_corpus *c = nullptr;
    int rc = rrx_corpus_create(device, d_text, len, st, &c);             // waits for the chunk's copy and index
    if (rc) return rc;
    const size_t n = c->nlines;
    rc = rrx_match_corpus(re, c, d_bits, st);
    if (!rc) rc = rrx_bitmap_to_bytes(device, d_bits, n, d_acc, st);
    if (!rc && line_off < cap) {
        const size_t take = n < cap - line_off ? n : cap - line_off;
        hipError_t e = hipMemcpyAsync(accept + line_off, d_acc, take, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail(e, "accept readback");
    }
    hipError_t e = hipStreamSynchronize(st);                             // the index arrays of `c` are freed next
    if (!rc && e != hipSuccess) rc = hip_fail(e, "chunk sync");
    rrx_corpus_free(c);
    *nlines_out = n;
    return rc;
}

int rrx_match_host(const rrx_regex *re, int device, const void *bytes, size_t nbytes, uint8_t *accept, size_t cap, size_t *nlines) {
    if (!re || (nbytes && !bytes) || !nlines) return fail(RRX_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(device));
    *nlines = 0;
    if (!nbytes) return RRX_OK;
    const uint8_t *host = static_cast<const uint8_t *>(bytes);
    const size_t kChunk = (size_t)256 << 20;
    const size_t buf_bytes = (nbytes < kChunk ? nbytes : kChunk) + 64;
    const size_t max_lines = buf_bytes;                                   // a chunk of n bytes holds at most n lines
    struct Lane {                                                         // a device buffer set and its stream
        DeviceArray<uint8_t> text, acc;
        DeviceArray<uint32_t> bits;
        hipStream_t st = nullptr;
        ~Lane() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }      // (runs before the buffers go)
    } lane[2];
    const int nbuf = nbytes > kChunk ? 2 : 1;
    int rc = RRX_OK;
    hipError_t e = hipSuccess;
    for (int i = 0; i < nbuf && e == hipSuccess; i++) {
        e = lane[i].text.alloc(device, buf_bytes);
        if (e == hipSuccess) e = lane[i].acc.alloc(device, max_lines + 64);
        if (e == hipSuccess) e = lane[i].bits.alloc(device, (max_lines / 32 + 4) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipStreamCreate(&lane[i].st);
    }
    if (e != hipSuccess) rc = hip_fail(e, "pipeline buffers");

    // chunk boundaries: right after the last '\n' of each window (a window without any '\n' is taken whole: the
    // line continues, and since a line must be matched by one launch such inputs fall back to one big chunk)
    std::vector<size_t> cuts{0};
    while (!rc && cuts.back() < nbytes) {
        size_t lo = cuts.back(), hi = lo + kChunk < nbytes ? lo + kChunk : nbytes;
        if (hi < nbytes) {
            size_t q = hi;
            while (q > lo && host[q - 1] != '\n') q--;
            if (q == lo) { rc = fail(RRX_ERR_UNSUPPORTED, "a single line longer than 256 MiB: use rrx_corpus_create on a device buffer"); break; }
            hi = q;
        }
        cuts.push_back(hi);
    }
    const size_t nchunks = cuts.size() - 1;
    size_t line_off = 0;
    // The caller's pages are NOT pinned: on this platform the runtime's own staged copy from pageable memory runs at
    // 49 GB/s (57 pinned), while pinning costs as much as the copy (hipHostRegister + hipHostUnregister: ~30 ms per
    // GiB).  Measured on 4 GiB: 42 GB/s unpinned, 31 GB/s pinning everything first, 33 GB/s pinning 64-MiB windows on
    // a helper thread ahead of the uploads.
    if (!rc) {
        e = hipMemcpyAsync(lane[0].text, host, cuts[1] - cuts[0], hipMemcpyHostToDevice, lane[0].st);
        if (e != hipSuccess) rc = hip_fail(e, "chunk upload");
    }
    for (size_t i = 0; i < nchunks && !rc; i++) {
        const int cur = (int)(i & 1) % nbuf, nxt = (int)((i + 1) & 1) % nbuf;
        if (i + 1 < nchunks) {                                             // next chunk's upload is queued before this chunk's work
            e = hipMemcpyAsync(lane[nxt].text, host + cuts[i + 1], cuts[i + 2] - cuts[i + 1], hipMemcpyHostToDevice, lane[nxt].st);
            if (e != hipSuccess) { rc = hip_fail(e, "chunk upload"); break; }
        }
        size_t n = 0;
        rc = match_host_chunk(re, device, lane[cur].text, cuts[i + 1] - cuts[i], lane[cur].st, lane[cur].bits, lane[cur].acc, accept, cap, line_off, &n);
        line_off += n;
    }
    for (int i = 0; i < nbuf; i++) if (lane[i].st) (void)hipStreamSynchronize(lane[i].st);      // both streams, before either lane's buffers go
    *nlines = line_off;
    return rc;
}

}  // extern "C"
