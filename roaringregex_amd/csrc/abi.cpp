// abi.cpp — the C ABI of librrx.so (include/rrx.h): handles and locks, device program upload, launches.  What a pattern compiles
// to and which table forms it gets is decided in plan.cpp.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rrx.h"
#include "device.hpp"
#include "frontend.hpp"
#include "lower.hpp"
#include "pack.hpp"
#include "plan.hpp"

using namespace rrx;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) { g_err = msg; return code; }
int hip_fail(hipError_t e, const char *what) {
    return fail(RRX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
int launched(int e, const char *what) { return e ? hip_fail((hipError_t)e, what) : RRX_OK; }     // (what a dev:: launcher returned)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_fail(e_, #expr); } while (0)

// One device allocation, freed on its own device.
struct DeviceAlloc {
    int device = -1;
    void *p = nullptr;
    DeviceAlloc() = default;
    DeviceAlloc(DeviceAlloc &&o) noexcept : device(o.device), p(o.p) { o.p = nullptr; }
    ~DeviceAlloc() { reset(); }
    void reset() { if (p) { (void)hipSetDevice(device); (void)hipFree(p); p = nullptr; } }
    hipError_t alloc(int dev, size_t bytes) {            // (leaves `dev` the current device)
        reset(); device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess && (e = hipMalloc(&p, bytes)) != hipSuccess) p = nullptr;
        return e;
    }
};

// An image uploaded to a device, and the descriptor(s) of it that the kernels take.
template <class D> struct OnDevice { DeviceAlloc mem; D d; };      // (mem.p == nullptr: a miss cached by items_table / items2_table)

// The only upload of program tables: `img` into a fresh allocation on `device` (16 bytes of tail beyond the image), its
// descriptors bound to it.  stream == nullptr: a synchronous copy; otherwise the copy is queued on `stream` and waited for.
hipError_t upload(int device, const Image &img, DeviceAlloc &out, hipStream_t stream = nullptr) {
    const std::vector<uint8_t> &b = img.bytes;
    hipError_t e = out.alloc(device, b.size() + 16);
    if (e == hipSuccess) e = stream ? hipMemcpyAsync(out.p, b.data(), b.size(), hipMemcpyHostToDevice, stream) : hipMemcpy(out.p, b.data(), b.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && stream) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) img.bind(out.p); else out.reset();
    return e;
}

// Everything that hangs off one LineTables on the device side (under rrx_regex::mu): the table, the host side of its items forms
// and, per device, what has been uploaded - its tables, its byte-stride items table (the plain table in the wide line-table format
// with one more column: 0..127 byte values, '\n' an ordinary byte, 128 = any byte >= 0x80, 129 = END OF ITEM: verdict of the row,
// back to the start row) and its stride-2 items table.  A regex has two: of its match table and of its contains table.
struct TableSet {
    const char *const word;                              // "match" / "contains": how its items launches are named in error texts
    LineTables own;
    LineTables &lt;                                      // `own`, or Programs::match
    ItemsForms items;
    uint32_t found = ~0u;                                // contains: the one accepting state if it is absorbing (build_contains)
    std::map<int, OnDevice<DeviceTables>> on_device;
    std::map<int, OnDevice<dev::LineDfaDevice>> items_on_device;
    std::map<int, OnDevice<dev::Dfa2Device>> items2_on_device;
    explicit TableSet(const char *w) : word(w), lt(own) {}
    TableSet(const char *w, LineTables &of) : word(w), lt(of) {}
};

// Small results a call has to hand back to the host (line totals, flags) are written by the call's last kernel into a slot
// of pinned, device-mapped host memory; the host then only waits for the stream.  (Round 2 read them with three
// hipMemcpyAsync into pageable stack variables and a synchronize: one call in twelve of the one-shot entry took 10.6 ms
// instead of 1.8 - BENCH_r02.json - with every kernel as fast as ever, profiles/r03_one_shot_calls.txt.)
struct Mailbox {
    volatile uint64_t *host = nullptr;
    uint64_t *dev = nullptr;
    int device = -1, slot = -1;
};
constexpr int kMailSlots = 64, kMailWords = 8;
struct MailPage { uint64_t *host = nullptr, *dev = nullptr; std::vector<int> free_slots; };
std::mutex g_mail_mu;
std::map<int, MailPage> g_mail;
int mailbox_acquire(int device, Mailbox *out) {
    std::lock_guard<std::mutex> lock(g_mail_mu);
    MailPage &pg = g_mail[device];
    if (!pg.host) {
        void *h = nullptr, *d = nullptr;
        hipError_t e = hipHostMalloc(&h, kMailSlots * kMailWords * sizeof(uint64_t), hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) { if (h) (void)hipHostFree(h); return hip_fail(e, "hipHostMalloc(mailbox)"); }
        pg.host = static_cast<uint64_t *>(h); pg.dev = static_cast<uint64_t *>(d);
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
// Returns the slot when the call leaves - but only once the device can no longer write it: a call that queued the mailing kernel
// and leaves before its stream has drained waits for the stream here, and a slot whose stream does not drain is never handed out again.
struct MailboxGuard {
    Mailbox m;
    hipStream_t stream = nullptr;
    bool queued = false;                                // the kernel that writes the slot has been launched on `stream`
    bool drained = false;                               // ... and the stream has been waited for since
    ~MailboxGuard() {
        if (queued && !drained && hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); return; }
        mailbox_release(m);
    }
};

}  // namespace

// The one accepting state of `d` if every byte class keeps it where it is (the FOUND state of a contains table), else ~0u.
static uint32_t absorbing_accepting_state(const DfaProgram &d) {
    uint32_t found = ~0u;
    for (uint32_t s = 0; s < d.nstates; s++) {
        if (!d.accepting[s]) continue;
        if (found != ~0u) return ~0u;
        found = s;
    }
    if (found != ~0u)
        for (uint32_t k = 0; k < d.ncls; k++)
            if (d.next[(size_t)found * d.ncls + k] != found) return ~0u;
    return found;
}

struct rrx_regex : Programs {                            // (plan.hpp: the programs, the match tables' forms, the engine)
    std::string pattern;
    // Order of the stride-2 table's rows and columns in LDS (empty: as numbered).  The order costs no memory and decides which
    // entries share an LDS bank: bank = (row slot * row words + column slot) mod 32.  State 0 (dead) keeps slot 0.
    std::vector<uint32_t> t2_row_slot, t2_col_slot;
    mutable TableOrderSearch t2_order;                   // the order search, in the background or in the caller of rrx_order_table
    mutable Dfa2OrderStats t2_order_stats;               // (under `mu`)
    std::atomic<int> opt_background_order{1};            // RRX_OPT_BACKGROUND_ORDER
    std::atomic<int> opt_search_anchored{1};             // RRX_OPT_SEARCH_ANCHORED
    std::atomic<int> opt_sampled_table{1};               // RRX_OPT_SAMPLED_TABLE
    std::atomic<int> opt_flush_slots{0};                 // RRX_OPT_FLUSH_SLOTS (0: from the corpus' mean line length)
    // ---- the sampled table: AUTO ended on the NFA lane engine because the subset construction explodes; the sets a
    // text sample reaches are interned into a table with an ESCAPE state, the batch entry runs the stride-2 kernel on it (two result
    // bits per line) and lets the NFA engine decide the lines that escaped.  Built once: by the first rrx_match_corpus against a
    // corpus that carries a sample (in the background), or by rrx_learn_table (in the caller's thread).
    int requested_engine = 0;
    mutable OnceTask sampled_build;
    mutable std::atomic<bool> sampled_ready{false};      // (set under `mu` after the programs below are complete)
    mutable DfaProgram sampled_dfa;
    mutable Dfa2Program sampled_dfa2;
    mutable SampledTableStats sampled_stats;
    mutable std::map<int, DeviceAlloc> sampled_escapes;    // device -> 16 bytes: the last launch's count of its escaped lines (under onepass_mu)
    // The same count, copied by every sampled launch into pinned host memory behind its kernels.
    // The NEXT launch looks at it without waiting (it shows the last launch that has finished): a corpus that escapes from the table
    // - not the text it was learnt from - retires the table (sampled_retired), the regex is back on the NFA engine at its own rate.
    mutable unsigned long long *h_sampled_seen = nullptr;  // hipHostMalloc, one slot per table generation (under onepass_mu)
    mutable unsigned long long sampled_prev_lines = 0;     // lines of the last sampled launch queued (under onepass_mu)
    mutable std::atomic<bool> sampled_retired{false};
    // (r4) A retired table is LEARNT AGAIN, from the sample of the corpus that retired it (the first one that carries a sample), up to
    // kSampledRelearns times: the build runs like the first one (beside the caller unless RRX_OPT_BACKGROUND_ORDER is 0), the regex stays
    // on the NFA engine meanwhile, and the new table is subject to the same two guards.  The old device tables are kept (`kept`) until
    // rrx_free (a launch queued on them may still be running).
    static constexpr uint32_t kSampledRelearns = 3;
    mutable uint32_t sampled_gen = 0;                      // generation of the table in use (under onepass_mu; slot of h_sampled_seen)
    mutable std::vector<std::unique_ptr<OnceTask>> sampled_relearn;      // (under onepass_mu)
    mutable std::map<int, OnDevice<dev::Dfa2Device>> sampled_on_device;
    bool sampled_eligible() const { return requested_engine == RRX_ENGINE_AUTO && engine == RRX_ENGINE_NFA && !has_dfa && has_nfa; }
    // pieces x piece_bytes of text -> the table; false: nothing usable came out (the engine stays as it is)
    bool build_sampled(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool replace = false) const {
        const Reduced red = reduce(trimmed);
        DfaProgram d;
        Dfa2Program d2;
        SampledTableStats st;
        bool ok = false;
        for (uint32_t budget = 2048; budget >= 64 && !ok; budget /= 2) {       // the largest table whose stride-2 form fits the LDS
            if (!lower_dfa_sampled(red, text, pieces, piece_bytes, budget, d, &st)) return false;
            ok = lower_dfa2_that_fits(d, d2);
        }
        if (!ok || d.escaped.empty()) return false;      // (no escape state: the closure closed the table - lower_dfa would have too)
        // A table its own sample escapes from is the wrong tool: every escaped line is read a second time by the NFA engine, so
        // text whose live sets are NOT few (random a/b lines under (a|b)*a(a|b){40}: every line escapes) would run at a fraction of
        // the plain NFA engine's rate.  More than 2 % of the sample's lines: the engine stays as it is.
        if (st.sample_escapes * 50 > st.sample_lines) return false;
        if (replace) {
            // no sampled launch is being queued while the programs change (onepass_mu, taken before mu as match_corpus_sampled does)
            std::lock_guard<std::mutex> launches(onepass_mu);
            std::lock_guard<std::mutex> lock(mu);
            for (auto &kv : sampled_on_device) kept.push_back(std::move(kv.second.mem));
            sampled_on_device.clear();
            sampled_dfa = std::move(d); sampled_dfa2 = std::move(d2); sampled_stats = st;
            sampled_gen++;                               // (its own slot of h_sampled_seen: a late count of the old table's launches does not reach it)
            sampled_prev_lines = 0;
            sampled_retired.store(false);
            return true;
        }
        std::lock_guard<std::mutex> lock(mu);
        sampled_dfa = std::move(d); sampled_dfa2 = std::move(d2); sampled_stats = st;
        sampled_ready.store(true, std::memory_order_release);
        return true;
    }
    // the table is retired and `c` carries a text sample: learn it again from that (once per retirement, kSampledRelearns times in all)
    void relearn_sampled(const uint8_t *sample, uint32_t pieces, uint32_t piece_bytes) const {
        OnceTask *task = nullptr;
        {
            std::lock_guard<std::mutex> launches(onepass_mu);
            if (!sampled_retired.load() || sampled_relearn.size() >= kSampledRelearns) return;
            if (!sampled_relearn.empty() && sampled_relearn.back()->state() != OnceTask::kDone) return;      // (one at a time)
            sampled_relearn.emplace_back(new OnceTask());
            task = sampled_relearn.back().get();
        }
        // (started outside the lock: with RRX_OPT_BACKGROUND_ORDER 0 the job runs right here, and it takes onepass_mu itself to swap the table in)
        auto text = std::make_shared<std::vector<uint8_t>>(sample, sample + (size_t)pieces * piece_bytes);
        (void)task->start([this, text, pieces, piece_bytes]() { (void)build_sampled(text->data(), pieces, piece_bytes, /*replace=*/true); },
                          /*background=*/opt_background_order.load() != 0);
    }
    int sampled_tables(int device, dev::Dfa2Device *out) const {
        std::lock_guard<std::mutex> lock(mu);
        const dev::Dfa2Device *d = nullptr;
        const int rc = upload_once(sampled_on_device, device, false, [&](Image &img, dev::Dfa2Device &t) { return pack_dfa2(sampled_dfa2, {}, {}, img, t); }, &d);
        if (!rc) *out = *d;
        return rc;
    }
    // Device memory that launches may still be reading, kept until rrx_free: the sampled tables of earlier generations, the
    // stride-2 tables uploaded again in the profiled order (under `mu`)
    mutable std::vector<DeviceAlloc> kept;
    bool t2_order_applies() const {                      // single-copy tables only: interleaved copies already keep lanes apart
        return match.has_dfa2 && dfa2_table_bytes(match.dfa2) * 2 > dev::kDfa2TableBudget;
    }
    // What happens to a found order (runs in the searching thread).  For devices whose tables are already up the stride-2 arrays
    // are built and uploaded again WITHOUT `mu` - launches go on meanwhile on the table as numbered; `mu` is taken twice, briefly:
    // to read which devices are up, and to swap the slot vectors and the descriptors.  A device that comes up in between gets the
    // numbered order and keeps it (its own arrays agree with each other; results never depend on the order).
    void apply_t2_order(std::vector<uint32_t> &&rows, std::vector<uint32_t> &&cols, const Dfa2OrderStats &st) const {
        std::vector<int> up;
        { std::lock_guard<std::mutex> lock(mu); for (auto &kv : match_set.on_device) up.push_back(kv.first); }
        std::vector<std::pair<int, OnDevice<dev::Dfa2Device>>> done;
        for (int device : up) {
            Image img;
            OnDevice<dev::Dfa2Device> t;
            (void)pack_dfa2(match.dfa2, rows, cols, img, t.d);
            hipStream_t st2 = nullptr;
            bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&st2, hipStreamNonBlocking) == hipSuccess &&
                      upload(device, img, t.mem, st2) == hipSuccess;
            if (st2) (void)hipStreamDestroy(st2);
            if (!ok) { (void)hipGetLastError(); continue; }                                    // (that device keeps the numbered order)
            done.emplace_back(device, std::move(t));
        }
        std::lock_guard<std::mutex> lock(mu);
        rrx_regex *self = const_cast<rrx_regex *>(this);
        self->t2_row_slot.swap(rows); self->t2_col_slot.swap(cols);
        t2_order_stats = st;
        for (auto &u : done) {
            auto it = match_set.on_device.find(u.first);
            if (it != match_set.on_device.end()) it->second.d.dfa2 = u.second.d;
            kept.push_back(std::move(u.second.mem));
        }
    }
    // First match against a corpus that carries a text sample: start the search in the background (the match itself, and the
    // next ones, run on the table as numbered until the new order is in) - unless the caller has forbidden library threads
    // (RRX_OPT_BACKGROUND_ORDER 0): then nothing happens here and rrx_order_table is the only way to an ordered table.
    // `now`: run it in the caller's thread (rrx_order_table).  Returns false if the order had been decided before.
    bool decide_t2_order(const uint8_t *sample, uint32_t lanes, uint32_t bytes_per_lane, bool now) const {
        if (t2_order.decided()) return false;
        if (!t2_order_applies() || !sample || lanes < 32) return t2_order.skip();
        if (!now && !opt_background_order.load()) return true;                   // (left undecided: rrx_order_table may still come)
        std::vector<uint8_t> copy(sample, sample + (size_t)lanes * bytes_per_lane);
        return t2_order.start(match.dfa2, std::move(copy), lanes, bytes_per_lane, /*background=*/!now,
                              [this](std::vector<uint32_t> &&r, std::vector<uint32_t> &&c, const Dfa2OrderStats &st) { apply_t2_order(std::move(r), std::move(c), st); });
    }
    dev::Dfa2Device dfa2_device(const DeviceTables *t) const { std::lock_guard<std::mutex> lock(mu); return t->dfa2; }
    mutable std::mutex mu;
    // The match tables by engine (tables()) and the contains tables (contains_tables(): built at their first use, build_contains),
    // each with its items tables (items_table / items2_table)
    mutable TableSet match_set{"match", match}, contains_set{"contains"};
    // search (built on first use; plan.hpp: plan_search)
    mutable int search_state = 0;        // 0 = not built, 1 = built, -1 = does not fit
    mutable SearchPlan search;
    mutable std::map<int, OnDevice<dev::SearchChunkDevice>> search_on_device;
    std::atomic<int> items_stride2{1};                 // RRX_OPT_ITEMS_STRIDE2 (0: the byte-stride items kernel for trim 1 as well)
    // Scratch of the single-string entries (rrx_match_string / rrx_match_cstr): one grow-only device buffer per device,
    // kept across calls (a hipMalloc + hipFree pair per string cost more than the match itself).  `scratch_mu` is held
    // for the whole call: those entries are synchronous, concurrent callers of one regex take turns.
    struct Scratch { DeviceAlloc mem; size_t cap = 0; };
    mutable std::mutex scratch_mu;
    mutable std::map<int, Scratch> scratch;
    int scratch_for(int device, size_t bytes, void **out) const {      // call with `scratch_mu` held
        Scratch &sc = scratch[device];
        if (sc.cap < bytes) {
            sc.cap = 0;
            const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
            hipError_t e = sc.mem.alloc(device, want);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(single-string scratch)");
            sc.cap = want;
        }
        *out = sc.mem.p;
        return RRX_OK;
    }

    // Scratch of the one-shot entry (rrx_match_device: per-stripe counts, their scan and the lanes' verdict streams) and of
    // one-call explicit items (rrx_match_extents: the item index).  One grow-only buffer per device, kept until rrx_free.
    // Users on different streams are ordered on the DEVICE by an event recorded after each use (the host never waits):
    // onepass_for(..., stream) makes `stream` wait for the last user, onepass_done(stream) marks the new last use; both under
    // `onepass_mu`, held from the one to the other.
    struct EventScratch {                                // (the last user has finished before `mem` is freed)
        DeviceAlloc mem; size_t cap = 0; hipEvent_t last = nullptr; bool used = false;
        ~EventScratch() { if (last) { (void)hipSetDevice(mem.device); (void)hipEventSynchronize(last); (void)hipEventDestroy(last); } }
    };
    mutable std::mutex onepass_mu;
    mutable std::map<int, EventScratch> onepass_scratch;
    int onepass_for(int device, size_t bytes, void **out, hipStream_t stream) const {      // call with `onepass_mu` held
        EventScratch &sc = onepass_scratch[device];
        if (!sc.last) {
            hipError_t e = hipEventCreateWithFlags(&sc.last, hipEventDisableTiming);
            if (e != hipSuccess) { sc.last = nullptr; return hip_fail(e, "hipEventCreate(scratch)"); }
        }
        if (sc.cap < bytes) {
            if (sc.mem.p) { (void)hipEventSynchronize(sc.last); sc.mem.reset(); sc.cap = 0; sc.used = false; }
            hipError_t e = sc.mem.alloc(device, bytes);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(one-pass scratch)");
            sc.cap = bytes;
        }
        if (sc.used) {
            hipError_t e = hipStreamWaitEvent(stream, sc.last, 0);
            if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent(scratch)");
        }
        *out = sc.mem.p;
        return RRX_OK;
    }
    int onepass_done(int device, hipStream_t stream) const {                               // call with `onepass_mu` held
        EventScratch &sc = onepass_scratch[device];
        hipError_t e = hipEventRecord(sc.last, stream);
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord(scratch)");
        sc.used = true;
        return RRX_OK;
    }

    // (device memory is freed by its owners, DeviceAlloc and EventScratch, once the body has waited for what may still use it)
    ~rrx_regex() {
        t2_order.wait();
        sampled_build.wait();
        for (auto &task : sampled_relearn) task->wait();
        if (h_sampled_seen) {                            // (a copy into it may still be queued on the devices that ran the sampled table)
            for (auto &kv : sampled_escapes) { (void)hipSetDevice(kv.first); (void)hipDeviceSynchronize(); }
            (void)hipHostFree(h_sampled_seen);
        }
    }
    // The image that `pack` fills (false: none) on `device`, uploaded at the first use (call with `mu` held).  No image or a failed
    // upload: an error, tried again at the next call - or with `keep_miss` a miss cached for good (*out = nullptr, RRX_OK).
    template <class D, class Pack> int upload_once(std::map<int, OnDevice<D>> &cache, int device, bool keep_miss, Pack pack, const D **out) const {
        auto it = cache.find(device);
        if (it == cache.end()) {
            Image img;
            OnDevice<D> t;
            const bool packed = pack(img, t.d);
            const hipError_t e = packed ? upload(device, img, t.mem) : hipSuccess;
            if (!keep_miss && !packed) return fail(RRX_ERR_UNSUPPORTED, "automaton too large for the device tables of its engine");
            if (!keep_miss && e != hipSuccess) return hip_fail(e, "device table upload");
            it = cache.emplace(device, std::move(t)).first;
        }
        *out = it->second.mem.p ? &it->second.d : nullptr;
        return RRX_OK;
    }
    // The items tables of `set` on `device`, for explicit items stepped stripe-wise: nullptr where it has none that fits (the caller
    // runs the other kernel) - no contains table at all; byte-stride: more states than 16-bit row offsets allow; stride-2 (a separator
    // byte per item, trim 1): no stride-2 line table, or the items form - one symbol more - is beyond the same LDS region.
    bool built(const TableSet &set) const { return &set == &match_set || build_contains() == RRX_OK; }      // (call with `mu` held)
    const dev::Dfa2Device *items2_table(TableSet &set, int device) const {
        std::lock_guard<std::mutex> lock(mu);
        const dev::Dfa2Device *d = nullptr;
        if (built(set)) (void)upload_once(set.items2_on_device, device, true, [&](Image &img, dev::Dfa2Device &t) { return set.items.pack2(set.lt, img, t); }, &d);
        return d;
    }
    const dev::LineDfaDevice *items_table(TableSet &set, int device) const {
        std::lock_guard<std::mutex> lock(mu);
        const dev::LineDfaDevice *d = nullptr;
        if (built(set)) (void)upload_once(set.items_on_device, device, true, [&](Image &img, dev::LineDfaDevice &t) { return set.items.pack(set.lt, img, t); }, &d);
        return d;
    }

    // Host side of the search tables (call with `mu` held).  RRX_OK also for a pattern that accepts the empty string: it needs
    // no table (search.nullable), search.fwd / search.rev are built all the same (rrx_program_words).
    int build_search() const {
        if (search_state == 0)
            search_state = plan_search(reduce(trimmed), opt_search_anchored.load() != 0, accepts_empty(), dev::search_chunks_lds_bytes, search) ? 1 : -1;
        return search_state == 1 ? RRX_OK
                                 : fail(RRX_ERR_UNSUPPORTED, "search tables too large for the device (the reverse DFA must fit 64 KiB of LDS, the forward "
                                                              "product table 65534 rows and 256 MiB)");
    }
    // The stripe-wise kernel's tables on `device` (uploaded once); *out = nullptr for a pattern that accepts the empty string.
    int search_tables(int device, const dev::SearchChunkDevice **out) const {
        std::lock_guard<std::mutex> lock(mu);
        int rc = build_search();
        if (rc) return rc;
        *out = nullptr;
        if (search.nullable) return RRX_OK;
        auto pack = [&](Image &img, dev::SearchChunkDevice &t) { pack_search(search.line2, search.fwd, search.rev, search.layout, img, t); return true; };
        return upload_once(search_on_device, device, false, pack, out);
    }

    // "Contains a match" (rrx_contains_corpus): the forward search table with its accepting states folded into one absorbing
    // state (lower.hpp: contains_dfa), in the forms of the match path and by its fit rules (plan.hpp: LineTables) - the stride-2
    // form, the wide / classed LDS line table, the global line table; a regex compiled with RRX_ENGINE_DFA / _DFA_GLOBAL keeps it
    // on the byte-stride LDS / global table.  Host side (call with `mu` held).
    // Its items forms join it to the items kernels (rrx_contains_extents / rrx_contains_items): in the byte-stride form column 0 and
    // column 128 (any byte >= 0x80) are filled from class 0, a live column here, which is what NUL and high bytes are to this table;
    // the stride-2 form exists where the contains table has one at all - not under RRX_ENGINE_DFA / _DFA_GLOBAL.  The lane-per-item
    // kernel runs on the plain arrays of contains_tables() and stops a lane in contains_set.found, the table's one accepting state if
    // that state is absorbing (~0u: none - the empty language).
    mutable int contains_state = 0;      // 0 = not built, 1 = built, -1 = no table
    int build_contains() const {
        if (contains_state == 0) {
            (void)build_search();                        // (what the search entries cannot use does not matter here: the forward table does)
            LineTables &lt = contains_set.lt;
            contains_state = search.fwd.nstates != 0 && contains_dfa(search.fwd, lt.dfa) && lt.decide(requested_engine) ? 1 : -1;
            if (contains_state == 1) contains_set.found = absorbing_accepting_state(lt.dfa);
        }
        return contains_state == 1 ? RRX_OK
                                   : fail(RRX_ERR_UNSUPPORTED, search.fwd.nstates ? "contains table too large for the device (the global form holds 2^24 entries)"
                                                                                  : "no contains table: the forward search automaton does not determinise within the state budget");
    }
    // The contains tables on `device` (uploaded once)
    int contains_tables(int device, const DeviceTables **out) const {
        std::lock_guard<std::mutex> lock(mu);
        const int rc = build_contains();
        return rc ? rc : upload_once(contains_set.on_device, device, false, [&](Image &img, DeviceTables &t) { contains_set.lt.pack({}, {}, img, t); return true; }, out);
    }

    // Upload the program for `device` once; returns the device-side descriptors.
    int tables(int device, const DeviceTables **out) const {
        std::lock_guard<std::mutex> lock(mu);
        return upload_once(match_set.on_device, device, false, [&](Image &img, DeviceTables &t) {
            if (engine == RRX_ENGINE_NFA_BLOCK || engine == RRX_ENGINE_NFA_SPARSE) {
                const bool sparse = engine == RRX_ENGINE_NFA_SPARSE;
                pack_wave_nfa(nfa_block, trimmed, sparse ? dev::sparse_rows(nfa_block.W) : dev::wave_words_per_lane(nfa_block.W), sparse, img, t.block);
            } else if (engine == RRX_ENGINE_NFA_WAVE) {
                return pack_group_nfa(nfa_wave, trimmed, img, t.group);      // (false: beyond the group-cooperative engine)
            } else if (engine == RRX_ENGINE_NFA) {
                pack_lane_nfa(nfa, img, t.nfa);
            } else {
                match.pack(t2_row_slot, t2_col_slot, img, t);
            }
            return true;
        }, out);
    }
};

struct rrx_corpus {
    int device = 0;
    const uint8_t *d_bytes = nullptr;
    size_t nbytes = 0, nstripes = 0, nlines = 0;
    uint32_t stripe = 0;            // bytes per lane for this corpus
    uint32_t *d_counts = nullptr;   // [nstripes] newlines per stripe, then one flags word and the two of dev::own_words_check
    uint64_t *d_base = nullptr;     // [nstripes+1] exclusive prefix
    bool has_high = false;          // some byte >= 0x80 occurs
    // The stride-2 batch kernel without a cleared bitmap (dev::match_stripes_dfa2 with exchange slots), decided with the index:
    // no bitmap word lies in the ranges of three workgroups, and the longest range is own_span words past its first one (a
    // regex whose LDS window is shorter takes the clear).  The slot arrays: one per stream that has matched this corpus - the
    // launches of one stream are ordered, which is all the exchange needs -, zeroed once, all zero again after every launch.
    bool own_words = false;
    uint32_t own_span = 0;
    static constexpr size_t kMaxSlotArrays = 64;         // (streams beyond these take the clear)
    mutable std::map<hipStream_t, unsigned long long *> slot_arrays;      // (under `mu`)
    // A sample of the text as the batch kernel's half-waves see it - the first kSampleBytes bytes of kSampleGroups x 32
    // consecutive stripes, lane-major, in pinned host memory - taken with the index on large corpora: what a table engine
    // orders its table by at its first match (order_dfa2).  nullptr: none.
    uint8_t *h_sample = nullptr;
    uint32_t sample_lanes = 0;
    // search only: offset of the first byte of every line, built on the first search of this corpus
    mutable std::mutex mu;
    mutable uint64_t *d_line_off = nullptr;     // [nlines + 1]
    // stripe-wise search: newline prefix per search chunk (the stripe index itself when the stripe is that size)
    mutable uint64_t *d_chunk_base = nullptr;   // [nchunks + 1 + scan scratch]; owned unless it aliases d_base
    mutable size_t nchunks = 0;
    mutable void *d_all_scratch = nullptr;      // rrx_search_all: per-chunk status words, total, ticket (zeroed per call)
};

static constexpr uint32_t kSampleGroups = 8, kSampleBytes = 256;     // 8 x 32 lanes x 128 pair steps = 1024 half-waves, 64 KiB
static constexpr size_t kSampleMinCorpus = (size_t)64 << 20;         // smaller corpora: the order search (tens of ms) would not pay

static constexpr size_t kLongStringBytes = 32 * 1024;   // shorter single strings stay on one lane (NFA engines)
// Table engines: the chunk maps by convergence cost a handful of short launches (60-80 us), a sequential lane 94 ns per byte
// (tools/probe/facade_latency.py: 1.9 ms for 20 KB against 59 us; 130 us for 1 KB): from 1 KiB on the chunks win.
static constexpr size_t kLongStringBytesTable = 1024;
static constexpr uint32_t kLongNfaMaxBits = 256;        // NFA engines: chunk relations cost bytes x positions lane steps

extern "C" {

const char *rrx_last_error(void) { return g_err.c_str(); }

int rrx_compile_ex(const char *pattern, int engine, rrx_regex **out) {
    if (!pattern || !out) return fail(RRX_ERR_ARG, "null argument");
    if (engine < RRX_ENGINE_AUTO || (engine > RRX_ENGINE_DFA2 && engine != RRX_ENGINE_NFA_BLOCK && engine != RRX_ENGINE_NFA_SPARSE)) return fail(RRX_ERR_ARG, "unknown engine");
    *out = nullptr;
    rrx_regex *re = new rrx_regex();
    try {
        re->pattern = pattern;
        re->requested_engine = engine;
        plan_engines(re->pattern, engine, *re);
    } catch (const PatternError &e) {
        delete re;
        return fail(RRX_ERR_PATTERN, e.what());
    } catch (const BudgetError &e) {
        delete re;
        return fail(RRX_ERR_UNSUPPORTED, e.what());
    } catch (const std::exception &e) {
        delete re;
        return fail(RRX_ERR_PATTERN, std::string("internal: ") + e.what());
    }
    if (!re->engine) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "automaton too large for the requested engine (%u useful states)", re->trimmed.n);
        delete re;
        return fail(RRX_ERR_UNSUPPORTED, msg);
    }
    *out = re;
    return RRX_OK;
}
int rrx_compile(const char *pattern, rrx_regex **out) { return rrx_compile_ex(pattern, RRX_ENGINE_AUTO, out); }
void rrx_free(rrx_regex *re) { delete re; }

uint32_t rrx_num_states(const rrx_regex *re) { return re->ref.states_n; }
int rrx_set_class(const rrx_regex *re) { return re->ref.set_class(); }
uint32_t rrx_ref_initial(const rrx_regex *re) { return re->ref.initial; }
int rrx_ref_is_final(const rrx_regex *re, uint32_t s) { return s < re->ref.states_n && re->ref.is_final[s]; }
uint32_t rrx_ref_row(const rrx_regex *re, uint32_t state, unsigned c, uint32_t *out, uint32_t cap) {
    std::vector<uint32_t> r = re->ref.row(state, c);
    for (size_t i = 0; i < r.size() && i < cap; i++) out[i] = r[i];
    return (uint32_t)r.size();
}
int rrx_engine(const rrx_regex *re) { return re->engine; }
const char *rrx_engine_name(const rrx_regex *re) { return re->engine_name(); }
uint32_t rrx_useful_states(const rrx_regex *re) { return re->trimmed.n; }
int rrx_order_table(rrx_regex *re, const void *sample, uint32_t lanes, uint32_t bytes_per_lane) {
    if (!re || !sample || lanes < 32 || bytes_per_lane < 2) return fail(RRX_ERR_ARG, "sample: at least 32 lanes of 2 bytes");
    if (!re->decide_t2_order(static_cast<const uint8_t *>(sample), lanes, bytes_per_lane, /*now=*/true))
        return fail(RRX_ERR_ARG, "the table order has been decided already");
    return RRX_OK;
}
int rrx_table_order(const rrx_regex *re, double *conflict_before, double *conflict_after) {
    const TableOrderSearch::State st = re->t2_order.state();          // (one atomic read; the thread object is its owner's)
    std::lock_guard<std::mutex> lock(re->mu);
    const bool profiled = st == TableOrderSearch::kDone && re->t2_row_slot.size() == re->match.dfa2.nstates && re->match.has_dfa2 && re->t2_order_stats.half_waves;
    if (conflict_before) *conflict_before = profiled ? re->t2_order_stats.before : 0.0;
    if (conflict_after) *conflict_after = profiled ? re->t2_order_stats.after : 0.0;
    return profiled ? 1 : st == TableOrderSearch::kRunning ? 2 : 0;   // 2: the search is running
}
int rrx_learn_table(rrx_regex *re, const void *text, size_t nbytes) {
    if (!re || !text || nbytes < 2 || nbytes > ((size_t)1 << 30)) return fail(RRX_ERR_ARG, "a text sample of 2 bytes to 1 GiB");
    if (!re->sampled_eligible()) return fail(RRX_ERR_UNSUPPORTED, "a sampled table serves automata that AUTO leaves on the NFA lane engine");
    const uint8_t *p = static_cast<const uint8_t *>(text);
    bool built = false;
    if (!re->sampled_build.start([&]() { built = re->build_sampled(p, 1, (uint32_t)nbytes); }, /*background=*/false))
        return fail(RRX_ERR_ARG, "the sampled table has been decided already");
    return built ? RRX_OK : fail(RRX_ERR_UNSUPPORTED, "no sampled table for this automaton and text: none fits the device, or more than 2 % of the text's own lines leave it");
}
int rrx_sampled_table(const rrx_regex *re, uint32_t *table_states, uint32_t *open_transitions) {
    const OnceTask::State st = re->sampled_build.state();
    const bool ready = re->sampled_ready.load(std::memory_order_acquire);
    std::lock_guard<std::mutex> lock(re->mu);
    if (table_states) *table_states = ready ? re->sampled_dfa.nstates : 0;
    if (open_transitions) *open_transitions = ready ? re->sampled_stats.open_transitions : 0;
    return ready ? (re->sampled_retired.load() ? 3 : 1) : st == OnceTask::kRunning ? 2 : 0;
}
int rrx_sampled_escapes(const rrx_regex *re, int device, uint64_t *lines) {
    if (!re || !lines) return fail(RRX_ERR_ARG, "null argument");
    *lines = 0;
    std::lock_guard<std::mutex> lock(re->onepass_mu);
    auto it = re->sampled_escapes.find(device);
    if (it == re->sampled_escapes.end() || !it->second.p) return RRX_OK;          // no sampled-table launch on this device yet
    HIP_TRY(hipSetDevice(device));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, it->second.p, sizeof v, hipMemcpyDeviceToHost));          // (synchronous: behind everything queued on the device)
    *lines = v;
    return RRX_OK;
}
int rrx_set_option(rrx_regex *re, int option, int64_t value) {
    if (!re) return fail(RRX_ERR_ARG, "null argument");
    if (option == RRX_OPT_BACKGROUND_ORDER) { re->opt_background_order.store(value ? 1 : 0); return RRX_OK; }
    if (option == RRX_OPT_FLUSH_SLOTS) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16 && value != 32) return fail(RRX_ERR_ARG, "flush period: 0 (automatic) or 1, 2, 4, 8, 16, 32 slots");
        re->opt_flush_slots.store((int)value);
        return RRX_OK;
    }
    if (option == RRX_OPT_SAMPLED_TABLE) { re->opt_sampled_table.store(value ? 1 : 0); return RRX_OK; }
    if (option == RRX_OPT_ITEMS_STRIDE2) { re->items_stride2.store(value ? 1 : 0); return RRX_OK; }
    if (option == RRX_OPT_SEARCH_ANCHORED) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->search_state != 0) return fail(RRX_ERR_ARG, "the search tables of this regex are built already");
        re->opt_search_anchored.store(value ? 1 : 0);
        return RRX_OK;
    }
    if (option == RRX_OPT_UNITS_PER_WORKGROUP) {             // the kernel is gone: the value is checked as it was, and ignored
        if (value < 0 || value > 65536) return fail(RRX_ERR_ARG, "units per workgroup: 0 (off) or 16 ... 65536");
        return RRX_OK;
    }
    return fail(RRX_ERR_ARG, "unknown option");
}
uint32_t rrx_byte_classes(const rrx_regex *re) { return re->trimmed.ncls; }
uint32_t rrx_words_per_set(const rrx_regex *re) { return re->has_nfa ? re->nfa.W : re->has_wave ? re->nfa_wave.W : re->has_block ? re->nfa_block.W : 0; }
int rrx_accepts_empty(const rrx_regex *re) { return re->accepts_empty(); }

size_t rrx_program_words(const rrx_regex *re, int kind, uint32_t *out, size_t cap) {
    std::vector<uint32_t> w;
    if (kind == RRX_ENGINE_NFA && re->has_nfa) {
        append_words(w, re->nfa, /*csr=*/false);
    } else if (kind == RRX_ENGINE_NFA_WAVE && re->has_wave) {
        append_words(w, re->nfa_wave, /*csr=*/false);
    } else if ((kind == RRX_ENGINE_NFA_BLOCK || kind == RRX_ENGINE_NFA_SPARSE) && re->has_block) {
        append_words(w, re->nfa_block, /*csr=*/true);
    } else if (kind == RRX_PROGRAM_SEARCH_LINE || kind == RRX_PROGRAM_SEARCH_LINE2 || kind == RRX_PROGRAM_SEARCH_FWD || kind == RRX_PROGRAM_SEARCH_REV) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->build_search()) return 0;
        const SearchPlan &s = re->search;
        if (kind == RRX_PROGRAM_SEARCH_FWD) append_words(w, s.fwd);
        else if (kind == RRX_PROGRAM_SEARCH_REV) append_words(w, s.rev);
        else if (kind == RRX_PROGRAM_SEARCH_LINE && s.line.nrows) append_words(w, s.line, s.fwd);
        else if (kind == RRX_PROGRAM_SEARCH_LINE2 && s.line2.nrows) append_words(w, s.line2, s.layout);
    } else if (kind == RRX_PROGRAM_CONTAINS_DFA || kind == RRX_PROGRAM_CONTAINS_DFA2) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->build_contains()) return 0;
        if (kind == RRX_PROGRAM_CONTAINS_DFA) append_words(w, re->contains_set.lt.dfa);
        else if (re->contains_set.lt.has_dfa2) append_words(w, re->contains_set.lt.dfa2);
    } else if (kind == RRX_PROGRAM_CONTAINS_DFA2_ITEMS || (kind == RRX_PROGRAM_DFA2_ITEMS && re->match.has_dfa2)) {
        TableSet &set = kind == RRX_PROGRAM_DFA2_ITEMS ? re->match_set : re->contains_set;
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->built(set) && set.items.stride2(set.lt)) append_words(w, set.items.dfa2, /*pair_dim=*/true);
    } else if (kind == RRX_PROGRAM_DFA2_ORDER && re->match.has_dfa2) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->t2_row_slot.size() != re->match.dfa2.nstates || re->t2_col_slot.size() != re->match.dfa2.ncols) return 0;
        w = {re->match.dfa2.nstates, re->match.dfa2.ncols};
        w.insert(w.end(), re->t2_row_slot.begin(), re->t2_row_slot.end());
        w.insert(w.end(), re->t2_col_slot.begin(), re->t2_col_slot.end());
    } else if (kind == RRX_PROGRAM_SAMPLED_DFA || kind == RRX_PROGRAM_SAMPLED_DFA2) {
        if (!re->sampled_ready.load(std::memory_order_acquire)) return 0;
        std::lock_guard<std::mutex> lock(re->mu);
        if (kind == RRX_PROGRAM_SAMPLED_DFA) append_words(w, re->sampled_dfa, /*escaped=*/true);
        else append_words(w, re->sampled_dfa2);
    } else if (kind == RRX_ENGINE_DFA2 && re->match.has_dfa2) {
        append_words(w, re->match.dfa2);
    } else if (kind == RRX_ENGINE_DFA && re->has_dfa) {
        append_words(w, re->match.dfa);
    }
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    return w.size();
}

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
    rrx_corpus *c = new rrx_corpus();
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
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->d_counts), (c->nstripes + 3) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_base), (c->nstripes + 1 + dev::scan_scratch_words(c->nstripes)) * sizeof(uint64_t));
    if (e != hipSuccess) { rrx_corpus_free(c); return hip_fail(e, "hipMalloc(line index)"); }
    uint32_t *d_flags = c->d_counts + c->nstripes;
    e = hipMemsetAsync(d_flags, 0, 3 * sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) { rrx_corpus_free(c); return hip_fail(e, "hipMemsetAsync(flags)"); }
    int rc = dev::count_newlines_per_stripe(c->d_bytes, nbytes, c->stripe, c->d_counts, c->nstripes, d_flags, stream);
    if (!rc) rc = dev::scan_counts(c->d_counts, c->d_base, c->d_base + c->nstripes + 1, c->nstripes, stream);
    if (!rc && c->nstripes) rc = dev::own_words_check(c->d_base, c->nstripes, c->d_bytes + nbytes - 1, d_flags + 1, stream);
    if (rc) { rrx_corpus_free(c); return hip_fail((hipError_t)rc, "line index launch"); }
    MailboxGuard mail;
    if (int mrc = mailbox_acquire(device, &mail.m)) { rrx_corpus_free(c); return mrc; }
    if (nbytes >= kSampleMinCorpus && c->nstripes >= 64 * kSampleGroups &&
        hipHostMalloc(reinterpret_cast<void **>(&c->h_sample), (size_t)kSampleGroups * 32 * kSampleBytes, hipHostMallocDefault) == hipSuccess) {
        c->sample_lanes = kSampleGroups * 32;
        for (uint32_t g = 0; g < kSampleGroups; g++) {            // group g: 32 consecutive stripes, the groups spread over the corpus
            const size_t first_stripe = (size_t)g * (c->nstripes / kSampleGroups);
            if (hipMemcpy2DAsync(c->h_sample + (size_t)g * 32 * kSampleBytes, kSampleBytes, c->d_bytes + first_stripe * c->stripe, c->stripe,
                                 kSampleBytes, 32, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize((hipStream_t)stream);      // the copies of the groups before this one may still be writing the buffer
                (void)hipHostFree(c->h_sample); c->h_sample = nullptr; c->sample_lanes = 0;
                break;
            }
        }
    }
    mail.stream = (hipStream_t)stream; mail.queued = true;
    rc = dev::mail_results(c->d_base + c->nstripes, d_flags, nbytes ? c->d_bytes + nbytes - 1 : nullptr, mail.m.dev, stream, d_flags + 1);
    if (rc) { rrx_corpus_free(c); return hip_fail((hipError_t)rc, "line index launch"); }
    e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rrx_corpus_free(c); return hip_fail(e, "line index readback"); }
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
            rrx_corpus_free(c);
            return rrx_corpus_create_ex(device, d_bytes, nbytes, want, stream, out);
        }
    }
    *out = c;
    return RRX_OK;
}
size_t rrx_corpus_num_lines(const rrx_corpus *c) { return c->nlines; }
size_t rrx_corpus_num_bytes(const rrx_corpus *c) { return c->nbytes; }
uint32_t rrx_corpus_stripe_bytes(const rrx_corpus *c) { return c->stripe; }
int rrx_corpus_one_launch(const rrx_corpus *c, uint32_t *span_words) {
    if (span_words) *span_words = c->own_words ? c->own_span : 0;
    return c->own_words ? 1 : 0;
}
void rrx_corpus_free(rrx_corpus *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_counts) (void)hipFree(c->d_counts);
    if (c->d_base) (void)hipFree(c->d_base);
    if (c->d_line_off) (void)hipFree(c->d_line_off);
    if (c->d_chunk_base && c->d_chunk_base != c->d_base) (void)hipFree(c->d_chunk_base);
    if (c->d_all_scratch) (void)hipFree(c->d_all_scratch);
    if (c->h_sample) (void)hipHostFree(c->h_sample);
    for (auto &kv : c->slot_arrays) (void)hipFree(kv.second);      // (hipFree waits for the launches that still use them)
    delete c;
}

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
    DeviceAlloc &count = re->sampled_escapes[c->device];
    if (!count.p) HIP_TRY(count.alloc(c->device, 16));
    unsigned long long *total = static_cast<unsigned long long *>(count.p);
    constexpr uint32_t kSlots = rrx_regex::kSampledRelearns + 1;
    if (!re->h_sampled_seen && hipHostMalloc(reinterpret_cast<void **>(&re->h_sampled_seen), kSlots * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess)
        for (uint32_t k = 0; k < kSlots; k++) re->h_sampled_seen[k] = 0;
    unsigned long long *const seen = re->h_sampled_seen ? re->h_sampled_seen + (re->sampled_gen < kSlots ? re->sampled_gen : kSlots - 1) : nullptr;
    if (seen) {
        // what the last FINISHED launch counted, against the size of the last launch queued (the same corpus in a scan loop; otherwise a hint)
        const unsigned long long esc_seen = seen[0];
        if (re->sampled_prev_lines >= 1024 && esc_seen * 20 > re->sampled_prev_lines) re->sampled_retired.store(true);   // > 5 % of the lines: the wrong table for this text
    }
    hipError_t he = hipMemsetAsync(wide, 0, wide_bytes, st);                     // (the kernel merges words with atomic OR)
    if (he == hipSuccess) he = hipMemsetAsync(total, 0, 16, st);
    int e = he != hipSuccess ? (int)he : dev::match_stripes_dfa2_two_bit(d2, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, wide, stream);
    if (!e) e = dev::split_two_bit(wide, c->nlines, d_accept_bits, escaped, total, list, cap, stream);
    if (!e) e = dev::recheck_escaped_nfa(t->nfa, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, escaped, c->nlines, list, total, cap, d_accept_bits, stream);
    if (!e && seen) {                                                            // behind the kernels: the count into pinned memory (nobody waits for it)
        if (hipMemcpyAsync(seen, total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) (void)hipGetLastError();
        re->sampled_prev_lines = c->nlines;
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
    unsigned long long *slots = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&slots), bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemsetAsync(slots, 0, bytes, stream) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(slots); return nullptr; }
    c->slot_arrays.emplace(stream, slots);
    return slots;
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
    if (re->sampled_eligible() && re->opt_sampled_table.load() && !c->has_high) {
        if (!re->sampled_build.decided() && c->h_sample) {
            auto text = std::make_shared<std::vector<uint8_t>>(c->h_sample, c->h_sample + (size_t)c->sample_lanes * kSampleBytes);
            const uint32_t pieces = c->sample_lanes;
            (void)re->sampled_build.start([re, text, pieces]() { (void)re->build_sampled(text->data(), pieces, kSampleBytes); },
                                          /*background=*/re->opt_background_order.load() != 0);
        }
        if (re->sampled_ready.load(std::memory_order_acquire) && re->sampled_retired.load() && c->h_sample)
            re->relearn_sampled(c->h_sample, c->sample_lanes, kSampleBytes);     // (this launch and the next ones: the NFA engine, until the new table is in)
        if (re->sampled_ready.load(std::memory_order_acquire) && !re->sampled_retired.load()) return match_corpus_sampled(re, c, t, d_accept_bits, stream);
    }
    // (a corpus with bytes >= 0x80 leaves the stride-2 table for the byte-stride one)
    if (re->engine != RRX_ENGINE_NFA_SPARSE && re->engine != RRX_ENGINE_NFA_BLOCK && re->engine != RRX_ENGINE_NFA_WAVE && re->engine != RRX_ENGINE_NFA)
        return launch_line_tables(re, c, re->match, t, /*stride2_over_high=*/false, d_accept_bits, stream);
    // the NFA kernels merge words with atomic OR: start from an all-zero bitmap
    HIP_TRY(hipMemsetAsync(d_accept_bits, 0, rrx_corpus_bitmap_words(c) * sizeof(uint32_t), (hipStream_t)stream));
    int e = re->engine == RRX_ENGINE_NFA_SPARSE
                ? dev::match_stripes_sparse_nfa(t->block, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream)
            : re->engine == RRX_ENGINE_NFA_BLOCK
                ? dev::match_stripes_wave_nfa(t->block, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream)
            : re->engine == RRX_ENGINE_NFA_WAVE
                ? dev::match_stripes_group_nfa(t->group, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream)
                : dev::match_stripes_nfa(t->nfa, c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, d_accept_bits, stream);
    return launched(e, "match_stripes launch");
}

// "Which lines contain a match": the batch kernels of rrx_match_corpus on the contains table (build_contains).  On a corpus with
// bytes >= 0x80 the stride-2 table keeps its kernel - the instantiation that steps such bytes as 0x00, which is their class.
int rrx_contains_corpus(const rrx_regex *re, const rrx_corpus *c, uint32_t *d_bits, void *stream) {
    if (!re || !c || (c->nlines && !d_bits)) return fail(RRX_ERR_ARG, "null argument");
    const DeviceTables *t;
    int rc = re->contains_tables(c->device, &t);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->nlines) return RRX_OK;
    return launch_line_tables(re, c, re->contains_set.lt, t, /*stride2_over_high=*/true, d_bits, stream);
}
const char *rrx_contains_engine_name(const rrx_regex *re) {
    if (!re) { (void)fail(RRX_ERR_ARG, "null argument"); return nullptr; }
    std::lock_guard<std::mutex> lock(re->mu);
    return re->build_contains() ? nullptr : re->contains_set.lt.name();
}
uint32_t rrx_contains_states(const rrx_regex *re) {
    if (!re) { (void)fail(RRX_ERR_ARG, "null argument"); return 0; }
    std::lock_guard<std::mutex> lock(re->mu);
    return re->build_contains() ? 0 : re->contains_set.lt.dfa.nstates;
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
    const bool sampled = re->sampled_eligible() && re->opt_sampled_table.load() && re->sampled_ready.load(std::memory_order_acquire) && !re->sampled_retired.load();
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

// per-line offsets of the corpus, built on the first search (cached in the corpus)
static int line_offsets(const rrx_corpus *c, void *stream) {
    {
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->d_line_off) {
            uint64_t *off = nullptr;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&off), (c->nlines + 1) * sizeof(uint64_t)));
            // entry nlines: one past the last '\n' - the kernel writes it when the corpus ends in '\n'; otherwise the
            // last line ends at the end of the data, as if a '\n' followed it
            const uint64_t past = (uint64_t)c->nbytes + 1;
            hipError_t he = hipMemcpyAsync(off + c->nlines, &past, sizeof past, hipMemcpyHostToDevice, (hipStream_t)stream);
            if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream);          // `past` leaves scope
            int le = he == hipSuccess ? dev::build_line_offsets(c->d_bytes, c->nbytes, c->stripe, c->d_base, c->nstripes, off, stream) : 0;
            if (he == hipSuccess && !le) he = hipStreamSynchronize((hipStream_t)stream);   // once per corpus: later searches may use other streams
            if (he != hipSuccess || le) { (void)hipFree(off); return he != hipSuccess ? hip_fail(he, "line offsets") : hip_fail((hipError_t)le, "line_offsets launch"); }
            c->d_line_off = off;
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
    uint32_t *counts = nullptr;
    uint64_t *base = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&counts), (c->nchunks + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&base), (c->nchunks + 1 + dev::scan_scratch_words(c->nchunks)) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemsetAsync(counts + c->nchunks, 0, sizeof(uint32_t), (hipStream_t)stream);
    int le = 0;
    if (e == hipSuccess) le = dev::count_newlines_per_stripe(c->d_bytes, c->nbytes, (uint32_t)chunk, counts, c->nchunks, counts + c->nchunks, stream);
    if (e == hipSuccess && !le) le = dev::scan_counts(counts, base, base + c->nchunks + 1, c->nchunks, stream);
    if (e == hipSuccess && !le) e = hipStreamSynchronize((hipStream_t)stream);     // once per corpus: later searches may use other streams
    if (counts) (void)hipFree(counts);
    if (e != hipSuccess || le) { if (base) (void)hipFree(base); return e != hipSuccess ? hip_fail(e, "search chunk index") : hip_fail((hipError_t)le, "search chunk index launch"); }
    c->d_chunk_base = base;
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
    if (!c->nlines) { HIP_TRY(hipMemsetAsync(d_first, 0, sizeof(uint64_t), st)); HIP_TRY(hipStreamSynchronize(st)); return RRX_OK; }
    if (ct) {
        const size_t sb = dev::search_all_scratch_bytes(c->nchunks);
        {
            std::lock_guard<std::mutex> lock(c->mu);
            if (!c->d_all_scratch) HIP_TRY(hipMalloc(&c->d_all_scratch, sb));
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
    uint32_t *d_count = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_count), (c->nlines + 1) * sizeof(uint32_t)));
    uint64_t *d_sums = nullptr;
    hipError_t he = hipMalloc(reinterpret_cast<void **>(&d_sums), dev::scan_scratch_words(c->nlines) * sizeof(uint64_t));
    if (he != hipSuccess) { (void)hipFree(d_count); return hip_fail(he, "hipMalloc"); }
    auto done = [&](int code) { (void)hipFree(d_count); (void)hipFree(d_sums); return code; };
    int e = dev::empty_matches(c->d_line_off, c->nlines, d_count, nullptr, nullptr, nullptr, stream);
    if (!e) e = dev::scan_counts(d_count, d_first, d_sums, c->nlines, stream);  // d_first[nlines] = total
    if (e) return done(hip_fail((hipError_t)e, "empty_matches / scan launch"));
    he = hipMemsetAsync(d_first, 0, sizeof(uint64_t), st);                      // the scan marks entry 0 as a stripe start: not here
    uint64_t tot = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&tot, d_first + c->nlines, sizeof tot, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return done(hip_fail(he, "search_all scan"));
    *total = (size_t)tot;
    if (tot && cap) {                                                            // matches beyond `cap` are counted, not written (as rrx.h says)
        e = dev::empty_matches(c->d_line_off, c->nlines, nullptr, d_first, d_start, d_end, stream, cap);
        if (e) rc = hip_fail((hipError_t)e, "empty_matches launch");
        if (!rc) { he = hipStreamSynchronize(st); if (he != hipSuccess) rc = hip_fail(he, "search_all fill"); }
    }
    return done(rc);
}

int rrx_bitmap_to_bytes(int device, const uint32_t *d_bits, size_t nlines, uint8_t *d_accept, void *stream) {
    if (nlines && (!d_bits || !d_accept)) return fail(RRX_ERR_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(d_accept) & 15) return fail(RRX_ERR_ARG, "byte buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(device));
    return launched(dev::expand_bits(d_bits, nlines, d_accept, stream), "expand_bits launch");
}

// below these a batch stays on the lane-per-item kernel (the index costs more than it saves)
static constexpr size_t kItemsStripesMin = (size_t)1 << 16;
static constexpr size_t kItemsStripesMinBytes = (size_t)8 << 20;
// A lane (lane group, workgroup) per item: the match set on the regex' engine, one byte per item; the contains set on the plain
// arrays of its table, the bitmap itself.
static int extents_lanes(const rrx_regex *re, const TableSet &set, const DeviceTables *t, const uint8_t *b, const uint64_t *d_off, size_t nitems,
                         uint32_t trim, dev::ItemVerdicts out, void *stream, const uint32_t *only_if = nullptr) {
    int e = &set == &re->contains_set ? dev::contains_extents_dfa(t->dfa, set.lt.global, set.found, b, d_off, nitems, trim, out.bits, stream, only_if)
            : re->engine == RRX_ENGINE_NFA_SPARSE ? dev::match_extents_sparse_nfa(t->block, b, d_off, nitems, trim, out.bytes, stream)
            : re->engine == RRX_ENGINE_NFA_BLOCK ? dev::match_extents_wave_nfa(t->block, b, d_off, nitems, trim, out.bytes, stream)
            : re->engine == RRX_ENGINE_NFA_WAVE ? dev::match_extents_group_nfa(t->group, b, d_off, nitems, trim, out.bytes, stream)
            : re->engine == RRX_ENGINE_NFA ? dev::match_extents_nfa(t->nfa, b, d_off, nitems, trim, out.bytes, stream)
                                         : dev::match_extents_dfa(t->dfa, b, d_off, nitems, trim, out.bytes, stream, only_if);
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

// A batch of items indexed once (item-end bitmap + stripe base), matched by many patterns: rrx_corpus' counterpart for an
// offsets array.  stripes = false: the batch does not admit the stripe-wise kernel (trim > 1, an empty item at trim 0,
// alignment); rrx_match_items then runs the lane-per-item kernel.
struct rrx_items {
    int device = 0;
    const uint8_t *d_bytes = nullptr;
    const uint64_t *d_off = nullptr;
    size_t nitems = 0, nbytes = 0;       // nbytes = off[nitems] - off[0]
    uint64_t first = 0;
    uint32_t trim = 0;
    bool stripes = false;
    DeviceAlloc d_index;
    mutable std::mutex mu;
    DeviceAlloc d_result;                // result bitmap of a match (one match at a time per handle)
};
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
    uint8_t *d_text[2] = {nullptr, nullptr}, *d_acc[2] = {nullptr, nullptr};
    uint32_t *d_bits[2] = {nullptr, nullptr};
    hipStream_t st[2] = {nullptr, nullptr};
    const int nbuf = nbytes > kChunk ? 2 : 1;
    int rc = RRX_OK;
    hipError_t e = hipSuccess;
    for (int i = 0; i < nbuf && e == hipSuccess; i++) {
        e = hipMalloc(reinterpret_cast<void **>(&d_text[i]), buf_bytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_acc[i]), max_lines + 64);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_bits[i]), (max_lines / 32 + 4) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipStreamCreate(&st[i]);
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
        e = hipMemcpyAsync(d_text[0], host, cuts[1] - cuts[0], hipMemcpyHostToDevice, st[0]);
        if (e != hipSuccess) rc = hip_fail(e, "chunk upload");
    }
    for (size_t i = 0; i < nchunks && !rc; i++) {
        const int cur = (int)(i & 1) % nbuf, nxt = (int)((i + 1) & 1) % nbuf;
        if (i + 1 < nchunks) {                                             // next chunk's upload is queued before this chunk's work
            e = hipMemcpyAsync(d_text[nxt], host + cuts[i + 1], cuts[i + 2] - cuts[i + 1], hipMemcpyHostToDevice, st[nxt]);
            if (e != hipSuccess) { rc = hip_fail(e, "chunk upload"); break; }
        }
        size_t n = 0;
        rc = match_host_chunk(re, device, d_text[cur], cuts[i + 1] - cuts[i], st[cur], d_bits[cur], d_acc[cur], accept, cap, line_off, &n);
        line_off += n;
    }
    for (int i = 0; i < nbuf; i++) if (st[i]) (void)hipStreamSynchronize(st[i]);
    for (int i = 0; i < 2; i++) {
        if (d_text[i]) (void)hipFree(d_text[i]);
        if (d_acc[i]) (void)hipFree(d_acc[i]);
        if (d_bits[i]) (void)hipFree(d_bits[i]);
        if (st[i]) (void)hipStreamDestroy(st[i]);
    }
    *nlines = line_off;
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
