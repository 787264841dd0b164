// handles.hpp — what the units of the C ABI of librrx.so (include/rrx.h) share: the error helpers, the owners of device and pinned
// memory, the one upload path, the mailbox, and the three handles.  The units: regex.cpp (rrx_regex: compile, accessors, options,
// program dumps, table order and sampled table, its tables on the device), corpus.cpp (rrx_corpus, the batch entries, the one-shot
// entry, the host pipeline), search.cpp, the units of explicit items - items.cpp (batches, match and contains), item_search.cpp
// (where the matches are), item_columns.cpp (replace and pieces); what they share is items.hpp -, strings.cpp (single strings),
// group.cpp (rrx_group: a pattern split at a capture group, with a handle of its own), multi.cpp (rrx_multi: a set of patterns on
// product tables, with a handle of its own).  What a pattern compiles to and which table
// forms it gets is decided in plan.cpp, the life of a sampled table in sampled.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rrx.h"
#include "device.hpp"
#include "lower.hpp"
#include "pack.hpp"
#include "plan.hpp"
#include "sampled.hpp"
#include "table_order.hpp"
#include "template.hpp"

// ---- errors: the calling thread's text behind rrx_last_error (regex.cpp)
std::string &last_error();
inline int fail(int code, const std::string &msg) { last_error() = msg; return code; }
inline int hip_fail(hipError_t e, const char *what) { return fail(RRX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
inline int launched(int e, const char *what) { return e ? hip_fail((hipError_t)e, what) : RRX_OK; }     // (what a dev:: launcher returned)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_fail(e_, #expr); } while (0)

// A result bitmap of n bits filled on `stream` without a kernel: all clear, or - ones - the first n bits set and the rest of the
// last word clear (contains on the NFA lane engine: the bitmap before the kernel; a nullable pattern; the empty language)
inline int fill_bitmap(uint32_t *d_bits, size_t n, bool ones, void *stream) {
    const size_t whole = ones ? n / 32 : (n + 31) / 32;
    if (whole) HIP_TRY(hipMemsetAsync(d_bits, ones ? 0xff : 0, whole * sizeof(uint32_t), (hipStream_t)stream));
    if (ones && (n & 31)) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_bits + whole), (int)((1u << (n & 31)) - 1u), 1, (hipStream_t)stream));
    return RRX_OK;
}

// ---- owners
// One device allocation, freed on its own device.
struct DeviceAlloc {
    int device = -1;
    void *p = nullptr;
    DeviceAlloc() = default;
    DeviceAlloc(DeviceAlloc &&o) noexcept : device(o.device), p(o.p) { o.p = nullptr; }
    DeviceAlloc &operator=(DeviceAlloc &&o) noexcept { if (this != &o) { reset(); device = o.device; p = o.p; o.p = nullptr; } return *this; }
    ~DeviceAlloc() { reset(); }
    void reset() { if (p) { (void)hipSetDevice(device); (void)hipFree(p); p = nullptr; } }
    hipError_t alloc(int dev, size_t bytes) {            // (leaves `dev` the current device)
        reset(); device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess && (e = hipMalloc(&p, bytes)) != hipSuccess) p = nullptr;
        return e;
    }
};
// One allocation of pinned host memory.
struct PinnedAlloc {
    void *p = nullptr;
    PinnedAlloc() = default;
    PinnedAlloc(const PinnedAlloc &) = delete;
    PinnedAlloc &operator=(const PinnedAlloc &) = delete;
    ~PinnedAlloc() { reset(); }
    void reset() { if (p) { (void)hipHostFree(p); p = nullptr; } }
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
        reset();
        hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void *release() { void *q = p; p = nullptr; return q; }      // (the mailbox pages: theirs for the life of the process)
};
// The same, read as arrays of T where the handles used to hold a T *
template <class T> struct DeviceArray : DeviceAlloc { operator T *() const { return static_cast<T *>(p); } };
template <class T> struct PinnedArray : PinnedAlloc { operator T *() const { return static_cast<T *>(p); } };

// An image uploaded to a device, and the descriptor(s) of it that the kernels take.
template <class D> struct OnDevice { DeviceAlloc mem; D d; };      // (mem.p == nullptr: a miss cached by items_table / items2_table)

// The only upload of program tables: `img` into a fresh allocation on `device` (16 bytes of tail beyond the image), its
// descriptors bound to it.  stream == nullptr: a synchronous copy; otherwise the copy is queued on `stream` and waited for.
hipError_t upload(int device, const rrx::Image &img, DeviceAlloc &out, hipStream_t stream = nullptr);

// Everything that hangs off one LineTables on the device side (under rrx_regex::mu): the table, the host side of its items forms
// and, per device, what has been uploaded - its tables, its byte-stride items table (the plain table in the wide line-table format
// with one more column: 0..127 byte values, '\n' an ordinary byte, 128 = any byte >= 0x80, 129 = END OF ITEM: verdict of the row,
// back to the start row) and its stride-2 items table.  A regex has two: of its match table and of its contains table.
struct TableSet {
    const char *const word;                              // "match" / "contains": how its items launches are named in error texts
    rrx::LineTables own;
    rrx::LineTables &lt;                                 // `own`, or Programs::match
    rrx::ItemsForms items;
    uint32_t found = ~0u;                                // contains: the one accepting state if it is absorbing (build_contains)
    std::map<int, OnDevice<rrx::DeviceTables>> on_device;
    std::map<int, OnDevice<rrx::dev::LineDfaDevice>> items_on_device;
    std::map<int, OnDevice<rrx::dev::Dfa2Device>> items2_on_device;
    explicit TableSet(const char *w) : word(w), lt(own) {}
    TableSet(const char *w, rrx::LineTables &of) : word(w), lt(of) {}
};

// The device side of the sampled table (sampled.hpp: SampledTable has the rest).
struct SampledOnDevice {
    std::map<int, OnDevice<rrx::dev::Dfa2Device>> tables;     // the table in use (under `mu`; earlier generations: rrx_regex::kept)
    std::map<int, DeviceAlloc> escapes;                  // device -> 16 bytes: the last launch's count of its escaped lines (under onepass_mu)
    // The same count, copied by every sampled launch into pinned host memory behind its kernels, one slot per table generation.
    // The NEXT launch looks at it without waiting (it shows the last launch that has finished): SampledTable::judge.
    PinnedArray<unsigned long long> seen;                // (under onepass_mu)
};

// ---- the mailbox (corpus.cpp)
// Small results a call has to hand back to the host (line totals, flags) are written by the call's last kernel into a slot
// of pinned, device-mapped host memory; the host then only waits for the stream.  (Round 2 read them with three
// hipMemcpyAsync into pageable stack variables and a synchronize: one call in twelve of the one-shot entry took 10.6 ms
// instead of 1.8 - BENCH_r02.json - with every kernel as fast as ever, profiles/r03_one_shot_calls.txt.)
struct Mailbox {
    volatile uint64_t *host = nullptr;
    uint64_t *dev = nullptr;
    int device = -1, slot = -1;
};
int mailbox_acquire(int device, Mailbox *out);
void mailbox_release(const Mailbox &m);
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

// ---- the handles
struct rrx_regex : rrx::Programs {                       // (plan.hpp: the programs, the match tables' forms, the engine)
    std::string pattern;
    std::atomic<int> opt_background_order{1};            // RRX_OPT_BACKGROUND_ORDER
    std::atomic<int> opt_search_anchored{1};             // RRX_OPT_SEARCH_ANCHORED
    std::atomic<int> opt_sampled_table{1};               // RRX_OPT_SAMPLED_TABLE
    std::atomic<int> opt_flush_slots{0};                 // RRX_OPT_FLUSH_SLOTS (0: from the corpus' mean line length)
    std::atomic<int> items_stride2{1};                   // RRX_OPT_ITEMS_STRIDE2 (0: the byte-stride items kernel for trim 1 as well)
    std::atomic<int> opt_contains_nfa{0};                // RRX_OPT_CONTAINS_NFA (0: tables only, 1: the NFA where there is no table, 2: always)
    mutable std::mutex mu;
    ~rrx_regex();                                        // waits for what may still use the members (threads, queued copies)

    // ---- tables on the device, uploaded at their first use
    // The match tables by engine (tables()) and the contains tables (contains_tables(): built at their first use, build_contains),
    // each with its items tables (items_table / items2_table)
    mutable TableSet match_set{"match", match}, contains_set{"contains"};
    // The image that `pack` fills (false: none) on `device`, uploaded at the first use (call with `mu` held).  No image or a failed
    // upload: an error, tried again at the next call - or with `keep_miss` a miss cached for good (*out = nullptr, RRX_OK).
    template <class D, class Pack> int upload_once(std::map<int, OnDevice<D>> &cache, int device, bool keep_miss, Pack pack, const D **out) const;
    int tables(int device, const rrx::DeviceTables **out) const;
    rrx::dev::Dfa2Device dfa2_device(const rrx::DeviceTables *t) const { std::lock_guard<std::mutex> lock(mu); return t->dfa2; }
    // Device memory that launches may still be reading, kept until rrx_free: the sampled tables of earlier generations, the
    // stride-2 tables uploaded again in the profiled order (under `mu`)
    mutable std::vector<DeviceAlloc> kept;

    // ---- contains (rrx_contains_corpus): the forward search table with its accepting states folded into one absorbing state
    mutable int contains_state = 0;      // 0 = not built, 1 = built, -1 = no table
    int build_contains() const;          // host side (call with `mu` held)
    int contains_tables(int device, const rrx::DeviceTables **out) const;
    // The items tables of `set` on `device`, for explicit items stepped stripe-wise: nullptr where it has none that fits (the caller
    // runs the other kernel) - no contains table at all; byte-stride: more states than 16-bit row offsets allow; stride-2 (a separator
    // byte per item, trim 1): no stride-2 line table, or the items form - one symbol more - is beyond the same LDS region.
    bool built(const TableSet &set) const { return &set == &match_set || build_contains() == RRX_OK; }      // (call with `mu` held)
    const rrx::dev::Dfa2Device *items2_table(TableSet &set, int device) const;
    const rrx::dev::LineDfaDevice *items_table(TableSet &set, int device) const;
    // ---- contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA): the lane program with the contains B rows (plan.hpp:
    // plan_contains_nfa), built at its first use whatever engine the regex was compiled for, uploaded once per device
    mutable int contains_nfa_state = 0;  // 0 = not built, 1 = built, -1 = no lane program
    mutable rrx::NfaProgram contains_nfa;
    mutable std::map<int, OnDevice<rrx::dev::NfaDevice>> contains_nfa_on_device;
    bool build_contains_nfa() const;     // host side (call with `mu` held); false: no lane program
    // THE ROUTE of the three contains entries and of rrx_contains_engine_name, decided here and nowhere else (call with `mu` held):
    // *nfa = the entry runs on the NFA lane engine - option 2, or option 1 where build_contains fails.  RRX_ERR_UNSUPPORTED where
    // it should and the pattern has no lane program (the text names both reasons), and, on the table route, what build_contains says.
    int contains_route(bool *nfa) const;
    // The route, and on the NFA route the program on `device`: *out = nullptr where no kernel is needed - a pattern that accepts the
    // empty string (every bit: *fill = true) and the empty language (no bit).  On the table route *nfa = false and nothing else is set.
    int contains_nfa_tables(int device, bool *nfa, const rrx::dev::NfaDevice **out, bool *fill) const;

    // ---- search (built on first use; plan.hpp: plan_search)
    mutable int search_state = 0;        // 0 = not built, 1 = built, -1 = does not fit
    mutable rrx::SearchPlan search;
    mutable std::map<int, OnDevice<rrx::dev::SearchChunkDevice>> search_on_device;
    int build_search() const;            // host side (call with `mu` held)
    // The stripe-wise kernel's tables on `device` (uploaded once); *out = nullptr for a pattern that accepts the empty string.
    int search_tables(int device, const rrx::dev::SearchChunkDevice **out) const;
    // The lane-per-item search kernel's tables on `device` (search.fwd and search.rev in their plain form, uploaded once); *out =
    // nullptr for a pattern that accepts the empty string.  RRX_ERR_UNSUPPORTED only where fwd or rev did not determinise: the fit
    // rule of the stripe-wise kernel (build_search's return code) plays no part.
    mutable std::map<int, OnDevice<rrx::dev::SearchItemsDevice>> search_items_on_device;
    int search_item_tables(int device, const rrx::dev::SearchItemsDevice **out) const;
    // The leftmost-longest search's two tables (plan.hpp: plan_search_longest), built at their first use beside `search`; they take
    // no part in build_search's fit rules.  search_longest_tables: on `device` (uploaded once); *out = nullptr for the empty language
    // (no table: nothing matches).  RRX_ERR_UNSUPPORTED only where one of the two does not determinise.
    mutable int search_longest_state = 0;        // 0 = not built, 1 = built, -1 = does not determinise
    mutable rrx::SearchLongestPlan search_longest;
    mutable std::map<int, OnDevice<rrx::dev::SearchLongestDevice>> search_longest_on_device;
    int build_search_longest() const;    // host side (call with `mu` held)
    int search_longest_tables(int device, const rrx::dev::SearchLongestDevice **out) const;

    // ---- the order of the stride-2 table's rows and columns in LDS (empty: as numbered).  The order costs no memory and decides
    // which entries share an LDS bank: bank = (row slot * row words + column slot) mod 32.  State 0 (dead) keeps slot 0.
    std::vector<uint32_t> t2_row_slot, t2_col_slot;
    mutable rrx::TableOrderSearch t2_order;              // the order search, in the background or in the caller of rrx_order_table
    mutable rrx::Dfa2OrderStats t2_order_stats;          // (under `mu`)
    bool t2_order_applies() const;                       // single-copy tables only: interleaved copies already keep lanes apart
    void apply_t2_order(std::vector<uint32_t> &&rows, std::vector<uint32_t> &&cols, const rrx::Dfa2OrderStats &st) const;
    bool decide_t2_order(const uint8_t *sample, uint32_t lanes, uint32_t bytes_per_lane, bool now) const;

    // ---- scratch of the single-string entries (rrx_match_string / rrx_match_cstr): one grow-only device buffer per device,
    // kept across calls (a hipMalloc + hipFree pair per string cost more than the match itself).  `scratch_mu` is held
    // for the whole call: those entries are synchronous, concurrent callers of one regex take turns.
    struct Scratch { DeviceAlloc mem; size_t cap = 0; };
    mutable std::mutex scratch_mu;
    mutable std::map<int, Scratch> scratch;
    int scratch_for(int device, size_t bytes, void **out) const;      // call with `scratch_mu` held

    // ---- scratch of the one-shot entry (rrx_match_device: per-stripe counts, their scan and the lanes' verdict streams), of
    // one-call explicit items (rrx_match_extents: the item index) and of the sampled launch.  One grow-only buffer per device, kept
    // until rrx_free.  Users on different streams are ordered on the DEVICE by an event recorded after each use (the host never
    // waits): onepass_for(..., stream) makes `stream` wait for the last user, onepass_done(stream) marks the new last use; both
    // under `onepass_mu`, held from the one to the other.
    struct EventScratch {                                // (the last user has finished before `mem` is freed)
        DeviceAlloc mem; size_t cap = 0; hipEvent_t last = nullptr; bool used = false;
        ~EventScratch() { if (last) { (void)hipSetDevice(mem.device); (void)hipEventSynchronize(last); (void)hipEventDestroy(last); } }
    };
    mutable std::mutex onepass_mu;
    mutable std::map<int, EventScratch> onepass_scratch;
    int onepass_for(int device, size_t bytes, void **out, hipStream_t stream) const;       // call with `onepass_mu` held
    int onepass_done(int device, hipStream_t stream) const;                                // call with `onepass_mu` held

    // ---- the sampled table (sampled.hpp).  A relearnt table replaces the one in use under onepass_mu and mu: the
    // old device tables go to `kept` (a launch queued on them may still be running).
    mutable SampledOnDevice sampled_dev;
    mutable rrx::SampledTable sampled{*this, mu, onepass_mu, [this] {
        for (auto &kv : sampled_dev.tables) kept.push_back(std::move(kv.second.mem));
        sampled_dev.tables.clear();
    }};
    int sampled_tables(int device, rrx::dev::Dfa2Device *out) const;
};

struct rrx_corpus {
    int device = 0;
    const uint8_t *d_bytes = nullptr;
    size_t nbytes = 0, nstripes = 0, nlines = 0;
    uint32_t stripe = 0;                 // bytes per lane for this corpus
    DeviceArray<uint32_t> d_counts;      // [nstripes] newlines per stripe, then one flags word and the two of dev::own_words_check
    DeviceArray<uint64_t> d_base;        // [nstripes+1] exclusive prefix
    bool has_high = false;               // some byte >= 0x80 occurs
    // The stride-2 batch kernel without a cleared bitmap (dev::match_stripes_dfa2 with exchange slots), decided with the index:
    // no bitmap word lies in the ranges of three workgroups, and the longest range is own_span words past its first one (a
    // regex whose LDS window is shorter takes the clear).  The slot arrays: one per stream that has matched this corpus - the
    // launches of one stream are ordered, which is all the exchange needs -, zeroed once, all zero again after every launch.
    // (Freed with the corpus: hipFree waits for the launches that still use them.)
    bool own_words = false;
    uint32_t own_span = 0;
    static constexpr size_t kMaxSlotArrays = 64;         // (streams beyond these take the clear)
    mutable std::map<hipStream_t, DeviceArray<unsigned long long>> slot_arrays;      // (under `mu`)
    // A sample of the text as the batch kernel's half-waves see it - the first kSampleBytes bytes of kSampleGroups x 32
    // consecutive stripes, lane-major, in pinned host memory - taken with the index on large corpora: what a table engine
    // orders its table by at its first match (order_dfa2).  Empty: none.
    PinnedArray<uint8_t> h_sample;
    uint32_t sample_lanes = 0;
    // search only: offset of the first byte of every line, built on the first search of this corpus
    mutable std::mutex mu;
    mutable DeviceArray<uint64_t> d_line_off;   // [nlines + 1]
    // stripe-wise search: newline prefix per search chunk - the stripe index itself (d_base) when the stripe is that size, else an
    // index of its own (d_chunk_own)
    mutable const uint64_t *d_chunk_base = nullptr;      // [nchunks + 1 + scan scratch]
    mutable DeviceArray<uint64_t> d_chunk_own;
    mutable size_t nchunks = 0;
    mutable DeviceArray<uint8_t> d_all_scratch; // rrx_search_all: per-chunk status words, total, ticket (zeroed per call)
};

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

// A replacement template (template.hpp: what the parser left) and, per device, its segment program and literals as the kernels of
// kernels_replace_template_items.hip take them, uploaded at the first use there (item_columns.cpp).
struct rrx_template {
    rrx::ReplaceTemplate t;
    mutable std::mutex mu;
    mutable std::map<int, OnDevice<rrx::dev::TemplateDevice>> on_device;       // (under `mu`)
    int on(int device, rrx::dev::TemplateDevice *out) const;
};
