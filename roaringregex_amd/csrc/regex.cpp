// regex.cpp — rrx_regex: compile and free, accessors, options, program dumps (rrx_program_words), the table order and sampled
// table entries, and the handle's own members: its tables on the device, uploaded at their first use, and its scratch.
#include <cstdio>

#include "handles.hpp"
#include "table_order.hpp"

using namespace rrx;

static thread_local std::string g_err;
std::string &last_error() { return g_err; }

hipError_t upload(int device, const Image &img, DeviceAlloc &out, hipStream_t stream) {
    const std::vector<uint8_t> &b = img.bytes;
    hipError_t e = out.alloc(device, b.size() + 16);
    if (e == hipSuccess) e = stream ? hipMemcpyAsync(out.p, b.data(), b.size(), hipMemcpyHostToDevice, stream) : hipMemcpy(out.p, b.data(), b.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && stream) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) img.bind(out.p); else out.reset();
    return e;
}

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

// ---- tables on the device
template <class D, class Pack> int rrx_regex::upload_once(std::map<int, OnDevice<D>> &cache, int device, bool keep_miss, Pack pack, const D **out) const {
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

// Upload the program for `device` once; returns the device-side descriptors.
int rrx_regex::tables(int device, const DeviceTables **out) const {
    std::lock_guard<std::mutex> lock(mu);
    return upload_once(match_set.on_device, device, false, [&](Image &img, DeviceTables &t) {
        switch (engine) {
        case RRX_ENGINE_NFA_BLOCK: pack_wave_nfa(nfa_block, trimmed, dev::wave_words_per_lane(nfa_block.W), false, img, t.block); break;
        case RRX_ENGINE_NFA_SPARSE: pack_wave_nfa(nfa_block, trimmed, dev::sparse_rows(nfa_block.W), true, img, t.block); break;
        case RRX_ENGINE_NFA_WAVE: return pack_group_nfa(nfa_wave, trimmed, img, t.group);      // (false: beyond the group-cooperative engine)
        case RRX_ENGINE_NFA: pack_lane_nfa(nfa, img, t.nfa); break;
        default: match.pack(t2_row_slot, t2_col_slot, img, t);
        }
        return true;
    }, out);
}

const dev::Dfa2Device *rrx_regex::items2_table(TableSet &set, int device) const {
    std::lock_guard<std::mutex> lock(mu);
    const dev::Dfa2Device *d = nullptr;
    if (built(set)) (void)upload_once(set.items2_on_device, device, true, [&](Image &img, dev::Dfa2Device &t) { return set.items.pack2(set.lt, img, t); }, &d);
    return d;
}
const dev::LineDfaDevice *rrx_regex::items_table(TableSet &set, int device) const {
    std::lock_guard<std::mutex> lock(mu);
    const dev::LineDfaDevice *d = nullptr;
    if (built(set)) (void)upload_once(set.items_on_device, device, true, [&](Image &img, dev::LineDfaDevice &t) { return set.items.pack(set.lt, img, t); }, &d);
    return d;
}

// Host side of the search tables (call with `mu` held).  RRX_OK also for a pattern that accepts the empty string: it needs
// no table (search.nullable), search.fwd / search.rev are built all the same (rrx_program_words).
int rrx_regex::build_search() const {
    if (search_state == 0)
        search_state = plan_search(reduce(trimmed), opt_search_anchored.load() != 0, accepts_empty(), dev::search_chunks_lds_bytes, search) ? 1 : -1;
    return search_state == 1 ? RRX_OK
                             : fail(RRX_ERR_UNSUPPORTED, "search tables too large for the device (the reverse DFA must fit 64 KiB of LDS, the forward "
                                                          "product table 65534 rows and 256 MiB)");
}
// The stripe-wise kernel's tables on `device` (uploaded once); *out = nullptr for a pattern that accepts the empty string.
int rrx_regex::search_tables(int device, const dev::SearchChunkDevice **out) const {
    std::lock_guard<std::mutex> lock(mu);
    int rc = build_search();
    if (rc) return rc;
    *out = nullptr;
    if (search.nullable) return RRX_OK;
    auto pack = [&](Image &img, dev::SearchChunkDevice &t) { pack_search(search.line2, search.fwd, search.rev, search.layout, img, t); return true; };
    return upload_once(search_on_device, device, false, pack, out);
}

// The lane-per-item search kernel's tables on `device` (uploaded once); *out = nullptr for a pattern that accepts the empty string.
// Whether the stripe-wise kernel's tables fit (build_search's return code) does not matter here: fwd and rev do.
int rrx_regex::search_item_tables(int device, const dev::SearchItemsDevice **out) const {
    std::lock_guard<std::mutex> lock(mu);
    (void)build_search();
    if (!search.fwd.nstates || !search.rev.nstates)
        return fail(RRX_ERR_UNSUPPORTED, "no search tables: the forward or the reverse search automaton does not determinise within the state budget");
    *out = nullptr;
    if (search.nullable) return RRX_OK;
    auto pack = [&](Image &img, dev::SearchItemsDevice &t) { return pack_search_items(search.fwd, search.rev, img, t); };
    return upload_once(search_items_on_device, device, false, pack, out);
}

// Host side of the leftmost-longest search's tables (call with `mu` held): the starts table and the anchored table, built once.
int rrx_regex::build_search_longest() const {
    if (search_longest_state == 0) search_longest_state = plan_search_longest(reduce(trimmed), accepts_empty(), search_longest) ? 1 : -1;
    return search_longest_state == 1 ? RRX_OK
                                     : fail(RRX_ERR_UNSUPPORTED, "no leftmost-longest search tables: the starts automaton or the anchored automaton "
                                                                  "does not determinise within the state budget");
}
// Those tables on `device` (uploaded once); *out = nullptr for the empty language.  A nullable pattern has them too: its anchored
// table finds the longest accepted prefix.
int rrx_regex::search_longest_tables(int device, const dev::SearchLongestDevice **out) const {
    std::lock_guard<std::mutex> lock(mu);
    const int rc = build_search_longest();
    if (rc) return rc;
    *out = nullptr;
    if (search_longest.empty) return RRX_OK;
    auto pack = [&](Image &img, dev::SearchLongestDevice &t) { return pack_search_longest(search_longest.starts, search_longest.anchored, img, t); };
    return upload_once(search_longest_on_device, device, false, pack, out);
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
int rrx_regex::build_contains() const {
    if (contains_state == 0) {
        (void)build_search();                        // (what the search entries cannot use does not matter here: the forward table does)
        LineTables &lt = contains_set.lt;
        contains_state = search.fwd.nstates != 0 && contains_dfa(search.fwd, lt.dfa) && lt.decide(requested) ? 1 : -1;
        if (contains_state == 1) contains_set.found = absorbing_accepting_state(lt.dfa);
    }
    return contains_state == 1 ? RRX_OK
                               : fail(RRX_ERR_UNSUPPORTED, search.fwd.nstates ? "contains table too large for the device (the global form holds 2^24 entries)"
                                                                              : "no contains table: the forward search automaton does not determinise within the state budget");
}
// The contains tables on `device` (uploaded once)
int rrx_regex::contains_tables(int device, const DeviceTables **out) const {
    std::lock_guard<std::mutex> lock(mu);
    const int rc = build_contains();
    return rc ? rc : upload_once(contains_set.on_device, device, false, [&](Image &img, DeviceTables &t) { contains_set.lt.pack({}, {}, img, t); return true; }, out);
}

// ---- contains on the NFA lane engine (RRX_OPT_CONTAINS_NFA)
bool rrx_regex::build_contains_nfa() const {
    if (contains_nfa_state == 0) contains_nfa_state = plan_contains_nfa(*this, contains_nfa) ? 1 : -1;
    return contains_nfa_state == 1;
}
int rrx_regex::contains_route(bool *nfa) const {
    const int mode = opt_contains_nfa.load();
    *nfa = false;
    if (mode == 0) return build_contains();
    if (mode == 1 && build_contains() == RRX_OK) return RRX_OK;
    if (!build_contains_nfa()) {
        // (option 2 asks for no table; whether there is one is still the first half of the answer)
        const std::string table = build_contains() == RRX_OK ? std::string("the contains table is set aside (RRX_OPT_CONTAINS_NFA 2)") : last_error();
        return fail(RRX_ERR_UNSUPPORTED, table + "; and no lane program for contains on the NFA lane engine: the pattern has more than 512 positions after reduction");
    }
    *nfa = true;
    return RRX_OK;
}
int rrx_regex::contains_nfa_tables(int device, bool *nfa, const dev::NfaDevice **out, bool *fill) const {
    *nfa = false; *out = nullptr; *fill = false;
    if (!opt_contains_nfa.load()) return RRX_OK;             // (the table route reports its own errors: contains_tables)
    std::lock_guard<std::mutex> lock(mu);
    const int rc = contains_route(nfa);
    if (rc || !*nfa) return rc;
    if (contains_nfa.accepts_empty) { *fill = true; return RRX_OK; }
    if (!trimmed.n) return RRX_OK;                           // the empty language
    return upload_once(contains_nfa_on_device, device, false, [&](Image &img, dev::NfaDevice &t) { pack_lane_nfa(contains_nfa, img, t); return true; }, out);
}

// ---- the order of the stride-2 table
bool rrx_regex::t2_order_applies() const {                      // single-copy tables only: interleaved copies already keep lanes apart
    return match.has_dfa2 && dfa2_table_bytes(match.dfa2) * 2 > dev::kDfa2TableBudget;
}
// What happens to a found order (runs in the searching thread).  For devices whose tables are already up the stride-2 arrays
// are built and uploaded again WITHOUT `mu` - launches go on meanwhile on the table as numbered; `mu` is taken twice, briefly:
// to read which devices are up, and to swap the slot vectors and the descriptors.  A device that comes up in between gets the
// numbered order and keeps it (its own arrays agree with each other; results never depend on the order).
void rrx_regex::apply_t2_order(std::vector<uint32_t> &&rows, std::vector<uint32_t> &&cols, const Dfa2OrderStats &st) const {
    std::vector<int> up;
    { std::lock_guard<std::mutex> lock(mu); for (auto &kv : match_set.on_device) up.push_back(kv.first); }
    std::vector<std::pair<int, OnDevice<dev::Dfa2Device>>> done;
    for (int device : up) {
        Image img;
        OnDevice<dev::Dfa2Device> t;
        (void)pack_dfa2(match.dfa2, rows, cols, img, t.d, 0, match.byte_pairs);
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
bool rrx_regex::decide_t2_order(const uint8_t *sample, uint32_t lanes, uint32_t bytes_per_lane, bool now) const {
    if (t2_order.decided()) return false;
    if (!t2_order_applies() || !sample || lanes < 32) return t2_order.skip();
    if (!now && !opt_background_order.load()) return true;                   // (left undecided: rrx_order_table may still come)
    std::vector<uint8_t> copy(sample, sample + (size_t)lanes * bytes_per_lane);
    return t2_order.start(match.dfa2, std::move(copy), lanes, bytes_per_lane, /*background=*/!now,
                          [this](std::vector<uint32_t> &&r, std::vector<uint32_t> &&c, const Dfa2OrderStats &st) { apply_t2_order(std::move(r), std::move(c), st); });
}

// ---- the sampled table on the device
int rrx_regex::sampled_tables(int device, dev::Dfa2Device *out) const {
    std::lock_guard<std::mutex> lock(mu);
    const dev::Dfa2Device *d = nullptr;
    const int rc = upload_once(sampled_dev.tables, device, false, [&](Image &img, dev::Dfa2Device &t) { return pack_dfa2(sampled.dfa2(), {}, {}, img, t); }, &d);
    if (!rc) *out = *d;
    return rc;
}

// ---- scratch
int rrx_regex::scratch_for(int device, size_t bytes, void **out) const {      // call with `scratch_mu` held
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

int rrx_regex::onepass_for(int device, size_t bytes, void **out, hipStream_t stream) const {      // call with `onepass_mu` held
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
int rrx_regex::onepass_done(int device, hipStream_t stream) const {                               // call with `onepass_mu` held
    EventScratch &sc = onepass_scratch[device];
    hipError_t e = hipEventRecord(sc.last, stream);
    if (e != hipSuccess) return hip_fail(e, "hipEventRecord(scratch)");
    sc.used = true;
    return RRX_OK;
}

// (device and pinned memory is freed by its owners once the body has waited for what may still use it)
rrx_regex::~rrx_regex() {
    t2_order.wait();
    sampled.wait();
    if (sampled_dev.seen)                            // (a copy into it may still be queued on the devices that ran the sampled table)
        for (auto &kv : sampled_dev.escapes) { (void)hipSetDevice(kv.first); (void)hipDeviceSynchronize(); }
}

extern "C" {

const char *rrx_last_error(void) { return g_err.c_str(); }

int rrx_compile_ex(const char *pattern, int engine, rrx_regex **out) {
    if (!pattern || !out) return fail(RRX_ERR_ARG, "null argument");
    if (engine < RRX_ENGINE_AUTO || (engine > RRX_ENGINE_DFA2 && engine != RRX_ENGINE_NFA_BLOCK && engine != RRX_ENGINE_NFA_SPARSE)) return fail(RRX_ERR_ARG, "unknown engine");
    *out = nullptr;
    rrx_regex *re = new rrx_regex();
    try {
        re->pattern = pattern;
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
    if (!re->sampled.eligible()) return fail(RRX_ERR_UNSUPPORTED, "a sampled table serves automata that AUTO leaves on the NFA lane engine");
    bool built = false;
    if (!re->sampled.start_first(static_cast<const uint8_t *>(text), 1, (uint32_t)nbytes, /*background=*/false, &built))
        return fail(RRX_ERR_ARG, "the sampled table has been decided already");
    return built ? RRX_OK : fail(RRX_ERR_UNSUPPORTED, "no sampled table for this automaton and text: none fits the device, or more than 2 % of the text's own lines leave it");
}
int rrx_sampled_table(const rrx_regex *re, uint32_t *table_states, uint32_t *open_transitions) {
    return re->sampled.status(table_states, open_transitions);
}
int rrx_sampled_escapes(const rrx_regex *re, int device, uint64_t *lines) {
    if (!re || !lines) return fail(RRX_ERR_ARG, "null argument");
    *lines = 0;
    std::lock_guard<std::mutex> lock(re->onepass_mu);
    auto it = re->sampled_dev.escapes.find(device);
    if (it == re->sampled_dev.escapes.end() || !it->second.p) return RRX_OK;          // no sampled-table launch on this device yet
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
    if (option == RRX_OPT_CONTAINS_NFA) {
        if (value < 0 || value > 2) return fail(RRX_ERR_ARG, "contains on the NFA lane engine: 0 (never), 1 (where there is no contains table) or 2 (always)");
        re->opt_contains_nfa.store((int)value);
        return RRX_OK;
    }
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

const char *rrx_contains_engine_name(const rrx_regex *re) {
    if (!re) { (void)fail(RRX_ERR_ARG, "null argument"); return nullptr; }
    std::lock_guard<std::mutex> lock(re->mu);
    bool nfa = false;
    if (re->contains_route(&nfa)) return nullptr;
    return nfa ? "nfa-shift-and" : re->contains_set.lt.name();
}
uint32_t rrx_contains_states(const rrx_regex *re) {
    if (!re) { (void)fail(RRX_ERR_ARG, "null argument"); return 0; }
    std::lock_guard<std::mutex> lock(re->mu);
    return re->build_contains() ? 0 : re->contains_set.lt.dfa.nstates;
}

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
        // (the two plain tables are dumped wherever they determinise - the lane-per-item search runs on them whether or not the
        // stripe-wise kernel's tables fit the device; the line tables only where that kernel has them)
        const bool fits = re->build_search() == RRX_OK;
        const SearchPlan &s = re->search;
        if (kind == RRX_PROGRAM_SEARCH_FWD) { if (s.fwd.nstates) append_words(w, s.fwd); }
        else if (kind == RRX_PROGRAM_SEARCH_REV) { if (s.rev.nstates) append_words(w, s.rev); }
        else if (!fits) return 0;
        else if (kind == RRX_PROGRAM_SEARCH_LINE && s.line.nrows) append_words(w, s.line, s.fwd);
        else if (kind == RRX_PROGRAM_SEARCH_LINE2 && s.line2.nrows) append_words(w, s.line2, s.layout);
    } else if (kind == RRX_PROGRAM_SEARCH_STARTS || kind == RRX_PROGRAM_SEARCH_ANCHORED) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->build_search_longest()) return 0;
        append_words(w, kind == RRX_PROGRAM_SEARCH_STARTS ? re->search_longest.starts : re->search_longest.anchored);
    } else if (kind == RRX_PROGRAM_CONTAINS_DFA || kind == RRX_PROGRAM_CONTAINS_DFA2) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->build_contains()) return 0;
        if (kind == RRX_PROGRAM_CONTAINS_DFA) append_words(w, re->contains_set.lt.dfa);
        else if (re->contains_set.lt.has_dfa2) append_words(w, re->contains_set.lt.dfa2);
    } else if (kind == RRX_PROGRAM_CONTAINS_NFA) {
        std::lock_guard<std::mutex> lock(re->mu);
        if (re->build_contains_nfa()) append_words(w, re->contains_nfa, /*csr=*/false);
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
        re->sampled.words(/*stride2=*/kind == RRX_PROGRAM_SAMPLED_DFA2, w);
    } else if (kind == RRX_ENGINE_DFA2 && re->match.has_dfa2) {
        append_words(w, re->match.dfa2);
    } else if (kind == RRX_ENGINE_DFA && re->has_dfa) {
        append_words(w, re->match.dfa);
    }
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    return w.size();
}

}  // extern "C"
