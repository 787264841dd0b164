// sampled.cpp — learn, install, judge, retire, relearn (sampled.hpp).  Plain C++: no HIP header, no device call.
#include "sampled.hpp"

#include "../../include/rrx.h"

namespace rrx {

bool learn_sampled(const Trimmed &trimmed, const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, SampledLearnt &out) {
    const Reduced red = reduce(trimmed);
    bool ok = false;
    for (uint32_t budget = kSampledMaxStates; budget >= kSampledMinStates && !ok; budget /= 2) {
        if (!lower_dfa_sampled(red, text, pieces, piece_bytes, budget, out.dfa, &out.stats)) return false;
        ok = lower_dfa2_that_fits(out.dfa, out.dfa2);
    }
    if (!ok || out.dfa.escaped.empty()) return false;    // (no escape state: the closure closed the table)
    // text whose live sets are NOT few (random a/b lines under (a|b)*a(a|b){40}: every line escapes) would run at a fraction of the
    // plain NFA engine's rate: the engine stays as it is
    return out.stats.sample_escapes * 100 <= out.stats.sample_lines * kSampleEscapePercent;
}

bool sampled_retires(unsigned long long escapes_seen, unsigned long long prev_lines) {
    return prev_lines >= kRetireMinLines && escapes_seen * 100 > prev_lines * kRetireEscapePercent;
}

bool SampledTable::eligible() const { return of_.requested == RRX_ENGINE_AUTO && of_.engine == RRX_ENGINE_NFA && !of_.has_dfa && of_.has_nfa; }

int SampledTable::status(uint32_t *table_states, uint32_t *open_transitions) const {
    const OnceTask::State st = first_.state();
    const bool there = ready();
    std::lock_guard<std::mutex> lock(mu_);
    if (table_states) *table_states = there ? dfa_.nstates : 0;
    if (open_transitions) *open_transitions = there ? stats_.open_transitions : 0;
    return there ? (retired() ? 3 : 1) : st == OnceTask::kRunning ? 2 : 0;
}

void SampledTable::words(bool stride2, std::vector<uint32_t> &w) const {
    if (!ready()) return;
    std::lock_guard<std::mutex> lock(mu_);
    if (stride2) append_words(w, dfa2_);
    else append_words(w, dfa_, /*escaped=*/true);
}

// The first install sets ready (under `mu`).  The replacing one runs while no sampled launch is being queued (`launch_mu`, taken
// before `mu` as the launch does): the next generation, its own pinned counter - a late count of the old table's launches does not
// reach it -, nothing queued yet, in use again.
bool SampledTable::learn_and_install(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool replace) {
    SampledLearnt l;
    if (!learn_sampled(of_.trimmed, text, pieces, piece_bytes, l)) return false;
    if (replace) {
        std::lock_guard<std::mutex> launches(launch_mu_);
        std::lock_guard<std::mutex> lock(mu_);
        on_swap_();
        dfa_ = std::move(l.dfa); dfa2_ = std::move(l.dfa2); stats_ = l.stats;
        gen_++;
        prev_lines_ = 0;
        retired_.store(false);
        return true;
    }
    std::lock_guard<std::mutex> lock(mu_);
    dfa_ = std::move(l.dfa); dfa2_ = std::move(l.dfa2); stats_ = l.stats;
    ready_.store(true, std::memory_order_release);
    return true;
}

bool SampledTable::start_first(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool background, bool *built) {
    if (first_.decided()) return false;
    if (!background) {
        return first_.start([&]() { const bool ok = learn_and_install(text, pieces, piece_bytes, false); if (built) *built = ok; }, false);
    }
    auto copy = std::make_shared<std::vector<uint8_t>>(text, text + (size_t)pieces * piece_bytes);
    return first_.start([this, copy, pieces, piece_bytes]() { (void)learn_and_install(copy->data(), pieces, piece_bytes, false); }, true);
}

bool SampledTable::relearn_due() const {
    if (!retired() || relearns_.size() >= kSampledRelearns) return false;
    return relearns_.empty() || relearns_.back()->state() == OnceTask::kDone;      // (one at a time)
}

void SampledTable::start_relearn(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool background) {
    OnceTask *task = nullptr;
    {
        std::lock_guard<std::mutex> launches(launch_mu_);
        if (!relearn_due()) return;
        relearns_.emplace_back(new OnceTask());
        task = relearns_.back().get();
    }
    auto copy = std::make_shared<std::vector<uint8_t>>(text, text + (size_t)pieces * piece_bytes);
    (void)task->start([this, copy, pieces, piece_bytes]() { (void)learn_and_install(copy->data(), pieces, piece_bytes, true); }, background);
}

void SampledTable::wait() {
    first_.wait();
    for (auto &task : relearns_) task->wait();
}

}  // namespace rrx
