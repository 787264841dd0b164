// sampled.hpp — the life of a sampled table, host only: no HIP.  AUTO ended on the NFA lane engine because the subset
// construction explodes; the sets a text sample reaches are interned into a table with an ESCAPE state, the batch entry runs the
// stride-2 kernel on it (two result bits per line) and lets the NFA engine decide the lines that escaped.  The table is LEARNT once -
// by the first rrx_match_corpus against a corpus that carries a sample (beside the caller), or by rrx_learn_table (in the caller's
// thread) -, INSTALLED, JUDGED by every launch on the escapes of the last launch that has finished, RETIRED when a corpus escapes from
// it (the regex is back on the NFA engine at its own rate) and then LEARNT AGAIN from the sample of the corpus that retired it, up to
// kSampledRelearns times.  What touches the device (the uploaded tables, the counters) is the ABI layer's: handles.hpp, SampledOnDevice.
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "lower.hpp"
#include "once_task.hpp"
#include "plan.hpp"

namespace rrx {

// State budgets of the learn step, tried from the largest down, halving: the largest table whose stride-2 form fits the LDS.
constexpr uint32_t kSampledMaxStates = 2048, kSampledMinStates = 64;
// A table its own sample escapes from is the wrong tool - every escaped line is read a second time by the NFA engine: more than
// this share of the sample's lines and nothing is installed.
constexpr uint32_t kSampleEscapePercent = 2;
// A corpus that escapes from the table - not the text it was learnt from - retires it: more than this share of the lines ...
constexpr uint32_t kRetireEscapePercent = 5;
// ... of a launch of at least this many lines (a handful of lines says nothing about the text).
constexpr unsigned long long kRetireMinLines = 1024;
// A retired table is learnt again this many times in all; then the regex stays on the NFA engine.
constexpr uint32_t kSampledRelearns = 3;

// The learn step: pieces x piece_bytes of text -> the table and its stride-2 form; false: nothing usable came out (no table fits
// the device, the closure closed the table - lower_dfa would have too -, or the sample itself escapes).
struct SampledLearnt { DfaProgram dfa; Dfa2Program dfa2; SampledTableStats stats; };
bool learn_sampled(const Trimmed &trimmed, const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, SampledLearnt &out);

// The retirement rule: `escapes_seen` lines escaped in the last launch that has finished, `prev_lines` lines had the last launch queued.
// the two belong to different launches; the fix judges a pair the device wrote for ONE launch - here.
bool sampled_retires(unsigned long long escapes_seen, unsigned long long prev_lines);

// Takes no lock of its own: `mu` guards the programs and the stats, `launch_mu` - taken BEFORE `mu` - is held by whoever queues a
// sampled launch and guards the generation, prev_lines and the relearn tasks.  Both are the owner's (rrx_regex: mu, onepass_mu).
struct SampledTable {
    // `on_swap`: runs under both locks when a relearnt table replaces the one in use (the owner puts its device tables aside)
    SampledTable(const Programs &of, std::mutex &mu, std::mutex &launch_mu, std::function<void()> on_swap)
        : of_(of), mu_(mu), launch_mu_(launch_mu), on_swap_(std::move(on_swap)) {}
    ~SampledTable() { wait(); }                          // (a build still running writes the members below: none goes before it has ended)

    bool eligible() const;                               // automata that AUTO leaves on the NFA lane engine
    bool ready() const { return ready_.load(std::memory_order_acquire); }
    bool retired() const { return retired_.load(); }
    bool in_use(bool option_on) const { return eligible() && option_on && ready() && !retired(); }
    // rrx_sampled_table: 0 none, 1 in use, 2 being built, 3 retired; the table's size where there is one
    int status(uint32_t *table_states, uint32_t *open_transitions) const;
    // rrx_program_words, RRX_PROGRAM_SAMPLED_DFA / _DFA2 (nothing before the first install)
    void words(bool stride2, std::vector<uint32_t> &w) const;
    const Dfa2Program &dfa2() const { return dfa2_; }    // call with `mu` held (the upload)

    // The first build.  false: decided before.  In the caller's thread `text` is read in place and *built says what came out;
    // in the background a copy is learnt from.
    bool start_first(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool background, bool *built = nullptr);
    // The table is retired: learn it again from this sample (once per retirement, kSampledRelearns times in all).  Call WITHOUT the
    // locks: with background == false the job runs right here and takes both to swap the table in.
    void start_relearn(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool background);
    void wait();                                         // returns when no build of this table is running any more

    // ---- call with `launch_mu` held
    uint32_t seen_slot() const { return gen_ < kSampledRelearns ? gen_ : kSampledRelearns; }      // of kSampledRelearns + 1 pinned counters
    void judge(unsigned long long escapes_seen) { if (sampled_retires(escapes_seen, prev_lines_)) retired_.store(true); }
    void queued(unsigned long long lines) { prev_lines_ = lines; }
    bool relearn_due() const;                            // retired, fewer than kSampledRelearns so far, the last one done

private:
    bool learn_and_install(const uint8_t *text, uint32_t pieces, uint32_t piece_bytes, bool replace);
    const Programs &of_;
    std::mutex &mu_, &launch_mu_;
    std::function<void()> on_swap_;
    OnceTask first_;
    std::atomic<bool> ready_{false};                     // (set under `mu` after the programs below are complete)
    std::atomic<bool> retired_{false};
    DfaProgram dfa_;                                     // (under `mu`)
    Dfa2Program dfa2_;
    SampledTableStats stats_;
    uint32_t gen_ = 0;                                   // generation of the table in use (under `launch_mu`)
    unsigned long long prev_lines_ = 0;                  // lines of the last sampled launch queued (under `launch_mu`)
    std::vector<std::unique_ptr<OnceTask>> relearns_;    // (under `launch_mu`)
};

}  // namespace rrx
