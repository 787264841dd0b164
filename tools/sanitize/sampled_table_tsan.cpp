// The sampled table's life (sampled.hpp: SampledTable - the library's own struct, with an owner that holds its two mutexes the way
// rrx_regex does) under ThreadSanitizer, CPU only.  Per round: three callers race the first build (the background path of
// rrx_match_corpus, the caller's-thread path of rrx_learn_table, and a late one that must be told "decided already"), pollers read
// the status and the programs the way rrx_sampled_table and rrx_program_words do, and a "launch" thread takes the launch lock, feeds
// escape counts to the retirement rule and asks for the relearn, until the retire -> relearn -> swap cycle has run kSampledRelearns
// times and a further retirement starts nothing.  On odd rounds the owner is destroyed right after the first build was decided, while
// it may still be running.  The pattern is the pair tests/test_lowering.py::test_sampled_table_decides_exactly_or_not_at_all learns
// (URL text under U2(x|y)*x(x|y){30}): its table has about a hundred states, a learn step takes a fraction of a second here.
// build + run: make -C tools/sanitize tsan
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rrx.h"
#include "../../roaringregex_amd/csrc/sampled.hpp"

using namespace rrx;

#define CHECK(cond, what) do { if (!(cond)) { std::printf("%s (round %d)\n", what, round); std::abort(); } } while (0)

struct Owner {                       // what rrx_regex keeps around the table
    Programs programs;
    std::mutex mu, launch_mu;        // rrx_regex::mu, rrx_regex::onepass_mu
    int on_device = 1, kept = 0;     // (under mu) the device tables of the generation in use / of the earlier ones
    int swaps = 0;                   // (under both) successful relearns
    SampledTable table{programs, mu, launch_mu, [this] { kept += on_device; swaps++; }};       // (last member: destroyed first, and ~SampledTable waits for a running build)
    explicit Owner(const Programs &p) : programs(p) {}
};

static std::vector<uint8_t> url_text(size_t nbytes) {
    std::mt19937 rng(11);
    auto word = [&](int lo, int hi, const char *alphabet, size_t n) { std::string s; for (int k = lo + (int)(rng() % (hi - lo + 1)); k > 0; k--) s += alphabet[rng() % n]; return s; };
    std::string text;
    while (text.size() < nbytes) {
        static const char *schemes[] = {"http", "https", "ftp"};
        std::string ln = std::string(schemes[rng() % 3]) + "://" + word(1, 10, "abcdefghijklmnopqrstuvwxyz0123456789-", 37) + "." + word(2, 4, "comnetrgdu", 10);
        if (rng() % 4 == 0) ln += ":" + word(1, 4, "0123456789", 10);
        for (int k = rng() % 4; k > 0; k--) ln += "/" + word(0, 8, "abcdefghijklmnopqrstuvwxyzABCXYZ019._~%-", 40);
        if (rng() % 3 == 0) ln += "?" + word(1, 12, "abcdefxyz019=&._-", 17);
        text += ln + "\n";
    }
    return std::vector<uint8_t>(text.begin(), text.end());
}

int main() {
    const std::string u2 = "(http|https|ftp)://([a-z0-9-]{1,16}\\.){1,3}[a-z]{2,6}(:[0-9]{1,5})?(/[A-Za-z0-9._~%-]*)*(\\?[A-Za-z0-9._~%=&-]*)?(#[A-Za-z0-9._~%-]*)?";
    Programs programs;
    plan_engines(u2 + "(x|y)*x(x|y){30}", RRX_ENGINE_AUTO, programs);
    const std::vector<uint8_t> sample = url_text(64 << 10);
    const uint32_t pieces = 256, piece_bytes = 256;      // (as a corpus' sample: 256 lanes of 256 bytes)
    int rounds_done = 0, swaps_total = 0;
    for (int round = 0; round < 4; round++) {
        auto owner = std::make_unique<Owner>(programs);
        Owner *o = owner.get();
        CHECK(o->table.eligible(), "NOT ELIGIBLE");
        const bool full = round % 2 == 0;
        std::atomic<int> first_builds{0}, decided{0};
        std::atomic<bool> stop{false};
        std::vector<std::thread> th;
        for (int k = 0; k < 3; k++)
            th.emplace_back([&, k] {
                if (k == 2) { while (decided.load() == 0) std::this_thread::yield(); }       // the late caller
                bool built = false;
                const bool won = k == 1 ? o->table.start_first(sample.data(), 1, (uint32_t)sample.size(), /*background=*/false, &built)
                                        : o->table.start_first(sample.data(), pieces, piece_bytes, /*background=*/true);
                if (k == 2 && won) { std::printf("THE LATE CALLER DECIDED\n"); std::abort(); }
                if (k == 1 && won && !built) { std::printf("NO TABLE FROM THE URL SAMPLE\n"); std::abort(); }
                if (won) first_builds++;
                decided++;
            });
        for (int k = 0; k < 2; k++)                                   // pollers: rrx_sampled_table, rrx_program_words
            th.emplace_back([&] {
                std::vector<uint32_t> w;
                while (!stop.load()) {
                    uint32_t states = 0, open = 0;
                    const int st = o->table.status(&states, &open);
                    if ((st == 1 || st == 3) != (states != 0)) { std::printf("STATUS %d WITH %u STATES\n", st, states); std::abort(); }
                    w.clear();
                    o->table.words(/*stride2=*/false, w);
                    if (st != 0 && st != 2 && (w.size() < 4 || w[0] == 0)) { std::printf("READY WITHOUT A PROGRAM\n"); std::abort(); }
                    w.clear();
                    o->table.words(/*stride2=*/true, w);
                    std::this_thread::yield();
                }
            });
        for (int k = 0; k < 3; k++) th[k].join();
        CHECK(first_builds.load() == 1, "NOT EXACTLY ONE FIRST BUILD");
        if (full) {
            // the launches: every one judges what the one before it "counted", a retired table is learnt again beside the caller or
            // in this thread, and after kSampledRelearns swaps a retirement is final
            uint32_t gen_seen = 0;
            int launches_after_cap = 0;
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(120);
            while (launches_after_cap < 3) {
                CHECK(std::chrono::steady_clock::now() < deadline, "A RELEARN DID NOT SWAP ITS TABLE IN");
                bool relearn = false;
                {
                    std::lock_guard<std::mutex> launches(o->launch_mu);
                    const uint32_t gen = o->table.seen_slot();                // (the generation, up to the cap)
                    CHECK(gen == gen_seen || gen == gen_seen + 1, "THE GENERATION JUMPED");
                    CHECK(gen <= kSampledRelearns && (int)gen == o->swaps, "GENERATION AND SWAPS DISAGREE");
                    if (gen != gen_seen) CHECK(!o->table.retired(), "RETIRED RIGHT AFTER A SWAP");
                    gen_seen = gen;
                    if (o->table.in_use(true)) {
                        { std::lock_guard<std::mutex> lock(o->mu); (void)o->table.dfa2().nstates; }      // (the upload)
                        o->table.judge(/*escapes_seen=*/10);                  // nothing queued yet, or 10 of 2000: stays
                        CHECK(!o->table.retired(), "RETIRED BY 0.5 %");
                        o->table.queued(2000);
                        o->table.judge(/*escapes_seen=*/101);                 // more than 5 % of 2000
                        CHECK(o->table.retired(), "NOT RETIRED BY 5.05 %");
                    }
                    relearn = o->table.ready() && o->table.retired();
                    if (gen == kSampledRelearns && relearn) { CHECK(!o->table.relearn_due(), "A FOURTH RELEARN IS DUE"); launches_after_cap++; }
                }
                if (relearn) o->table.start_relearn(sample.data(), pieces, piece_bytes, /*background=*/(gen_seen & 1) == 0);
                std::this_thread::yield();
            }
            o->table.wait();
            std::lock_guard<std::mutex> launches(o->launch_mu);
            CHECK(o->swaps == (int)kSampledRelearns && o->kept == (int)kSampledRelearns && o->table.seen_slot() == kSampledRelearns, "NOT kSampledRelearns SWAPS");
            swaps_total += o->swaps;
        }
        stop = true;                                                  // odd rounds: the destructor meets a running first build
        for (size_t k = 3; k < th.size(); k++) th[k].join();
        owner.reset();                                                // ~SampledTable joins the build, then the members go
        rounds_done++;
    }
    std::printf("sampled table: %d rounds raced, %d relearns swapped in, no report\n", rounds_done, swaps_total);
    return 0;
}
