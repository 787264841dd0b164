// once_task.hpp — a piece of host work that is decided once per object and may run beside the caller.
#pragma once
#include <atomic>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>

namespace rrx {

// A piece of host work that is decided ONCE per object and may run beside the caller (host only: no device call in here).
// start() or skip() moves kIdle on, everything else only READS the atomic state - the std::thread is touched by its owner
// alone (start under `mu_`, wait()).  The job runs in the deciding caller's thread or in a thread of its own (joined by
// wait() / the destructor); the state becomes kDone when it returns.
class OnceTask {
public:
    enum State { kIdle = 0, kRunning = 1, kDone = 2, kSkipped = 3 };
    OnceTask() = default;
    OnceTask(const OnceTask &) = delete;
    OnceTask &operator=(const OnceTask &) = delete;
    ~OnceTask() { wait(); }
    State state() const { return (State)state_.load(std::memory_order_acquire); }
    bool decided() const { return state() != kIdle; }
    // fn() runs without try / catch - an exception ends the process or leaves kRunning for good; the fix goes here.
    bool start(std::function<void()> job, bool background) {      // false: decided before (by another caller)
        std::unique_lock<std::mutex> lock(mu_);        // held from the decision to the thread being in place: wait() sees both or neither
        int expected = kIdle;
        if (!state_.compare_exchange_strong(expected, kRunning, std::memory_order_acq_rel)) return false;
        auto body = [this](std::function<void()> fn) {
            fn();
            state_.store(kDone, std::memory_order_release);
        };
        if (!background) { lock.unlock(); body(std::move(job)); return true; }
        thread_ = std::thread(body, std::move(job));
        return true;
    }
    bool skip() {               // kIdle -> kSkipped; false: decided before
        int expected = kIdle;
        return state_.compare_exchange_strong(expected, kSkipped, std::memory_order_acq_rel);
    }
    void wait() {               // returns when no job of this object is running in a thread of its own any more
        std::lock_guard<std::mutex> lock(mu_);
        if (thread_.joinable()) thread_.join();
    }
private:
    std::atomic<int> state_{kIdle};
    std::mutex mu_;             // guards thread_
    std::thread thread_;
};

}  // namespace rrx
