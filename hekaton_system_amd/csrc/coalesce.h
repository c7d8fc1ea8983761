// coalesce.h — concurrent calls that share a key meet in one batch (hk_prove's coalescer).
// Plain C++17, no HIP: tests/test_prove_coalesce_cpu.py and tests/test_prove_gather_cpu.py build it under
// -fsanitize=thread around a fake prover.
//
// A caller queues its item (FIFO) and then, under the lock, either finds its result ready, or - when fewer than
// `max_running` batches are in progress - becomes a leader: it takes up to `max_batch` queued items of the key whose oldest
// item is oldest (its own item is a candidate like any other), runs them with the lock released, stores every member's
// result and wakes the waiters.  A leader whose own item was not in its batch goes back to waiting (or leads again).
// Waiters hold nothing but their queue entry.
//
// gather_us = 0: no waiting window, a leader takes whatever is queued.  Callers that loop then settle into groups of
// uneven sizes that rotate through the lanes and the queue (the callers a finished batch releases are never the next batch).
// gather_us = W > 0 adds two rules, both decided under the same lock:
//   balance  a leader takes at most target = ceil(C / max_running) items, C = the callers in circulation: those queued or
//            in a running batch, plus those counted as returning;
//   gather   the n members of a batch that ends count as returning until each calls submit() again (an arrival takes one
//            off the oldest open entry) or until W after that batch ended, when what is left of its count is dropped.
//            A caller that could lead but finds fewer than `target` items of the oldest key while callers are still
//            returning waits for the next arrival or the earliest open deadline, then decides again.
// A lone caller never waits (its own arrival clears the only open entry: C = 1, target = 1), and callers that never come
// back cost at most W once: every wait ends at a deadline at most W after some batch ended.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <mutex>
#include <vector>

namespace hk {

template <class Key, class Item, class Result>
class Coalescer {
public:
    struct Member {
        Key key;
        const Item* item;
        Result result;
        bool done = false;
    };
    // on_exception: the result every member of a batch gets when the batch function throws
    Coalescer(size_t max_running, size_t max_batch, Result on_exception, long gather_us = 0)
        : max_running_(max_running ? max_running : 1), max_batch_(max_batch ? max_batch : 1), on_exception_(on_exception),
          gather_(gather_us > 0 ? gather_us : 0) {}
    Coalescer(const Coalescer&) = delete;
    Coalescer& operator=(const Coalescer&) = delete;

    // run(key, Member* const* members, size_t n) fills members[i]->result for every i; it runs without the lock
    template <class Fn> Result submit(const Key& key, const Item& item, Fn&& run) {
        Member me;
        me.key = key;
        me.item = &item;
        const bool gather = gather_.count() > 0;
        std::unique_lock<std::mutex> lk(mu_);
        if (gather) {
            expire(Clock::now());
            if (!returning_.empty()) {                      // this arrival is one of the callers the oldest batch released
                returning_n_--;
                if (--returning_.front().n == 0) returning_.pop_front();
            }
            inside_++;
            cv_.notify_all();                               // a leader may be gathering
        }
        queue_.push_back(&me);
        for (;;) {
            if (me.done) return me.result;
            if (running_ < max_running_ && !queue_.empty()) {
                const Key k = queue_.front()->key;
                size_t take = max_batch_;
                if (gather) {
                    expire(Clock::now());
                    const size_t target = (inside_ + returning_n_ + max_running_ - 1) / max_running_;
                    if (target < take) take = target;
                    size_t have = 0;
                    for (const Member* m : queue_) have += m->key == k;
                    if (have < take && returning_n_ > 0) {
                        // a wall-clock deadline: wait_until on system_clock is pthread_cond_timedwait, which ThreadSanitizer
                        // intercepts (steady_clock goes through pthread_cond_clockwait, which gcc 11's does not)
                        cv_.wait_until(lk, returning_.front().deadline);
                        continue;
                    }
                }
                std::vector<Member*> batch;
                for (auto it = queue_.begin(); it != queue_.end() && batch.size() < take;) {
                    if ((*it)->key == k) { batch.push_back(*it); it = queue_.erase(it); }
                    else ++it;
                }
                running_++;
                lk.unlock();
                try {
                    run(k, batch.data(), batch.size());
                } catch (...) {
                    for (Member* m : batch) m->result = on_exception_;
                }
                lk.lock();
                running_--;
                for (Member* m : batch) m->done = true;     // a member may return (and its Member go) once this is set
                if (gather) {                               // the members leave the circulation's first group for its second here
                    inside_ -= batch.size();
                    returning_n_ += batch.size();
                    returning_.push_back({Clock::now() + gather_, batch.size()});
                }
                cv_.notify_all();
                continue;
            }
            cv_.wait(lk);
        }
    }

private:
    typedef std::chrono::system_clock Clock;
    struct Returning { Clock::time_point deadline; size_t n; };     // a finished batch: n > 0 members not yet back
    void expire(Clock::time_point now) {
        while (!returning_.empty() && now >= returning_.front().deadline) {
            returning_n_ -= returning_.front().n;
            returning_.pop_front();
        }
    }

    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Member*> queue_;       // entries live on their callers' stacks until done
    size_t running_ = 0;
    size_t inside_ = 0;               // callers queued or in a running batch (counted with gather_ > 0 only)
    size_t returning_n_ = 0;          // sum of returning_[i].n
    std::deque<Returning> returning_; // oldest first: deadlines ascend (one window for all)
    const size_t max_running_, max_batch_;
    const Result on_exception_;
    const std::chrono::microseconds gather_;
};

}  // namespace hk
