// coalesce.h — concurrent calls that share a key meet in one batch (hk_prove's coalescer).
// Plain C++17, no HIP: tests/test_prove_coalesce_cpu.py builds it under -fsanitize=thread around a fake prover.
//
// A caller queues its item (FIFO) and then, under the lock, either finds its result ready, or - when fewer than
// `max_running` batches are in progress - becomes a leader: it takes up to `max_batch` queued items of the key whose oldest
// item is oldest (its own item is a candidate like any other), runs them with the lock released, stores every member's
// result and wakes the waiters.  There is no waiting window: a lone caller leads at once, a batch of one.  A leader whose
// own item was not in its batch goes back to waiting (or leads again).  Waiters hold nothing but their queue entry.
#pragma once
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
    Coalescer(size_t max_running, size_t max_batch, Result on_exception)
        : max_running_(max_running ? max_running : 1), max_batch_(max_batch ? max_batch : 1), on_exception_(on_exception) {}
    Coalescer(const Coalescer&) = delete;
    Coalescer& operator=(const Coalescer&) = delete;

    // run(key, Member* const* members, size_t n) fills members[i]->result for every i; it runs without the lock
    template <class Fn> Result submit(const Key& key, const Item& item, Fn&& run) {
        Member me;
        me.key = key;
        me.item = &item;
        std::unique_lock<std::mutex> lk(mu_);
        queue_.push_back(&me);
        for (;;) {
            if (me.done) return me.result;
            if (running_ < max_running_ && !queue_.empty()) {
                std::vector<Member*> batch;
                const Key k = queue_.front()->key;
                for (auto it = queue_.begin(); it != queue_.end() && batch.size() < max_batch_;) {
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
                cv_.notify_all();
                continue;
            }
            cv_.wait(lk);
        }
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Member*> queue_;       // entries live on their callers' stacks until done
    size_t running_ = 0;
    const size_t max_running_, max_batch_;
    const Result on_exception_;
};

}  // namespace hk
