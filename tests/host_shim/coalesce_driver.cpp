// Host driver of hk::Coalescer (hekaton_system_amd/csrc/coalesce.h) around a fake prover, built with -fsanitize=thread by
// tests/test_prove_coalesce_cpu.py.  argv: max_running threads calls_per_thread keys.  Prints "ok ..." or "FAIL ..." lines
// and exits non-zero on the first failed check.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../hekaton_system_amd/csrc/coalesce.h"

struct Item { int key, thread, seq; long value; };
struct Result { int status; long out; int batch; };

static const int CHUNK = 8;
static std::atomic<int> running{0}, max_seen{0}, errors{0};
static std::mutex log_mu;
static std::vector<std::vector<Item>> batches;        // every batch in the order it started

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); errors++; } } while (0)

int main(int argc, char** argv) {
    const int K = argc > 1 ? std::atoi(argv[1]) : 1, T = argc > 2 ? std::atoi(argv[2]) : 8;
    const int N = argc > 3 ? std::atoi(argv[3]) : 200, KEYS = argc > 4 ? std::atoi(argv[4]) : 3;
    hk::Coalescer<int, Item, Result> q(K, CHUNK, Result{-1, 0, 0});
    // the fake prover: key 2's value 13 makes the whole batch fail (status 7); value 29 throws
    auto run = [&](const int& key, hk::Coalescer<int, Item, Result>::Member* const* ms, size_t n) {
        int now = ++running;
        for (int m = max_seen.load(); now > m && !max_seen.compare_exchange_weak(m, now);) {}
        CHECK(now <= K, "more than %d batches running (%d)", K, now);
        CHECK(n >= 1 && n <= (size_t)CHUNK, "batch of %zu", n);
        std::vector<Item> b;
        bool fail = false, thr = false;
        for (size_t i = 0; i < n; i++) {
            CHECK(ms[i]->key == key && ms[i]->item->key == key, "member of key %d in a batch of key %d", ms[i]->item->key, key);
            b.push_back(*ms[i]->item);
            fail = fail || (key == 2 && ms[i]->item->value % 50 == 13);
            thr = thr || (key == 2 && ms[i]->item->value % 50 == 29);
        }
        { std::lock_guard<std::mutex> lk(log_mu); batches.push_back(b); }
        std::this_thread::sleep_for(std::chrono::microseconds(200 + 50 * n));
        --running;
        if (thr) throw std::runtime_error("fake prover");
        for (size_t i = 0; i < n; i++) ms[i]->result = Result{fail ? 7 : 0, ms[i]->item->value * 3 + key, (int)n};
    };
    std::vector<std::thread> th;
    std::atomic<int> done{0};
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            for (int i = 0; i < N; i++) {
                Item it{(t + i) % KEYS, t, i, (long)t * 1000 + i};
                Result r = q.submit(it.key, it, run);
                bool f2 = it.key == 2;
                // a member's status is its batch's: OK, the fake error 7, or the exception's -1
                CHECK(r.status == 0 || (f2 && (r.status == 7 || r.status == -1)), "thread %d call %d status %d", t, i, r.status);
                if (r.status == 0) CHECK(r.out == it.value * 3 + it.key, "thread %d call %d got %ld", t, i, r.out);
                if (r.status != -1) CHECK(r.batch >= 1 && r.batch <= CHUNK, "batch size %d", r.batch);
            }
            done++;
        });
    for (auto& x : th) x.join();                       // returns only if no caller was left waiting
    CHECK(done == T, "%d of %d threads finished", done.load(), T);
    // FIFO: within a key, a thread's calls run in the order it made them (each waits for its own), and every batch
    // holds the oldest queued items of its key - two members of one thread never share a batch
    std::vector<std::vector<int>> last(KEYS, std::vector<int>(T, -1));
    size_t total = 0, multi = 0;
    for (auto& b : batches) {
        total += b.size();
        multi += b.size() > 1;
        std::vector<int> seen(T, 0);
        for (auto& it : b) {
            CHECK(!seen[it.thread]++, "two calls of thread %d in one batch", it.thread);
            CHECK(it.seq > last[it.key][it.thread], "thread %d call %d ran after call %d", it.thread, it.seq, last[it.key][it.thread]);
            last[it.key][it.thread] = it.seq;
        }
    }
    CHECK(total == (size_t)T * N, "%zu items ran, %d submitted", total, T * N);
    if (T > 1) CHECK(multi > 0, "no batch held more than one call");
    if (T == 1) CHECK(multi == 0, "a lone caller was batched");
    std::printf("%s K=%d threads=%d calls=%d batches=%zu multi=%zu max_running=%d\n", errors ? "FAIL" : "ok", K, T, T * N,
                batches.size(), multi, max_seen.load());
    return errors ? 1 : 0;
}
