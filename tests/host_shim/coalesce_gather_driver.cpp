// Host driver of hk::Coalescer's gather window (hekaton_system_amd/csrc/coalesce.h) around a fake
// prover, built with -fsanitize=thread by tests/test_prove_gather_cpu.py.
// argv: max_running threads calls_of_thread_0 keys gather_us work_us [calls_of_the_other_threads = calls_of_thread_0]
// Checks the coalescer's invariants as tests/host_shim/coalesce_driver.cpp does, then prints one line
//   ok|FAIL K=.. threads=.. items=.. batches=.. max_running=.. elapsed_ms=.. sizes=1:a,2:b,...
// (sizes: how many batches of each size ran) and exits non-zero when a check failed.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
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
    if (argc < 7) { std::printf("FAIL usage: K threads calls keys gather_us work_us [calls_others]\n"); return 2; }
    const int K = std::atoi(argv[1]), T = std::atoi(argv[2]), N0 = std::atoi(argv[3]), KEYS = std::atoi(argv[4]);
    const long W = std::atol(argv[5]), WORK = std::atol(argv[6]);
    const int N1 = argc > 7 ? std::atoi(argv[7]) : N0;
    typedef hk::Coalescer<int, Item, Result> Q;
    Q q(K, CHUNK, Result{-1, 0, 0}, W);
    // the fake prover: key 2's value 13 (mod 50) makes the whole batch fail (status 7); value 29 throws
    auto run = [&](const int& key, Q::Member* const* ms, size_t n) {
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
        std::this_thread::sleep_for(std::chrono::microseconds(WORK));
        --running;
        if (thr) throw std::runtime_error("fake prover");
        for (size_t i = 0; i < n; i++) ms[i]->result = Result{fail ? 7 : 0, ms[i]->item->value * 3 + key, (int)n};
    };
    std::vector<std::thread> th;
    std::atomic<int> done{0};
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t] {
            for (int i = 0, n = t ? N1 : N0; i < n; i++) {
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
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    CHECK(done == T, "%d of %d threads finished", done.load(), T);
    // FIFO: within a key, a thread's calls run in the order it made them, and two members of one thread never share a batch
    std::vector<std::vector<int>> last(KEYS, std::vector<int>(T, -1));
    std::map<size_t, size_t> sizes;
    size_t total = 0;
    for (auto& b : batches) {
        total += b.size();
        sizes[b.size()]++;
        std::vector<int> seen(T, 0);
        for (auto& it : b) {
            CHECK(!seen[it.thread]++, "two calls of thread %d in one batch", it.thread);
            CHECK(it.seq > last[it.key][it.thread], "thread %d call %d ran after call %d", it.thread, it.seq, last[it.key][it.thread]);
            last[it.key][it.thread] = it.seq;
        }
    }
    const size_t want = (size_t)N0 + (size_t)(T - 1) * N1;
    CHECK(total == want, "%zu items ran, %zu submitted", total, want);
    std::printf("%s K=%d threads=%d items=%zu batches=%zu max_running=%d elapsed_ms=%.1f sizes=", errors ? "FAIL" : "ok", K, T,
                total, batches.size(), max_seen.load(), ms);
    bool first = true;
    for (auto& s : sizes) { std::printf("%s%zu:%zu", first ? "" : ",", s.first, s.second); first = false; }
    std::printf("\n");
    return errors ? 1 : 0;
}
