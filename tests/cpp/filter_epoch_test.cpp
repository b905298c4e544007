// filter_epoch_test.cpp — CPU test of csrc/filter_epoch.hpp: the per-handle epochs that tell
// whether a prepared filter still describes its handle. Stand-alone, plain g++ (no HIP).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../cuda-acceleratedvectordatabaseengine_amd/csrc/filter_epoch.hpp"

static int g_checks = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(x)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                             \
        }                                                             \
    } while (0)

int main() {
    using vdbe::FilterEpochs;
    int a = 0, b = 0;  // two "handles": only their addresses are used
    {
        FilterEpochs t;
        // a handle nobody asked about has no epoch, and 0 is never live
        CHECK(!t.live(&a, 0));
        CHECK(!t.live(&a, 1));
        CHECK(t.size() == 0);
        t.bump(&a);  // no filter exists: nothing to record
        CHECK(t.size() == 0);
        // get draws once and then repeats
        const uint64_t ea = t.get(&a);
        CHECK(ea != 0);
        CHECK(t.get(&a) == ea);
        CHECK(t.live(&a, ea));
        CHECK(!t.live(&a, ea + 1));
        CHECK(!t.live(&b, ea));
        // another handle draws another value
        const uint64_t eb = t.get(&b);
        CHECK(eb != 0 && eb != ea);
        CHECK(t.live(&b, eb) && !t.live(&a, eb) && !t.live(&b, ea));
        // bump: the old value is stale for good, the other handle is not concerned
        t.bump(&a);
        CHECK(!t.live(&a, ea));
        const uint64_t ea2 = t.get(&a);
        CHECK(ea2 != ea && ea2 != eb && ea2 > ea);
        CHECK(t.live(&a, ea2));
        CHECK(t.live(&b, eb));
        // erase: nothing of the handle is live; a recycled address draws a value never seen
        t.erase(&a);
        CHECK(!t.live(&a, ea) && !t.live(&a, ea2));
        CHECK(t.size() == 1);
        t.bump(&a);
        CHECK(t.size() == 1);
        const uint64_t ea3 = t.get(&a);
        CHECK(ea3 != ea && ea3 != ea2 && ea3 != eb);
        CHECK(!t.live(&a, ea) && !t.live(&a, ea2) && t.live(&a, ea3));
        t.erase(&a);
        t.erase(&a);  // (twice is fine)
        t.erase(&b);
        CHECK(t.size() == 0);
    }
    {
        // a recycled address over many lives: every value is new
        FilterEpochs t;
        std::vector<uint64_t> seen;
        for (int i = 0; i < 1000; ++i) {
            const uint64_t e = t.get(&a);
            for (uint64_t old : seen) CHECK(!t.live(&a, old));
            CHECK(seen.empty() || e > seen.back());
            seen.push_back(e);
            if (i % 3 == 0) t.bump(&a);
            else t.erase(&a);
            CHECK(!t.live(&a, e));
            if (seen.size() > 8) seen.erase(seen.begin());
        }
    }
    {
        // the process's table is one object
        CHECK(&vdbe::filter_epochs() == &vdbe::filter_epochs());
    }
    {
        // two threads: one bumps and re-reads `a`, one reads `a` and works on `b`. A value read
        // before a bump is never live after it, and values of one handle only grow.
        FilterEpochs t;
        std::atomic<bool> stop{false};
        std::atomic<uint64_t> bumps{0};
        bool ok_writer = true, ok_reader = true;
        (void)t.get(&a);
        std::thread writer([&] {
            uint64_t last = 0;
            for (int i = 0; i < 20000; ++i) {
                const uint64_t e = t.get(&a);
                if (e <= last) ok_writer = false;
                last = e;
                t.bump(&a);
                if (t.live(&a, e)) ok_writer = false;
                bumps.fetch_add(1);
            }
            stop = true;
        });
        std::thread reader([&] {
            uint64_t last = 0;
            while (!stop) {
                const uint64_t e = t.get(&a);
                if (e < last) ok_reader = false;  // (the same value twice between two bumps is fine)
                last = e;
                (void)t.live(&a, e);
                const uint64_t f = t.get(&b);
                t.bump(&b);
                if (t.live(&b, f)) ok_reader = false;
                t.erase(&b);
            }
        });
        writer.join();
        reader.join();
        CHECK(ok_writer);
        CHECK(ok_reader);
        CHECK(bumps == 20000);
        CHECK(t.live(&a, t.get(&a)));
    }
    std::printf("all checks passed (%d checks)\n", g_checks);
    return 0;
}
