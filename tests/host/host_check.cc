// Stand-alone check of the command-line host's plumbing (ctucopy_amd/host/pipeline.h) and file readers / writers (files.h):
// no engine library, no GPU.  tests/test_host_pipeline_cpu.py builds it under ThreadSanitizer and under Address+UB sanitizers
// and runs it: exit status 0 and a silent stderr are the result.  usage: host_check <scratch directory>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "files.h"
#include "pipeline.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static void check_chan() {
    {  // a producer of 200 items and a consumer see them in order, through one slot
        Chan<int> c(1);
        std::vector<int> got;
        std::thread prod([&] {
            for (int i = 0; i < 200; i++) c.push(i);
            c.close();
        });
        int v;
        while (c.pop(v)) got.push_back(v);
        prod.join();
        CHECK(got.size() == 200);
        for (size_t i = 0; i < got.size(); i++) CHECK(got[i] == (int)i);
    }
    {  // pop drains what was queued and then returns false; push after close returns false
        Chan<int> c(1);
        int v = 0;
        CHECK(c.push(7));
        c.close();
        CHECK(!c.push(8));
        CHECK(c.pop(v) && v == 7);
        CHECK(!c.pop(v));
    }
    {  // a producer blocked on a full channel wakes on close
        Chan<int> c(1);
        CHECK(c.push(1));
        std::atomic<bool> about_to_push{false};
        bool pushed = true;
        std::thread prod([&] {
            about_to_push = true;
            pushed = c.push(2);
        });
        while (!about_to_push) std::this_thread::yield();
        for (int i = 0; i < 100; i++) std::this_thread::yield();  // (whether it already waits or not, close() must end it)
        c.close();
        prod.join();
        CHECK(!pushed);
    }
}

static void check_parallel_for() {
    std::vector<std::atomic<int>> seen(1000);
    for (auto &s : seen) s = 0;
    std::string what;
    try {
        parallel_for(8, seen.size(), [&](size_t i) {
            seen[i]++;
            if (i == 700 || i == 41) throw std::runtime_error(std::to_string(i));
        });
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    CHECK(what == "41");  // the lowest failing index: what a sequential loop would have hit first
    for (auto &s : seen) CHECK(s == 1);
    int calls = 0;
    parallel_for(8, 0, [&](size_t) { calls++; });
    CHECK(calls == 0);
}

static void check_per_gpu() {
    std::atomic<int> ran{0};
    std::vector<std::thread::id> ids(4);
    std::string what;
    try {
        per_gpu(4, [&](int g) {
            ids[g] = std::this_thread::get_id();
            ran++;
            if (g == 3 || g == 1) throw std::runtime_error(std::to_string(g));
        });
    } catch (const std::runtime_error &e) {
        what = e.what();
        CHECK(ran == 4);  // every thread was joined before the exception came out
    }
    CHECK(what == "1");
    for (int a = 0; a < 4; a++) {  // a thread per ordinal, none of them the caller
        CHECK(ids[a] != std::this_thread::get_id());
        for (int b = a + 1; b < 4; b++) CHECK(ids[a] != ids[b]);
    }
}

static int allocs = 0, frees = 0, frees_at_last_alloc = 0;
static void *counting_alloc(size_t n) {
    allocs++;
    frees_at_last_alloc = frees;
    return std::malloc(n);
}
static void counting_free(void *p) {
    frees++;
    std::free(p);
}

static void check_pin_pool() {
    {
        PinPool pool(counting_alloc, counting_free);
        void *pa, *pb, *pc;
        {
            PinBuf a = pool.get(10000), b = pool.get(100000), c = pool.get(50000);
            pa = a.get(), pb = b.get(), pc = c.get();
            CHECK(allocs == 3 && a.get_deleter().cap >= 10000);
        }
        CHECK(pool.idle.size() == 3);
        PinBuf fit = pool.get(40000);  // the smallest idle buffer that holds it, not the first and not the largest
        CHECK(fit.get() == pc && allocs == 3 && frees == 0);
        PinBuf big = pool.get(200000);  // nothing fits: the smallest idle one is freed, then a new one is made
        CHECK(allocs == 4 && frees == 1 && frees_at_last_alloc == 1);
        CHECK(big.get() != nullptr && big.get_deleter().cap >= 200000);
        CHECK(pool.idle.size() == 1 && pool.idle.begin()->second == pb);
        (void)pa;
        try {  // a handle dropped while the stack unwinds goes back to the pool
            PinBuf h = pool.get(90000);
            CHECK(h.get() == pb && pool.idle.empty());
            throw 1;
        } catch (int) {
        }
        CHECK(pool.idle.size() == 1 && pool.idle.begin()->second == pb);
        PinBuf moved = std::move(fit);  // move-only: one owner, one return
        CHECK(!fit && moved.get() == pc);
    }
    CHECK(allocs == 4 && frees == 4);  // after the pool has died
}

static void check_files(const std::string &dir) {
    {  // WAVE out and in again
        std::vector<int16_t> x(1000), y(1000, 0);
        for (size_t i = 0; i < x.size(); i++) x[i] = (int16_t)(i * 37 - 15000);
        const std::string p = dir + "/a.wav";
        write_wave(p, x.data(), x.size(), 16000);
        const ctu::Opts o = ctu::Opts::from_args({"-fs", "16000", "-format_in", "wave", "-format_out", "htk", "-preset", "mfcc", "-i", p, "-o", dir + "/a.htk"});
        CHECK(probe_samples(o, p) == 1000);
        decode_into(o, p, y.data(), y.size());
        CHECK(x == y);
    }
    for (int big = 0; big < 2; big++) {  // HTK features out and in again, both byte orders
        std::vector<float> rows(3 * 13);
        for (size_t i = 0; i < rows.size(); i++) rows[i] = 0.37f * (float)i - 3.f;
        ctu_dims d{};
        d.swap_out = big, d.htk_period = 100000, d.row_floats = 13, d.htk_kind = 6;
        const std::string p = dir + (big ? "/b.htk" : "/l.htk");
        write_htk(p, rows.data(), 3, d);
        ctu::Opts o;
        o.format_in = "htk", o.nfeacoefs = 13, o.swap_in = big != 0;
        CHECK(probe_samples(o, p) == 3 && probe_htk_rows(o, p) == 3);
        std::vector<uint32_t> w(rows.size());
        read_htk_rows(o, p, w.data(), 3);
        for (size_t i = 0; i < w.size(); i++) {  // the payload as it stands in the file: the float's bits, in the file's byte order
            uint32_t bits;
            std::memcpy(&bits, &rows[i], 4);
            CHECK((big ? __builtin_bswap32(w[i]) : w[i]) == bits);
        }
    }
    {  // A-law: every byte through g711_to_linear
        std::vector<uint8_t> codes(100);
        for (size_t i = 0; i < codes.size(); i++) codes[i] = (uint8_t)(2 * i + 3);
        const std::string p = dir + "/a.al";
        write_file(p, codes, "cannot write the a-law file");
        ctu::Opts o;
        o.format_in = "alaw";
        CHECK(probe_samples(o, p) == 100);
        std::vector<int16_t> y(100);
        decode_into(o, p, y.data(), y.size());
        for (size_t i = 0; i < y.size(); i++) CHECK(y[i] == g711_to_linear(codes[i], true));
    }
    for (const char *fmt : {"raw", "wave"}) {  // a missing file: the reference's texts (src/io/in.cc)
        ctu::Opts o;
        o.format_in = fmt, o.fs = 16000;
        std::string what;
        try {
            probe_samples(o, dir + "/missing");
        } catch (const Fatal &e) {
            what = e.what();
        }
        CHECK(what == (std::string(fmt) == "wave" ? "IN: Cannot open file!" : "IN: Cannot open data file!"));
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::printf("usage: host_check <scratch directory>\n");
        return 2;
    }
    check_chan();
    check_parallel_for();
    check_per_gpu();
    check_pin_pool();
    check_files(argv[1]);
    std::printf(failures ? "%d check(s) failed\n" : "host_check ok\n", failures);
    return failures ? 1 : 0;
}
