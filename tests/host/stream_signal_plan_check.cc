// Stand-alone check of the signal descriptors of the push planner (ctucopy_amd/csrc/stream_plan.h: PushGeom::signal, SignalPush,
// PushLayout::capacity, stream_plan_finish's signal form): no engine library, no GPU, no HIP.  tests/test_stream_signal_plan_cpu.py
// builds it under Address+UB sanitizers and runs it: exit status 0, a final "stream_signal_plan_check ok" and a silent stderr are the
// result.  Random pushes over a few streams, and pushes that complete 0, 1 and many frames, each against the restatement below, which
// counts frames one by one and samples frame by frame; the capacity exactly enough and one sample short.  (There is no parity to
// check: a stream's tail is owned by one workgroup, which reads it ahead of a barrier - stream_signal_kernels.h.)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "stream_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

// ---- the restatement: frame t is complete once the file holds window + t * wshift samples; every complete frame finishes wshift samples
static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((int64_t)window + F * wshift <= total) F++;
    return F;
}
static int64_t samples_of(int64_t total, int window, int wshift) {
    int64_t n = 0;
    for (int64_t t = 0; (int64_t)window + t * wshift <= total; t++) n += wshift;
    return n;
}

struct Arrays {
    std::vector<StreamPush> push;
    std::vector<SignalPush> sig;
    std::vector<int> heads, tail;
    std::vector<int64_t> counts, consumed;
    std::vector<uint8_t> hsel;
    PushLayout L;
    Arrays(int n_streams, int max_chains, unsigned char fill) {
        const int nh = chain_deal(n_streams, max_chains).heads();
        push.resize(n_streams); sig.resize(n_streams); heads.resize(nh); tail.resize(nh);
        counts.resize(n_streams); consumed.resize(n_streams); hsel.resize(n_streams);
        std::memset(push.data(), fill, push.size() * sizeof(StreamPush));
        std::memset(sig.data(), fill, sig.size() * sizeof(SignalPush));
        std::memset(heads.data(), fill, heads.size() * sizeof(int));
        std::memset(tail.data(), fill, tail.size() * sizeof(int));
        std::memset(counts.data(), fill, counts.size() * 8);
        std::memset(consumed.data(), fill, consumed.size() * 8);
        std::memset(hsel.data(), fill, hsel.size());
        L.push = push.data(); L.sig = sig.data(); L.heads = heads.data(); L.tail = tail.data();
        L.row_counts = counts.data(); L.consumed = consumed.data(); L.hsel = hsel.data();
    }
};

static int pushes_checked = 0, frames_seen[3] = {0, 0, 0};  // pushes of a stream that completed no frame, one, more

static void check_push(const PushGeom &g0, const std::vector<int64_t> &consumed, const std::vector<uint8_t> &hsel, const std::vector<int32_t> &ids,
                       const std::vector<int64_t> &ns, const std::vector<int64_t> &off) {
    const int n = (int)ids.size(), n_streams = (int)consumed.size();
    PushGeom g = g0;
    g.arena_samples = g.tile_cap = INT64_MAX / 2;
    // ---- what the push must be
    std::vector<int64_t> F0(n), T(n), out0(n), row0(n), cnt(n);
    int64_t oo = 0, ro = 0, most = 0;
    for (int i = 0; i < n; i++) {
        const int64_t c = consumed[ids[i]];
        F0[i] = frames_of(c, g.window, g.wshift);
        T[i] = frames_of(c + ns[i], g.window, g.wshift) - F0[i];
        cnt[i] = samples_of(c + ns[i], g.window, g.wshift) - samples_of(c, g.window, g.wshift);
        out0[i] = oo; row0[i] = ro;
        oo += cnt[i]; ro += T[i];
        if (cnt[i] > most) most = cnt[i];
        frames_seen[T[i] == 0 ? 0 : T[i] == 1 ? 1 : 2]++;
    }
    const std::vector<int64_t> consumed_before = consumed;
    // ---- no capacity given, exactly enough, and room to spare: the same plan
    for (int64_t capacity : {(int64_t)-1, oo, oo + 7}) {
        Arrays a(n_streams, g.max_chains, 0xAB);
        a.L.capacity = capacity;
        CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L));
        const PushLayout &L = a.L;
        CHECK(!L.over_capacity && L.rows_out == oo && L.base_rows == ro && L.most == most);
        int64_t sum = 0;
        for (int i = 0; i < n; i++) {
            const SignalPush &q = L.sig[i];
            CHECK(q.out0 == out0[i] && q.row0 == row0[i] && q.row0 == L.push[i].row0 && q.F0 == F0[i] && q.id == ids[i] && q.T == T[i]);
            CHECK(L.row_counts[i] == cnt[i] && cnt[i] == T[i] * g.wshift);
            CHECK(L.consumed[i] == consumed[ids[i]] + ns[i]);
            CHECK(L.hsel[i] == hsel[ids[i]]);  // (no row history on a signal set: nothing flips)
            sum += L.row_counts[i];
        }
        CHECK(sum == L.rows_out);
    }
    // ---- one sample short: refused, as the capacity's fault, with the caller's mirrors as they were
    if (oo > 0) {
        Arrays a(n_streams, g.max_chains, 0);
        a.L.capacity = oo - 1;
        CHECK(!stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L));
        CHECK(a.L.over_capacity);
        a.L.capacity = 0;
        CHECK(!stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L) && a.L.over_capacity);
    } else {
        Arrays a(n_streams, g.max_chains, 0);
        a.L.capacity = 0;  // a push that completes no frame needs no room
        CHECK(stream_plan_push(g, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L) && !a.L.over_capacity);
    }
    // ---- an arena too small is not the capacity's fault
    {
        Arrays a(n_streams, g.max_chains, 0);
        PushGeom tight = g;
        tight.arena_samples = 1;
        a.L.capacity = oo;
        CHECK(!stream_plan_push(tight, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L) && !a.L.over_capacity);
    }
    // ---- without signal state the same push counts rows, and a capacity is not looked at
    {
        Arrays a(n_streams, g.max_chains, 0);
        PushGeom rows = g;
        rows.signal = false;
        a.L.sig = nullptr;
        a.L.capacity = 0;
        CHECK(stream_plan_push(rows, consumed.data(), hsel.data(), n, ids.data(), ns.data(), off.data(), a.L) && !a.L.over_capacity);
        CHECK(a.L.rows_out == ro);
        for (int i = 0; i < n; i++) CHECK(a.L.row_counts[i] == T[i]);
    }
    CHECK(consumed == consumed_before);
    pushes_checked++;
}

static void check_finish(int window, int wshift) {
    for (int64_t F = 0; F <= 4; F++)
        for (int64_t extra : {(int64_t)0, (int64_t)1, (int64_t)wshift - 1}) {
            const int64_t total = F == 0 ? extra * 3 : (int64_t)window + (F - 1) * wshift + extra;
            if (frames_of(total, window, wshift) != F) continue;
            const FinishLayout f = stream_plan_finish(window, wshift, 0, 0, total, 5, 1, false, true);
            CHECK(f.frames == F && !f.too_short);
            CHECK(f.pending == (F > 0 ? window - wshift : 0));  // ctu_streams_signal_step's
            CHECK(f.sig.id == 5 && f.sig.T == 0 && f.sig.out0 == 0 && f.sig.row0 == 0 && f.sig.F0 == F);
            // the row form of the same stream is untouched by the new argument's default
            const FinishLayout r = stream_plan_finish(window, wshift, 0, 0, total, 5, 1);
            CHECK(r.frames == F && r.pending == 0 && !r.too_short);
        }
}

int main() {
    std::mt19937 rng(20240923u);
    auto below = [&](int64_t m) { return (int64_t)(rng() % (uint64_t)m); };
    const int win[5][2] = {{512, 256}, {256, 128}, {400, 160}, {512, 128}, {400, 161}};
    for (const auto &ws : win) {
        check_finish(ws[0], ws[1]);
        for (int chained = 0; chained < 2; chained++)
            for (int max_chains : {1, 3, 17}) {
                const int n_streams = 1 + (int)below(12);
                const int64_t max_push = 1 + below(3 * TILE * ws[1]);
                PushGeom g{};
                g.window = ws[0]; g.wshift = ws[1]; g.H = 0; g.wmax = 0;
                g.held = false; g.signal = true;
                g.chained = chained != 0; g.max_chains = max_chains; g.max_wg = 3;
                std::vector<int64_t> consumed((size_t)n_streams, 0);
                std::vector<uint8_t> hsel((size_t)n_streams, 0);
                std::vector<int32_t> order((size_t)n_streams);
                for (int round = 0; round < 24; round++) {
                    for (int i = 0; i < n_streams; i++) order[(size_t)i] = i;
                    std::shuffle(order.begin(), order.end(), rng);
                    const int n = 1 + (int)below(n_streams);
                    std::vector<int32_t> ids(order.begin(), order.begin() + n);
                    std::vector<int64_t> ns((size_t)n), off((size_t)n);
                    int64_t at = 0;
                    for (int i = 0; i < n; i++) {
                        const int64_t c = consumed[(size_t)ids[i]];
                        const int64_t next = (int64_t)g.window + frames_of(c, g.window, g.wshift) * g.wshift;  // samples at the next frame
                        int64_t v = 0;
                        switch (below(7)) {
                            case 0: v = 0; break;
                            case 1: v = 1; break;
                            case 2: v = next - 1 - c; break;                    // just short of a frame
                            case 3: v = next - c; break;                        // exactly one
                            case 4: v = next - c + g.wshift - 1; break;         // still one
                            case 5: v = next - c + (TILE + 3) * g.wshift; break;  // many: past a tile
                            default: v = below(max_push + 1); break;
                        }
                        ns[(size_t)i] = std::max<int64_t>(0, v);
                        off[(size_t)i] = at;
                        at += ns[(size_t)i] + below(3);
                    }
                    check_push(g, consumed, hsel, ids, ns, off);
                    for (int i = 0; i < n; i++) consumed[(size_t)ids[i]] += ns[(size_t)i];
                    if (below(4) == 0) consumed[(size_t)below(n_streams)] = 0;  // a stream finishes now and then
                }
            }
    }
    CHECK(frames_seen[0] > 50 && frames_seen[1] > 50 && frames_seen[2] > 50);
    if (failures) {
        std::printf("stream_signal_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("pushes of a stream by frames completed: none %d, one %d, more %d\n", frames_seen[0], frames_seen[1], frames_seen[2]);
    std::printf("stream_signal_plan_check ok (%d pushes)\n", pushes_checked);
    return 0;
}
