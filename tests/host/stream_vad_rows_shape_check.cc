// Stand-alone check of the stream set that holds detector state behind row state (ctucopy_amd/csrc/stream_set_shape.h and stream_plan.h
// with CTU_STREAMS_VAD_ROW_STATE beside CTU_STREAMS_ROW_STATE and CTU_STREAMS_VAD_STATE): no engine library, no GPU, no HIP.
// tests/test_streams_vad_rows_cpu.py builds it with opts.cc and design.cc, once plainly and once under Address + UB sanitizers, and runs
// it: exit status 0, a final "stream_vad_rows_shape_check ok" and a silent stderr are the result.
//
// The table below is the expectation, every figure worked out by hand for sets of N = 3 streams and pushes of up to 1000 samples over a
// plan of 40 frames at 8 kHz (window 200, shift 80, base rows of 13 floats):
//   halo      delay + h: the sum of the chain's windows (or the stacking window; 0 with CMS alone) and h = (vad_filter_order - 1) / 2
//   g.H, vh   the two parts, kept apart: the plan counts calls by H and wmax, rows h behind them
//   C         history rows: what the row state keeps, max(2 H, H + L - 1), and h more - the rows held back are rebuilt from base rows
//   crec      doubles of the criterion record: 1 (energy) or -vad_lpc_coefs (Burg cepstra)
//   vsink     decisions of a push nobody asked for: the plan's frames and max(halo, wmax + 1) per stream
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "stream_set_shape.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 40) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static const char *CHAINS = "internal: a streamed configuration with chains of whole utterances";

enum : uint32_t { ROW = CTU_STREAMS_ROW_STATE, NR = CTU_STREAMS_NR_STATE, VAD = CTU_STREAMS_VAD_STATE, VROW = CTU_STREAMS_VAD_ROW_STATE, ALL = ROW | VAD | VROW };

static StreamSetFacts facts(bool big = false, bool per_wave = false) {
    StreamSetFacts f;
    f.ss = 0; f.big = big; f.ss_file = false; f.wave1k = false; f.mode = 1;
    f.per_wave = per_wave; f.chain_slots = 4096; f.max_wg = 512;
    return f;
}

struct Row {
    const char *name, *args;
    uint32_t flags;
    StreamSetFacts f;
    // ---- expected
    const char *refusal;
    bool vad, vad_rows, held, chained;
    int halo, H, wmax, vh, C, crec;
    int64_t crec_n, hist, vsink, vbase, means, xstate;
};

#define F8 "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97"
#define EN " -vad_out_mode vad -vad_cri_mode energy -vad_filter_order "
#define BG " -vad burg -vad_out_mode vad -vad_cri_mode cepdist -vad_cepdist_mode lpc -vad_filter_order "

static const Row rows[] = {
    // name, args, flags, facts | refusal, vad, vad_rows, held, chained, halo, H, wmax, vh, C, crec, crec_n, hist, vsink, vbase, means, xstate
    {"energy, order 3, d_a", F8 EN "3 -fea_delta d_a", ALL, facts(),
     nullptr, true, true, true, false, 5, 4, 2, 1, 9, 1, 3, 702, 55, 0, 96, 0},
    {"Burg (14), order 7, d_a_t", F8 BG "7 -fea_delta d_a_t", ALL, facts(),
     nullptr, true, true, true, false, 9, 6, 2, 3, 15, 14, 42, 1170, 67, 0, 96, 0},
    {"Burg (32), order 3, d_a", F8 BG "3 -vad_lpc_coefs 32 -fea_delta d_a", ALL, facts(),
     nullptr, true, true, true, false, 5, 4, 2, 1, 9, 32, 96, 702, 55, 0, 96, 0},
    {"energy, order 3, -fea_trap 9", F8 EN "3 -fea_trap 9", ALL, facts(),
     nullptr, true, true, true, false, 5, 4, 4, 1, 9, 1, 3, 702, 55, 0, 96, 0},
    {"energy, order 3, -fea_Z_exp", F8 EN "3 -fea_Z_exp 500", ALL, facts(),
     nullptr, true, true, true, false, 1, 0, 0, 1, 1, 1, 3, 78, 43, 0, 96, 0},
    {"energy, order 1, -fea_Z_exp", F8 EN "1 -fea_Z_exp 500", ALL, facts(),
     nullptr, true, true, true, false, 0, 0, 0, 0, 0, 1, 3, 1, 43, 0, 96, 0},
    {"energy, order 5, -fea_Z_block (length_b 48)", F8 EN "5 -fea_Z_block 500", ALL, facts(),
     nullptr, true, true, true, false, 2, 0, 0, 2, 49, 1, 3, 3822, 46, 0, 96, 0},
    {"energy, order 3, d_a with -fea_Z_block", F8 EN "3 -fea_delta d_a -fea_Z_block 500", ALL, facts(),
     nullptr, true, true, true, false, 5, 4, 2, 1, 52, 1, 3, 4056, 55, 0, 96, 0},
    {"C4 with -fea_Z_exp, the noise state beside the three", F8 " -nr_mode exten -nr_a 2" BG "3 -vad_thr_mode adapt -fea_Z_exp 500", ALL | NR, facts(false, true),
     nullptr, true, true, true, true, 1, 0, 0, 1, 1, 14, 42, 78, 43, 0, 96, 384},
    // the three flags beside a configuration that has only one of the two: the set it always was
    {"d_a without the VAD module", F8 " -fea_delta d_a", ALL, facts(),
     nullptr, false, false, true, false, 4, 4, 2, 0, 8, 0, 0, 624, 0, 0, 96, 0},
    {"the VAD module (order 3) without a chain", F8 EN "3", ALL, facts(),
     nullptr, true, false, true, false, 1, 1, 0, 0, 1, 0, 0, 78, 43, 520, 96, 0},
    // an engine and a set that do not fit each other: what streams_unsupported_reason / streams_flags_unknown should have refused
    {"the VAD module behind d_a on large frames", "-fs 16000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -w 100" EN "3 -fea_delta d_a", ALL, facts(true),
     CHAINS, false, false, false, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the new flag without the detector state", F8 EN "3 -fea_delta d_a", ROW | VROW, facts(),
     CHAINS, false, false, false, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
};

static ctu::Design design_of(const char *args) {
    std::vector<std::string> a;
    std::istringstream ss(args);
    for (std::string t; ss >> t;) a.push_back(t);
    return ctu::Design(ctu::Opts::from_args(a));
}

static void check_row(const Row &r) {
    const ctu::Design d = design_of(r.args);
    const StreamSetShape s = stream_set_shape(d, r.flags, r.f, 3, 1000);
    const int before = failures;
    if (r.refusal) {
        CHECK(s.refusal && std::strcmp(s.refusal, r.refusal) == 0);
    } else {
        CHECK(s.refusal == nullptr);
        CHECK(s.vad == r.vad && s.vad_rows == r.vad_rows && s.g.held == r.held && s.chained == r.chained && s.g.vad == r.vad);
        CHECK(!s.trap && !s.signal && !s.ss);
        CHECK(s.g.window == 200 && s.g.wshift == 80 && s.D == d.D && s.hw == 13);
        CHECK(s.g.H == r.H && s.g.wmax == r.wmax && s.g.vh == r.vh);
        CHECK(s.C == r.C);
        CHECK(s.crec == r.crec && s.crec_n() == r.crec_n);
        CHECK(s.hist_n() == r.hist);
        CHECK(s.vsink_n(40) == r.vsink);
        CHECK(s.vbase_n(40) == r.vbase);
        CHECK(s.means_n() == r.means);
        CHECK(s.xstate_floats == r.xstate);
        CHECK(s.longest == 1207);
        // the halo of ctu_streams_config_check_ex, which has no engine: the two halos added up, and the filter's part on request
        int H = -1, wmax = -1, vh = -1;
        stream_set_halo(d, r.flags, &H, &wmax);
        CHECK(H == r.halo && wmax == r.wmax);
        stream_set_halo(d, r.flags, &H, &wmax, &vh);
        CHECK(H == r.halo && wmax == r.wmax && vh == r.vh && H - vh == r.H);
    }
    std::printf("%-56s %s\n", r.name, failures == before ? "ok" : "FAILED");
}

// frames, calls and rows, counted one by one
static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((window - wshift) + (F + 1) * wshift <= total) F++;
    return F;
}
static int64_t calls_of(int H, int wmax, int64_t F) {
    int64_t C = 0;
    for (int64_t f = 1; f <= F; f++) C = H == 0 ? f : (f >= wmax + 2 && f > H ? f - H : C);
    return C;
}

static int steps_checked = 0;
static void check_delivered() {
    // energy, order 3, d_a along a file, by hand: frames -> (calls, rows)
    const int hand[][3] = {{0, 0, 0}, {3, 0, 0}, {4, 0, 0}, {5, 1, 0}, {6, 2, 1}, {10, 6, 5}, {40, 36, 35}};
    for (const auto &q : hand) {
        CHECK(stream_rows_out(4, 2, q[0]) == q[1]);
        CHECK(stream_vad_rows_out(4, 2, 1, q[0]) == q[2]);
    }
    // -fea_trap 9 at order 3: no call before frame wmax + 2 = 6 exists, then two at once
    CHECK(stream_rows_out(4, 4, 5) == 0 && stream_rows_out(4, 4, 6) == 2 && stream_vad_rows_out(4, 4, 1, 6) == 1);
    const int shapes[][5] = {{200, 80, 4, 2, 1}, {200, 80, 6, 2, 3}, {200, 80, 4, 4, 1}, {200, 80, 0, 0, 1}, {200, 80, 0, 0, 0}, {400, 160, 4, 2, 0},
                             {400, 160, 2, 2, 15}, {33, 1, 4, 2, 2}};
    for (const auto &q : shapes) {
        const int window = q[0], wshift = q[1], H = q[2], wmax = q[3], h = q[4];
        StreamSetShape s;
        s.g.window = window; s.g.wshift = wshift; s.g.H = H; s.g.wmax = wmax; s.g.vh = h;
        for (int64_t total = 0; total <= window + 30 * wshift; total += (wshift > 7 ? 7 : 1)) {
            const int64_t F = frames_of(total, window, wshift), C = calls_of(H, wmax, F), R = C > h ? C - h : 0;
            int64_t pending = -1;
            CHECK(stream_vad_rows_step(window, wshift, h, H, wmax, total, &pending) == R && pending == F - R);
            CHECK(stream_vad_rows_step(window, wshift, h, H, wmax, total, nullptr) == R);
            pending = -1;
            CHECK(s.delivered(total, &pending) == R && pending == F - R);
            if (h == 0) CHECK(stream_rows_step(window, wshift, H, wmax, total, nullptr) == R);
            steps_checked++;
        }
    }
}

// the push plan and the finish plan of such a set, by hand
static void check_plans() {
    PushGeom g{};
    g.window = 200; g.wshift = 80; g.H = 4; g.wmax = 4; g.vh = 1;  // energy, order 3, -fea_trap 9
    g.held = true; g.vad = true; g.chained = false;
    g.max_chains = 4096; g.max_wg = 512; g.arena_samples = 1 << 20; g.tile_cap = 1 << 10;
    const int N = 2;
    std::vector<StreamPush> push(N);
    std::vector<RowPush> rp(N);
    std::vector<VadCalls> calls(N);
    std::vector<int> replay(N);
    std::vector<int64_t> counts(N), next(N), consumed(N, 0);
    std::vector<uint8_t> hsel(N, 0), nh(N);
    auto plan = [&](int64_t n0, int64_t n1) {
        PushLayout L;
        L.push = push.data(); L.rows = rp.data(); L.calls = calls.data(); L.replay = replay.data();
        L.row_counts = counts.data(); L.consumed = next.data(); L.hsel = nh.data();
        const int32_t ids[2] = {0, 1};
        const int64_t ns[2] = {n0, n1}, off[2] = {0, n0};
        CHECK(stream_plan_push(g, consumed.data(), hsel.data(), N, ids, ns, off, L));
        for (int i = 0; i < N; i++) {
            consumed[i] = next[i];
            hsel[i] = nh[i];
        }
        return L;
    };
    // stream 0: five frames, then one - call 0 reads frame 4, the one ahead of the second push; stream 1: six frames at once
    PushLayout L = plan(200 + 4 * 80, 200 + 5 * 80);
    CHECK(L.n_replay == 2 && L.base_rows == 11 && L.rows_out == 1 && L.most == 1);
    CHECK(rp[0].F0 == 0 && rp[0].Tn == 5 && rp[0].r0 == 0 && rp[0].nr == 0 && calls[0].c0 == 0 && calls[0].nc == 0);
    CHECK(rp[1].F0 == 0 && rp[1].Tn == 6 && rp[1].r0 == 0 && rp[1].nr == 1 && rp[1].out0 == 0 && calls[1].c0 == 0 && calls[1].nc == 2);
    L = plan(80, 80);
    CHECK(L.n_replay == 2 && L.base_rows == 2 && L.rows_out == 2);
    CHECK(rp[0].F0 == 5 && rp[0].Tn == 1 && rp[0].r0 == 0 && rp[0].nr == 1 && calls[0].c0 == 0 && calls[0].nc == 2);
    CHECK(calls[0].c0 + g.H - rp[0].F0 == -1);  // the first call's frame, counted from the push's first
    CHECK(rp[1].F0 == 6 && rp[1].Tn == 1 && rp[1].r0 == 1 && rp[1].nr == 1 && rp[1].out0 == 1 && calls[1].c0 == 2 && calls[1].nc == 1);
    CHECK(calls[1].c0 + g.H - rp[1].F0 == 0);
    L = plan(0, 79);  // no frame: no calls, no rows, not replayed
    CHECK(L.n_replay == 0 && L.rows_out == 0 && calls[0].nc == 0 && calls[1].nc == 0 && calls[0].c0 == 2 && calls[1].c0 == 3);

    // finish: (H, wmax, h, frames) -> too_short, pending, the calls still owed
    struct Fin { int H, wmax, h; int64_t T; bool too_short; int64_t pending, c0; int nc; };
    const Fin fins[] = {
        {4, 2, 1, 0, false, 0, 0, 0},   {4, 2, 1, 3, true, 0, 0, 0},    {4, 2, 1, 4, false, 4, 0, 4},   {4, 2, 1, 5, false, 5, 1, 4},
        {4, 2, 1, 6, false, 5, 2, 4},   {4, 2, 1, 96, false, 5, 92, 4}, {6, 2, 3, 3, true, 0, 0, 0},    {6, 2, 3, 4, false, 4, 0, 4},
        {6, 2, 3, 9, false, 9, 3, 6},   {6, 2, 3, 10, false, 9, 4, 6},  {0, 0, 3, 3, false, 0, 3, 0},   {0, 0, 3, 4, false, 3, 4, 0},
        {4, 4, 1, 5, true, 0, 0, 0},    {4, 4, 1, 6, false, 5, 2, 4},   {2, 2, 15, 15, false, 0, 13, 0}, {2, 2, 15, 16, false, 16, 14, 2},
    };
    for (const Fin &q : fins) {
        const FinishLayout f = stream_plan_finish(200, 80, q.H, q.wmax, q.T ? 200 + (q.T - 1) * 80 + 5 : 0, 1, 1, false, false, q.h);
        CHECK(f.frames == q.T && f.too_short == q.too_short && f.pending == q.pending);
        CHECK(f.calls.c0 == q.c0 && f.calls.nc == q.nc);
        CHECK(f.row.F0 == q.T && f.row.Tn == 0 && f.row.nr == q.pending && f.row.id == 1 && f.row.hsel == 1);
        CHECK(q.pending == 0 || f.row.r0 == q.T - q.pending);
        // with h = 0 the plan is the row state's
        const FinishLayout a = stream_plan_finish(200, 80, q.H, q.wmax, q.T ? 200 + (q.T - 1) * 80 + 5 : 0, 1, 1), b = stream_plan_finish(200, 80, q.H, q.wmax, q.T ? 200 + (q.T - 1) * 80 + 5 : 0, 1, 1, false, false, 0);
        CHECK(a.pending == b.pending && a.too_short == b.too_short && a.row.r0 == b.row.r0 && a.row.nr == b.row.nr);
    }
}

int main() {
    for (const Row &r : rows) check_row(r);
    check_delivered();
    check_plans();
    if (failures) {
        std::printf("stream_vad_rows_shape_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_vad_rows_shape_check ok: %d shape rows, %d totals stepped\n", (int)(sizeof rows / sizeof rows[0]), steps_checked);
    return 0;
}
