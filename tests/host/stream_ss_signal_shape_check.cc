// Stand-alone check of the stream set that holds subtraction state and signal state together (ctucopy_amd/csrc/stream_set_shape.h with
// CTU_STREAMS_SS_SIGNAL_STATE): no engine library, no GPU, no HIP.  tests/test_stream_ss_signal_shape_cpu.py builds it with opts.cc and
// design.cc under Address+UB sanitizers and runs it: exit status 0, a final "stream_ss_signal_shape_check ok" and a silent stderr are the
// result.  (tests/host/stream_set_shape_check.cc holds every other kind of set.)
//
// The table is the expectation, worked out by hand: such a set is the feature path's *ss set (chains of whole streams, a slot of
// xs_ss_floats(NJ) floats per stream: 2 * 64 * NJ + 136, NJ = 3 on 256 points and 5 on 512) and a signal set (a tail of window - wshift
// doubles per stream, rounded up to even; no rows, no halo) at once.  Engine facts as on a chip of 256 CUs (max_wg 512, 4096 wave chains).
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

enum : uint32_t { ROW = CTU_STREAMS_ROW_STATE, NR = CTU_STREAMS_NR_STATE, VAD = CTU_STREAMS_VAD_STATE, SIG = CTU_STREAMS_SIGNAL_STATE,
                  LARGE = CTU_STREAMS_LARGE_STATE, TRAP = CTU_STREAMS_TRAP_STATE, SS = CTU_STREAMS_SS_STATE, BOTH = CTU_STREAMS_SS_SIGNAL_STATE,
                  ALL3 = SS | SIG | BOTH };

// engine facts of a *ss engine: EngineTables::ss (1 hwss, 2 fwss, 3 2fwss), sel.mode (1: 256 points), chains per wave
static StreamSetFacts facts(int ss, int mode, bool big = false, bool ss_file = false, int chain_slots = 4096) {
    StreamSetFacts f;
    f.ss = ss; f.big = big; f.ss_file = ss_file; f.wave1k = false; f.mode = mode;
    f.per_wave = true; f.chain_slots = chain_slots; f.max_wg = 512;
    return f;
}

struct Row {
    const char *name, *args;
    uint32_t flags;
    StreamSetFacts f;
    int N;
    int64_t M;
    // ---- expected
    const char *refusal;
    int window, wshift, tstride, cstride;
    int64_t xstate;
    int heads;
    int64_t longest, otail;
};

#define S16 "-fs 16000 -format_in raw -format_out raw -w 25 -s 12.5 -vad burg -nr_mode "
#define S8 "-fs 8000 -format_in raw -format_out raw -w 25 -s 12.5 -vad burg -nr_mode "

static const Row rows[] = {
    // name, args, flags, facts, N, M | refusal, window, wshift, tstride, cstride, xstate, heads, longest, otail
    {"fwss, 512 points", S16 "fwss", ALL3, facts(2, 0), 3, 1000, nullptr, 400, 200, 200, 400, 776, 8, 1407, 600},
    {"hwss, 512 points", S16 "hwss", ALL3, facts(1, 0), 3, 1000, nullptr, 400, 200, 200, 400, 776, 8, 1407, 600},
    {"2fwss, 512 points, every flag", S16 "2fwss", ALL3 | ROW | NR | VAD | LARGE | TRAP, facts(3, 0), 3, 1000, nullptr, 400, 200, 200, 400, 776, 8, 1407, 600},
    {"fwss, 256 points", S8 "fwss", ALL3, facts(2, 1), 3, 1000, nullptr, 200, 100, 100, 200, 520, 8, 1207, 300},
    {"hwss, 256 points", S8 "hwss", ALL3, facts(1, 1), 3, 1000, nullptr, 200, 100, 100, 200, 520, 8, 1207, 300},
    {"2fwss, 256 points", S8 "2fwss -nr_p 0.9 -nr_q 0.95", ALL3, facts(3, 1), 3, 1000, nullptr, 200, 100, 100, 200, 520, 8, 1207, 300},
    {"fwss, 512 points, -w 20 -s 10", S16 "fwss -w 20 -s 10", ALL3, facts(2, 0), 3, 1000, nullptr, 320, 160, 160, 320, 776, 8, 1327, 480},
    {"fwss, 512 points, -s 10: tail 240", S16 "fwss -s 10", ALL3, facts(2, 0), 5, 400, nullptr, 400, 160, 240, 400, 776, 8, 807, 1200},
    {"fwss, 256 points, -s 10.125: odd tail 119", S8 "fwss -s 10.125", ALL3, facts(2, 1), 3, 1000, nullptr, 200, 81, 120, 200, 520, 8, 1207, 360},
    {"fwss, 256 points, 20 streams on 4 chain slots", S8 "fwss", ALL3, facts(2, 1, false, false, 4), 20, 1000, nullptr, 200, 100, 100, 200, 520, 8, 1207, 2000},
    {"fwss, 512 points, pushes of one sample", S16 "fwss", ALL3, facts(2, 0), 3, 1, nullptr, 400, 200, 200, 400, 776, 8, 600 /* window + wshift */, 600},
    // an engine and a set that do not fit each other: what streams_unsupported_reason should have refused
    {"speech output without the flag", S16 "fwss", SS | SIG, facts(2, 0), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
    {"speech output with the signal state alone", S16 "fwss", SIG | NR, facts(2, 0), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the flag without the signal state", S8 "hwss", SS | BOTH, facts(1, 1), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the flag without the subtraction state", S8 "hwss", SIG | BOTH, facts(1, 1), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
    {"on large frames", "-fs 44100 -format_in raw -format_out raw -w 24 -s 12.5 -vad burg -nr_mode fwss", ALL3 | LARGE, facts(2, 0, true, false, 2048), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
    {"with -vad file=", "-fs 8000 -format_in raw -format_out raw -w 25 -s 12.5 -vad file=x -nr_mode fwss", ALL3, facts(2, 1, false, true), 3, 1000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0},
};

static ctu::Design design_of(const char *args) {
    std::vector<std::string> a;
    std::istringstream ss(args);
    for (std::string t; ss >> t;) a.push_back(t);
    return ctu::Design(ctu::Opts::from_args(a));
}

// frames, counted one by one
static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((window - wshift) + (F + 1) * wshift <= total) F++;
    return F;
}

static int steps_checked = 0;
static void check_row(const Row &r) {
    const ctu::Design d = design_of(r.args);
    const StreamSetShape s = stream_set_shape(d, r.flags, r.f, r.N, r.M);
    const int before = failures;
    if (r.refusal) {
        CHECK(s.refusal && std::strcmp(s.refusal, r.refusal) == 0);
    } else {
        CHECK(s.refusal == nullptr);
        CHECK(s.ss && s.signal && s.chained && !s.vad && !s.trap && !s.ola_big);
        CHECK(s.g.signal && s.g.chained && !s.g.vad && !s.g.held);
        CHECK(s.g.window == r.window && s.g.wshift == r.wshift && s.g.H == 0 && s.g.wmax == 0);
        CHECK(s.g.max_wg == 512 && s.g.max_chains == r.f.chain_slots);
        CHECK(s.n_streams == r.N && s.C == 0);
        CHECK(s.tstride == r.tstride && s.tstride % 2 == 0 && s.tstride >= r.window - r.wshift);
        CHECK(s.cstride == r.cstride);
        CHECK(s.xstate_floats == r.xstate && s.xstate_floats == xs_ss_floats(r.f.mode == 1 ? 3 : 5));
        CHECK(s.n_heads == r.heads);
        CHECK(s.longest == r.longest);
        CHECK(s.otail_n() == r.otail && s.otail_n() == (int64_t)r.N * r.tstride);
        CHECK(s.vsink_n(40) == 0 && s.vbase_n(40) == 0 && s.hist_n() == 0 && s.means_n() == 0 && s.cols_n(40) == 0);
        int H = -1, wmax = -1;
        stream_set_halo(d, r.flags, &H, &wmax);
        CHECK(H == 0 && wmax == 0);
        // what a stream has delivered: samples, wshift per frame, and the tail a finish adds once there is a frame
        for (int64_t total = 0; total <= 3 * r.window; total++) {
            const int64_t F = frames_of(total, r.window, r.wshift);
            int64_t pending = -1, want = -1;
            CHECK(s.delivered(total, &pending) == F * r.wshift && pending == (F > 0 ? r.window - r.wshift : 0));
            CHECK(s.delivered(total) == stream_signal_step(r.window, r.wshift, total, &want) && want == pending);
            steps_checked++;
        }
    }
    std::printf("%-50s %s\n", r.name, failures == before ? "ok" : "FAILED");
}

int main() {
    CHECK(BOTH == 2048 && xs_ss_floats(3) == 520 && xs_ss_floats(5) == 776);
    for (const Row &r : rows) check_row(r);
    if (failures) {
        std::printf("stream_ss_signal_shape_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_ss_signal_shape_check ok: %d shape rows, %d totals stepped\n", (int)(sizeof rows / sizeof rows[0]), steps_checked);
    return 0;
}
