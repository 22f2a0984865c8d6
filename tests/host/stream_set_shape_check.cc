// Stand-alone check of what a stream set is (ctucopy_amd/csrc/stream_set_shape.h): no engine library, no GPU, no HIP.
// tests/test_stream_set_shape_cpu.py builds it with opts.cc and design.cc under Address+UB sanitizers and runs it: exit status 0, a final
// "stream_set_shape_check ok" and a silent stderr are the result.
//
// The table below is the expectation.  Every figure in it was worked out by hand from ctu_streams_create_ex as it stood before the shape
// had a unit of its own (the kinds of state, the halo of stream_halo / stream_vad_halo / stream_trap_halo, held, C, hw, tstride, the
// per-stream size of xstate by the kernel that runs, the chain heads, the allocation sizes, the longest slot), for sets of N streams
// and pushes of up to M samples over a plan of `tf` frames.  The engine facts of a row are what build_engine_tables / plan_geom give
// for its command line on a chip of 256 CUs with two front-end workgroups per CU (max_wg 512; 512 * 8 wave chains, 256 * 8 workgroup
// chains of bigfft_kernel).
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
static const char *BEYOND = "internal: a signal set beyond the 512-point front end";

enum : uint32_t { ROW = CTU_STREAMS_ROW_STATE, NR = CTU_STREAMS_NR_STATE, VAD = CTU_STREAMS_VAD_STATE, SIG = CTU_STREAMS_SIGNAL_STATE,
                  LARGE = CTU_STREAMS_LARGE_STATE, TRAP = CTU_STREAMS_TRAP_STATE, SS = CTU_STREAMS_SS_STATE };

// engine facts: {ss, big, ss_file, wave1k, mode, per_wave, chain_slots, max_wg}
static StreamSetFacts facts(int ss, bool big, bool wave1k, int mode, bool per_wave, int chain_slots = 4096, bool ss_file = false) {
    StreamSetFacts f;
    f.ss = ss; f.big = big; f.ss_file = ss_file; f.wave1k = wave1k; f.mode = mode;
    f.per_wave = per_wave; f.chain_slots = chain_slots; f.max_wg = 512;
    return f;
}

struct Row {
    const char *name, *args;
    uint32_t flags;
    StreamSetFacts f;
    int N;
    int64_t M, tf;
    // ---- expected
    const char *refusal;
    int kinds;  // bits: 1 vad, 2 trap, 4 signal, 8 ola_big, 16 chained, 32 ss
    int window, wshift, H, wmax;
    bool held;
    int C, hw, tstride, cstride;
    int64_t xstate;
    int heads;
    int64_t longest, vsink, vbase, hist, means, otail, cols;
};

#define F8 "-fs 8000 -format_in raw -format_out htk -preset mfcc -preem 0.97"
#define F16 "-fs 16000 -format_in raw -format_out htk -preset mfcc -preem 0.97"
#define S16 "-fs 16000 -format_in raw -format_out raw -preset mfcc"
#define VADOUT " -vad_out_mode bin -vad_filter_order "

static const Row rows[] = {
    // name, args, flags, facts, N, M, tf | refusal, kinds, window, wshift, H, wmax, held, C, hw, tstride, cstride, xstate, heads, longest, vsink, vbase, hist, means, otail, cols
    {"plain C2", F8, 0, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 0, 0, false, 0, 13, 0, 200, 0, 8, 1207, 0, 0, 0, 0, 0, 0},
    {"plain C2, 20 streams", F8, 0, facts(0, false, false, 1, false), 20, 1000, 40,
     nullptr, 0, 200, 80, 0, 0, false, 0, 13, 0, 200, 0, 24, 1207, 0, 0, 0, 0, 0, 0},
    {"plain C2, 20 streams on 4 chain slots", F8, 0, facts(0, false, false, 1, false, 4), 20, 1000, 40,
     nullptr, 0, 200, 80, 0, 0, false, 0, 13, 0, 200, 0, 8, 1207, 0, 0, 0, 0, 0, 0},
    {"plain 16 kHz, pushes of one sample", F16, 0, facts(0, false, false, 0, false), 3, 1, 3,
     nullptr, 0, 400, 160, 0, 0, false, 0, 13, 0, 400, 0, 8, 560, 0, 0, 0, 0, 0, 0},
    {"d_a delta chain", F8 " -fea_delta d_a", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 4, 2, true, 8, 13, 0, 200, 0, 8, 1207, 0, 0, 624, 96, 0, 0},
    {"d_a delta chain, short pushes", F8 " -fea_delta d_a", ROW, facts(0, false, false, 1, false), 3, 100, 6,
     nullptr, 0, 200, 80, 4, 2, true, 8, 13, 0, 200, 0, 8, 440, 0, 0, 624, 96, 0, 0},
    {"-fea_trap 7 stacking", F8 " -fea_trap 7", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 3, 3, true, 6, 13, 0, 200, 0, 8, 1207, 0, 0, 468, 96, 0, 0},
    {"-fea_Z_exp", F8 " -fea_Z_exp 500", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 0, 0, true, 0, 13, 0, 200, 0, 8, 1207, 0, 0, 1, 96, 0, 0},
    {"-fea_Z_block (length_b 48)", F8 " -fea_Z_block 500", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 0, 0, true, 47, 13, 0, 200, 0, 8, 1207, 0, 0, 3666, 96, 0, 0},
    {"d_a with -fea_Z_block", F8 " -fea_delta d_a -fea_Z_block 500", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 0, 200, 80, 4, 2, true, 51, 13, 0, 200, 0, 8, 1207, 0, 0, 3978, 96, 0, 0},
    {"VAD, filter order 1", F8 VADOUT "1", VAD, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 1, 200, 80, 0, 0, false, 0, 13, 0, 200, 0, 8, 1207, 40, 0, 0, 0, 0, 0},
    {"VAD, filter order 1, empty plan", F8 VADOUT "1", VAD, facts(0, false, false, 1, false), 3, 1000, 0,
     nullptr, 1, 200, 80, 0, 0, false, 0, 13, 0, 200, 0, 8, 1207, 1, 0, 0, 0, 0, 0},
    {"VAD, filter order 3", F8 VADOUT "3", VAD, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 1, 200, 80, 1, 0, true, 1, 13, 0, 200, 0, 8, 1207, 43, 520, 78, 96, 0, 0},
    {"VAD, filter order 3, empty plan", F8 VADOUT "3", VAD, facts(0, false, false, 1, false), 3, 1000, 0,
     nullptr, 1, 200, 80, 1, 0, true, 1, 13, 0, 200, 0, 8, 1207, 3, 13, 78, 96, 0, 0},
    {"VAD, filter order 31", F8 VADOUT "31", VAD, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 1, 200, 80, 15, 14, true, 15, 13, 0, 200, 0, 8, 1400, 85, 520, 1170, 96, 0, 0},
    {"trapdct, traplen 3", F8 " -fea_kind trapdct,3,2", TRAP, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 2, 200, 80, 1, 0, true, 2, 26, 0, 200, 0, 8, 1207, 0, 0, 312, 96, 0, 40},
    {"trapdct, traplen 3, empty plan", F8 " -fea_kind trapdct,3,2", TRAP, facts(0, false, false, 1, false), 3, 1000, 0,
     nullptr, 2, 200, 80, 1, 0, true, 2, 26, 0, 200, 0, 8, 1207, 0, 0, 312, 96, 0, 1},
    {"trapdct, traplen 101", F8 " -fea_kind trapdct,101,16", TRAP, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 2, 200, 80, 50, 49, true, 100, 26, 0, 200, 0, 8, 4200, 0, 0, 15600, 96, 0, 50},
    {"trapdct, traplen 255", F8 " -fea_kind trapdct,255,16", TRAP, facts(0, false, false, 1, false), 3, 1000, 40,
     nullptr, 2, 200, 80, 127, 126, true, 254, 26, 0, 200, 0, 8, 10360, 0, 0, 39624, 96, 0, 127},
    {"exten, 256 points", F8 " -nr_mode exten", NR, facts(0, false, false, 1, true), 3, 1000, 40,
     nullptr, 16, 200, 80, 0, 0, false, 0, 13, 0, 200, 384, 8, 1207, 0, 0, 0, 0, 0, 0},
    {"exten, 512 points", F16 " -nr_mode exten", NR, facts(0, false, false, 0, true), 3, 1000, 40,
     nullptr, 16, 400, 160, 0, 0, false, 0, 13, 0, 400, 640, 8, 1407, 0, 0, 0, 0, 0, 0},
    {"exten on wave1k", F16 " -nr_mode exten -w 50", NR | LARGE, facts(0, true, true, 0, true), 3, 1000, 40,
     nullptr, 16, 800, 160, 0, 0, false, 0, 13, 0, 800, 1152, 8, 1807, 0, 0, 0, 0, 0, 0},
    {"exten on bigfft, 1024 points", F16 " -nr_mode exten -w 50", NR | LARGE, facts(0, true, false, 0, true, 2048), 3, 1000, 40,
     nullptr, 16, 800, 160, 0, 0, false, 0, 13, 0, 800, 1536, 8, 1807, 0, 0, 0, 0, 0, 0},
    {"exten on bigfft, 2048 points", F16 " -nr_mode exten -w 100", NR | LARGE, facts(0, true, false, 0, true, 2048), 3, 1000, 40,
     nullptr, 16, 1600, 160, 0, 0, false, 0, 13, 0, 1600, 2560, 8, 2607, 0, 0, 0, 0, 0, 0},
    {"exten on bigfft, 4096 points", F16 " -nr_mode exten -w 200", NR | LARGE, facts(0, true, false, 0, true, 2048), 3, 1000, 40,
     nullptr, 16, 3200, 160, 0, 0, false, 0, 13, 0, 3200, 4608, 8, 4207, 0, 0, 0, 0, 0, 0},
    {"exten with d_a and trap flags unused", F8 " -nr_mode exten -fea_delta d_a", NR | ROW | TRAP | VAD, facts(0, false, false, 1, true), 3, 1000, 40,
     nullptr, 16, 200, 80, 4, 2, true, 8, 13, 0, 200, 384, 8, 1207, 0, 0, 624, 96, 0, 0},
    {"hwss, 256 points", F8 " -nr_mode hwss -vad burg", SS, facts(1, false, false, 1, true), 3, 1000, 40,
     nullptr, 48, 200, 80, 0, 0, false, 0, 13, 0, 200, 520, 8, 1207, 0, 0, 0, 0, 0, 0},
    {"fwss, 512 points", F16 " -nr_mode fwss -vad burg", SS, facts(2, false, false, 0, true), 3, 1000, 40,
     nullptr, 48, 400, 160, 0, 0, false, 0, 13, 0, 400, 776, 8, 1407, 0, 0, 0, 0, 0, 0},
    {"2fwss, 256 points", F8 " -nr_mode 2fwss -vad burg", SS, facts(3, false, false, 1, true), 3, 1000, 40,
     nullptr, 48, 200, 80, 0, 0, false, 0, 13, 0, 200, 520, 8, 1207, 0, 0, 0, 0, 0, 0},
    {"2fwss, 512 points, with d_a", F16 " -nr_mode 2fwss -vad burg -fea_delta d_a", SS | ROW, facts(3, false, false, 0, true), 3, 1000, 40,
     nullptr, 48, 400, 160, 4, 2, true, 8, 13, 0, 400, 776, 8, 1407, 0, 0, 624, 96, 0, 0},
    {"speech, tail 240", S16, SIG, facts(0, false, false, 0, false), 3, 1000, 40,
     nullptr, 4, 400, 160, 0, 0, false, 0, 0, 240, 400, 0, 8, 1407, 0, 0, 0, 0, 720, 0},
    {"speech, odd tail 239", S16 " -s 10.0625", SIG, facts(0, false, false, 0, false), 3, 1000, 40,
     nullptr, 4, 400, 161, 0, 0, false, 0, 0, 240, 400, 0, 8, 1407, 0, 0, 0, 0, 720, 0},
    {"speech, no tail (-s = -w)", S16 " -s 25", SIG, facts(0, false, false, 0, false), 3, 1000, 40,
     nullptr, 4, 400, 400, 0, 0, false, 0, 0, 2, 400, 0, 8, 1407, 0, 0, 0, 0, 6, 0},
    {"speech behind exten (preset exten)", "-fs 16000 -format_in raw -format_out raw -preset exten", SIG | NR, facts(0, false, false, 0, true), 3, 1000, 40,
     nullptr, 20, 512, 256, 0, 0, false, 0, 0, 256, 512, 640, 8, 1519, 0, 0, 0, 0, 768, 0},
    {"speech, tail at OLA_TAIL_MAX", S16 " -w 64 -s 32", SIG | LARGE, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     nullptr, 4, 1024, 512, 0, 0, false, 0, 0, 512, 1024, 0, 8, 2031, 0, 0, 0, 0, 1536, 0},
    {"speech, tail at OLA_TAIL_MAX, no large flag", S16 " -w 64 -s 32", SIG, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     BEYOND, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"speech, tail OLA_TAIL_MAX + 1", S16 " -w 64 -s 31.9375", SIG | LARGE, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     nullptr, 12, 1024, 511, 0, 0, false, 0, 0, 514, 1024, 0, 8, 2031, 0, 0, 0, 0, 1542, 0},
    {"speech, tail 768", S16 " -w 64 -s 16", SIG | LARGE, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     nullptr, 12, 1024, 256, 0, 0, false, 0, 0, 768, 1024, 0, 8, 2031, 0, 0, 0, 0, 2304, 0},
    {"speech, tail 768, no large flag", S16 " -w 64 -s 16", SIG, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     BEYOND, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"speech, tail at OLA_BIG_TAIL_MAX", S16 " -w 512.125 -s 256.125", SIG | LARGE, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     nullptr, 12, 8194, 4098, 0, 0, false, 0, 0, 4096, 8200, 0, 8, 12292 /* window + wshift: more than lead, carry and push */, 0, 0, 0, 0, 12288, 0},
    {"speech, tail OLA_BIG_TAIL_MAX + 1", S16 " -w 512.125 -s 256.0625", SIG | LARGE, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     BEYOND, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    // an engine and a set that do not fit each other: what streams_unsupported_reason should have refused
    {"chains of exten without noise state", F8 " -nr_mode exten", ROW, facts(0, false, false, 1, true), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"chains of exten with subtraction state only", F8 " -nr_mode exten", SS, facts(0, false, false, 1, true), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the VAD module without detector state", F8 VADOUT "3", ROW, facts(0, false, false, 1, false), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"hwss without subtraction state", F8 " -nr_mode hwss -vad burg", NR, facts(1, false, false, 1, true), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"hwss on large frames", F16 " -nr_mode hwss -vad burg -w 100", SS, facts(1, true, false, 0, true, 2048), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"hwss with -vad file=", F8 " -nr_mode hwss -vad file=x", SS, facts(1, false, false, 1, true, 4096, true), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"exten on large frames without the large flag", F16 " -nr_mode exten -w 100", NR, facts(0, true, false, 0, true, 2048), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the VAD module on large frames", F16 VADOUT "3 -w 100", VAD, facts(0, true, false, 0, false, 2048), 3, 1000, 40,
     CHAINS, 0, 0, 0, 0, 0, false, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
};

static ctu::Design design_of(const char *args) {
    std::vector<std::string> a;
    std::istringstream ss(args);
    for (std::string t; ss >> t;) a.push_back(t);
    return ctu::Design(ctu::Opts::from_args(a));
}

static void check_row(const Row &r) {
    const ctu::Design d = design_of(r.args);
    const StreamSetShape s = stream_set_shape(d, r.flags, r.f, r.N, r.M);
    const int before = failures;
    if (r.refusal) {
        CHECK(s.refusal && std::strcmp(s.refusal, r.refusal) == 0);
    } else {
        CHECK(s.refusal == nullptr);
        const int kinds = (s.vad ? 1 : 0) | (s.trap ? 2 : 0) | (s.signal ? 4 : 0) | (s.ola_big ? 8 : 0) | (s.chained ? 16 : 0) | (s.ss ? 32 : 0);
        CHECK(kinds == r.kinds);
        CHECK(s.g.vad == s.vad && s.g.signal == s.signal && s.g.chained == s.chained);
        CHECK(s.g.window == r.window && s.g.wshift == r.wshift && s.g.H == r.H && s.g.wmax == r.wmax && s.g.held == r.held);
        CHECK(s.g.max_wg == r.f.max_wg && s.g.max_chains == r.f.chain_slots);
        CHECK(s.n_streams == r.N);
        CHECK(s.C == r.C);
        CHECK(s.hw == r.hw);
        CHECK(s.tstride == r.tstride);
        CHECK(s.cstride == r.cstride);
        CHECK(s.xstate_floats == r.xstate);
        CHECK(s.n_heads == r.heads);
        CHECK(s.longest == r.longest);
        CHECK(s.vsink_n(r.tf) == r.vsink);
        CHECK(s.vbase_n(r.tf) == r.vbase);
        CHECK(s.hist_n() == r.hist);
        CHECK(s.means_n() == r.means);
        CHECK(s.otail_n() == r.otail);
        CHECK(s.cols_n(r.tf) == r.cols);
        // the halo of ctu_streams_config_check_ex, which has no engine, is the set's
        int H = -1, wmax = -1;
        stream_set_halo(d, r.flags, &H, &wmax);
        CHECK(H == r.H && wmax == r.wmax);
    }
    std::printf("%-50s %s\n", r.name, failures == before ? "ok" : "FAILED");
}

// frames and rows, counted one by one
static int64_t frames_of(int64_t total, int window, int wshift) {
    int64_t F = 0;
    while ((window - wshift) + (F + 1) * wshift <= total) F++;
    return F;
}
static int64_t rows_of(int H, int wmax, int64_t F) {
    int64_t R = 0;
    for (int64_t f = 1; f <= F; f++)  // with frame f the file has f frames: without a halo its row goes out; with one, every row up to f - H once frame wmax + 2 exists
        R = H == 0 ? f : (f >= wmax + 2 && f > H ? f - H : R);
    return R;
}

static int steps_checked = 0;
static void check_steps() {
    const int shapes[][4] = {{200, 80, 0, 0}, {200, 80, 4, 2}, {200, 80, 3, 3}, {200, 80, 1, 0}, {200, 80, 15, 14}, {400, 160, 50, 49}, {64, 64, 2, 2},
                             {33, 1, 4, 2}, {512, 256, 0, 0}, {25, 7, 1, 0}};
    for (const auto &q : shapes) {
        const int window = q[0], wshift = q[1], H = q[2], wmax = q[3];
        for (int64_t total = 0; total <= 3 * window; total++) {
            const int64_t F = frames_of(total, window, wshift), R = rows_of(H, wmax, F);
            CHECK(stream_step_args_ok(window, wshift, total));
            CHECK(stream_frames(total, window, wshift) == F && stream_rows_out(H, wmax, F) == R);
            int64_t pending = -1;
            CHECK(stream_rows_step(window, wshift, H, wmax, total, &pending) == R && pending == F - R);
            CHECK(stream_rows_step(window, wshift, H, wmax, total, nullptr) == R);
            pending = -1;
            CHECK(stream_signal_step(window, wshift, total, &pending) == F * wshift && pending == (F > 0 ? window - wshift : 0));
            // a set's own view of the same: rows of a set with rows out, samples of a set with signal state
            StreamSetShape s;
            s.g.window = window; s.g.wshift = wshift; s.g.H = H; s.g.wmax = wmax;
            CHECK(s.delivered(total, &pending) == R && pending == F - R);
            s.signal = true;
            CHECK(s.delivered(total, &pending) == F * wshift && pending == (F > 0 ? window - wshift : 0));
            steps_checked++;
        }
    }
    CHECK(!stream_step_args_ok(0, 1, 0) && !stream_step_args_ok(8, 0, 0) && !stream_step_args_ok(8, 9, 0) && !stream_step_args_ok(8, 8, -1));
}

int main() {
    CHECK(std::strcmp(CHAINS, "internal: a streamed configuration with chains of whole utterances") == 0);
    for (const Row &r : rows) check_row(r);
    check_steps();
    if (failures) {
        std::printf("stream_set_shape_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_set_shape_check ok: %d shape rows, %d totals stepped\n", (int)(sizeof rows / sizeof rows[0]), steps_checked);
    return 0;
}
