// Stand-alone check of the stream set that holds subtraction state on large transforms (ctucopy_amd/csrc/stream_set_shape.h with
// CTU_STREAMS_SS_LARGE_STATE beside CTU_STREAMS_SS_STATE): no engine library, no GPU, no HIP.  tests/test_stream_ss_large_shape_cpu.py
// builds it with opts.cc and design.cc under Address+UB sanitizers and runs it: exit status 0, a final "stream_ss_large_shape_check ok"
// and a silent stderr are the result.  (tests/host/stream_set_shape_check.cc holds every other kind of set.)
//
// The table is the expectation, worked out by hand: such a set is a feature-path *ss set on workgroup chains of whole streams, eight a
// CU (2048 on a chip of 256 CUs), with a slot of xs_ss_big_floats(NIT) floats per stream, NIT = wfft / 256 and NB = NIT / 2 + 1:
// 2 * NB * 256 doubles of Navg | Nravg and 64 + 4 eight-byte cells of the detector's record -
//   NIT 8:  2 * (2 * 5 * 256 + 68) = 5256 floats,   NIT 16:  2 * (2 * 9 * 256 + 68) = 9352 floats.
// The chain heads of a push are chain_deal's: min(N, slots) chains in ceil(chains / 8) groups of eight entries.  The slot of the set's
// plan is lead 8 + window - 1 + max_push samples, and no shorter than window + (wmax + 1) hops.
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
                  LARGE = CTU_STREAMS_LARGE_STATE, TRAP = CTU_STREAMS_TRAP_STATE, SS = CTU_STREAMS_SS_STATE, SSSIG = CTU_STREAMS_SS_SIGNAL_STATE,
                  SSLARGE = CTU_STREAMS_SS_LARGE_STATE, BOTH = SS | SSLARGE };

// engine facts: EngineTables::ss (1 hwss, 2 fwss, 3 2fwss; 0: exten), big, ss_file, sel.mode, chains of whole utterances
static StreamSetFacts facts(int ss, bool big, bool ss_file = false, int chain_slots = 2048, int mode = 0) {
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
    int window, wshift, cstride;
    int64_t xstate;
    int heads;
    int64_t longest;
    int H, wmax, C;   // the chain behind the subtraction (row state), rows of a history
};

#define F44 "-fs 44100 -format_in raw -format_out htk -preset mfcc -preem 0.97 -vad burg -nr_mode "
#define F48 "-fs 48000 -format_in raw -format_out htk -preset mfcc -preem 0.97 -w 64 -s 20 -vad burg -nr_mode "
#define S44 "-fs 44100 -format_in raw -format_out raw -preset exten -vad burg -nr_mode "

static const Row rows[] = {
    // name, args, flags, facts, N, M | refusal, window, wshift, cstride, xstate, heads, longest, H, wmax, C
    {"fwss, 2048 points (NIT 8)", F44 "fwss", BOTH, facts(2, true), 3, 5000, nullptr, 1103, 441, 1104, 5256, 8, 6110, 0, 0, 0},
    {"hwss, 2048 points", F44 "hwss -fea_kind spec -nr_a 2 -nr_b 1.5", BOTH, facts(1, true), 3, 5000, nullptr, 1103, 441, 1104, 5256, 8, 6110, 0, 0, 0},
    {"2fwss, 2048 points, every flag", F44 "2fwss", BOTH | ROW | NR | VAD | SIG | LARGE | TRAP | SSSIG, facts(3, true), 3, 5000, nullptr, 1103, 441, 1104, 5256, 8, 6110, 0, 0, 0},
    {"fwss, 4096 points (NIT 16)", F48 "fwss", BOTH, facts(2, true), 3, 5000, nullptr, 3072, 960, 3072, 9352, 8, 8079, 0, 0, 0},
    {"2fwss, 4096 points", F48 "2fwss -nr_p 0.9 -nr_q 0.95", BOTH, facts(3, true), 9, 960, nullptr, 3072, 960, 3072, 9352, 16, 4039, 0, 0, 0},
    {"2fwss + d_a + CMS, row state", F44 "2fwss -fea_delta d_a -fea_Z_exp 500", BOTH | ROW, facts(3, true), 3, 5000, nullptr, 1103, 441, 1104, 5256, 8, 6110, 4, 2, 8},
    {"... pushes of one sample: the shortest file of the chain", F44 "2fwss -fea_delta d_a -fea_Z_exp 500", BOTH | ROW, facts(3, true), 3, 1, nullptr, 1103, 441, 1104, 5256, 8,
     2426 /* window + 3 hops */, 4, 2, 8},
    {"2100 streams on 2048 chain slots", F44 "fwss", BOTH, facts(2, true), 2100, 1544, nullptr, 1103, 441, 1104, 5256, 2048, 2654, 0, 0, 0},
    {"20 streams on 4 chain slots", F48 "fwss", BOTH, facts(2, true, false, 4), 20, 5000, nullptr, 3072, 960, 3072, 9352, 8, 8079, 0, 0, 0},
    // the flag beside the 256- / 512-point front end's set changes nothing of it: xs_ss_floats(5) = 776 floats on wave chains
    {"fwss, 512 points: the small front end's slot", "-fs 16000 -format_in raw -format_out htk -preset mfcc -vad burg -nr_mode fwss", BOTH, facts(2, false, false, 4096), 3, 1000, nullptr,
     400, 160, 400, 776, 8, 1407, 0, 0, 0},
    // an engine and a set that do not fit each other: what streams_unsupported_reason should have refused
    {"large frames without the flag", F44 "fwss", SS, facts(2, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"large frames with the large-transform state of exten instead", F44 "fwss", SS | NR | LARGE | ROW, facts(2, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"the flag without the subtraction state", F44 "fwss", SSLARGE | NR, facts(2, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"with -vad file=", "-fs 44100 -format_in raw -format_out htk -preset mfcc -vad file=x -nr_mode fwss", BOTH, facts(2, true, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"speech output on large frames", S44 "fwss", BOTH | SIG | SSSIG | LARGE, facts(2, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
    {"exten on large frames: the flag is not exten's", "-fs 44100 -format_in raw -format_out htk -preset mfcc -nr_mode exten", BOTH | NR, facts(0, true), 3, 5000, CHAINS, 0, 0, 0, 0, 0, 0, 0, 0, 0},
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
        CHECK(s.ss && s.chained && !s.signal && !s.vad && !s.trap && !s.ola_big);
        CHECK(s.g.chained && !s.g.signal && !s.g.vad && s.g.held == (r.C > 0));
        CHECK(s.g.window == r.window && s.g.wshift == r.wshift && s.g.H == r.H && s.g.wmax == r.wmax);
        CHECK(s.g.max_wg == 512 && s.g.max_chains == r.f.chain_slots);
        CHECK(s.n_streams == r.N && s.C == r.C && s.D == d.D);
        CHECK(s.cstride == r.cstride && s.tstride == 0);
        CHECK(s.xstate_floats == r.xstate && s.xstate_floats % 2 == 0);
        if (r.f.big) CHECK(s.xstate_floats == xs_ss_big_floats(d.wfft / 256) && 2 * (xs_ss_big_doubles(d.wfft / 256) + 68) == s.xstate_floats);
        CHECK(s.n_heads == r.heads && s.n_heads % 8 == 0 && s.n_heads >= std::min(r.N, r.f.chain_slots));
        CHECK(s.longest == r.longest);
        CHECK(s.otail_n() == 0 && s.vsink_n(40) == 0 && s.vbase_n(40) == 0 && s.cols_n(40) == 0);
        CHECK((s.hist_n() > 0) == (r.C > 0) && (s.means_n() > 0) == (r.C > 0));
        if (r.C > 0) CHECK(s.hw == d.Dbase && s.hist_n() == (int64_t)2 * r.N * r.C * d.Dbase && s.means_n() == (int64_t)r.N * 32);
        int H = -1, wmax = -1;
        stream_set_halo(d, r.flags, &H, &wmax);
        CHECK(H == r.H && wmax == r.wmax);
        // rows: all of a push's frames without a chain, H fewer once frame wmax + 2 exists with one
        int64_t pending = -1;
        const int64_t total = r.window + 9 * (int64_t)r.wshift;   // ten frames
        CHECK(s.delivered(total, &pending) == 10 - r.H && pending == r.H);
    }
    std::printf("%-62s %s\n", r.name, failures == before ? "ok" : "FAILED");
}

int main() {
    CHECK(SSLARGE == 8192 && xs_ss_big_floats(8) == 5256 && xs_ss_big_floats(16) == 9352);
    CHECK(xs_ss_big_doubles(8) == 2560 && xs_ss_big_doubles(16) == 4608);
    for (const Row &r : rows) check_row(r);
    if (failures) {
        std::printf("stream_ss_large_shape_check: %d failures\n", failures);
        return 1;
    }
    std::printf("stream_ss_large_shape_check ok: %d shape rows\n", (int)(sizeof rows / sizeof rows[0]));
    return 0;
}
