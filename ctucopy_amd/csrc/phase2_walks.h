// Compile-time walk signatures of frontend_kernel's phase 2 (the filter-bank walk of the preset banks).
//
// build_phase2 (tables.cc) deals the bands to slots of eight cells; every cell of slot s walks slot_chunk[s+1] - slot_chunk[s]
// chunks of four bins.  For a preset bank these counts are always the same, so the kernel can walk them straight-line: chunk
// counts, weight addresses and DCT operand addresses become immediates (frontend_kernel.h, phase 2).  A bank that matches no
// entry below takes the generic walk over the run-time records.
//
// The numbers are build_phase2's own output: ctu_config_table(..., "phase2_walk") prints them, tests/test_phase2_walk.py pins
// that the three preset configurations still match.
#pragma once

#include "layout_constants.h"  // FEAT_*, GEN_*: this header is plain C++ too, tables.cc matches banks against it

namespace {

// chunks per slot; slots = sizeof...(NCH); first chunk of slot s = sum of the counts before it
template <int... NCH>
struct walk_sig {
    static constexpr int NS = sizeof...(NCH);
    static constexpr int nch(int s) {
        constexpr int v[NS + 1] = {NCH..., 0};
        return v[s];
    }
    static constexpr int first(int s) {
        int f = 0;
        for (int i = 0; i < s; i++) f += nch(i);
        return f;
    }
};
struct walk_generic {
    static constexpr int NS = 0;  // the walk over the run-time records
};

// A named entry: the signature and the one front-end instantiation that is compiled with it (all entries: 512-point mode,
// 25 ms windows at 16 kHz, i.e. NZ = 13 / MODE 0, 16 coefficient rows, no export).
constexpr int WALK_WFFT = 512, WALK_NZ = 13;
template <int INDEX, int FEAT_, int GEN_, int LPO_, bool MD_, int... NCH>
struct walk_entry : walk_sig<NCH...> {
    static constexpr int index = INDEX, FEAT = FEAT_, GEN = GEN_, LPO = LPO_;
    static constexpr bool MD = MD_;
};
// mel, 26 bands, 512 points, 16 kHz: -preset mfcc (the benchmark's headline)
typedef walk_entry<0, FEAT_DCTC, GEN_PLAIN, 0, true, 13, 6, 4, 2> walk_mel26_512;
// Bark bank of -preset plpc at 16 kHz (PLP: intensity-loudness law, LP order 12)
typedef walk_entry<1, FEAT_LP, GEN_INLD, 12, true, 29, 11, 4> walk_bark_plp_512;
// mel, 23 bands (-fb_definition 23filters): the band front end of the TRAP-DCT chain
typedef walk_entry<2, FEAT_BANDS, GEN_PLAIN, 0, false, 13, 6, 3> walk_mel23_512;

template <class F>
void for_each_walk(F &&f) {
    f(walk_mel26_512{});
    f(walk_bark_plp_512{});
    f(walk_mel23_512{});
}

}  // namespace
