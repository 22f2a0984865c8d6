// Every constant, enum and build switch that host-only code shares with the kernels: plain C++, no HIP.
// Included by kernel_common.h (the kernels), by accept.cc / tables.cc (what is accepted, which instantiation runs, what the tables
// hold), by plan_host.h / plan.cc (the plan of an offline run) and by stream_plan.h (the push planner); all of these but the kernels
// compile without hipcc.  The kernel headers define none of these themselves.
//
// Build switches: CTU_STAMP below and CTU_DIAG are all there are - no other file of csrc/ or host/ defines one
// (tests/test_build_switches_cpu.py) - and both are instruments, not alternatives: every kernel has one code path.  An A/B is a
// comparison of two commits' libraries (tools/build_variant.sh, CTU_ENGINE_LIB), or of a switch that lives for one pull request.
// (CTU_DIAG is only ever tested: a -DCTU_DIAG build reads CTU_DEBUG_MODE at run time.)
#pragma once

#include <cstdint>

#ifndef CTU_STAMP
#define CTU_STAMP 0     // diagnostic build: per-wave s_memtime sums per code segment of frontend_kernel (never in production)
#endif

namespace {

constexpr int TILE = 64;       // frames per tile (= lanes of the per-frame phase)
constexpr int WG = 512;        // threads per workgroup (8 waves)
constexpr int NWAVE = WG / 64;
constexpr int PCM_ALIGN = 8;   // utterance starts are multiples of this many samples
constexpr int PCM_HEAD = 8;    // samples of padding before the first utterance (x[-2..-1] of frame 0 is loaded)
constexpr int PCM_TAIL = 512;  // padding after the last one: the generic instantiation loads 16 rows of 32 samples whatever the window
constexpr int ROWS_ALIGN = 4;  // HTK feature input: utterance starts in the arena are multiples of this many 32-bit words (16 bytes)
// What an utterance of n samples takes of the PCM arena, and one of n words of the arena of feature files: the one statement of the
// two layout rules (plan.cc: arena_layout, rows_arena_layout; stream_plan.h: the slot of a pushed stream)
constexpr int64_t pcm_slot(int64_t n) { return (n + PCM_ALIGN - 1) / PCM_ALIGN * PCM_ALIGN; }
constexpr int64_t rows_slot(int64_t n) { return (n + ROWS_ALIGN - 1) / ROWS_ALIGN * ROWS_ALIGN; }

// Tile record (32 bytes, read with one scalar load: load_rec, kernel_common.h): where the tile's first frame starts in the PCM
// arena, where its first output row goes, how many of its 64 frame slots are real, the frame index of
// slot 0 inside its utterance, the next tile this workgroup / wave walks (-1 = done), the utterance's frame count.
// Filled by the planner of an offline run (plan.cc) and, push after push, by stream_stitch_kernel.
struct TileRec {
    int64_t sbase, rbase;
    int nvalid, t0, next, T;  // T = frames of the tile's utterance
};

constexpr int LDS_2WG = 80 * 1024;     // two workgroups per CU fit when a workgroup's LDS stays at or under this
constexpr int ROWS_WG_PER_CU = 8;      // rows_ingest_kernel: workgroups of four waves per CU: 32 waves, each with a tile of 64 rows in flight
constexpr int VFC_STRIDE = 16;         // vad_kernels.h: floats per frame in the cepstra scratch: the fused path's 14 coefficients, 64-byte rows
// Waves per SIMD a front-end instantiation is compiled for (frontend_kernel's launch bounds; PlanGeom sizes the chains by it).
constexpr int FE_LB = 4;     // waves per SIMD the front end's register allocator must leave room for (2 workgroups x 8 waves / 4 SIMDs)
constexpr int FE_SY_LB = 2;  // register budget of the synthesis instantiations (SY): 256 VGPRs, one workgroup per CU.  Measured (profiles/r03_ab_sy_register_budget.txt): at 128 VGPRs they spill 200 bytes per lane; 2 -> -25 % kernel time, 3 -> -21 %
// The fused detector paths of the 512-point mode (VF / SS with MODE 0) keep both passes' transform outputs and a 25-sample
// lattice per lane alive: 256 VGPRs, one workgroup per CU (their staging area takes the LDS of the second one anyway).
constexpr int fe_waves_per_simd(int mode, bool vf, bool ss, bool sy = false) {
    return ((vf || ss) && mode == 0) ? 2 : (sy ? FE_SY_LB : FE_LB);
}

constexpr int PSTRIDE = 260;   // floats per P-tile row: 257 bins padded so rows stay 16-byte aligned (b128 reads in phase 2)
constexpr int MAX_LP = 23;     // LP order / cepstral order limit: the front end accumulates MAXC = 24 lags (R[0..23]) per frame, lp_tail_kernel keeps one frame's recursion in a lane's registers
constexpr int GEN_PLAIN = 0, GEN_INLD = 1, GEN_EXTEN = 2, GEN_FULL = 3, GEN_DC1 = 4;  // front-end option specialisations (frontend_kernel.h)
constexpr int MAXC = 24;       // most coefficients accumulated per frame in phase 2 (cepstra incl. c0, or LP lags): the in-kernel limit.  A dctc chain of
                               // 25 to 64 values runs its front end band-valued and takes dct_wide_kernel (dctw_kernel.h) for the DCT

// Per-lane constant record, one per l16 = lane & 15, streamed from L1 every pass instead of pinning
// 70+ VGPRs:  [0,32) Hamming pairs (w[32j+2l], w[32j+2l+1]) j=0..15 | [32,64) 1/0 "sample is inside the
// window" pairs for DC removal | [64,96) inter-stage twiddles W256^(l*k1), k1=1..15 (+pad) |
// [96,112) W512^(l+16*k2), k2=0..7
constexpr int LC_WIN = 0, LC_MASK = 32, LC_TW = 64, LC_UT = 96, LANEC = 112;
// The records are copied into LDS per workgroup: PCM streaming keeps evicting them from L1 and a miss costs
// ~1k cycles.  Row stride 116 floats makes the 16 lanes' ds_read_b128 conflict-free (116 mod 64 = 52).
constexpr int LTW_STRIDE = 116, LTW_FLOATS = 16 * LTW_STRIDE;

// Kernel variants by feature tail.  BANDS covers spec / logspec / the log-mel scratch of TRAP and of the wide DCT tail (runtime flags
// band_log, band_to_scratch); LP covers lpc and lpa (runtime flag lp_is_lpa).
enum FeatMode { FEAT_BANDS = 0, FEAT_DCTC = 2, FEAT_LP = 3, FEAT_LPD = 4 };  // LPD: LP analysis with the autocorrelation and the recursions in double

// The fused detector paths (vad_fused.h)
constexpr int VF_NC = 14;         // cepstral coefficients of the fused path (-vad_lpc_coefs default: Burg order 13)
constexpr int SS_NC = 16;         // the *ss modes' detector uses -fea_ncepcoefs coefficients (src/nr/nr.cc:266-268: 12 in the presets): the lattice is
                                  // unrolled for up to 16 (one coefficient per lane of a frame's 16) and stops at the run-time count (KParams::ss_nc)
// A stream's slot of subtraction state (a set with CTU_STREAMS_SS_STATE; frontend_kernel<..., SS, ..., XS>), in floats, nj = ceil(K / 64):
// Navg[64 nj] | Nravg[64 nj] (element 64 j + lane), then on an 8-byte boundary the detector's record as doubles - c0[64] (one per lane),
// dMean, dMean2, threshold - and nseg as the int in the first word of the last pair
constexpr int xs_ss_floats(int nj) { return 2 * 64 * nj + 2 * 64 + 2 * 3 + 2; }
// ... and on 2048- / 4096-point frames (CTU_STREAMS_SS_LARGE_STATE beside it; bigss_kernel<NIT, true>, ss_decide_stream_kernel), nit = wfft / 256,
// NB = nit / 2 + 1 bins per thread: everything in 8-byte cells - Navg[NB][256] | Nravg[NB][256] as doubles, bin tid + 256 r at [r][tid]
// (a workgroup's loads and stores are 2 KiB contiguous), then the detector's record - c0[64] (one per lane), dMean, dMean2, threshold as
// doubles and nseg as a 64-bit integer.  The set's buffer is one of floats: the count is even, so every slot starts on an 8-byte boundary.
constexpr int xs_ss_big_doubles(int nit) { return 2 * 256 * (nit / 2 + 1); }  // (where the detector's record starts, in doubles)
constexpr int xs_ss_big_floats(int nit) { return 2 * (xs_ss_big_doubles(nit) + 64 + 4); }
static_assert(xs_ss_big_floats(8) % 2 == 0 && xs_ss_big_floats(16) % 2 == 0 && xs_ss_big_floats(8) == 5256 && xs_ss_big_floats(16) == 9352,
              "a slot of doubles in a buffer of floats: an even count keeps every slot base 8-byte aligned");
constexpr int VF_WINDOW = 200;    // the window the fused path is built for (8 kHz, 25 ms); other windows take the separate kernels
constexpr int VF_SPL = 13;        // samples per lane of a frame: 16 lanes x 13 = 208 >= window
// The 512-point mode (16 kHz, 25 ms): one frame per 16-lane group, four frames per half step
constexpr int VF0_WINDOW = 400;   // the window the fused path of the 512-point mode is built for
constexpr int VF0_SPL = 25;       // 16 lanes x 25 = 400 samples
constexpr int VF0_FSTRIDE = 432;  // floats per staged frame: >= 416 (13 rows of 32 samples are written) and = 16 (mod 32): the two frame
                                  // groups of a half wave read 25 l16 + j from different banks
constexpr int VF0_STAGE = 4 * VF0_FSTRIDE;  // floats of staging per wave (behind the tables: these instantiations run one workgroup per CU)

constexpr int VAD_FEA_WIDE = 8;  // vad_kernels.h: entries per lane of the `fea` criterion on vectors of more than 32 entries: up to 512
constexpr int TB_OFF = 56;       // trap_kernel.h: tile origin tc - 56: a multiple of 8 not below half = 50
constexpr int TB_TT = 264;       // trapdct_split16_kernel: tile row in frames: 8 * 15 + 127 < 256 used; 528 bytes per row spreads the bands over the banks and keeps 16-byte alignment
constexpr int TM_BADW = 10;      // trapdct_mfma_kernel: mask words a band over the tile's frames, 64 + 4 * 64 = 320 at the most
constexpr int TB_BADW = 8;       // trapdct_split16_kernel: 256 tile frames
constexpr int TRAP_COMP_STEPS = 26;  // tap groups of the short fp32 instantiations (traplen <= 104): one accumulator chain over the context
constexpr int TRAP_COMP_RUN = 2;     // tap groups (8 taps) of one accumulator chain beyond that (trap_comp_close, trap_kernel.h, which says why 2)
constexpr int TRAP_MAX_LEN = 255, TRAP_MAX_NDCT = 32;
constexpr int LDS_DEFAULT = 64 * 1024, LDS_RAISED = 160 * 1024;  // dynamic LDS a launch gets as it is / behind allow_big_lds (engine.hip)

// The launch shape of offline TRAP-DCT (trap_kernel.h), stated once: build_trap (tables.cc) builds the tables of the kernel named here,
// stage_trap (engine.hip) launches it with these bytes, unsupported_reason (accept.cc) admits what it can launch, and
// ctu_config_table(..., "trap_path") reports it.
//   split16  trapdct_split16_kernel: at most 16 coefficients, a context that fits the 128 padded taps behind the tile origin tc - TB_OFF
//            whatever the frame phase (traplen <= 113), at most 24 bands (NF = 6 loads per lane; 42 KB of LDS: two workgroups per CU)
//   else     trapdct_mfma_kernel<nrb, nsm>: nrb row blocks of 16 coefficients; nsm = TRAP_COMP_STEPS tap groups compiled in for contexts
//            of up to 104 frames, 64 guarded at run time (and summed in compensated runs) beyond
// lds_bytes: the tile(s), then the mask of non-finite frames.  big_lds: more than a launch gets as it is - the launch raises the limit first.
struct TrapPath {
    int split16, nrb, nsm, lds_bytes, big_lds;
};
constexpr TrapPath trap_path(int B, int traplen, int ndct) {
    const int half = (traplen - 1) / 2, ns = (traplen + 3) / 4;
    TrapPath p{0, 0, 0, 0, 0};
    p.split16 = ndct <= 16 && half <= TB_OFF && 7 + (TB_OFF - half) + traplen <= 128 && B <= 24;
    if (p.split16) {
        constexpr int NT16 = 2;  // fp16 terms per value
        p.lds_bytes = NT16 * B * TB_TT * 2 + ((B + 3) & ~3) * 4 + 2 * (4 * NT16 * 64) * 16 + (B * TB_BADW + 4) * 4;
    } else {
        p.nrb = ndct <= 16 ? 1 : 2;
        p.nsm = ns <= TRAP_COMP_STEPS ? TRAP_COMP_STEPS : 64;
        p.lds_bytes = (64 + 4 * (p.nsm == 64 ? ns : p.nsm)) * (B | 1) * 4 + (B * TM_BADW + 1) * 4;
    }
    p.big_lds = p.lds_bytes > LDS_DEFAULT;
    return p;
}
// The bands the fp32 kernel's tile takes at the longest context (64 + 256 frames of B | 1 floats in the default 64 KiB): B <= 51
constexpr bool trap_bands_fit(int B) { return (64 + 4 * 64) * (B | 1) * 4 <= LDS_DEFAULT; }
static_assert(trap_bands_fit(51) && !trap_bands_fit(52) && trap_path(51, TRAP_MAX_LEN, TRAP_MAX_NDCT).lds_bytes <= LDS_RAISED &&
                  trap_path(51, TRAP_MAX_LEN, TRAP_MAX_NDCT).big_lds && !trap_path(24, 113, 16).big_lds,
              "every accepted TRAP shape launches: behind allow_big_lds where the mask takes the request past 64 KiB");
constexpr int DCTW_KC = 64, DCTW_MAX = 64;  // dctw_kernel.h: bands per chunk of the contraction, most values per frame (four row blocks of 16)

// The DUAL instantiations of frontend_kernel (its phase 1).  They take their window table scaled by 1/2 (tables.cc asks this same function).
constexpr bool fe_dual(int nz, int mode, bool vx, int gen, bool vf, bool ss, bool sy) {
    return mode == 0 && (gen == GEN_PLAIN || gen == GEN_INLD) && !vx && nz < 16 && !vf && !ss && !sy;
}

// VAD module parameters (src/vad/vad.cc, src/vad/vad.h; filled by tables.cc, used by vad_kernels.h and by the fused path of the front end)
struct VadParams {
    int K, wfft, window, ncoef;  // ncoef = vad_lpc_coefs (cepdist lpc) or the length of the vector OUT sees (cepdist fea: every block of a delta / stacking chain)
    int krow, kstride;           // cepdist lpc: the exported spectra's row length and the step from one of the K bins to the next (K, 1
                                 // unless an FFT size below 256 rides on the 256-point mode: then K and wfft are the configuration's own)
    int cri;                     // 0 energy, 1 cepdist-lpc, 2 cepdist-fea
    int thr;                     // 0 absolute, 1 perc, 2 adapt, 3 dyn
    int energy_db, cep_init, filter_order;
    double cep_p, abs_thr, perc_thr, adapt_q, adapt_za, dyn_perc, dyn_min, qmaxinc, qmaxdec, qmindec, qmininc;
    int perc_init, adapt_init, dyn_init;
    int D, ncep, c0_slot;        // cepdist-fea: where the internal vector sits in a written row
    int fea_blk;                 // cepdist-fea behind a delta chain: entries per block of the vector (fea_ncepcoefs + 1); 0: one block
    int delay;                   // delta / stacking ahead of the writer: the detector is called when a delayed vector comes out, on the
                                 // criterion of the newest input frame min(call + delay, T - 1) (src/io/batch.cc:172-192,230-241,251-291)
    int e_slot, e_delay;         // -fea_E: the writer reads the energy through a pointer when the median filter releases a
                                 // vector, so row j carries the energy of row min(j + e_delay, T - 1); e_slot < 0: no such column
};

}  // namespace
