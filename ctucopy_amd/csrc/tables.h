// Which front-end instantiation a configuration runs on and what its tables hold (tables.cc): host only, HIP-free.
// The boundary: accept.cc and tables.cc decide and lay out - one plain value, EngineTables, from a ctu::Design - and engine.hip uploads
// that value and launches by it.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "accept.h"
#include "design.h"
#include "layout_constants.h"
#include "phase2_walks.h"

namespace ctu {

// The front-end instantiation an engine runs on: frontend_kernel's template arguments as values (walk: the entry of phase2_walks.h, -1 =
// the generic walk).  fe_select decides it once, at create; fe_compiled says which exist; launch_frontend turns it into the launch.
// All zero (walk -1) for the large-FFT kernels, whose choice is the FFT size alone.
struct FeSel {
    int nz = 0, feat = 0, mode = 0;  // mode 0: 512-point FFT, 1: 256-point FFT (two frames per complex transform)
    bool vx = false;
    int nc = 0, gen = 0, lpo = 0;
    bool md = false, vf = false, ss = false, sy = false;
    int walk = -1;
};
// The front end of FFT sizes of 1024 to 4096 points (build_engine_tables decides it once; the run dispatches on it, ctu_engine_kernel_name
// names it): wave1k_kernel, bigfft_kernel's export ahead of bigss_kernel (hwss / fwss / 2fwss), or bigfft_kernel alone
enum BigPath { BIG_NONE, BIG_WAVE1K, BIG_SS, BIG_FFT };

// Which combinations of frontend_kernel's template arguments are compiled (launch_frontend instantiates exactly these).
constexpr bool fe_compiled(const FeSel &k) {
    const bool bands = k.feat == FEAT_BANDS, lpo_ok = k.lpo == 0 || k.lpo == 12;
    if ((k.nz != 13 && k.nz != 16) || (k.mode != 0 && k.mode != 1)) return false;
    if (!bands && k.feat != FEAT_DCTC && k.feat != FEAT_LP && k.feat != FEAT_LPD) return false;
    if (k.nc != 16 && !(k.nc == MAXC && !bands)) return false;  // MAXC: coefficient rows of more than 16 cepstra / LP lags
    if (k.gen == GEN_DC1 && k.nz != 16) return false;          // -remove_dc1: the generic row count only
    if ((k.vf || k.ss) && k.nz != 13) return false;            // the detector paths: the 25 ms frame shapes (13 rows cover every shorter window)
    if (k.vx) return k.gen == GEN_FULL && !k.lpo && !k.md && !k.vf && !k.ss && !k.sy;  // the export costs registers: run-time flags only
    if (k.sy) return bands && !k.lpo && !k.md && !k.vf && (k.gen == GEN_FULL || (k.gen == GEN_DC1 && !k.ss));
    if (k.vf) return k.feat == FEAT_DCTC && k.md && k.nc == 16 && !k.lpo && !k.ss && (k.gen == GEN_PLAIN || k.gen == GEN_EXTEN);
    if (k.ss)  // the plain chain with the detector's lattice unrolled for the presets' 12 coefficients (LPO = 12) or for up to 16, or run-time flags
        return k.nc == 16 && ((k.gen == GEN_FULL && !k.lpo && !k.md) || (k.gen == GEN_PLAIN && lpo_ok && (bands ? !k.md : (k.feat == FEAT_DCTC && k.md))));
    if (k.md) return k.nc == 16 && ((k.feat == FEAT_DCTC && !k.lpo && (k.gen == GEN_PLAIN || k.gen == GEN_EXTEN)) || (k.feat == FEAT_LP && k.gen == GEN_INLD && lpo_ok));
    switch (k.gen) {
        case GEN_PLAIN: return !k.lpo && k.feat != FEAT_LPD;  // (the double LP tail has run-time flags only)
        case GEN_INLD: return k.feat == FEAT_LP && k.nc == 16 && lpo_ok;
        case GEN_EXTEN: return bands && !k.lpo;
        default: return (k.gen == GEN_FULL || k.gen == GEN_DC1) && !k.lpo;
    }
}
// Is W the walk entry compiled for exactly this instantiation?
template <class W>
constexpr bool walk_serves(const FeSel &k) {
    return k.nz == WALK_NZ && k.mode == 0 && !k.vx && k.nc == 16 && k.feat == W::FEAT && k.gen == W::GEN && k.lpo == W::LPO && k.md == W::MD && !k.vf && !k.ss && !k.sy;
}
// The name that keys the profiles: the walk, the export and the row width are not shown.
std::string fe_name(const FeSel &k);

// FFT sizes below 256 (windows up to 128 samples): the N-point spectrum of a frame is every (256/N)-th bin of its
// 256-point spectrum, because the frame is zero beyond the window either way.  The engine runs the 256-point mode
// with the filter bank spread onto those bins (zero weight in between); sums over bins step by kstride.
struct Spread {
    int kstride = 1;               // > 1: an FFT size below 256 carried by the 256-point mode
    int user_wfft = 0, user_K = 0;  // the configuration's own FFT size and bin count (what ctu_engine_dims reports)
};
Spread spread_small_fft(Design &d);

// The table area of the 512 / 256-point front end: the image of its LDS tables followed by the lifter, and where the parts sit (see
// KParams for the layout).  Default: the empty area of the large-FFT kernels and of speech output.
struct Phase2Tables {
    std::vector<float> ft = std::vector<float>(4, 0.f);  // LDS image followed by the lifter
    std::vector<int> it = std::vector<int>(4, 0);        // slot_chunk[NS+1] | row_slot[nfea]
    std::vector<int> cells, slot_chunk;
    int lift_off = 0, tab_floats = 0, ck_off = 0, cf_off = 0, cfd_off = 0, am_off = 0, han_off = 0, NS = 0, CW = 4;
    int ncoef_out = 0;  // DCTC: coefficients written per row (the large-FFT kernels' coefficient table as well)
    bool md = false;    // lane map of the MFMA tail: lane = frame + 8 h + 16 kk, group = kk + 4 h
};
void build_phase2(const Design &d, Phase2Tables &t);
// Rebuilds every band's dense weight row from the chunk tables and returns the largest deviation from the
// float-rounded filter bank (0 when the tables are consistent).
double check_phase2(const Design &d, const Phase2Tables &t);
// The compiled walk signature (phase2_walks.h) that this bank matches, or -1.
int match_walk(const Design &d, const std::vector<int> &slot_chunk);
// The instantiation a configuration runs on, from the design (after spread_small_fft) and its phase-2 tables (none with speech output).
FeSel fe_select(const Design &d, const Phase2Tables *t);

// Everything create decides and lays out for the kernels, as one plain value: scalars and the images engine.hip uploads word for word
// (float pairs and 16-byte records as their words).  ctu_config_table(..., "host_tables") reports it (host_tables_report).
struct EngineTables {
    FeSel sel;                // the front-end instantiation (all zero for the large-FFT kernels)
    int feat = FEAT_DCTC;     // the feature tail: sel.feat, or the large-FFT kernels' own
    bool big = false;         // FFT sizes of 1024 to 4096 points (bigfft_kernel.h)
    BigPath path = BIG_NONE;  // BIG_WAVE1K: 1024-point frames on wave1k_kernel (one wave per frame); CTU_WAVE1K=0 keeps them on bigfft_kernel
    int ss = 0;               // hwss / fwss / 2fwss (1 / 2 / 3) on frontend_kernel<..., SS>, or with `big` on bigss_kernel (bigss_kernel.h)
    bool ss_file = false;     // -vad file=<f>: the decisions come from a byte stream
    bool dctw = false;        // dctc with more than MAXC values per frame: the front end runs band-valued into the plan's logmel, dct_wide_kernel follows
    bool trap_bf16 = false;   // TRAP on the bf16 / fp16 matrix pipe (trapG16)
    size_t lds_bytes = 0;     // dynamic LDS of the front-end launch
    int dctw_nout = 0, dctw_chunks = 0, big_fb_total = 0;
    Phase2Tables p2;          // ftab = p2.ft, itab = p2.it, and the offsets of the parameter block
    std::vector<float> lanec;       // [16][LANEC] per-lane constant records
    std::vector<float> trapG;       // TRAP-DCT: the folded table [ndct][traplen]
    std::vector<uint32_t> trapG16;  // its A fragments [8 phases][4 k-steps][2 or 3 terms][64 lanes] of four words (trap_kernel.h)
    std::vector<float> dctw_tab;    // A operands of dct_wide_kernel
    // the large-FFT kernels' tables (big_tw: cos, -sin pairs)
    std::vector<float> big_win, big_tw, big_fbw, big_coef, big_lifter;
    std::vector<int> big_range, big_slot, big_seg;
    std::vector<double> big_coef_d;
    std::vector<double> big_han;    // hwss / fwss / 2fwss at 2048 / 4096 points: the detector's Hann window [window] (bigssdet_kernel)
};
// `d`: after spread_small_fft.  Needs no device.  Environment: CTU_PHASE2_GENERIC=1 (the generic walk for every bank), CTU_WAVE1K=0,
// and in CTU_DIAG builds CTU_DEBUG_MODE.
EngineTables build_engine_tables(const Design &d);

// ctu_config_table(..., "host_tables"): the scalars and images of EngineTables and the fields of VadParams, in the order
// include/ctu_engine.h documents.
std::vector<double> host_tables_report(Design &d);

}  // namespace ctu

namespace {

// The VAD module's parameter block for the kernels (after spread_small_fft).
inline VadParams vad_params(const ctu::Design &d, const ctu::Spread &sp) {
    const ctu::Opts &o = d.o;
    VadParams vp;
    std::memset(&vp, 0, sizeof vp);
    vp.K = d.K; vp.wfft = d.wfft; vp.window = d.window;
    vp.krow = d.K; vp.kstride = sp.kstride;
    if (sp.kstride > 1) {  // an FFT size below 256 on the 256-point mode: the detector's inverse transform keeps the configuration's size
        vp.K = sp.user_K;
        vp.wfft = sp.user_wfft;
    }
    vp.cri = o.vad_cri_mode == "energy" ? 0 : (o.vad_cepdist_mode == "lpc" ? 1 : 2);
    vp.ncoef = vp.cri == 1 ? o.vad_lpc_coefs : ctu::vad_fea_entries(d);
    vp.fea_blk = (d.post_order > 0 && !d.post_stack) ? o.fea_ncepcoefs + 1 : 0;
    vp.thr = o.vad_thr_mode == "absolute" ? 0 : o.vad_thr_mode == "perc" ? 1 : o.vad_thr_mode == "adapt" ? 2 : 3;
    vp.energy_db = o.vad_energy_db; vp.cep_init = o.vad_cepdist_init; vp.filter_order = o.vad_filter_order;
    vp.cep_p = o.vad_cepdist_p; vp.abs_thr = o.vad_absolute_thr; vp.perc_thr = o.vad_perc_thr;
    vp.adapt_q = o.vad_adapt_q; vp.adapt_za = o.vad_adapt_za; vp.dyn_perc = o.vad_dyn_perc; vp.dyn_min = o.vad_dyn_min;
    vp.qmaxinc = o.vad_dyn_qmaxinc; vp.qmaxdec = o.vad_dyn_qmaxdec; vp.qmindec = o.vad_dyn_qmindec; vp.qmininc = o.vad_dyn_qmininc;
    vp.perc_init = o.vad_perc_init; vp.adapt_init = o.vad_adapt_init; vp.dyn_init = o.vad_dyn_init;
    vp.D = d.D; vp.ncep = o.fea_ncepcoefs; vp.c0_slot = d.post_stack ? -2 : (d.row_slot.empty() ? -1 : d.row_slot[0]);  // -2: stacked rows keep the internal order (c0 first)
    vp.delay = 0;
    for (int j = 0; j < d.post_order; j++) vp.delay += d.post_w[j];
    if (d.kind == ctu::FeaKind::TrapDct) vp.delay = (o.fea_trapdct_traplen - 1) / 2;
    vp.e_slot = o.fea_E ? (d.post_order > 0 ? d.D - 1 : d.e_slot) : -1;
    vp.e_delay = (o.vad_filter_order - 1) / 2;
    return vp;
}

}  // namespace
