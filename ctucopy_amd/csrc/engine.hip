// MI355X (gfx950) engine: host side of the C ABI (include/ctu_engine.h) - table design for the kernels, plans
// (batch layout, tile chains), launches.  The kernels live in the headers included below, in one translation unit:
//   kernel_common.h    constants (layout_constants.h: those host-only code shares), the kernel parameter block, DPP / LDS helpers, tile records
//   frontend_kernel.h  PCM -> pre-emphasis * Hamming -> 512/256-pt real FFT in registers -> |.|^2 (P tile in LDS)
//                      -> exten NR -> banded filter bank -> ^0.33 / log -> DCT-II + lifter | cosine iDFT + Levinson
//   vad_kernels.h      Burg-cepstral criterion (packed inverse FFT + lattice), the detector's recurrences per utterance (one wave, or one
//                      lane for the fused path)
//   lp_tail_kernel.h   Levinson-Durbin and a -> c, one frame per lane
//   wave1k_kernel.h    1024-point frames, one wave per frame
//   trap_kernel.h      TRAP-DCT as fp32 MFMA Toeplitz contraction
//   dctw_kernel.h      DCT-II tail of 25 to 64 values per frame (hi-res MFCC) over the band logarithms a front end left in scratch
//   post_kernels.h     delta chain / stacking, CMS, per-speaker CMVN over resident rows
//   rows_in_kernels.h  HTK feature input: byte order and slot of every word of the files' rows
//   signal_kernels.h   speech-enhancement output: inverse transform, overlap-add
//   bigfft_kernel.h    1024 .. 4096-point frames, a workgroup per frame; bigburg_kernel.h the Burg-cepstral criterion / detector there;
//   bigss_kernel.h     hwss / fwss / 2fwss on 2048 / 4096-point frames along chains of whole utterances
//   stream_kernels.h   streaming input: carry | new samples into the slots of a push arena, the tile records of the push, the next carry
//   stream_rows_kernels.h  streaming input with row state: delta chain / stacking and CMS by absolute frame index, the base-row history
//   stream_plan.h      streaming input, host only and HIP-free: the descriptors of a push and the planner that fills them (slots, chains, rows)
//   streams_host.h     streaming input, host side: the stream set, create / push (check, plan, commit, launch) / finish
//
// Data layout in HBM
//   pcm   : one packed int16 arena; utterance i starts at sample_off[i] (multiple of 8 samples)
//   rows  : float32 [total_frames][D] in writer order (c1..cN, c0[, E]), utterance i at row_off[i]
//   tiles : 32-byte records; a tile is <= 64 consecutive frames of ONE utterance, workgroups walk chains of tiles
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <string>
#include <vector>

#include "../../include/ctu_engine.h"
#include "design.h"
#include "opts.h"


#include "kernel_common.h"
#include "vad_kernels.h"
#include "vad_fused.h"
#include "frontend_kernel.h"
#include "trap_kernel.h"
#include "dctw_kernel.h"
#include "decode_kernels.h"
#include "rows_in_kernels.h"
#include "bigfft_kernel.h"
#include "lp_tail_kernel.h"
#include "wave1k_kernel.h"
#include "bigburg_kernel.h"
#include "bigss_kernel.h"
#include "stream_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
thread_local std::string g_create_error;

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    void upload(const std::vector<T> &h) {
        release();
        n = h.size();
        if (!n) return;
        HIP_TRY(hipMalloc(&p, n * sizeof(T)));
        HIP_TRY(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    void alloc(size_t count) {
        release();
        n = count;
        if (n) HIP_TRY(hipMalloc(&p, n * sizeof(T)));
    }
    void reserve(size_t count) {  // grows, never shrinks: a buffer kept from call to call
        if (n < count) alloc(count);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// The front-end instantiation an engine runs on: frontend_kernel's template arguments as values (walk: the entry of phase2_walks.h, -1 =
// the generic walk).  fe_select decides it once, at create; fe_compiled says which exist; launch_frontend turns it into the launch.
// All zero (walk -1) for the large-FFT kernels, whose choice is the FFT size alone.
struct FeSel {
    int nz = 0, feat = 0, mode = 0;
    bool vx = false;
    int nc = 0, gen = 0, lpo = 0;
    bool md = false, vf = false, ss = false, sy = false;
    int walk = -1;
};
// The front end of FFT sizes of 1024 to 4096 points (build_tables decides it once; the run dispatches on it, ctu_engine_kernel_name names it):
// wave1k_kernel, bigfft_kernel's export ahead of bigss_kernel (hwss / fwss / 2fwss), or bigfft_kernel alone
enum BigPath { BIG_NONE, BIG_WAVE1K, BIG_SS, BIG_FFT };

}  // namespace

#include "post_kernels.h"
#include "stream_rows_kernels.h"
#include "stream_vad_kernels.h"
#include "signal_kernels.h"

struct ctu_engine {
    std::unique_ptr<ctu::Design> design;
    int device = 0;
    int n_cu = 256;
    int user_wfft = 0, user_K = 0;
    int kstride = 1;            // > 1: an FFT size below 256 carried by the 256-point mode (ctu_engine_create)
    std::string err, kname;
    FeSel sel;     // the front-end instantiation (build_tables); feat / mode / md / vf / sy / ss below are assigned with it
    int feat = FEAT_DCTC;
    int mode = 0;  // 0: 512-point FFT, 1: 256-point FFT (two frames per complex transform)
    DevBuf<float> lanec, ftab, trapG;
    DevBuf<uint4> trapG16;   // TRAP on the bf16 matrix pipe: A fragments [8 phases][4 k-steps][3 terms][64 lanes] (trap_kernel.h)
    bool trap_bf16 = false;
    bool dctw = false;       // dctc with more than MAXC values per frame: the front end runs band-valued into the plan's logmel, dct_wide_kernel follows
    DevBuf<float> dctw_tab;  // its A operands (build_dctw)
    int dctw_nout = 0, dctw_chunks = 0;
    DevBuf<int> itab;
    // FFT sizes of 1024 to 4096 points (bigfft_kernel.h)
    bool big = false;
    BigPath path = BIG_NONE;    // BIG_WAVE1K: 1024-point frames on wave1k_kernel (one wave per frame); CTU_WAVE1K=0 keeps them on bigfft_kernel
    int big_fb_total = 0;
    DevBuf<float> big_win, big_fbw, big_coef, big_lifter;
    DevBuf<float2> big_tw;
    DevBuf<int> big_range, big_slot, big_seg;
    DevBuf<double> big_coef_d;
    DevBuf<double> big_han;     // hwss / fwss / 2fwss at 2048 / 4096 points: the detector's Hann window [window] (bigssdet_kernel)
    int lift_off = 0, tab_floats = 0, ck_off = 0, cf_off = 0, cfd_off = 0, am_off = 0, NS = 0, CW = 4, ncoef_out = 0;
    bool md = false;        // DCT tail on the matrix cores (frontend_kernel<..., MD>): tables are laid out for its lane map
    int walk_launched = -1; // what the last front-end launch ran: sel.walk, -1 before the first run (ctu_engine_phase2_walk)
    bool vf = false;        // Burg-cepstral VAD criterion fused into the front end (frontend_kernel<..., VF>)
    bool sy = false;        // speech-enhancement output with the inverse transform inside the front end (frontend_kernel<..., SY>)
    int ss = 0;             // hwss / fwss / 2fwss (1 / 2 / 3) on frontend_kernel<..., SS>, or with `big` on bigss_kernel (bigss_kernel.h)
    std::vector<float> ss_stale;  // the spectrum vector the last file of the previous run left behind (zeros at first)
    // -vad file=<f>: ONE byte stream for all files of the process, a byte per frame, never rewound (nr.cc:205-209, 273, 297-302)
    bool ss_file = false;
    std::vector<unsigned char> vad_stream;
    int64_t vad_pos = 0;
    int han_off = 0;
    bool per_wave = false;  // chains per wave (state along an utterance lives in a wave's registers)
    size_t lds_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool host_timed = false;    // the last run was a host run cut into ranges: host_kernel_ms = sum over the ranges' front-end launches
    float host_kernel_ms = 0.f;
    bool in_signal_call = false;
    bool rows_in = false;   // -format_in htk: runs start from rows (ctu_engine_run_rows), no front end, no tables
    // CMVN (row N2): statistic slot <-> row column maps, and per-call scratch
    std::vector<int> col_of_slot, slot_of_col;
    DevBuf<int> d_col_of_slot, d_slot_of_col, d_spk;
    DevBuf<double> d_stat_a, d_stat_b;
    DevBuf<unsigned long long> stamps;
    std::set<const void *> attr_done;  // kernels whose dynamic-LDS limit has been raised on this engine's device
    bool do_vad = false;
    VadParams vp;
    KParams kp0;    // the kernels' parameter blocks as far as design and tables fix them (ctu_engine_create); a run adds its buffers
    BigParams bp0;  // (`big` only)
};

// What a run covers of a plan's buffers: a plan's own extent is the whole of it (plan_layout, plan_chains, ctu_plan_create), a push of
// a stream set runs the front of its set's plan with the extent of the push (streams_host.h).  Every stage launches by the extent it is
// given; a plan is not written once it is created.
struct RunExtent {
    int n_tiles = 0;
    int grid = 0;                  // workgroups of the front-end launch (tile chains are built for it)
    int64_t total_frames = 0;
    const int *heads = nullptr;    // first tile of every chain: a plan's wg_first, or the heads a push was dealt onto (null: a plan over rows)
    void *xstate = nullptr;        // a stream set with noise state: exten's state of every stream (null: none, every file starts afresh)
};

struct ctu_plan {
    ctu_engine *eng = nullptr;
    int n_utt = 0;
    std::vector<int64_t> nsamples, sample_off, row_off, frames;
    int64_t total_samples = 0;
    RunExtent ext;              // the whole plan
    DevBuf<TileRec> tiles;
    DevBuf<int> wg_first;
    // host-buffer runs: device copies of the arena / rows / VAD bytes, kept for the life of the plan
    DevBuf<int16_t> h_pcm;
    DevBuf<uint32_t> h_words;   // (a plan over rows: the files' words)
    DevBuf<float> h_rows;
    DevBuf<uint8_t> h_vad;
    // host-buffer runs of large batches: consecutive utterance ranges as plans of their own, run on two streams so that
    // the upload of one range overlaps the kernels and the download of the previous one (ctu_engine_run_host)
    std::vector<std::unique_ptr<ctu_plan>> parts;
    std::vector<int> part_first;       // first utterance of every part, n_utt at the end
    int parts_for = 0;                 // the range count `parts` was built for (ctu_engine_run_host)
    // VAD majority filter out of phase (ctu_plan_set_vad_ring): which frame's vector every written row carries (-1: an untouched ring
    // slot = zeros; absolute row numbers), and a copy of the rows to gather from
    std::vector<int> ring_hidx;        // per utterance, empty = all in phase
    DevBuf<int> ring_src;              // [total_frames]
    DevBuf<float> ring_tmp;            // [total_frames][D]
    hipStream_t part_stream[2] = {nullptr, nullptr};
    ~ctu_plan() {
        for (hipStream_t st : part_stream)
            if (st) (void)hipStreamDestroy(st);
    }
    DevBuf<int> tile_utt;            // utterance of every tile (SS); the stream of every tile (a stream set with noise state)
    DevBuf<float> ss_seed, ss_last;  // SS: noise seeds per utterance [n_utt][K] and the vectors the utterances leave behind
    DevBuf<unsigned char> ss_dirty;  // SS: utterances a pass of the seed iteration recomputes
    DevBuf<unsigned char> ss_vbits;  // SS: the detector's decision of every frame (first pass), reused by the later passes
    DevBuf<float2> xri;         // VAD scratch
    DevBuf<float> pnr;
    DevBuf<float> pss;          // hwss / fwss / 2fwss with speech output at 2048 / 4096 points: the subtracted magnitudes (pnr stays as exported)
    DevBuf<double> vad_ci;
    DevBuf<float> vad_cf;      // fused Burg-cepstral VAD: cepstra of every frame [total_frames][VFC_STRIDE] ahead of vad_lanes_kernel
    DevBuf<int> vf_order;      // utterances with at least one frame, longest first (a wave of vad_lanes_kernel takes 16 in a row)
    int n_live = 0;
    DevBuf<int64_t> d_row_off;
    DevBuf<double> dc1m;       // -remove_dc1: frame means, then
    DevBuf<float> dc1;         // the offsets the frames subtract (decode_kernels.h)
    int max_frames = 0;        // longest utterance of the plan
    // scratch between the kernels of one run; owned by the plan, so plans can run concurrently on different streams
    DevBuf<float> logmel;      // TRAP: log-mel rows [total_frames][B]
    DevBuf<double> lp_r;       // LP kinds: autocorrelation lags [total_frames][lporder + 1] (used as float rows by the fp32 path) ahead of lp_tail_kernel
    DevBuf<float> base_rows;   // front-end rows ahead of the delta / stacking / CMS passes [total_frames][Dbase]
    DevBuf<float> ybuf;        // signal output: time-domain frames ahead of the overlap-add [total_frames][window]
    std::vector<int64_t> out_samples;   // signal output: samples written per utterance
    DevBuf<long long> d_sample_off;
    // TRAP
    DevBuf<int4> utt_info;
    DevBuf<int> trap_chunks, trap_chunks128;   // (utterance, first frame) of every 64- / 128-frame chunk
    int n_trap_chunks = 0, n_trap_chunks128 = 0;
};

namespace {

void set_error(ctu_engine *e, const std::string &m) { e->err = m; }

// The frame of every call that reaches the device: what `body` returns, or CTU_ERR_DEVICE with "ENGINE: <what>" as the engine's
// last error when it throws (HIP_TRY, DevBuf).
template <class F>
int guarded(ctu_engine *e, F &&body) {
    try {
        return body();
    } catch (const std::exception &ex) {
        set_error(e, std::string("ENGINE: ") + ex.what());
        return CTU_ERR_DEVICE;
    }
}

// dctc with more values per frame (cepstra and c0) than phase 2 of the front ends accumulates: dct_wide_kernel behind a band-valued front end
bool dct_wide(const ctu::Design &d) { return !d.rows_in && !d.signal_out && d.kind == ctu::FeaKind::Dctc && d.nfea > MAXC; }
bool ss_eligible(const ctu::Design &d);
bool ss_big_eligible(const ctu::Design &d);
bool vf_eligible(const ctu::Design &d);
int ss_mode_of(const ctu::Opts &o);

// Entries of the vector the VAD's `fea` criterion measures: VADcri_cepdist sizes itself on the vector it is handed (src/vad/vad.cc:182),
// which is the one OUT sees (src/io/batch.cc:76,122-130) - behind a delta or stacking chain every block of the chain's output
// (fea_delta.cc:47), not the base vector alone.
int vad_fea_entries(const ctu::Design &d) {
    const int fea_c = d.o.fea_ncepcoefs + 1;
    if (d.post_order == 0) return d.nfea;
    return d.post_stack ? fea_c * (2 * d.post_w[0] + 1) : fea_c * (d.post_order + 1);
}

// the passes behind the front end - or behind the ingest of feature files: delta chain / stacking, CMVN, CMS
std::string post_unsupported_reason(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    if (d.post_order > 0) {
        if (d.kind != ctu::FeaKind::Dctc && d.kind != ctu::FeaKind::Lpc) return "delta / stacking on non-cepstral kinds (the reference sizes the chain as fea_ncepcoefs+1, src/fea/fea_delta.cc:22-28)";
        if (!o.fea_c0) return "delta / stacking without -fea_c0 (the reference's writers leave slots of the row unwritten, src/io/out.cc:190-201)";
        int wsum = 0;
        for (int j = 0; j < d.post_order; j++) {
            if (d.post_w[j] > 16) return "delta / stacking window above 16 frames";
            wsum += d.post_w[j];
        }
        if (wsum > 24) return "delta windows adding up to more than 24 frames (LDS tile of the chain)";
        if ((size_t)(64 + 2 * wsum) * d.Dbase > 256 * 12) return "delta / stacking tile (64 frames and both halos, times the base row's columns) above 3072 floats (post_kernel's prefetch registers)";
    }
    if (o.stat_cmvn || o.apply_cmvn) {
        if (d.kind != ctu::FeaKind::Dctc && d.kind != ctu::FeaKind::Lpc) return "CMVN on non-cepstral kinds";
        if (!o.fea_c0) return "CMVN without -fea_c0 (c0 is part of the statistics but not of the written row)";
        if (d.post_stack) return "CMVN on stacked vectors";
        if (d.cms) return "CMVN together with CMS (the reference warns and lets CMVN win, src/io/opts.cc:262-264)";
        // the statistics are taken over every frame and the VAD runs on the normalised vectors of the last pass (src/io/batch.cc:193-204,230-241):
        // a criterion on those vectors would need the statistics first
        if (o.do_vad() && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "fea") return "the `fea` VAD criterion together with CMVN";
    }
    if (d.cms) {
        if (d.kind != ctu::FeaKind::Dctc && d.kind != ctu::FeaKind::Lpc) return "CMS on non-cepstral kinds (the reference walks fea_ncepcoefs+1 entries whatever the vector holds, src/fea/post_impl.cc:203-240)";
        if (d.post_stack) return "CMS on stacked vectors";
        if (d.cms == 2 && (o.length_b < 1 || o.length_b > 512)) return "block CMS window outside 1..512 frames";
        if (d.cms_cols > 32) return "more than 32 CMS columns";
        if (d.cms == 1 && d.post_order == 0 && d.Dbase > 32) return "exponential CMS on rows of more than 32 columns (cms_exp_kernel has a lane per column of a 32-lane half wave)";
        if (d.cms == 2 && (size_t)(64 + o.length_b - 1) * d.cms_cols * sizeof(float) > 64 * 1024) return "block CMS tile above 64 KiB of LDS";
    }
    return "";
}

// -format_in htk (src/io/batch.cc:57-60, src/io/in.cc:623-709): what DESIGN.md section 4.8 derives from the reference
std::string rows_unsupported_reason(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    // no FEA object is built, so -fea_kind only picks the header's kind code and the writers' size rule (src/io/out.cc:95-113,148-153)
    if (d.kind == ctu::FeaKind::TrapDct) return "trapdct on input features (HTK feature input builds no FEA, src/io/batch.cc:57-60)";
    if (d.kind == ctu::FeaKind::None) return "fea_kind outside dctc | lpc | spec | logspec with HTK feature input";
    if (d.kind == ctu::FeaKind::Lpa) return "fea_kind lpa with HTK feature input (the writers drop the vector's last entry as if it held a0, src/io/out.cc:108,178)";
    if ((d.kind == ctu::FeaKind::Dctc || d.kind == ctu::FeaKind::Lpc) && !o.fea_c0)
        return "HTK feature input without -fea_c0 (the writers drop the vector's last entry, whatever it holds, src/io/out.cc:109-110,178)";
    // BATCH::init_out (src/io/batch.cc:98-119) picks the energy pointer OUT is built with: for dctc without -fea_rawenergy and with
    // -nr_when beforeFB it is nr->E (:101-108) - a load through the NR object that feature input never builds (:43,57-60; NR::E is a
    // member, src/nr/nr.h:59): the reference dies in its constructor.  The other branches pass in->E (:99,105,114) and are defined.
    if (d.kind == ctu::FeaKind::Dctc && !o.fea_rawenergy && !o.nr_when_afterFB)
        return "fea_kind dctc with HTK feature input needs -fea_rawenergy on or -nr_when afterFB (BATCH::init_out otherwise reads nr->E of the NR object it never "
               "builds for feature input, src/io/batch.cc:101-108,57-60: the reference crashes at start)";
    if ((o.stat_cmvn || o.apply_cmvn) && (o.fea_Z_exp > 0 || o.fea_Z_block > 0))
        return "CMVN together with CMS (the reference warns and lets CMVN win, src/io/opts.cc:262-264)";
    if (o.fea_E) return "-fea_E with HTK feature input (the writers read one entry past the vector, src/io/out.cc:111,178; in->E is never computed)";
    // every VAD option: the criteria read in->_Xsabs, which htkIN never fills, or (-vad_cepdist_mode in | fea) index the vector as c0-first
    if (o.do_vad()) return o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "in" ? "-vad_cepdist_mode in (HTK feature input)" : "VAD together with HTK feature input";
    if (o.nr_mode != "none" || o.rasta) return "noise reduction with HTK feature input (no NR object is built, src/io/batch.cc:57-60,224)";
    if ((d.post_order > 0 || o.stat_cmvn || o.apply_cmvn) && o.nfeacoefs != o.fea_ncepcoefs + 1)
        return "delta / stacking / CMS / CMVN on feature files whose -nfeacoefs differs from fea_ncepcoefs+1 (the chain is sized on fea_ncepcoefs+1 whatever the "
               "vector holds, src/fea/fea_delta.cc:22-28, src/fea/post_impl.cc:208)";
    if (o.format_out == "pfile" && !d.post_stack && o.nfeacoefs != o.fea_ncepcoefs + 1 && (d.kind == ctu::FeaKind::Dctc || d.kind == ctu::FeaKind::Lpc))
        return "pfile output of feature files whose -nfeacoefs differs from fea_ncepcoefs+1 (pfileOUT rotates fea_ncepcoefs+1 entries and leaves the rest unwritten, src/io/out.cc:292-300)";
    return post_unsupported_reason(d);
}

// reasons a valid ctucopy configuration is outside the accelerated path
std::string unsupported_reason(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    if (d.signal_out) {  // row N3: IN -> NR -> sigOUT
        if (o.format_in == "htk") return "HTK feature input with signal output";
        if (o.fea_kind == "td-iir-mfcc") return "fea_kind outside the spectral path";
        if (o.dither != 0.) return "-dither != 0 makes outputs depend on file order (src/io/in.cc:205,454)";
        if (o.remove_dc1) {
            if (d.window / d.wshift > 8) return "-remove_dc1 with more than 8 frames over a sample (window / shift above 8)";
            if (o.fea_E && o.fea_rawenergy) return "-remove_dc1 together with -fea_rawenergy";
        }
        if (o.nr_mode != "none" && o.nr_mode != "exten" && !ss_eligible(d) && !ss_big_eligible(d))
            return "hwss / fwss / 2fwss with signal output outside the detector paths (windows of 129 .. 208 samples on 256 points or 257 .. 400 on 512 with -vad burg and 2 to 16 cepstral coefficients, 2048 / 4096 points with 2 to 32, or -vad file=...; DC removal on, no -remove_dc1; 1024 points not yet)";
        if (o.rasta) return "-nr_rasta";
        // BATCH only constructs its VAD on the feature paths (init_out, src/io/batch.cc:70-76); with signal output save_frame() calls
        // through the never-assigned pointer (batch.cc:230-241): the reference crashes, there is nothing to reproduce
        if (o.do_vad()) return "VAD together with signal output (the reference dereferences a VAD it never constructs there, src/io/batch.cc:62-66,230-241)";
        if (d.wfft > 4096) return "FFT size above 4096";
        if (d.wfft >= 1024) {  // bigfft_kernel exports the spectra, bigsynth_kernel transforms back: the plain chain, exten, and at
                               // 2048 / 4096 points hwss / fwss / 2fwss (bigss_kernel between the two)
            if (o.nr_mode != "none" && o.nr_mode != "exten" && !ss_big_eligible(d)) return "hwss / fwss / 2fwss with signal output at 1024 points (2048 and 4096 run)";
        }
        else if (d.wfft != 512 && d.wfft != 256) return "signal output at an FFT size below 256";
        if (d.window % 2 && d.wfft < 1024) return "odd window length with signal output at an FFT size below 1024";
        if (d.window < 32) return "window shorter than 32 samples";
        return "";
    }
    if (d.rows_in) return rows_unsupported_reason(d);
    if (o.fea_kind == "td-iir-mfcc" || o.fea_kind == "none") return "fea_kind outside the spectral feature path";
    if (o.dither != 0.) return "-dither != 0 makes outputs depend on file order (src/io/in.cc:205,454)";
    if (o.remove_dc1) {
        if (d.window / d.wshift > 8) return "-remove_dc1 with more than 8 frames over a sample (window / shift above 8)";
        if (o.fea_E && o.fea_rawenergy) return "-remove_dc1 together with -fea_rawenergy";
        if (o.do_vad() && !(o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "fea")) return "-remove_dc1 together with a VAD criterion on the spectrum";
    }
    if (dct_wide(d)) {  // what dct_wide_kernel's band-valued front end does not carry
        if (d.nfea > DCTW_MAX) return "more than 64 cepstral values per frame (-fea_ncepcoefs above 63: dct_wide_kernel has four row blocks of 16)";
        if (o.nr_mode != "none" && o.nr_mode != "exten")
            return "hwss / fwss / 2fwss with more than 24 cepstral values per frame (the detector's order is -fea_ncepcoefs; its paths take 2 to 16 coefficients on 256 / 512 points and a dctc chain of at most 24 values on 2048 / 4096)";
        if (o.do_vad()) return "the VAD module beside more than 24 cepstral values per frame (the detector's stages sit behind DCTC-valued front ends)";
        if (o.nr_when_afterFB) return "-nr_when afterFB with more than 24 cepstral values per frame";
    }
    if (o.nr_mode != "none" && o.nr_mode != "exten") {
        // -vad_apply_mode silence zeroes in->_Xsabs behind a non-speech frame (src/vad/vad.cc:727-736).  The features of the frame are
        // out by then and the next get_frame() rewrites the vector, so on every other chain the mode changes nothing - but these
        // modes seed the next file's noise estimate from that very vector (src/nr/nr.cc:212-221)
        if (o.vad_apply_mode == "silence") return "-vad_apply_mode silence together with hwss / fwss / 2fwss (it zeroes the vector the next file's noise estimate starts from)";
        if (!ss_eligible(d) && !ss_big_eligible(d)) return "hwss / fwss / 2fwss outside the detector paths (windows of 129 .. 208 samples on 256 points or 257 .. 400 on 512 with -vad burg, 2 to 16 cepstral coefficients and at most 16 cepstral / LP coefficients; 2048 / 4096 points with 2 to 32 detector coefficients and at most 64 bands; or -vad file=...; DC removal on, no -remove_dc1, no trapdct, no -nr_when afterFB, no CMVN, no VAD module beside it; 1024 points not yet)";
    }
    if (o.nr_when_afterFB) {
        if (d.signal_out) return "-nr_when afterFB together with signal output";
        if (d.B > 64) return "-nr_when afterFB with more than 64 bands";
    }
    if (o.rasta) return "-nr_rasta";
    if (const std::string why = post_unsupported_reason(d); !why.empty()) return why;
    if (o.fea_E && d.kind == ctu::FeaKind::TrapDct) return "-fea_E with trapdct (the energy lags the features by 50 frames in the reference)";
    if (o.do_vad()) {
        // trapdct delays the writer by half a context (src/fea/fea_trap.cc:53-127): the detector runs when a vector comes out, on the
        // newest input frame's criterion - the delta chains' mechanism (vp.delay); the `fea` criterion would read 368-entry vectors
        if (d.kind == ctu::FeaKind::TrapDct && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode != "lpc") return "the `fea` VAD criterion on TRAP vectors";
        if (o.vad_cri_mode != "energy" && o.vad_cri_mode != "cepdist") return "";  // rejected with the reference's text at create
        if (o.vad_cri_mode == "cepdist") {
            if (o.vad_cepdist_mode == "in") return "-vad_cepdist_mode in (HTK feature input)";
            if (o.vad_cepdist_mode == "fea" && d.kind != ctu::FeaKind::Dctc && d.kind != ctu::FeaKind::Lpc) return "-vad_cepdist_mode fea on non-cepstral features";
            const int nc = o.vad_cepdist_mode == "lpc" ? o.vad_lpc_coefs : d.nfea;
            if (nc > 32 || nc < 2) return "more than 32 (or fewer than 2) VAD cepstral coefficients";
            if (o.vad_cepdist_mode == "fea" && vad_fea_entries(d) > 64 * VAD_FEA_WIDE) return "the `fea` VAD criterion on stacked vectors of more than 512 entries";
        }
        if (o.vad_filter_order > 31) return "VAD filter order above 31";
        // behind a delayed chain the flush calls the detector again on the vector VAD::silence_frame zeroed (src/vad/vad.cc:727-736): the Burg
        // criterion divides by its energy and the reference aborts (src/vdet/Burg.h:72); the energy and `fea` criteria read the zeros unharmed
        if (o.vad_apply_mode == "silence" && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" && (d.post_order > 0 || d.kind == ctu::FeaKind::TrapDct))
            return "-vad_apply_mode silence with the lpc criterion behind a delta, stacking or trapdct chain (the reference aborts in its Burg estimator at the flush)";
    }
    if (d.wfft >= 1024) {  // bigfft_kernel.h: the plain chain
        if (d.wfft > 4096) return "FFT size above 4096";
        // exten on the spectrum at 1024 points: wave1k_kernel carries the recurrence along per-wave chains of utterances
        // exten on the spectrum at 1024 .. 4096 points: wave1k_kernel / bigfft_kernel carry the recurrence along chains of whole utterances
        const bool big_exten = o.nr_mode == "exten" && !o.nr_when_afterFB && !d.signal_out;
        // hwss / fwss / 2fwss at 2048 / 4096 points: bigss_kernel (bigss_kernel.h) on the spectra bigfft_kernel exports
        if ((o.nr_mode != "none" || o.nr_when_afterFB) && !big_exten && !ss_big_eligible(d))
            return "noise reduction with an FFT size above 512 (exten on the spectrum at 1024 .. 4096 points and hwss / fwss / 2fwss at 2048 / 4096 excepted)";
        // the VAD on 1024 .. 4096-point frames: the energy of the vector the NR left (wave1k_kernel / bigfft_kernel store it per frame),
        // the cepstral distance on the output vectors, and the Burg-cepstral criterion on the spectra bigfft_kernel exports
        // (bigburg_kernel.h).  Every criterion unsupported_reason lets through above is one of the three.
        if (d.B > 64) return "more than 64 bands with an FFT size above 512";
    }
    else if (d.wfft != 512 && d.wfft != 256) return "FFT size below 32";
    if (d.window < 32) return "window shorter than 32 samples";
    if (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) {
        if (o.fea_lporder >= d.B) return "LP order not below the number of bands: the normal equations are singular and the reference's output is rounding noise";
        if (o.fea_lporder > MAX_LP || o.fea_ncepcoefs > MAX_LP) return "LP order / cepstral order above 23 (the front end accumulates 24 lags per frame)";
    }
    if (d.B > 512) return "more than 512 filter bank channels";
    if (d.kind == ctu::FeaKind::TrapDct && o.fea_trapdct_ndct > 32) return "more than 32 TRAP DCT coefficients";
    if (d.kind == ctu::FeaKind::TrapDct && o.fea_trapdct_traplen > 255) return "TRAP longer than 255 frames";
    if (d.kind == ctu::FeaKind::TrapDct && (size_t)(64 + 256) * (d.B | 1) * 4 > 64 * 1024) return "too many bands for the TRAP tile";
    return "";
}

// Streaming input (ctu_streams_create): what an accepted configuration carries from one frame of a file to the next beyond the samples
// themselves.  A stream set keeps samples (stream_kernels.h), so every such chain is refused by the option that brings the state in.
// With CTU_STREAMS_ROW_STATE the set keeps base rows and running means as well (stream_rows_kernels.h): the delta chain, stacking and CMS pass.
// With CTU_STREAMS_NR_STATE it keeps the noise estimate of -nr_mode exten on the spectrum (256- and 512-point front end): that passes too.
std::string streams_unsupported_reason(const ctu::Design &d, uint32_t flags = 0) {
    const ctu::Opts &o = d.o;
    if (d.rows_in) return "-format_in htk (HTK feature input: there are no samples to stream)";
    if (d.signal_out) return "-format_out raw | wave (speech output: the overlap-add runs across a file's frames)";
    const bool nr_state = (flags & CTU_STREAMS_NR_STATE) != 0;
    if (o.nr_mode == "exten" && nr_state) {  // the state of exten on the spectrum travels with the stream (frontend_kernel<..., XS>)
        if (o.nr_when_afterFB) return "-nr_when afterFB (exten behind the filter bank keeps its noise estimate per band, inside the filter-bank walk: a stream set carries the estimate per bin)";
        if (d.wfft >= 1024) return "-nr_mode exten on " + std::to_string(d.wfft) + "-point frames (-w: the noise estimate of the large transforms lives in their own kernels, a stream set carries the one of the 256- and 512-point front end)";
    } else if (o.nr_mode != "none") return "-nr_mode " + o.nr_mode + " (the noise estimate runs from frame to frame of a file)";
    if (o.remove_dc1) return "-remove_dc1 (a frame's offset stays subtracted from the samples the later frames share with it)";
    if (o.do_vad() && !(flags & CTU_STREAMS_VAD_STATE)) return "the VAD module (-vad_apply_mode / -vad_out_mode: thresholds and the majority filter run along the file)";
    if (o.do_vad()) {  // the detector's state travels with the stream (stream_vad_kernels.h); what it cannot carry is refused by name
        const bool burg = o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc";
        if (o.vad_apply_mode == "drop") return "-vad_apply_mode drop (the row count of a push would depend on the data)";
        if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "fea") return "-vad_cepdist_mode fea (the criterion reads finished rows)";
        if (d.kind == ctu::FeaKind::TrapDct) return "-fea_kind trapdct (a vector spans traplen frames)";
        if (d.post_order > 0)
            return std::string(d.post_stack ? "-fea_trap" : "-fea_delta") + " together with the VAD module (the detector is called when a vector reaches the writer, on frame min(t + H, T - 1))";
        if (d.cms) return std::string(d.cms == 1 ? "-fea_Z_exp" : "-fea_Z_block") + " together with the VAD module (CMS behind the detector's delayed rows is not carried by a stream set)";
        if (o.fea_E && (o.vad_filter_order - 1) / 2 > 0) return "-fea_E with the VAD module's majority filter (the offline run shifts the energy column along the file)";
        if (d.wfft >= 1024) return "the VAD module on 1024-point and larger frames (-w: a stream set carries the detector behind the 256- and 512-point front end)";
        if (o.nr_mode == "exten" && !(burg && vf_eligible(d)))
            return "-nr_mode exten with a VAD criterion outside the fused shapes (25 ms frames at 8 or 16 kHz, the lpc criterion with 14 coefficients: the exported spectra are not carried behind exten's state)";
    }
    if (d.kind == ctu::FeaKind::TrapDct) return "-fea_kind trapdct (a vector spans traplen frames)";
    const bool row_state = (flags & CTU_STREAMS_ROW_STATE) != 0;
    if (d.post_order > 0 && !row_state) return d.post_stack ? "-fea_trap (stacking spans 2 * trap_win + 1 frames)" : "-fea_delta (the delta chain spans the frames of its windows)";
    if (d.cms && !row_state) return d.cms == 1 ? "-fea_Z_exp (CMS: the running mean runs along the file)" : "-fea_Z_block (CMS: the block mean spans its window of frames)";
    if (o.stat_cmvn || o.apply_cmvn) return "-stat_cmvn / -apply_cmvn (CMVN: statistics over whole lists)";
    if (d.wshift > d.window) return "-s above -w (frames that leave samples out)";
    return "";
}

// Host-side image of the phase-2 LDS tables (see KParams for the layout).
struct Phase2Tables {
    std::vector<float> ft;   // LDS image followed by the lifter
    std::vector<int> it;     // slot_chunk[NS+1] | row_slot[nfea]
    std::vector<int> cells, slot_chunk;
    int lift_off = 0, tab_floats = 0, ck_off = 0, cf_off = 0, cfd_off = 0, am_off = 0, han_off = 0, NS = 0, CW = 4, ncoef_out = 0;
    bool md = false;  // lane map of the MFMA tail: lane = frame + 8 h + 16 kk, group = kk + 4 h
};

// The DCT tail runs on the matrix cores for the plain cepstral chains (what fe_select instantiates with MD).
#ifndef CTU_MD
#define CTU_MD 1
#endif
#ifndef CTU_VF
#define CTU_VF 1
#endif
#ifndef CTU_SY
#define CTU_SY 1  // 0: speech-enhancement output through the exported spectra and synth_kernel (round 1's path)
#endif
// the plain cepstral chain: what the specialised instantiations (GEN_PLAIN / GEN_EXTEN with MD) cover
bool plain_cepstral(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    return !o.nr_when_afterFB && d.kind == ctu::FeaKind::Dctc && d.nfea <= 16 && !o.fea_E && o.fb_power && o.remove_dc && !o.remove_dc1 && !o.fb_inld && !d.signal_out;
}
// the frame shapes the fused detector paths are built for: 8 kHz / 25 ms (256-point mode, two frames per complex transform) and
// 16 kHz / 25 ms (512-point mode, 16 lanes x 25 samples) - vad_fused.h
bool fused_frame_shape(const ctu::Design &d) {
    return (d.wfft == 256 && d.window == VF_WINDOW) || (d.wfft == 512 && d.window == VF0_WINDOW);
}
// the *ss modes' detector: any window its lanes' 13 / 25 samples cover in the two transform sizes (the run-time-flag instantiations look
// the window's end up at run time); the shapes above keep their straight-line instantiations on the plain chain
bool ss_frame_shape(const ctu::Design &d) {
    return (d.wfft == 256 && d.window > 128 && d.window <= 16 * VF_SPL) || (d.wfft == 512 && d.window > 256 && d.window <= 16 * VF0_SPL);
}
// Burg-cepstral VAD criterion fused into the front end (vad_fused.h): 14 coefficients (the preset's detector)
bool vf_eligible(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    return CTU_VF && CTU_MD && plain_cepstral(d) && o.do_vad() && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" &&
           fused_frame_shape(d) && o.vad_lpc_coefs == VF_NC && d.post_order == 0;
}
// the compressed-band LP chain (PLP and friends: -fb_inld, at most 16 lags, no energy column, no NR, no VAD): its cosine iDFT
// (src/fea/fea_impl.cc:181-198) is the same contraction over the bands as the DCT and takes the same MFMA tail
#ifndef CTU_LP_MD
#define CTU_LP_MD 1  // 0: the lags on the VALU (cell_accumulate + cells_reduce), for A/B
#endif
bool lp_md_eligible(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    return CTU_MD && CTU_LP_MD && (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) && o.fb_inld && o.fea_lporder + 1 <= 16 && !o.nr_when_afterFB && !o.fea_E &&
           o.fb_power && o.remove_dc && !o.remove_dc1 && !d.signal_out && !o.do_vad() && o.nr_mode == "none";
}
bool md_eligible(const ctu::Design &d) {
    // (the *ss modes on another window than the presets' run the run-time-flag instantiation, which has no MFMA tail)
    return (CTU_MD && plain_cepstral(d) && (!d.o.do_vad() || vf_eligible(d)) && !(ss_mode_of(d.o) && !fused_frame_shape(d))) || lp_md_eligible(d);
}
// hwss / fwss / 2fwss with the Burg cepstral detector (frontend_kernel<..., SS>): 25 ms frames at 8 or 16 kHz, the
// presets' 12 cepstral coefficients for the detector, the plain chain into cepstra or band energies
#ifndef CTU_SS_CACHE
#define CTU_SS_CACHE 1  // 0: every pass of the seed iteration runs the detector again (A/B)
#endif
int ss_mode_of(const ctu::Opts &o) { return o.nr_mode == "hwss" ? 1 : o.nr_mode == "fwss" ? 2 : o.nr_mode == "2fwss" ? 3 : 0; }
// the same modes ahead of sigOUT (-format_out raw|wave): the NR object works on in->_Xsabs - magnitudes, -fb_power is forced off there -
// and the enhanced frames go back to the time domain inside the front end (frontend_kernel<..., SS, SY>)
bool ss_signal_eligible(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= SS_NC) || o.vadmode == "file";
    return CTU_SY && d.signal_out && ss_mode_of(o) && det_ok && ss_frame_shape(d) && o.remove_dc && !o.remove_dc1 && !o.rasta && !o.do_vad();
}
bool ss_eligible(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    if (d.signal_out) return ss_signal_eligible(d);
    // cepstra / LP coefficients in the sixteen-row accumulators, or band energies; everything behind the front end (the LP tail, delta /
    // stacking, CMS, CMVN) runs on the rows of the last pass of the seed iteration
    const bool lp = d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa;
    const bool kind_ok = (d.kind == ctu::FeaKind::Dctc && d.nfea <= 16) || (lp && o.fea_lporder + 1 <= 16) || d.kind == ctu::FeaKind::Spec || d.kind == ctu::FeaKind::LogSpec;
    // -vad file=<f> (nr.cc:205-209, 297-302): the decisions come from a byte stream instead of the detector; same kernel, same frame shapes
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= SS_NC) || o.vadmode == "file";
    // CMVN is two passes over the list in the reference (statistics, then the rows): the second starts from the noise vector the first
    // left behind, and no oracle restates that - refused rather than guessed
    return CTU_MD && ss_mode_of(o) && det_ok && !o.nr_when_afterFB && ss_frame_shape(d) && kind_ok && o.remove_dc && !o.remove_dc1 && !o.do_vad() && !d.signal_out && !o.rasta &&
           !o.stat_cmvn && !o.apply_cmvn;
}

// the same modes on 2048- and 4096-point frames (bigss_kernel.h): spectra exported once, a workgroup per frame for the detector's cepstra
// (2 to 32 coefficients: bigburg_kernel's two instantiations), a workgroup per chain of utterances for the subtraction.  What
// ss_eligible excludes for reasons that do not depend on the size stays excluded; 1024 points (wave1k_kernel's size) stay refused whole.
bool ss_big_eligible(const ctu::Design &d) {
    const ctu::Opts &o = d.o;
    if (!ss_mode_of(o) || (d.wfft != 2048 && d.wfft != 4096) || d.window <= d.wfft / 2) return false;
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= 32) || o.vadmode == "file";
    if (!det_ok || !o.remove_dc || o.remove_dc1 || o.rasta || o.do_vad()) return false;
    if (d.signal_out) return true;
    const bool kind_ok = d.kind == ctu::FeaKind::Dctc || d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa || d.kind == ctu::FeaKind::Spec ||
                         d.kind == ctu::FeaKind::LogSpec;
    return kind_ok && !o.nr_when_afterFB && !o.stat_cmvn && !o.apply_cmvn && d.B <= 64;
}

void build_phase2(const ctu::Design &d, Phase2Tables &t) {
    t.md = md_eligible(d);
    // ---- phase-2 tables.  Bands are dealt to (slot, group) cells: sorted by width, eight per slot, so that the
    // eight lanes of a frame walk bands of similar width in lock step.  A band is cut into 4-bin chunks whose
    // bin range stays inside [0,K); weights outside the band's own [first,last] are zero.
    const int B = d.B;
    std::vector<int> order(B);
    for (int b = 0; b < B; b++) order[b] = b;
    auto width = [&](int b) { return d.fb_last[b] - d.fb_first[b] + 1; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return width(x) > width(y); });
    const int NS = (B + 7) / 8;
    int ncoef = 0;
    const std::vector<double> *coef_tab = nullptr;
    const bool dctc = d.kind == ctu::FeaKind::Dctc && !dct_wide(d);  // (wide: a band-valued front end, no coefficient rows)
    if (dctc) { coef_tab = &d.dct; ncoef = d.nfea; }
    else if (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) { coef_tab = &d.idft; ncoef = d.o.fea_lporder + 1; }
    if (ncoef > MAXC) throw std::runtime_error("more cepstral / LP coefficients than the kernel accumulates");
    const int CW = ncoef <= 16 ? 16 : MAXC;  // the kernel has straight-line code for these two widths
    std::vector<int> slot_chunk(NS + 1, 0);
    std::vector<float> cw;                  // chunk weights [NC][8][4]
    std::vector<int> cell(NS * 8 * 2, 0);   // {first bin of the chunk run, band index or -1}
    const int CWS = CW + 4;  // row stride: 20 or 28 floats = 5 or 7 16-byte units, distinct mod 16 over the 8 groups
    std::vector<float> cf((size_t)NS * 8 * CWS, 0.f);
    // LP analysis on uncompressed band energies (no -fb_inld): the same rows in double for the double tail (FEAT_LPD)
    const bool lpd = (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) && !d.o.fb_inld;
    std::vector<double> cfd(lpd ? (size_t)NS * 8 * CW : 0, 0.0);
    // DCTC: coefficient row r of a cell is the value written to output slot r (c1..cN, then c0)
    std::vector<int> coef_of_slot;
    if (dctc) {
        coef_of_slot.assign(d.nfea, -1);
        int nout = 0;
        for (int i = 0; i < d.nfea; i++)
            if (d.row_slot[i] >= 0) {
                coef_of_slot[d.row_slot[i]] = i;
                nout = std::max(nout, d.row_slot[i] + 1);
            }
        t.ncoef_out = nout;
    }
    auto chunks_of = [&](int b) {  // chunks of 4 bins from the aligned start of the band to its last bin
        const int k0 = d.fb_first[b] & ~3;
        return (d.fb_last[b] - k0) / 4 + 1;
    };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return chunks_of(x) > chunks_of(y); });
    for (int sl = 0; sl < NS; sl++) {
        int nch = 0;
        for (int g = 0; g < 8 && sl * 8 + g < B; g++) nch = std::max(nch, chunks_of(order[sl * 8 + g]));
        if (4 * nch > PSTRIDE) throw std::runtime_error("filter band wider than the spectrum");
        slot_chunk[sl] = (int)cw.size() / 32;
        // Phase 2 reads P with one ds_read_b128 per lane; the 16-byte unit a lane touches is
        // (frame + kstart/4 + chunk) mod 16 (rows are 65 units apart).  A b128 wave access is served in four groups of
        // 16 lanes = {frame f: groups 0-3, f+1: groups 4-7, f+2: groups 4-7, f+3: groups 0-3}; collisions depend only
        // on a_g = kstart_g/4.  Search the assignment of this slot's bands to groups (and up to `slack` leading
        // zero chunks) for the fewest colliding lane pairs.
        std::vector<int> perm(8), best_perm(8), lead(8, 0), best_lead(8, 0);
        for (int g = 0; g < 8; g++) perm[g] = best_perm[g] = sl * 8 + g < B ? order[sl * 8 + g] : -1;
        auto a_of = [&](int b, int ld) { return b < 0 ? -1000 : (std::min(d.fb_first[b] & ~3, PSTRIDE - 4 * nch) / 4 - ld); };
        auto cost = [&](const std::vector<int> &pm, const std::vector<int> &ld) {
            int c = 0, a[8];
            for (int g = 0; g < 8; g++) a[g] = a_of(pm[g], ld[g]);
            // a ds_read_b128 is served in four groups of 16 lanes: {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32
            static const int grp[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                           {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
            for (int q = 0; q < 4; q++) {
                int unit[16];
                for (int i = 0; i < 16; i++) {
                    const int lane = grp[q & 1][i] + 32 * (q >> 1);
                    const int f8 = t.md ? (lane & 7) : (lane >> 3), g = t.md ? (((lane >> 3) & 1) * 4 + (lane >> 4)) : (lane & 7);
                    unit[i] = a[g] < -500 ? -1 - i : ((a[g] + f8) % 16 + 16) % 16;  // rows are 65 units apart
                }
                for (int i = 0; i < 16; i++)
                    for (int j = i + 1; j < 16; j++) c += (unit[i] >= 0 && unit[i] == unit[j]);
            }
            return c;
        };
        {
            int best = cost(perm, lead);
            uint32_t rng = 12345u + sl;
            for (int it = 0; it < 4000 && best > 0; it++) {
                std::vector<int> pm = best_perm, ld = best_lead;
                rng = rng * 1664525u + 1013904223u;
                const int i = (rng >> 8) % 8, j = (rng >> 16) % 8;
                std::swap(pm[i], pm[j]);
                std::swap(ld[i], ld[j]);
                rng = rng * 1664525u + 1013904223u;
                const int g = (rng >> 8) % 8;
                if (pm[g] >= 0) {
                    // leading zero chunks are allowed while the run still starts at >= 0 and ends beyond the last bin
                    const int k0 = std::min(d.fb_first[pm[g]] & ~3, PSTRIDE - 4 * nch);
                    const int mx = std::min({3, k0 / 4, (k0 + 4 * nch - (d.fb_last[pm[g]] + 1)) / 4});
                    ld[g] = mx > 0 ? (int)((rng >> 20) % (mx + 1)) : 0;
                }
                const int c = cost(pm, ld);
                if (c <= best) {
                    best = c;
                    best_perm = pm;
                    best_lead = ld;
                }
            }
        }
        std::vector<int> kstart(8, 0);
        for (int g = 0; g < 8; g++) {
            cell[(sl * 8 + g) * 2 + 1] = -1;
            if (best_perm[g] < 0) continue;
            const int b = best_perm[g];
            // aligned start; the run of nch chunks must end inside the row's PSTRIDE floats (bins >= K get weight 0
            // but are read, so the kernel keeps them finite: it zeroes the row padding once per workgroup)
            kstart[g] = std::min(d.fb_first[b] & ~3, PSTRIDE - 4 * nch) - 4 * best_lead[g];
            cell[(sl * 8 + g) * 2] = kstart[g];
            cell[(sl * 8 + g) * 2 + 1] = b;
            for (int i = 0; i < ncoef; i++) {
                const int src = dctc ? coef_of_slot[i] : i;
                if (src >= 0) cf[((size_t)sl * 8 + g) * CWS + i] = (float)(*coef_tab)[(size_t)src * B + b];
                if (src >= 0 && lpd) cfd[((size_t)sl * 8 + g) * CW + i] = (*coef_tab)[(size_t)src * B + b];
            }
        }
        for (int ch = 0; ch < nch; ch++)
            for (int g = 0; g < 8; g++)
                for (int i = 0; i < 4; i++) {
                    float w = 0.f;
                    if (best_perm[g] >= 0) {
                        const int b = best_perm[g], k = kstart[g] + 4 * ch + i;
                        if (k >= d.fb_first[b] && k <= d.fb_last[b]) w = (float)d.fb[b][k];
                    }
                    cw.push_back(w);
                }
    }
    slot_chunk[NS] = (int)cw.size() / 32;
    std::vector<float> ft(cw);
    t.cells = cell;
    t.slot_chunk = slot_chunk;
    auto push_ints = [&](const std::vector<int> &v) {
        for (int x : v) {
            float f;
            std::memcpy(&f, &x, 4);
            ft.push_back(f);
        }
        while (ft.size() & 3) ft.push_back(0.f);
    };
    t.ck_off = (int)ft.size();
    {   // the kernel's records: {first bin, band or -1, first chunk of the slot, chunks of the slot}; one more slot of idle cells, which
        // the walk prefetches behind the last one
        std::vector<int> rec4((size_t)(NS + 1) * 8 * 4, 0);
        for (int sl = 0; sl <= NS; sl++)
            for (int g = 0; g < 8; g++) {
                int *r = &rec4[(size_t)(sl * 8 + g) * 4];
                r[0] = sl < NS ? cell[(sl * 8 + g) * 2] : 0;
                r[1] = sl < NS ? cell[(sl * 8 + g) * 2 + 1] : -1;
                r[2] = slot_chunk[std::min(sl, NS)];
                r[3] = sl < NS ? slot_chunk[sl + 1] - slot_chunk[sl] : 0;
            }
        push_ints(rec4);
    }
    t.cf_off = (int)ft.size();
    if (!t.md) ft.insert(ft.end(), cf.begin(), cf.end());  // the MFMA tail reads the am table below instead
    while (ft.size() & 3) ft.push_back(0.f);
    if (t.md) {
        // A operands of the DCT MFMAs: for slot sl and half h, lane m + 16 kk holds row m of the folded DCT table (LP chain: of
        // the cosine iDFT table) at the band of cell (sl, group kk + 4 h); zero for idle cells and for rows >= the number of output slots
        t.am_off = (int)ft.size();
        for (int sl = 0; sl < NS; sl++)
            for (int h = 0; h < 2; h++)
                for (int lane = 0; lane < 64; lane++) {
                    const int m = lane & 15, g = (lane >> 4) + 4 * h;
                    const int b = cell[(sl * 8 + g) * 2 + 1];
                    float v = 0.f;
                    if (dctc) {
                        if (b >= 0 && m < t.ncoef_out && coef_of_slot[m] >= 0) v = (float)(*coef_tab)[(size_t)coef_of_slot[m] * B + b];
                    } else if (b >= 0 && m < ncoef) v = (float)(*coef_tab)[(size_t)m * B + b];  // LP: row m = lag m
                    ft.push_back(v);
                }
    }
    if (lpd) {
        t.cfd_off = (int)ft.size();  // a multiple of 4 floats: 8-byte aligned in LDS
        for (double v : cfd) {
            float h[2];
            std::memcpy(h, &v, 8);
            ft.push_back(h[0]);
            ft.push_back(h[1]);
        }
        while (ft.size() & 3) ft.push_back(0.f);
    }
    if (ss_eligible(d)) {
        // Hann window of the *ss modes' detector, han[i] = 0.5 (1 - cos(2 * 3.141592653 / window * i)) (src/vdet/CepstralDet.h:133-136)
        t.han_off = (int)ft.size();
        const double m = 2 * 3.141592653 / d.window;
        for (int i = 0; i < 16 * (d.wfft == 512 ? VF0_SPL : VF_SPL); i++) ft.push_back(i < d.window ? (float)(0.5 * (1 - std::cos(m * i))) : 0.f);
    }
    t.tab_floats = (int)ft.size();
    t.NS = NS;
    t.CW = CW;
    t.lift_off = (int)ft.size();
    for (double v : d.lifter) ft.push_back((float)v);
    ft.push_back(0.f);
    t.ft = ft;
    std::vector<int> it(slot_chunk);
    it.insert(it.end(), d.row_slot.begin(), d.row_slot.end());
    t.it = it;
}

// Rebuilds every band's dense weight row from the chunk tables and returns the largest deviation from the
// float-rounded filter bank (0 when the tables are consistent).
double check_phase2(const ctu::Design &d, const Phase2Tables &t) {
    double worst = 0;
    std::vector<int> seen(d.B, 0);
    for (int sl = 0; sl < t.NS; sl++)
        for (int g = 0; g < 8; g++) {
            const int kstart = t.cells[(sl * 8 + g) * 2], b = t.cells[(sl * 8 + g) * 2 + 1];
            if (b < 0) continue;
            seen[b]++;
            std::vector<double> row(PSTRIDE, 0.0);
            for (int ch = t.slot_chunk[sl]; ch < t.slot_chunk[sl + 1]; ch++)
                for (int i = 0; i < 4; i++) {
                    const int k = kstart + 4 * (ch - t.slot_chunk[sl]) + i;
                    if (k < 0 || k >= PSTRIDE) return 1e30;
                    row[k] += t.ft[(size_t)(ch * 8 + g) * 4 + i];
                }
            for (int k = 0; k < PSTRIDE; k++) {
                const double want = (k < d.K && k >= d.fb_first[b] && k <= d.fb_last[b]) ? (double)(float)d.fb[b][k] : 0.0;
                if (std::fabs(row[k] - want) > 0 && getenv("CTU_P2_DEBUG")) fprintf(stderr, "sl %d g %d band %d k %d kstart %d first %d last %d row %g want %g nch %d\n", sl, g, b, k, kstart, d.fb_first[b], d.fb_last[b], row[k], want, t.slot_chunk[sl+1]-t.slot_chunk[sl]);
                worst = std::max(worst, std::fabs(row[k] - want));
            }
        }
    for (int b = 0; b < d.B; b++)
        if (seen[b] != 1) return 1e30;
    return worst;
}

// The compiled walk signature (phase2_walks.h) that this bank matches, or -1: the chunk counts per slot must be the entry's and the
// frames the shape the entries are compiled for.  The one place that compares banks; fe_select uses the match where the
// instantiation it chose is the one the entry was compiled with, every other instantiation walks generically.  A
// straight-line walk is correct for every bank with these counts (first bins and band indices stay per-lane records).
int match_walk(const ctu::Design &d, const std::vector<int> &slot_chunk) {
    if (d.wfft != WALK_WFFT || (d.window + 31) / 32 != WALK_NZ) return -1;
    int found = -1;
    for_each_walk([&](auto w) {
        typedef decltype(w) W;
        if (found >= 0 || (int)slot_chunk.size() != W::NS + 1) return;
        for (int s = 0; s <= W::NS; s++)
            if (slot_chunk[s] != W::first(s)) return;
        found = W::index;
    });
    return found;
}

#ifndef CTU_TRAP_BF16
#define CTU_TRAP_BF16 1  // 0: TRAP-DCT on the fp32 matrix pipe only (trapdct_mfma_kernel)
#endif
#ifndef CTU_TRAP_F16
#define CTU_TRAP_F16 1   // 1: two fp16 terms, three products; 0: three bf16 terms, six products (trap_kernel.h)
#endif
// A operands of trapdct_bf16_kernel: G shifted by the frame phase c, zero-padded to 128 taps, each value split into three
// bf16 terms (round to nearest even at every step, as the device splits the data)
void build_trap_bf16(ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const int tl = d.o.fea_trapdct_traplen, nd = d.o.fea_trapdct_ndct, half = (tl - 1) / 2;
    e->trap_bf16 = CTU_TRAP_BF16 && nd <= 16 && half <= TB_OFF && 7 + (TB_OFF - half) + tl <= 128 && d.B <= 24;  // 24 bands: 62 KB of LDS (tile 38 KB + two fragment buffers 24 KB): two workgroups per CU
    if (!e->trap_bf16) return;
    auto rn = [](float v) {
        uint32_t u;
        std::memcpy(&u, &v, 4);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    };
    auto up = [](uint16_t h) {
        uint32_t u = (uint32_t)h << 16;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    const bool f16 = CTU_TRAP_F16;
    const int NT = f16 ? 2 : 3;
    std::vector<uint4> tab((size_t)8 * 4 * NT * 64);
    for (int c = 0; c < 8; c++)
        for (int s_ = 0; s_ < 4; s_++)
            for (int lane = 0; lane < 64; lane++) {
                const int m = lane & 15, q = lane >> 4;
                uint16_t term[3][8];
                for (int i = 0; i < 8; i++) {
                    const int j = 32 * s_ + 8 * q + i - c - (TB_OFF - half);
                    const float v = (m < nd && j >= 0 && j < tl) ? (float)d.trap[(size_t)m * tl + j] : 0.f;
                    if (f16) {
                        const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
                        std::memcpy(&term[0][i], &h, 2);
                        std::memcpy(&term[1][i], &l, 2);
                        term[2][i] = 0;
                    } else {
                        term[0][i] = rn(v);
                        const float r1 = v - up(term[0][i]);
                        term[1][i] = rn(r1);
                        term[2][i] = rn(r1 - up(term[1][i]));
                    }
                }
                for (int sp = 0; sp < NT; sp++) {
                    uint4 w;
                    w.x = term[sp][0] | ((uint32_t)term[sp][1] << 16);
                    w.y = term[sp][2] | ((uint32_t)term[sp][3] << 16);
                    w.z = term[sp][4] | ((uint32_t)term[sp][5] << 16);
                    w.w = term[sp][6] | ((uint32_t)term[sp][7] << 16);
                    tab[(((size_t)c * 4 + s_) * NT + sp) * 64 + lane] = w;
                }
            }
    e->trapG16.upload(tab);
}

void build_big_tables(ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const double pi = 3.14159265358979323846;
    std::vector<float> win(d.hamming.begin(), d.hamming.end());
    e->big_win.upload(win);
    std::vector<float2> tw((size_t)d.wfft / 2);
    for (int m = 0; m < d.wfft / 2; m++) {
        const double a = 2.0 * pi * (double)m / (double)d.wfft;
        tw[m] = make_float2((float)std::cos(a), (float)-std::sin(a));
    }
    e->big_tw.upload(tw);
    std::vector<float> fbw;
    std::vector<int> range((size_t)d.B * 3);
    for (int b = 0; b < d.B; b++) {
        range[3 * b] = d.fb_first[b];
        range[3 * b + 1] = d.fb_last[b];
        range[3 * b + 2] = (int)fbw.size();
        for (int k = d.fb_first[b]; k <= d.fb_last[b]; k++) fbw.push_back((float)d.fb[b][k]);
    }
    e->big_fb_total = (int)fbw.size();
    if (fbw.empty()) fbw.push_back(0.f);
    e->big_fbw.upload(fbw);
    e->big_range.upload(range);
    {
        // wave1k_kernel's bank: the bands' bin runs cut into at most 64 segments of at most S bins (the smallest S that fits)
        std::vector<int> seg(256 + 2 * (size_t)std::max(d.B, 1), 0);
        if (d.B <= 64) {
            int S = 1;
            for (;; S++) {
                int n = 0;
                for (int b = 0; b < d.B; b++) n += std::max(1, (d.fb_last[b] - d.fb_first[b] + 1 + S - 1) / S);
                if (n <= 64) break;
            }
            int lane = 0;
            for (int b = 0; b < d.B; b++) {
                const int w = d.fb_last[b] - d.fb_first[b] + 1, ns = std::max(1, (w + S - 1) / S);
                seg[256 + 2 * b] = lane;
                seg[256 + 2 * b + 1] = ns;
                for (int i = 0; i < ns; i++, lane++) {
                    const int k0 = d.fb_first[b] + i * S, cnt = std::max(0, std::min(S, w - i * S));
                    seg[4 * lane] = b;
                    seg[4 * lane + 1] = k0;
                    seg[4 * lane + 2] = cnt;
                    seg[4 * lane + 3] = range[3 * b + 2] + i * S;
                }
            }
        }
        e->big_seg.upload(seg);
    }
    e->ncoef_out = 0;
    std::vector<float> coef(4, 0.f);
    std::vector<double> coef_d(4, 0.0);
    std::vector<int> slot(4, -1);
    const bool wide = dct_wide(d);  // a band-valued front end, no coefficient rows
    if (d.kind == ctu::FeaKind::Dctc && !wide) {
        // row r of the table is the value written to output slot r (c1..cN, then c0): norm and lifter are in d.dct
        std::vector<int> coef_of_slot(d.nfea, -1);
        int nout = 0;
        for (int i = 0; i < d.nfea; i++)
            if (d.row_slot[i] >= 0) {
                coef_of_slot[d.row_slot[i]] = i;
                nout = std::max(nout, d.row_slot[i] + 1);
            }
        e->ncoef_out = nout;
        coef.assign((size_t)std::max(nout, 1) * d.B, 0.f);
        slot.assign(std::max(nout, 1), -1);
        for (int r = 0; r < nout; r++) {
            slot[r] = coef_of_slot[r];
            if (coef_of_slot[r] >= 0)
                for (int b = 0; b < d.B; b++) coef[(size_t)r * d.B + b] = (float)d.dct[(size_t)coef_of_slot[r] * d.B + b];
        }
    } else if (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) {
        coef_d.assign(d.idft.begin(), d.idft.end());
        slot.assign(d.row_slot.begin(), d.row_slot.end());
        while (slot.size() < (size_t)MAX_LP + 2) slot.push_back(-1);
    }
    e->big_coef.upload(coef);
    e->big_coef_d.upload(coef_d);
    e->big_slot.upload(slot);
    std::vector<float> lif(d.lifter.begin(), d.lifter.end());
    lif.push_back(0.f);
    e->big_lifter.upload(lif);
    e->lds_bytes = 0;
    e->mode = 0;
    // the tables of the 512 / 256-point kernels stay empty
    e->ftab.upload(std::vector<float>(4, 0.f));
    e->itab.upload(std::vector<int>(4, 0));
    e->lanec.upload(std::vector<float>(16 * LANEC, 0.f));
    if (d.kind == ctu::FeaKind::TrapDct) {
        std::vector<float> g(d.trap.begin(), d.trap.end());
        e->trapG.upload(g);
        build_trap_bf16(e);
    }
    switch (d.kind) {
        case ctu::FeaKind::Dctc: e->feat = wide ? FEAT_BANDS : FEAT_DCTC; break;
        case ctu::FeaKind::Lpc:
        case ctu::FeaKind::Lpa: e->feat = FEAT_LP; break;
        default: e->feat = FEAT_BANDS; break;
    }
}

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
std::string fe_name(const FeSel &k) {
    const char *feat = k.feat == FEAT_DCTC ? "DCTC" : k.feat == FEAT_BANDS ? "BANDS" : k.feat == FEAT_LP ? "LP" : "LPD";
    const char *gen = k.gen == GEN_PLAIN ? "plain" : k.gen == GEN_INLD ? "inld" : k.gen == GEN_EXTEN ? "exten" : "full";
    return "frontend_kernel<" + std::to_string(k.nz) + ", " + feat + ", MODE " + std::to_string(k.mode) + ", " + gen + (k.md ? ", MD" : "") + (k.vf ? ", VF" : "") +
           (k.ss ? ", SS" : "") + (k.sy ? ", SY" : "") + ">";
}

// The instantiation a configuration runs on, from the design (after ctu_engine_create has spread an FFT size below 256 onto the 256-point
// mode) and its phase-2 tables (`t`; none with speech output).  Needs no device.  Specialised instantiations (see GEN in
// frontend_kernel.h): the plain chain, plain + intensity-loudness law for the 16-coefficient LP path (PLP), plain + exten for
// 16-coefficient DCT / band outputs; the cepstral ones of these run their DCT tail on the matrix cores (MD, tables laid out for it by
// build_phase2).  Everything else, and every run with the VAD export, reads its flags at run time.
FeSel fe_select(const ctu::Design &d, const Phase2Tables *t) {
    const ctu::Opts &o = d.o;
    FeSel k;
    if (d.wfft >= 1024) return k;
    const bool signal = d.signal_out, exten = o.nr_mode == "exten";
    // ---- what the configuration and its tables fix
    k.mode = d.wfft == 256;
    k.sy = signal && CTU_SY;
    k.ss = ss_eligible(d);
    k.vf = !signal && vf_eligible(d);
    k.md = t && t->md;             // the tables are laid out for the MFMA tail's lane map
    k.nc = t ? t->CW : 16;         // rows of MAXC entries: more than 16 cepstra / LP lags
    if (signal || dct_wide(d) || (d.kind != ctu::FeaKind::Dctc && d.kind != ctu::FeaKind::Lpc && d.kind != ctu::FeaKind::Lpa)) k.feat = FEAT_BANDS;
    else k.feat = d.kind == ctu::FeaKind::Dctc ? FEAT_DCTC : o.fb_inld ? FEAT_LP : FEAT_LPD;
    // rows of samples per lane that can be non-zero.  The 13-row instantiations serve the 25 ms windows (the *ss modes: every window of
    // at most 13 rows - the window table is zero beyond the window); every other window, and -remove_dc1, takes the generic row count
    const int rows = k.mode ? (d.window + 15) / 16 : (d.window + 31) / 32;
    k.nz = (!o.remove_dc1 && (rows == 13 || (k.ss && rows < 13))) ? 13 : 16;
    // the spectra leave the kernel for the VAD kernels (Burg-cepstral and energy criteria) or, in builds without SY, for synth_kernel
    k.vx = (signal && !k.sy) || (o.do_vad() && !k.vf && !signal && (o.vad_cri_mode == "energy" || o.vad_cepdist_mode == "lpc"));
    bool diag = false;
#ifdef CTU_DIAG  // phase ablation (ctu_engine_run: kp.dbg) is a run-time flag
    diag = getenv("CTU_DEBUG_MODE") && atoi(getenv("CTU_DEBUG_MODE")) != 0;
#endif
    // the plain chain: every flag a specialised GEN turns into a constant has its default
    const bool base = !k.vx && !o.fea_E && o.fb_power && o.remove_dc && !o.remove_dc1 && !diag && !signal && !o.nr_when_afterFB;
    const bool lp12 = o.fea_lporder == 12 && o.fea_ncepcoefs == 12 && d.kind != ctu::FeaKind::Lpa;  // the PLP preset exactly: order and number of cepstra fixed at compile time (LPO)
    // ---- GEN and LPO, top to bottom
    k.gen = GEN_FULL;
    if (o.remove_dc1) k.gen = GEN_DC1;  // no spectrum export
    else if (k.sy) {}                   // speech output: no phase 2, the flags at run time
    else if (k.ss) {
        // the straight-line lattices name the window's last sample: the presets' windows, cepstra on the matrix cores or plain band outputs.
        // Energy columns, -fb_inld, -fb_power off, the LP kinds, other windows: the flags at run time
        const bool preset_win = d.window == (k.mode ? VF_WINDOW : VF0_WINDOW);
        if (preset_win && ((k.md && k.feat == FEAT_DCTC) || (k.feat == FEAT_BANDS && base && !o.fb_inld))) {
            k.gen = GEN_PLAIN;
            k.lpo = o.fea_ncepcoefs == 12 ? 12 : 0;  // the detector's order is -fea_ncepcoefs
        }
    }
    else if (k.vf) k.gen = exten ? GEN_EXTEN : GEN_PLAIN;
    else if (k.md && k.feat == FEAT_LP) {  // the compressed-band LP chain: lags by the MFMA tail, the recursions in lp_tail_kernel
        k.gen = GEN_INLD;
        k.lpo = lp12 ? 12 : 0;
    }
    else if (k.md) k.gen = exten ? GEN_EXTEN : GEN_PLAIN;
    else if (k.vx) {}
    else if (base && !o.fb_inld && !exten && k.feat != FEAT_LPD) k.gen = GEN_PLAIN;
    else if (base && o.fb_inld && !exten && k.nc == 16 && k.feat == FEAT_LP) {
        k.gen = GEN_INLD;
        k.lpo = lp12 ? 12 : 0;
    }
    else if (base && !o.fb_inld && exten && k.feat == FEAT_BANDS) k.gen = GEN_EXTEN;
    // ---- the straight-line filter-bank walk, where the bank matches the entry compiled for exactly this instantiation
    if (t) {  // CTU_PHASE2_GENERIC=1: the generic walk for every bank (A/B and identity checks inside one build)
        const char *g = getenv("CTU_PHASE2_GENERIC");
        const int m = (g && atoi(g) != 0) ? -1 : match_walk(d, t->slot_chunk);
        for_each_walk([&](auto w) {
            if (m == w.index && walk_serves<decltype(w)>(k)) k.walk = m;
        });
    }
    // what the eligibility rules (md_eligible, vf_eligible, ss_eligible) promise the tree above: the instantiation exists, and a specialised
    // GEN's constants are the configuration's flags
    const bool flags_ok = k.gen == GEN_FULL || k.gen == GEN_DC1 || (base && o.fb_inld == (k.gen == GEN_INLD) && exten == (k.gen == GEN_EXTEN));
    if (!fe_compiled(k) || !flags_ok) throw std::runtime_error("internal: no front-end instantiation for this configuration (" + fe_name(k) + ")");
    return k;
}

// A operands of dct_wide_kernel (dctw_kernel.h): [chunk][row block][k-step][lane], lane m + 16 k holding row m of the block at band
// 64 chunk + 4 step + k.  Row r of the table is the value written to row column r (c1..cN, then c0): norm and lifter are in d.dct.
void build_dctw(ctu_engine *e) {
    const ctu::Design &d = *e->design;
    std::vector<int> coef_of_slot(d.nfea, -1);
    int nout = 0;
    for (int i = 0; i < d.nfea; i++)
        if (d.row_slot[i] >= 0) {
            coef_of_slot[d.row_slot[i]] = i;
            nout = std::max(nout, d.row_slot[i] + 1);
        }
    if (nout <= 16 || nout > DCTW_MAX) throw std::runtime_error("internal: row width outside dct_wide_kernel's row blocks");
    const int nrb = (nout + 15) / 16, chunks = (d.B + DCTW_KC - 1) / DCTW_KC, KS = DCTW_KC / 4;
    std::vector<float> tab((size_t)chunks * nrb * KS * 64, 0.f);
    for (int c = 0; c < chunks; c++)
        for (int rb = 0; rb < nrb; rb++)
            for (int s_ = 0; s_ < KS; s_++)
                for (int lane = 0; lane < 64; lane++) {
                    const int r = rb * 16 + (lane & 15), b = c * DCTW_KC + 4 * s_ + (lane >> 4);
                    if (r < nout && b < d.B && coef_of_slot[r] >= 0)
                        tab[(((size_t)c * nrb + rb) * KS + s_) * 64 + lane] = (float)d.dct[(size_t)coef_of_slot[r] * d.B + b];
                }
    e->dctw_tab.upload(tab);
    e->dctw_nout = nout;
    e->dctw_chunks = chunks;
}

void build_tables(ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const double pi = 3.14159265358979323846;
    e->big = d.wfft >= 1024;
    e->dctw = dct_wide(d);
    if (e->dctw) build_dctw(e);
    if (e->big) {
        // (-remove_dc1 at 1024 points takes bigfft_kernel<4>, which reads the frames' offsets)
        // (and speech output and the Burg-cepstral VAD criterion: the spectra's export is bigfft_kernel's)
        const bool burg = d.o.do_vad() && d.o.vad_cri_mode == "cepdist" && d.o.vad_cepdist_mode == "lpc";
        const bool wave1k = d.wfft == 1024 && !d.o.remove_dc1 && !d.signal_out && !burg && !(getenv("CTU_WAVE1K") && atoi(getenv("CTU_WAVE1K")) == 0);
        build_big_tables(e);
        e->ss = ss_big_eligible(d) ? ss_mode_of(d.o) : 0;
        e->ss_file = e->ss && d.o.vadmode == "file";
        e->path = wave1k ? BIG_WAVE1K : e->ss ? BIG_SS : BIG_FFT;
        if (e->ss && !e->ss_file) {
            // Hann window of the detector, han[i] = 0.5 (1 - cos(2 * 3.141592653 / window * i)) (src/vdet/CepstralDet.h:133-136)
            std::vector<double> han((size_t)d.window);
            const double m = 2 * 3.141592653 / d.window;
            for (int i = 0; i < d.window; i++) han[(size_t)i] = 0.5 * (1 - std::cos(m * i));
            e->big_han.upload(han);
        }
        return;
    }
    // ---- the 512 / 256-point front end: the phase-2 tables (none with speech output), then the instantiation, then what follows from it
    Phase2Tables t;
    if (!d.signal_out) {
        build_phase2(d, t);
        if (check_phase2(d, t) != 0.0) throw std::runtime_error("internal: phase-2 chunk tables do not reproduce the filter bank");
    }
    const FeSel k = e->sel = fe_select(d, d.signal_out ? nullptr : &t);
    e->mode = k.mode;
    e->feat = k.feat;
    e->md = k.md;
    e->vf = k.vf;
    e->sy = k.sy;
    e->ss = k.ss ? ss_mode_of(d.o) : 0;
    e->ss_file = e->ss && d.o.vadmode == "file";
    // The DUAL instantiations (frontend_kernel.h: the plain chain, with or without the intensity-loudness law) take their window scaled by 1/2: the packed transform's untangle owes the
    // power spectrum a factor 1/4, and a power of two on the window goes through every rounding of the chain unchanged - the rows are
    // bit for bit those of 0.25f * (re^2 + im^2), two multiplications per bin pair cheaper.
    const float wscale = fe_dual(k.nz, k.mode, k.vx, k.gen, k.vf, k.ss, k.sy) ? 0.5f : 1.f;
    // ---- per-lane constant records (see LC_* above)
    const bool mode1 = k.mode == 1;
    std::vector<float> lc(16 * LANEC, 0.f);
    for (int l = 0; l < 16; l++) {
        float *r = lc.data() + l * LANEC;
        for (int j = 0; j < 16; j++)
            for (int h = 0; h < 2; h++) {
                // MODE 0: lane l holds samples 32j+2l, +1 of row j; MODE 1: sample 16j+l (second slot unused)
                const int i = mode1 ? (h ? d.window : 16 * j + l) : 32 * j + 2 * l + h;
                r[LC_WIN + 2 * j + h] = i < d.window ? (float)d.hamming[i] * wscale : 0.f;
                r[LC_MASK + 2 * j + h] = i < d.window ? 1.f : 0.f;
            }
        for (int k1 = 1; k1 < 16; k1++) {
            const double a = -2 * pi * (double)(k1 * l) / 256.0;
            r[LC_TW + 2 * (k1 - 1)] = (float)std::cos(a);
            r[LC_TW + 2 * (k1 - 1) + 1] = (float)std::sin(a);
        }
        for (int k2 = 0; k2 < 8; k2++) {
            const double a = -2 * pi * (double)(l + 16 * k2) / 512.0;
            r[LC_UT + 2 * k2] = (float)std::cos(a);
            r[LC_UT + 2 * k2 + 1] = (float)std::sin(a);
        }
    }
    e->lanec.upload(lc);
    if (d.signal_out) {  // nothing is projected: empty table area
        e->ncoef_out = 0; e->ck_off = 0; e->cf_off = 0; e->tab_floats = 0; e->NS = 0; e->CW = 16; e->lift_off = 0;
        e->ftab.upload(std::vector<float>(4, 0.f));
        e->itab.upload(std::vector<int>(4, 0));
        if (e->ss) {  // the detector's Hann window is the only table (as build_phase2 lays it out for the feature path)
            std::vector<float> ft;
            const double m = 2 * 3.141592653 / d.window;
            for (int i = 0; i < 16 * (d.wfft == 512 ? VF0_SPL : VF_SPL); i++) ft.push_back(i < d.window ? (float)(0.5 * (1 - std::cos(m * i))) : 0.f);
            e->han_off = 0;
            e->tab_floats = (int)ft.size();
            ft.push_back(0.f);  // (where the lifter sits on the feature path)
            e->lift_off = e->tab_floats;
            e->ftab.upload(ft);
        }
    } else {
        e->ncoef_out = t.ncoef_out;
        e->ck_off = t.ck_off;
        e->cf_off = t.cf_off;
        e->cfd_off = t.cfd_off;
        e->am_off = t.am_off;
        e->han_off = t.han_off;
        e->tab_floats = t.tab_floats;
        e->NS = t.NS;
        e->CW = t.CW;
        e->lift_off = t.lift_off;
        e->ftab.upload(t.ft);
        e->itab.upload(t.it);
        if (d.kind == ctu::FeaKind::TrapDct) {
            std::vector<float> g(d.trap.begin(), d.trap.end());
            e->trapG.upload(g);
            build_trap_bf16(e);
        }
    }
    e->lds_bytes = ((size_t)TILE * PSTRIDE + e->tab_floats + LTW_FLOATS + (d.o.nr_when_afterFB ? NWAVE * 128 : 0) +
                    ((k.vf || k.ss) && !k.mode ? NWAVE * VF0_STAGE : 0)) * sizeof(float);  // 512-point detector paths: staged frames per wave
    if (e->lds_bytes > 160 * 1024) throw std::runtime_error("configuration needs more than 160 KiB of LDS");
}

// Kernels whose dynamic LDS may pass the 64 KiB default: the 160 KiB attribute is set once per engine (= per device) and instantiation.
template <class K>
void allow_big_lds(ctu_engine *e, K kern) {
    const void *fp = reinterpret_cast<const void *>(kern);
    if (!e->attr_done.count(fp)) {
        HIP_TRY(hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        e->attr_done.insert(fp);
    }
}
// One front-end launch.
template <class K>
void launch_fe(ctu_engine *e, K kern, dim3 grid, hipStream_t s, const KParams &kp) {
    allow_big_lds(e, kern);
    hipLaunchKernelGGL(kern, grid, dim3(WG), e->lds_bytes, s, kp);
}

// f(integral_constant<int, C>) for the C that v equals
template <int... C, class F>
void lift(int v, F &&f) {
    (void)((v == C && (f(std::integral_constant<int, C>{}), true)) || ...);
}
// The front-end launch of an engine: its FeSel lifted to template arguments, one at a time; fe_compiled decides which leaves exist.
// `xs`: the launch of a stream set with noise state (frontend_kernel<..., XS>; the generic walk: the same rows bit for bit).
// (with detector state as well: the fused Burg-cepstral criterion behind exten, C4's front end - its cepstra go to the scratch by frame, nothing of it runs along a file)
constexpr bool fe_streamed(const FeSel &k) { return !k.vx && !k.ss && !k.sy && (k.gen == GEN_EXTEN || (k.gen == GEN_FULL && !k.vf)); }
void launch_frontend(ctu_engine *e, dim3 grid, hipStream_t s, const KParams &kp, bool xs = false) {
    const FeSel &k = e->sel;
#define V(x) decltype(x)::value
    lift<13, 16>(k.nz, [&](auto NZ) {
    lift<FEAT_BANDS, FEAT_DCTC, FEAT_LP, FEAT_LPD>(k.feat, [&](auto FEAT) {
    lift<0, 1>(k.mode, [&](auto MODE) {
    lift<0, 1>(k.vx, [&](auto VX) {
    lift<16, MAXC>(k.nc, [&](auto NC) {
    lift<GEN_PLAIN, GEN_INLD, GEN_EXTEN, GEN_FULL, GEN_DC1>(k.gen, [&](auto GEN) {
    lift<0, 12>(k.lpo, [&](auto LPO) {
    lift<0, 1>(k.md, [&](auto MD) {
    lift<0, 1>(k.vf, [&](auto VF) {
    lift<0, 1>(k.ss, [&](auto SS) {
    lift<0, 1>(k.sy, [&](auto SY) {
        constexpr FeSel K{V(NZ), V(FEAT), V(MODE), V(VX) != 0, V(NC), V(GEN), V(LPO), V(MD) != 0, V(VF) != 0, V(SS) != 0, V(SY) != 0, -1};
        if constexpr (fe_compiled(K) && fe_streamed(K)) {
            if (xs) {
                launch_fe(e, &frontend_kernel<K.nz, K.feat, K.mode, K.vx, K.nc, K.gen, K.lpo, K.md, K.vf, K.ss, K.sy, walk_generic, true>, grid, s, kp);
                return;
            }
        }
        if constexpr (fe_compiled(K)) {
            if (xs) throw std::runtime_error("internal: no streamed front-end instantiation for this configuration (" + fe_name(K) + ")");
            bool walked = false;
            for_each_walk([&](auto w) {
                typedef decltype(w) W;
                if constexpr (walk_serves<W>(K)) {
                    if (k.walk == W::index) {
                        launch_fe(e, &frontend_kernel<K.nz, K.feat, K.mode, K.vx, K.nc, K.gen, K.lpo, K.md, K.vf, K.ss, K.sy, W>, grid, s, kp);
                        walked = true;
                    }
                }
            });
            if (!walked) launch_fe(e, &frontend_kernel<K.nz, K.feat, K.mode, K.vx, K.nc, K.gen, K.lpo, K.md, K.vf, K.ss, K.sy>, grid, s, kp);
        }
    }); }); }); }); }); }); }); }); }); }); });
#undef V
    e->walk_launched = xs ? -1 : k.walk;
}
// A launch with dynamic LDS: past the 64 KiB default the instantiation's limit is raised first.
template <class K, class... A>
void launch_lds(ctu_engine *e, K kern, dim3 grid, dim3 block, size_t shm, hipStream_t s, const A &...args) {
    if (shm > 64 * 1024) allow_big_lds(e, kern);
    hipLaunchKernelGGL(kern, grid, block, shm, s, args...);
}

// ---- what ctu_plan_create allocates for and the runs launch by, one name each
// The LP kinds' recursions run in lp_tail_kernel, on the lags the front end or wave1k_kernel left (bigfft_kernel and bigss_kernel finish the LP
// analysis themselves; nothing is projected with speech output)
bool lp_tail_runs(const ctu_engine *e) { return (e->feat == FEAT_LP || e->feat == FEAT_LPD) && (!e->big || e->path == BIG_WAVE1K) && !e->design->signal_out; }
// its lags are double: LP analysis on uncompressed band energies, and wave1k_kernel's lags
bool lags_double(const ctu_engine *e) { return e->feat == FEAT_LPD || e->big; }
// hwss / fwss / 2fwss with speech output at 2048 / 4096 points: the synthesis reads the subtracted magnitudes (pss), pnr stays as exported
bool synth_reads_pss(const ctu_engine *e) { return e->big && e->ss && e->design->signal_out; }
// NIT of the large-FFT kernels (samples per thread of a workgroup's 256): 4, 8 or 16
int big_nit(const ctu_engine *e) { return e->design->wfft / 256; }

// The parameter block of the 256 / 512-point front end as far as design and tables fix it (after build_tables and e->vp).
KParams engine_kparams(const ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const bool signal = d.signal_out;
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    kp.band_log = d.kind != ctu::FeaKind::Spec;
    kp.band_to_scratch = d.kind == ctu::FeaKind::TrapDct ? 1 : e->dctw ? 2 : 0;  // 2: the bands to the scratch, the energy column (-fea_E) to its slot of the row
    kp.lp_is_lpa = d.kind == ctu::FeaKind::Lpa;
    kp.syn_scale = 1.0f / (float)d.wfft;
    kp.vad_export = (signal && !e->sy) ? 1 : ((!e->do_vad || e->vf || signal) ? 0 : (e->vp.cri == 1 ? 1 : (e->vp.cri == 0 ? 2 : 0)));
    kp.vad_nc = e->vp.ncoef;
    kp.ss_mode = e->ss; kp.ss_init = d.o.nr_initsegs; kp.ss_nc = d.o.fea_ncepcoefs; kp.han_off = e->han_off;
    kp.nr_b = (float)d.o.nr_b; kp.ss_q = d.o.nr_q;
    kp.skip_phase2 = signal ? 1 : 0;
    kp.lanec = e->lanec.p; kp.ftab = e->ftab.p; kp.itab = e->itab.p;
    kp.tab_floats = e->tab_floats; kp.ck_off = e->ck_off; kp.cf_off = e->cf_off; kp.cfd_off = e->cfd_off; kp.am_off = e->am_off;
    kp.NS = e->NS; kp.CW = e->CW; kp.ncoef_out = e->ncoef_out; kp.lift_off = e->lift_off;
    kp.K = d.K; kp.window = d.window; kp.wshift = d.wshift; kp.B = d.B; kp.nfea = d.nfea; kp.D = d.Dbase;
    kp.e_slot = d.e_slot;
    if (d.o.fea_E && !signal) {  // energy routing of src/io/batch.cc:98-119
        if (d.o.fea_rawenergy) kp.e_mode = 4;
        else if (d.kind == ctu::FeaKind::Dctc) kp.e_mode = d.o.nr_when_afterFB ? 5 : 1;
        else if (d.kind == ctu::FeaKind::Lpc || d.kind == ctu::FeaKind::Lpa) kp.e_mode = 2;
        else kp.e_mode = 3;
    }
    kp.ncep = d.o.fea_ncepcoefs; kp.lporder = d.o.fea_lporder; kp.lp_stride = d.o.fea_lporder + 1;
    kp.preem = d.o.preem; kp.inv_window = 1.0f / (float)d.window; kp.inv_window_d = 1.0 / (double)d.window;
    kp.remove_dc = d.o.remove_dc; kp.kstride = e->kstride;
    kp.remove_dc1 = d.o.remove_dc1 ? 1 : 0; kp.dc1_J = d.window / d.wshift;
    kp.fb_power = d.o.fb_power; kp.fb_inld = d.o.fb_inld; kp.lifter_on = d.o.fea_lifter > 1;
    kp.nr_exten = d.o.nr_mode == "exten"; kp.nr_after_fb = d.o.nr_when_afterFB ? 1 : 0;
    kp.nr_p = (float)d.o.nr_p; kp.nr_p_d = d.o.nr_p; kp.nr_a = (float)d.o.nr_a;
    kp.per_wave = e->per_wave ? 1 : 0;
    return kp;
}
// ... and of the large-FFT kernels, from the block above
BigParams engine_bigparams(const ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const KParams &kp = e->kp0;
    BigParams bp;
    std::memset(&bp, 0, sizeof bp);
    bp.win = e->big_win.p; bp.tw = e->big_tw.p; bp.fbw = e->big_fbw.p; bp.fb_range = e->big_range.p;
    bp.coef = e->big_coef.p; bp.coef_d = e->big_coef_d.p; bp.lifter = e->big_lifter.p; bp.row_slot = e->big_slot.p;
    bp.wfft = d.wfft; bp.K = d.K; bp.window = d.window; bp.wshift = d.wshift; bp.B = d.B; bp.D = kp.D;
    bp.ncoef_out = e->ncoef_out; bp.feat = e->feat; bp.e_mode = kp.e_mode; bp.e_slot = kp.e_slot;
    bp.remove_dc = kp.remove_dc; bp.fb_power = kp.fb_power; bp.fb_inld = kp.fb_inld; bp.band_log = kp.band_log;
    bp.band_to_scratch = kp.band_to_scratch; bp.lp_is_lpa = kp.lp_is_lpa; bp.lporder = kp.lporder; bp.ncep = kp.ncep;
    bp.lifter_on = kp.lifter_on; bp.preem = kp.preem;
    bp.fb_total = e->big_fb_total;
    bp.seg = e->big_seg.p;
    bp.nr_exten = kp.nr_exten; bp.nr_p = kp.nr_p; bp.nr_a = kp.nr_a;
    bp.dc1_J = kp.dc1_J;
    bp.xri_only = d.signal_out ? 1 : 0;
    if (e->ss) {
        bp.ss_mode = e->ss; bp.ss_init = d.o.nr_initsegs; bp.ss_a = d.o.nr_a; bp.ss_b = d.o.nr_b; bp.ss_p = d.o.nr_p;
    }
    return bp;
}
// A run's blocks: the engine's, with the caller's buffers and the plan's scratch.
KParams run_kparams(const ctu_engine *e, const ctu_plan *pl, const RunExtent &x, const int16_t *d_pcm, float *d_rows) {
    const ctu::Design &d = *e->design;
    KParams kp = e->kp0;
    kp.pcm = d_pcm;
    kp.rows = (d.post_order > 0 || d.cms) ? pl->base_rows.p : d_rows;
    kp.logmel = pl->logmel.p; kp.xri = pl->xri.p; kp.pnr = pl->pnr.p; kp.ybuf = pl->ybuf.p;
    kp.vad_ci = pl->vad_ci.p; kp.vad_cf = pl->vad_cf.p; kp.lp_r = pl->lp_r.p; kp.dc1 = pl->dc1.p;
    kp.tiles = pl->tiles.p; kp.wg_first = x.heads; kp.tile_utt = pl->tile_utt.p;
    kp.xstate = x.xstate;
    kp.ss_seed = pl->ss_seed.p; kp.ss_last = pl->ss_last.p; kp.ss_dirty = pl->ss_dirty.p; kp.ss_vbits = pl->ss_vbits.p;
#ifdef CTU_DIAG  // phase ablation (1 = phase 1 only, 2 = phase 2 only): diagnostic builds only
    kp.dbg = getenv("CTU_DEBUG_MODE") ? atoi(getenv("CTU_DEBUG_MODE")) : 0;
#endif
    return kp;
}
BigParams run_bigparams(const ctu_engine *e, const ctu_plan *pl, const RunExtent &x, const KParams &kp) {
    BigParams bp = e->bp0;
    bp.pcm = kp.pcm; bp.rows = kp.rows; bp.logmel = kp.logmel; bp.tiles = pl->tiles.p; bp.n_tiles = x.n_tiles;
    bp.chain_first = x.heads; bp.n_chains = (int)pl->wg_first.n;  // (the count is the plan's: no stream set runs chains on the large-FFT kernels)
    bp.vad_en = (e->do_vad && e->vp.cri == 0) ? pl->pnr.p : nullptr;
    bp.dc1 = pl->dc1.p;
    // the spectra leave bigfft_kernel for bigsynth_kernel, bigburg_kernel (which reads them; the rows are projected as well) or bigss_kernel
    const bool exported = e->design->signal_out || (e->do_vad && e->vp.cri == 1) || e->ss;
    bp.xri = exported ? pl->xri.p : nullptr; bp.pnr = exported ? pl->pnr.p : nullptr;
    bp.pss = pl->pss.p;
    bp.ss_seed = pl->ss_seed.p; bp.ss_last = pl->ss_last.p; bp.ss_dirty = pl->ss_dirty.p; bp.ss_vbits = pl->ss_vbits.p; bp.tile_utt = pl->tile_utt.p;
    return bp;
}

// ------------------------------------------------------------------------------------------------
// the stages of a run, in ctu_engine_run's order
// ------------------------------------------------------------------------------------------------
// -remove_dc1: the frames' means, then the offsets the frames subtract (decode_kernels.h)
void stage_dc1(const ctu_engine *e, const ctu_plan *pl, hipStream_t s, const int16_t *d_pcm) {
    const ctu::Design &d = *e->design;
    const int gx = std::max(1, std::min((pl->max_frames + 3) / 4, 64));
    hipLaunchKernelGGL(dc1_means_kernel, dim3(gx, pl->n_utt), dim3(256), 0, s, d_pcm, pl->utt_info.p, pl->d_sample_off.p, pl->dc1m.p, pl->n_utt, d.window, d.wshift);
    hipLaunchKernelGGL(dc1_offsets_kernel, dim3((pl->n_utt + 63) / 64), dim3(64), 0, s, pl->dc1m.p, pl->utt_info.p, pl->dc1.p, pl->n_utt, d.window, d.wshift);
}

// bigfft_kernel: a workgroup per frame over the tile list, as many as fit the chip at once; with exten one workgroup per chain of utterances
void launch_bigfft(ctu_engine *e, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const LdsFit fit = bigfft_lds(*e->design, e->feat, e->ncoef_out, e->big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the large-FFT kernel");
    if (bp.nr_exten && !e->per_wave) throw std::runtime_error("internal: exten without chains");
    const dim3 g((unsigned)std::max(1, bp.nr_exten ? bp.n_chains : std::min(x.n_tiles, e->n_cu * fit.per_cu)));
    lift<4, 8, 16>(big_nit(e), [&](auto nit) {
        constexpr int NIT = decltype(nit)::value;
        if (bp.nr_exten) launch_lds(e, &bigfft_kernel<NIT, true>, g, dim3(256), fit.bytes, s, bp);
        else launch_lds(e, &bigfft_kernel<NIT>, g, dim3(256), fit.bytes, s, bp);
    });
}
// 1024 points: one wave per frame, the transform in registers (wave1k_kernel.h); tiles are dealt to waves
void stage_wave1k(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const ctu::Design &d = *e->design;
    const LdsFit fit = wave1k_lds(d, e->feat, e->ncoef_out, e->big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the 1024-point kernel");
    if (bp.nr_exten && !e->per_wave) throw std::runtime_error("internal: exten without per-wave chains");
    // exten: one wave per chain of utterances, every chain gets its wave whatever fits the chip at once
    const int wg = bp.nr_exten ? std::max(1, (bp.n_chains + W1K_WAVES - 1) / W1K_WAVES)
                               : std::max(1, std::min((x.n_tiles + W1K_WAVES - 1) / W1K_WAVES, e->n_cu * fit.per_cu));
    lift<0, 1>(bp.nr_exten, [&](auto ex) {
        launch_lds(e, &wave1k_kernel<decltype(ex)::value != 0>, dim3(wg), dim3(64 * W1K_WAVES), fit.bytes, s, bp, (void *)pl->lp_r.p, d.o.fea_lporder + 1);
    });
}
// hwss / fwss / 2fwss at 2048 / 4096 points (bigss_kernel.h): the spectra once (bigfft_kernel with the export on and the projection off),
// the detector's cepstra and decisions once; returns the launch of bigss_kernel, one pass of the seed iteration (run_ss_chain)
std::function<void()> stage_bigss_front(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const ctu::Design &d = *e->design;
    if (d.wfft != 2048 && d.wfft != 4096) throw std::runtime_error("internal: SS engine without an SS instantiation");
    BigParams xp = bp;
    xp.xri_only = 1;
    launch_bigfft(e, x, s, xp);
    HIP_TRY(hipGetLastError());
    if (!e->ss_file) {
        const LdsFit fit = bigburg_lds(d.wfft);
        const dim3 bg((unsigned)std::min<int64_t>(x.total_frames, (int64_t)e->n_cu * fit.per_cu));
        const int nc = d.o.fea_ncepcoefs, two = e->ss == 3;
        lift<8, 16>(big_nit(e), [&](auto nit) {
            lift<16, 32>(nc <= 16 ? 16 : 32, [&](auto cap) {
                launch_lds(e, &bigssdet_kernel<decltype(nit)::value, decltype(cap)::value>, bg, dim3(256), fit.bytes, s, pl->xri.p, pl->pnr.p, pl->vad_ci.p, d.wfft,
                           d.window, nc, (int64_t)x.total_frames, e->big_tw.p, e->big_han.p, (float)d.o.nr_a, two);
            });
        });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ss_decide_kernel, dim3((unsigned)pl->n_utt), dim3(64), 0, s, pl->vad_ci.p, pl->d_row_off.p, pl->n_utt, nc, d.o.nr_initsegs,
                           (double)d.o.nr_p, (double)d.o.nr_q, pl->ss_vbits.p);
        HIP_TRY(hipGetLastError());
    }
    const LdsFit fit = bigss_lds(d, e->feat, e->ncoef_out, e->big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the large-FFT kernel");
    if (!e->per_wave) throw std::runtime_error("internal: hwss / fwss / 2fwss without chains");
    return [e, s, &bp, shm = fit.bytes] {
        lift<8, 16>(big_nit(e), [&](auto nit) {
            launch_lds(e, &bigss_kernel<decltype(nit)::value>, dim3((unsigned)std::max(1, bp.n_chains)), dim3(256), shm, s, bp);
        });
    };
}

// hwss / fwss / 2fwss: a file's noise estimate starts from the vector the previous file of the list left
// behind (src/nr/nr.cc:212-221), which chains the whole list.  Everything but that seed is independent per
// file, so the list is run with the seeds known so far until they stop changing: pass j fixes the seeds of
// the first j files for good, and a seed's influence dies out as p^(noise updates), so real lists settle in
// two or three passes.  Synchronous: each pass reads the vectors back.  `pass` launches one pass (the front end on kp, or bigss_kernel).
// CTU_ERR_INPUT, with vad_pos and ss_stale untouched, when the -vad file= stream ends inside the run.
template <class Pass>
int run_ss_chain(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, KParams &kp, Pass &&pass) {
    const ctu::Design &d = *e->design;
    const size_t nk = (size_t)pl->n_utt * d.K;
    std::vector<float> seed(nk, 0.f), last(nk, 0.f), next(nk, 0.f);
    if (e->ss_stale.size() != (size_t)d.K) e->ss_stale.assign(d.K, 0.f);
    // new_file() seeds the estimate from the vector and then scales the vector by 0.1 (nr.cc:217-220, 402-407); a
    // file with a frame overwrites it in its first get_frame(), a file without one (window - wshift <= N < window)
    // leaves it scaled.  So file i starts from what the last file with a frame ahead of it left - or, ahead of the
    // first such file, what the previous run left (the reference keeps the vector for the life of the process,
    // base/types.h:35-38) - times 0.1 for every frameless file in between.
    auto scaled = [&](float *dst, const float *src, int skipped) {
        double f = 1.0;
        for (int z = 0; z < skipped; z++) f *= 0.1;
        for (int k = 0; k < d.K; k++) dst[k] = (float)((double)src[k] * f);
    };
    auto propagate = [&](std::vector<float> &dst) {  // seeds of every file from `last` (files with frames) and e->ss_stale
        int prev = -1, skipped = 0;
        for (int i = 0; i < pl->n_utt; i++) {
            scaled(&dst[(size_t)i * d.K], prev >= 0 ? &last[(size_t)prev * d.K] : e->ss_stale.data(), skipped);
            if (pl->frames[i] > 0) {
                prev = i;
                skipped = 0;
            } else
                skipped++;
        }
        return std::make_pair(prev, skipped);
    };
    propagate(seed);  // `last` is still zero: only the seeds ahead of the first file with a frame are final
    // An utterance's rows and last vector depend on its samples and its seed only: a pass recomputes just the utterances
    // whose seed changed since the pass before (all of them in the first one).
    std::vector<unsigned char> dirty(std::max(pl->n_utt, 1), 1);
    if (e->ss_file) {
        // -vad file=<f>: `char vad = fgetc(fvad); if (vad != EOF) return bool(vad); else throw` (nr.cc:297-302), one byte per frame in
        // list order, the stream running on from file to file and from run to run.  Every byte but NUL is speech; a byte 0xFF
        // compares equal to EOF in the reference's (signed) char and ends the run like the end of the file does.
        const int64_t nf = x.total_frames;
        std::vector<unsigned char> vb((size_t)std::max<int64_t>(nf, 1), 0);
        for (int64_t i = 0; i < nf; i++) {
            if (e->vad_pos + i >= (int64_t)e->vad_stream.size() || e->vad_stream[(size_t)(e->vad_pos + i)] == 0xFF) {
                set_error(e, "NR: Unexpected end of VAD file!");
                return CTU_ERR_INPUT;
            }
            vb[(size_t)i] = e->vad_stream[(size_t)(e->vad_pos + i)] != 0;
        }
        HIP_TRY(hipMemcpyAsync(pl->ss_vbits.p, vb.data(), (size_t)nf, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));  // vb leaves scope
        e->vad_pos += nf;
    }
    for (int iter = 0;; iter++) {
        // the detector never sees a subtracted spectrum (nr.cc:278-295): its decisions are those of the first pass
        kp.ss_cached = e->ss_file ? 1 : (iter > 0 ? CTU_SS_CACHE : 0);
        HIP_TRY(hipMemcpyAsync(pl->ss_seed.p, seed.data(), nk * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(pl->ss_dirty.p, dirty.data(), dirty.size(), hipMemcpyHostToDevice, s));
        pass();
        HIP_TRY(hipMemcpyAsync(last.data(), pl->ss_last.p, nk * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        propagate(next);
        bool any = false;
        for (int i = 0; i < pl->n_utt; i++) {
            dirty[i] = std::memcmp(&next[(size_t)i * d.K], &seed[(size_t)i * d.K], d.K * sizeof(float)) != 0;
            any = any || dirty[i];
        }
        if (!any) break;
        if (iter > pl->n_utt) throw std::runtime_error("internal: noise seeds of the *ss chain did not settle");
        seed = next;
    }
    // what this run leaves for the next one
    const auto tail = propagate(next);
    std::vector<float> keep(d.K);
    scaled(keep.data(), tail.first >= 0 ? &last[(size_t)tail.first * d.K] : e->ss_stale.data(), tail.second);
    e->ss_stale = keep;
    return CTU_OK;
}

// Levinson-Durbin and a -> c on the lags the front end or wave1k_kernel left, one frame per lane (lp_tail_kernel.h)
void stage_lp_tail(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const KParams &kp) {
    LpTailParams tp;
    tp.lags = pl->lp_r.p; tp.rows = kp.rows; tp.total_frames = x.total_frames;
    tp.lifter = e->big ? e->big_lifter.p : e->ftab.p + e->lift_off;
    tp.row_slot = e->big ? e->big_slot.p : e->itab.p + e->NS + 1;
    tp.stride = kp.lp_stride; tp.D = kp.D; tp.lporder = kp.lporder; tp.ncep = kp.ncep; tp.is_lpa = kp.lp_is_lpa;
    tp.lifter_on = kp.lifter_on; tp.e_mode = kp.e_mode; tp.e_slot = kp.e_slot;
    tp.inv_stride = (unsigned)((1ull << 32) / (unsigned)tp.stride) + 1u;
    tp.inv_D = (unsigned)((1ull << 32) / (unsigned)tp.D) + 1u;
    const LdsFit fit = lp_tail_lds(tp.stride, tp.D, lags_double(e));
    const dim3 tg((unsigned)std::max<int64_t>(1, std::min<int64_t>((x.total_frames + 255) / 256, (int64_t)e->n_cu * fit.per_cu)));
    if (lags_double(e)) launch_lds(e, &lp_tail_kernel<double, 0>, tg, dim3(256), fit.bytes, s, tp);
    else if (kp.lporder == 12 && kp.ncep == 12 && !kp.lp_is_lpa) launch_lds(e, &lp_tail_kernel<float, 12>, tg, dim3(256), fit.bytes, s, tp);
    else launch_lds(e, &lp_tail_kernel<float, 0>, tg, dim3(256), fit.bytes, s, tp);
    HIP_TRY(hipGetLastError());
}

// The VAD's Burg-cepstral criterion outside the fused path, on the spectra the front end exported: bigburg_kernel at 1024 .. 4096 points
// (a workgroup per frame), vad_burg_kernel below (a wave per frame; Q samples per lane: windows of up to 256 samples, or longer)
void stage_burg_vad(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s) {
    const ctu::Design &d = *e->design;
    const int cap = e->vp.ncoef <= 16 ? 16 : 32;
    if (e->vp.cri == 1 && e->big && x.total_frames > 0) {
        const LdsFit fit = bigburg_lds(d.wfft);
        const dim3 g((unsigned)std::min<int64_t>(x.total_frames, (int64_t)e->n_cu * fit.per_cu));
        lift<4, 8, 16>(big_nit(e), [&](auto nit) {
            lift<16, 32>(cap, [&](auto nc) {
                launch_lds(e, &bigburg_kernel<decltype(nit)::value, decltype(nc)::value>, g, dim3(256), fit.bytes, s, pl->xri.p, pl->pnr.p, pl->vad_ci.p, e->vp,
                           (int64_t)x.total_frames, e->big_tw.p);
            });
        });
    } else if (e->vp.cri == 1 && !e->vf && !e->big) {
        const dim3 g((unsigned)std::min<int64_t>((x.total_frames + 3) / 4, (int64_t)e->n_cu * 4));
        const size_t bshm = (512 + (size_t)4 * 2 * (d.wfft / 2 + 4)) * 2 * sizeof(vreal);
        lift<4, 8>(d.window <= 256 ? 4 : 8, [&](auto q) {
            lift<16, 32>(cap, [&](auto nc) {
                hipLaunchKernelGGL((vad_burg_kernel<decltype(q)::value, decltype(nc)::value>), g, dim3(256), bshm, s, pl->xri.p, pl->pnr.p, pl->vad_ci.p, e->vp,
                                   x.total_frames);
            });
        });
    }
    HIP_TRY(hipGetLastError());
}

// TRAP-DCT over the log-mel rows (trap_kernel.h): the 16-bit matrix pipe where the tables fit it, else fp32 MFMA
void stage_trap(ctu_engine *e, const ctu_plan *pl, hipStream_t s, float *d_rows) {
    const ctu::Design &d = *e->design;
    const int tl = d.o.fea_trapdct_traplen, nd = d.o.fea_trapdct_ndct;
    const int ns = (tl + 3) / 4;
    if (e->trap_bf16) {
        constexpr int NT16 = CTU_TRAP_F16 ? 2 : 3;
        const size_t shm16 = (size_t)NT16 * d.B * TB_TT * 2 + (size_t)((d.B + 3) & ~3) * 4 + 2 * (4 * NT16 * 64) * 16;
        hipLaunchKernelGGL((trapdct_split16_kernel<CTU_TRAP_F16 != 0>), dim3(std::max(pl->n_trap_chunks128, 1)), dim3(512), shm16, s,
                           pl->logmel.p, d_rows, e->trapG16.p, pl->utt_info.p, pl->trap_chunks128.p, pl->n_trap_chunks128, d.B, nd, d.D);
    } else {
        const size_t shm = (size_t)(64 + 4 * (ns <= 26 ? 26 : ns)) * (d.B | 1) * sizeof(float);
        lift<1, 2>(nd <= 16 ? 1 : 2, [&](auto nrb) {
            lift<26, 64>(ns <= 26 ? 26 : 64, [&](auto nsm) {
                hipLaunchKernelGGL((trapdct_mfma_kernel<decltype(nrb)::value, decltype(nsm)::value>), dim3(pl->n_trap_chunks), dim3(256), shm, s, pl->logmel.p, d_rows,
                                   e->trapG.p, pl->utt_info.p, pl->trap_chunks.p, d.B, tl, nd, d.D);
            });
        });
    }
    HIP_TRY(hipGetLastError());
}

// The wide DCT tail (dctw_kernel.h) over the band logarithms the front end left, into the rows the front end would have written
void stage_dctw(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const KParams &kp) {
    DctwParams wp;
    wp.logmel = pl->logmel.p; wp.rows = kp.rows; wp.atab = e->dctw_tab.p; wp.total_frames = x.total_frames;
    wp.B = kp.B; wp.D = kp.D; wp.nout = e->dctw_nout; wp.chunks = e->dctw_chunks;
    wp.n_tiles = (int)((x.total_frames + DCTW_TILE - 1) / DCTW_TILE);
    const dim3 g((unsigned)std::max(1, std::min(wp.n_tiles, e->n_cu * 8)));
    lift<2, 3, 4>((wp.nout + 15) / 16, [&](auto nrb) { hipLaunchKernelGGL(dct_wide_kernel<decltype(nrb)::value>, g, dim3(256), 0, s, wp); });
    HIP_TRY(hipGetLastError());
}

// Delta chain / stacking from the base rows into the caller's rows (post_kernels.h)
// (the parameter block and the LDS bytes are also stream_post_kernel's)
PostParams post_params(const ctu::Design &d, size_t *shm) {
    PostParams pp;
    std::memset(&pp, 0, sizeof pp);
    pp.fea_c = d.o.fea_ncepcoefs + 1; pp.Dbase = d.Dbase; pp.D = d.D;
    pp.order = d.post_order; pp.stack = d.post_stack ? 1 : 0; pp.has_e = d.o.fea_E ? 1 : 0;
    int H = 0;
    for (int j = 0; j < d.post_order; j++) {
        pp.w[j] = d.post_w[j];
        int den = 0;
        for (int i = 1; i <= d.post_w[j]; i++) den += i * i;
        pp.inv_den[j] = (float)(1.0 / (2.0 * den));
        H += d.post_w[j];
    }
    const int R = 64 + 2 * H;
    *shm = ((size_t)R * d.Dbase + (size_t)(d.post_stack ? 0 : d.post_order) * R * pp.fea_c) * sizeof(float);
    if ((size_t)R * d.Dbase > 256 * 12) throw std::runtime_error("delta tile larger than the prefetch registers");
    return pp;
}
void stage_post(ctu_engine *e, const ctu_plan *pl, hipStream_t s, float *d_rows) {
    const ctu::Design &d = *e->design;
    size_t shm = 0;
    const PostParams pp = post_params(d, &shm);
    const int pgrid = std::min(pl->n_trap_chunks, e->n_cu * 8);
    const bool std39 = !d.post_stack && d.post_order == 2 && pp.fea_c == 13 && d.Dbase == 13 && d.D == 39 && pp.w[0] == 2 && pp.w[1] == 2;
    lift<0, 1>(std39, [&](auto v) {
        hipLaunchKernelGGL(post_kernel<decltype(v)::value != 0>, dim3(pgrid), dim3(256), shm, s, pl->base_rows.p, d_rows, pl->utt_info.p, pl->trap_chunks.p, pl->n_trap_chunks, pp);
    });
    HIP_TRY(hipGetLastError());
}

// CMS, exponential or over a block window (post_kernels.h)
CmsParams cms_params(const ctu::Design &d) {
    CmsParams cp;
    std::memset(&cp, 0, sizeof cp);
    cp.ncols = d.cms_cols; cp.Dbase = d.Dbase; cp.D = d.D; cp.copy_rest = d.post_order > 0 ? 0 : 1;
    cp.L = d.o.length_b; cp.z = d.o.fea_Z_exp; cp.omz = 1 - d.o.fea_Z_exp;
    return cp;
}
void stage_cms(ctu_engine *e, const ctu_plan *pl, hipStream_t s, float *d_rows) {
    const ctu::Design &d = *e->design;
    const CmsParams cp = cms_params(d);
    if (d.cms == 1) hipLaunchKernelGGL(cms_exp_kernel, dim3((pl->n_utt + 1) / 2), dim3(64), 0, s, pl->base_rows.p, d_rows, pl->utt_info.p, pl->n_utt, cp);
    else
        hipLaunchKernelGGL(cms_block_kernel, dim3(pl->n_trap_chunks), dim3(256), (size_t)(64 + cp.L - 1) * cp.ncols * sizeof(float), s, pl->base_rows.p, d_rows,
                           pl->utt_info.p, pl->trap_chunks.p, cp);
    HIP_TRY(hipGetLastError());
}

// The fused path left the lattice's output of every frame behind: the coefficient recursion and a -> c one frame per lane,
// then the detector's recurrences, sixteen utterances per wave
void stage_fused_vad(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, uint8_t *d_vad, bool replay) {
    if (CTU_VF_A2C)
        hipLaunchKernelGGL((vad_a2c_kernel<VF_NC>), dim3((unsigned)((x.total_frames + 255) / 256)), dim3(256), 0, s, pl->vad_cf.p, (int64_t)x.total_frames);
    if (replay) lift<0, 1, 2, 3>(e->vp.thr, [&](auto thr) {
        hipLaunchKernelGGL((vad_lanes_kernel<VF_NC, decltype(thr)::value>), dim3((pl->n_live + 15) / 16), dim3(64), 0, s, pl->vad_cf.p, pl->vf_order.p, pl->n_live,
                           pl->d_row_off.p, d_vad, e->vp);
    });
    HIP_TRY(hipGetLastError());
}

// After the post passes: the `fea` criterion reads the vector the writer sees (CMS applied), and the energy
// column is shifted in the finished rows.
void stage_vad_decide(ctu_engine *e, const ctu_plan *pl, hipStream_t s, float *d_rows, uint8_t *d_vad) {
    hipLaunchKernelGGL(vad_decide_kernel, dim3(pl->n_utt), dim3(64), 0, s, pl->vad_ci.p, pl->pnr.p, d_rows, pl->d_row_off.p, pl->n_utt, d_vad, e->vp);
    HIP_TRY(hipGetLastError());
}

// A file with no more frames than the majority filter delays never gets the filter `ready` (src/vad/vad.h:126-136), so
// BATCH::flush_vad's loop does not start (src/vad/vad.cc:742-745, src/io/batch.cc:243-249): the reference writes neither a
// row nor a decision for it.  Its decision bytes become NUL ("nothing written"); ctu_engine_run_host reports 0 rows.
void stage_short_files(ctu_engine *e, const ctu_plan *pl, hipStream_t s, uint8_t *d_vad) {
    hipLaunchKernelGGL(vad_short_files_kernel, dim3((unsigned)((pl->n_utt + 255) / 256)), dim3(256), 0, s, d_vad, pl->d_row_off.p, pl->n_utt,
                       (e->design->o.vad_filter_order - 1) / 2);
    HIP_TRY(hipGetLastError());
}

// The list behaviour of the reference's majority filter (ctu_plan_set_vad_ring): every column but the energy (which does not
// go through the ring, src/io/batch.cc:101-120) of row k := the vector of frame ring_src[k], or zeros
void stage_ring_gather(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, float *d_rows) {
    const ctu::Design &d = *e->design;
    const size_t n = (size_t)x.total_frames * d.D;
    HIP_TRY(hipMemcpyAsync(pl->ring_tmp.p, d_rows, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(vad_ring_gather_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65535u * 16)), dim3(256), 0, s, pl->ring_tmp.p, d_rows,
                       pl->ring_src.p, (int64_t)x.total_frames, d.D, d.o.fea_E ? (d.post_order > 0 ? d.D - 1 : d.e_slot) : -1);
    HIP_TRY(hipGetLastError());
}

// Speech output at 1024 .. 4096 points (ctu_engine_run_signal): a workgroup per frame
void launch_bigsynth(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, float inv_n) {
    const ctu::Design &d = *e->design;
    const LdsFit fit = bigsynth_lds(d.wfft);
    const int g = (int)std::min<int64_t>(x.total_frames, (int64_t)e->n_cu * fit.per_cu);
    lift<4, 8, 16>(big_nit(e), [&](auto nit) {
        launch_lds(e, &bigsynth_kernel<decltype(nit)::value>, dim3(g), dim3(256), fit.bytes, s, pl->xri.p, synth_reads_pss(e) ? pl->pss.p : pl->pnr.p, pl->ybuf.p,
                   (long long)x.total_frames, d.wfft, d.window, inv_n, e->big_tw.p);
    });
    HIP_TRY(hipGetLastError());
}

#if CTU_STAMP
void dump_stamps(ctu_engine *e, int grid, hipStream_t s, const char *sf) {
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(e->stamps.n);
    HIP_TRY(hipMemcpy(h.data(), e->stamps.p, h.size() * 8, hipMemcpyDeviceToHost));
    double sum[16] = {0};
    for (size_t w = 0; w < (size_t)grid * NWAVE; w++)
        for (int i = 0; i < 16; i++) sum[i] += (double)h[w * 16 + i];
    if (FILE *f = fopen(sf, "w")) {
        double tot = 0;
        for (int i = 0; i < 16; i++) tot += sum[i];
        for (int i = 0; i < 16; i++) fprintf(f, "seg %2d  mean cycles per wave %12.0f  share %.3f\n", i, sum[i] / (grid * NWAVE), sum[i] / tot);
        fclose(f);
    }
}
#endif

std::vector<std::string> to_args(int argc, const char *const *argv) {
    std::vector<std::string> a;
    for (int i = 0; i < argc; i++) a.emplace_back(argv[i] ? argv[i] : "");
    return a;
}

// FFT sizes below 256 (windows up to 128 samples): the N-point spectrum of a frame is every (256/N)-th bin of its
// 256-point spectrum, because the frame is zero beyond the window either way.  The engine runs the 256-point mode
// with the filter bank spread onto those bins (zero weight in between); sums over bins step by the stride returned.
int spread_small_fft(ctu::Design &d) {
    if (!(d.wfft < 256 && d.wfft >= 32 && !d.signal_out)) return 1;
    const int S = 256 / d.wfft;
    for (auto &row : d.fb) {
        std::vector<double> wide(129, 0.0);
        for (int k = 0; k < d.K; k++) wide[(size_t)k * S] = row[k];
        row.swap(wide);
    }
    for (int &f : d.fb_first) f *= S;
    for (int &l : d.fb_last) l *= S;
    d.K = 129;
    d.wfft = 256;
    return S;
}

void fill_dims(const ctu::Design &d, ctu_dims *out) {
    out->fs = d.o.fs;
    out->window = d.window;
    out->wshift = d.wshift;
    out->wfft = d.wfft;
    out->nbins = d.K;
    out->nbands = d.B;
    out->row_floats = d.D;
    out->htk_kind = d.htk_kind;
    out->htk_period = d.period;
    out->has_vad = d.o.do_vad() ? 1 : 0;
    out->swap_out = d.o.swap_out ? 1 : 0;
    out->pcm_align = PCM_ALIGN;
    out->signal_out = d.signal_out ? 1 : 0;
    out->rows_in = d.rows_in ? 1 : 0;
    out->row_floats_in = d.rows_in ? d.Dbase : 0;
    out->swap_in = d.o.swap_in ? 1 : 0;
}

}  // namespace

extern "C" {

const char *ctu_create_error(void) { return g_create_error.c_str(); }

int ctu_config_dims(int argc, const char *const *argv, ctu_dims *out) {
    try {
        ctu::Opts o = ctu::Opts::from_args(to_args(argc, argv));
        ctu::Design d(o);
        fill_dims(d, out);
        return CTU_OK;
    } catch (const std::exception &ex) {
        g_create_error = ex.what();
        return CTU_ERR_OPTS;
    }
}

int64_t ctu_config_table(int argc, const char *const *argv, const char *name, double *out, int64_t cap) {
    try {
        ctu::Opts o = ctu::Opts::from_args(to_args(argc, argv));
        ctu::Design d(o);
        std::vector<double> v;
        const std::string n = name ? name : "";
        if (n == "hamming") v = d.hamming;
        else if (n == "fbank") for (const auto &row : d.fb) v.insert(v.end(), row.begin(), row.end());
        else if (n == "fb_first") v.assign(d.fb_first.begin(), d.fb_first.end());
        else if (n == "fb_last") v.assign(d.fb_last.begin(), d.fb_last.end());
        else if (n == "dct") v = d.dct;
        else if (n == "idft") v = d.idft;
        else if (n == "trap") v = d.trap;
        else if (n == "lifter") v = d.lifter;
        else if (n == "phase2_check") {
            Phase2Tables t;
            build_phase2(d, t);
            v = {check_phase2(d, t), (double)t.slot_chunk.back(), (double)t.NS};
        }
        else if (n == "phase2_walk") {  // chunks per slot, then the index of the compiled walk signature (phase2_walks.h) or -1
            Phase2Tables t;
            build_phase2(d, t);
            for (int sl = 0; sl < t.NS; sl++) v.push_back(t.slot_chunk[sl + 1] - t.slot_chunk[sl]);
            v.push_back((double)match_walk(d, t.slot_chunk));
        }
        else if (n == "frontend") {  // the instantiation ctu_engine_create selects: frontend_kernel's template arguments, the walk's index last
            spread_small_fft(d);
            Phase2Tables t;
            if (!d.signal_out && d.wfft < 1024) build_phase2(d, t);
            const FeSel k = fe_select(d, d.signal_out ? nullptr : &t);
            v = {(double)k.nz, (double)k.feat, (double)k.mode, (double)k.vx, (double)k.nc, (double)k.gen, (double)k.lpo, (double)k.md, (double)k.vf,
                 (double)k.ss, (double)k.sy, (double)k.walk};
        }
        else {
            g_create_error = "unknown table name";
            return CTU_ERR_INPUT;
        }
        for (int64_t i = 0; i < (int64_t)v.size() && i < cap; i++) out[i] = v[i];
        return (int64_t)v.size();
    } catch (const std::exception &ex) {
        g_create_error = ex.what();
        return CTU_ERR_OPTS;
    }
}

int ctu_engine_create(int argc, const char *const *argv, int device, ctu_engine **out) {
    if (!out) return CTU_ERR_INPUT;
    *out = nullptr;
    std::unique_ptr<ctu_engine> e(new ctu_engine);
    try {
        ctu::Opts o = ctu::Opts::from_args(to_args(argc, argv));
        e->design.reset(new ctu::Design(o));
        ctu::Design &d = *e->design;
        e->user_wfft = d.wfft;  // what ctu_engine_dims reports: the configuration's own FFT size and bin count (= ctu_config_dims)
        e->user_K = d.K;
        e->kstride = spread_small_fft(d);
    } catch (const std::exception &ex) {
        g_create_error = ex.what();
        return CTU_ERR_OPTS;
    }
    {
        const ctu::Opts &o = e->design->o;
        if (o.do_vad()) {  // constructor checks of src/vad/vad.cc:639-660, :149-195 and src/vad/vad.h:96-99
            const char *bad = nullptr;
            if (o.vad_cri_mode != "energy" && o.vad_cri_mode != "cepdist") bad = "VAD: unknown vad_cri_mode!";
            else if (o.vad_thr_mode != "absolute" && o.vad_thr_mode != "perc" && o.vad_thr_mode != "adapt" && o.vad_thr_mode != "dyn") bad = "VAD: unknown vad_thr_mode!";
            else if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode != "lpc" && o.vad_cepdist_mode != "fea" && o.vad_cepdist_mode != "in") bad = "VADcri_cepdist: unknown vad_cepdist_mode!";
            else if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" && !o.phase_needed) bad = "VADcri_cepdist: cannot perform iFFT!";
            else if (o.vad_filter_order < 1 || o.vad_filter_order % 2 == 0) bad = "medianFilter: filter order must be positive, odd number!";
            if (bad) {
                g_create_error = bad;
                return CTU_ERR_OPTS;
            }
        }
    }
    const std::string why = unsupported_reason(*e->design);
    if (!why.empty()) {
        g_create_error = "ENGINE: configuration not on the accelerated path: " + why;
        return CTU_ERR_UNSUPPORTED;
    }
    if (ss_mode_of(e->design->o) && e->design->o.vadmode == "file") {  // hwssNR::hwssNR opens it (nr.cc:205-209); ctu_engine_set_vad_stream replaces it
        FILE *f = std::fopen(e->design->o.filevad.c_str(), "rb");
        if (!f) {
            g_create_error = "NR: Unable to open VAD file!\n";
            return CTU_ERR_OPTS;
        }
        unsigned char tmp[1 << 16];
        size_t got;
        while ((got = std::fread(tmp, 1, sizeof tmp, f)) > 0) e->vad_stream.insert(e->vad_stream.end(), tmp, tmp + got);
        std::fclose(f);
    }
    try {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw std::runtime_error("no HIP device (the engine has no CPU fallback)");
        if (device < 0 || device >= ndev) throw std::runtime_error("HIP device ordinal out of range");
        HIP_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        e->device = device;
        e->n_cu = prop.multiProcessorCount;
        e->rows_in = e->design->rows_in;
        if (e->rows_in) e->kname = "rows_ingest_kernel";  // no front end: no tables, no parameter blocks
        else build_tables(e.get());
        {
            const ctu::Opts &o = e->design->o;
            const ctu::Design &d = *e->design;
            e->do_vad = o.do_vad();
            e->per_wave = o.nr_mode == "exten" || e->ss;  // state along an utterance (exten, the *ss modes): a wave per chain
            VadParams &vp = e->vp;
            std::memset(&vp, 0, sizeof vp);
            vp.K = d.K; vp.wfft = d.wfft; vp.window = d.window;
            vp.krow = d.K; vp.kstride = e->kstride;
            if (e->kstride > 1) {  // an FFT size below 256 on the 256-point mode: the detector's inverse transform keeps the configuration's size
                vp.K = e->user_K;
                vp.wfft = e->user_wfft;
            }
            vp.cri = o.vad_cri_mode == "energy" ? 0 : (o.vad_cepdist_mode == "lpc" ? 1 : 2);
            vp.ncoef = vp.cri == 1 ? o.vad_lpc_coefs : vad_fea_entries(d);
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
        }
        if (!e->rows_in) e->kp0 = engine_kparams(e.get());
        if (e->big) e->bp0 = engine_bigparams(e.get());
        HIP_TRY(hipEventCreate(&e->ev0));
        HIP_TRY(hipEventCreate(&e->ev1));
    } catch (const std::exception &ex) {
        g_create_error = std::string("ENGINE: ") + ex.what();
        return CTU_ERR_DEVICE;
    }
    *out = e.release();
    return CTU_OK;
}

void ctu_engine_destroy(ctu_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    delete e;
}

const char *ctu_last_error(const ctu_engine *e) { return e ? e->err.c_str() : "null engine"; }

int ctu_engine_dims(const ctu_engine *e, ctu_dims *out) {
    if (!e || !out) return CTU_ERR_INPUT;
    fill_dims(*e->design, out);
    out->wfft = e->user_wfft;
    out->nbins = e->user_K;
    return CTU_OK;
}

int64_t ctu_num_frames(const ctu_engine *e, int64_t n) {
    if (e->rows_in) return n < 0 ? -1 : n;  // the "samples" of a feature file are its rows
    const int pre = e->design->window - e->design->wshift;
    if (n < pre) return -1;
    return (n - pre) / e->design->wshift;
}

int64_t ctu_arena_layout(const int64_t *utt_nsamples, int32_t n_utt, int64_t *sample_off) {
    if (n_utt < 0 || (n_utt && !utt_nsamples)) return CTU_ERR_INPUT;
    int64_t so = PCM_HEAD;
    for (int i = 0; i < n_utt; i++) {
        if (utt_nsamples[i] < 0) return CTU_ERR_INPUT;
        if (sample_off) sample_off[i] = so;
        so += (utt_nsamples[i] + PCM_ALIGN - 1) / PCM_ALIGN * PCM_ALIGN;
    }
    if (sample_off) sample_off[n_utt] = so;
    return so + PCM_TAIL;  // loads run to the end of the last 32-sample row of a frame
}

int64_t ctu_rows_arena_layout(const int64_t *utt_rows, int32_t n_utt, int32_t width, int64_t *word_off) {
    if (n_utt < 0 || width < 1 || (n_utt && !utt_rows)) return CTU_ERR_INPUT;
    int64_t wo = 0;
    for (int i = 0; i < n_utt; i++) {
        if (utt_rows[i] < 0) return CTU_ERR_INPUT;
        if (word_off) word_off[i] = wo;
        wo += (utt_rows[i] * width + ROWS_ALIGN - 1) / ROWS_ALIGN * ROWS_ALIGN;
    }
    if (word_off) word_off[n_utt] = wo;
    return wo;  // rows_ingest_kernel reads an utterance's own words only: no padding around the arena
}

namespace {
// The host side of a plan between the three steps of ctu_plan_create: plan_layout fills it, plan_chains links the tiles, plan_alloc uploads it.
struct PlanHost {
    std::vector<TileRec> tiles;
    std::vector<int> uts;       // first tile of every utterance, n_tiles at the end
    std::vector<int4> uinfo;    // (first row: low, high word; frames; 0) of every utterance
    std::vector<int> chunks;    // (utterance, first frame) of every 64-frame chunk
    std::vector<int> wg_first;  // first tile of every chain (plan_chains)
};

// Step 1, host only, for both kinds of plan: where every utterance sits in the arena and in the rows, the refusals, its tiles and
// 64-frame chunks, the totals.  The two kinds differ in the arena's layout rule, in what a length counts (ctu_num_frames: samples
// against the rows themselves, -format_in htk), in the arena elements between two frames, and in a refusal each.
int plan_layout(ctu_engine *e, ctu_plan *pl, const int64_t *utt_n, int32_t n_utt, PlanHost &h) {
    static_assert(TILE == 64, "the chunk list of the TRAP / delta / CMS / CMVN passes (64 frames per workgroup) is the tile list");
    const ctu::Design &d = *e->design;
    const bool rows = e->rows_in;
    pl->eng = e;
    pl->n_utt = n_utt;
    pl->nsamples.assign(utt_n, utt_n + n_utt);
    pl->sample_off.resize(n_utt + 1);
    pl->row_off.resize(n_utt + 1);
    pl->frames.resize(n_utt);
    pl->total_samples = rows ? ctu_rows_arena_layout(utt_n, n_utt, d.Dbase, pl->sample_off.data()) : ctu_arena_layout(utt_n, n_utt, pl->sample_off.data());
    if (pl->total_samples < 0) {
        set_error(e, "ENGINE: negative utterance length");
        return CTU_ERR_INPUT;
    }
    const int64_t stride = rows ? d.Dbase : d.wshift;  // arena elements from one frame to the next
    int wmax = 0;
    for (int j = 0; j < d.post_order; j++) wmax = std::max(wmax, d.post_w[j]);
    h.uts.assign(n_utt + 1, 0);
    h.uinfo.resize(n_utt);
    std::vector<TileRec> tiles;  // local, moved into `h` behind the loop: pushing through `h` measured 3 % on plan creation (profiles/host_pipeline_ab.txt)
    std::vector<int> chunks;
    int64_t ro = 0;
    for (int i = 0; i < n_utt; i++) {
        const int64_t T = ctu_num_frames(e, utt_n[i]);
        if (T < 0) {
            set_error(e, "IO: Signal shorter than one frame!");  // src/io/in.cc:277
            return CTU_ERR_INPUT;
        }
        if (rows && T > 0x7fffffff / 2) {
            set_error(e, "ENGINE: feature file too long");
            return CTU_ERR_INPUT;
        }
        // With exactly window+1 frames a stage never takes its steady-state branch, so its flush starts from ring
        // slot 0 instead of the oldest slot and the emitted rows mix frames (src/fea/fea_delta.cc:118,183-186);
        // with fewer it reads slots that were never written.  Neither is a feature worth reproducing.
        if (d.post_order > 0 && T > 0 && T < wmax + 2) {
            set_error(e, "ENGINE: delta / stacking on fewer than window+2 frames is ill-defined in the reference (src/fea/fea_delta.cc:74-130,178-206)");
            return CTU_ERR_INPUT;
        }
        if (!rows && d.kind == ctu::FeaKind::TrapDct && T > 0 && T < (d.o.fea_trapdct_traplen + 1) / 2) {
            set_error(e, "ENGINE: trapdct on fewer than (traplen+1)/2 frames is undefined in the reference (src/fea/fea_trap.cc:64-70)");
            return CTU_ERR_INPUT;
        }
        const int64_t so = pl->sample_off[i];
        pl->row_off[i] = ro;
        pl->frames[i] = T;
        h.uts[i] = (int)tiles.size();
        for (int64_t t0 = 0; t0 < T; t0 += TILE) {
            TileRec r;
            r.sbase = so + t0 * stride;
            r.rbase = ro + t0;
            r.nvalid = (int)std::min<int64_t>(TILE, T - t0);
            r.t0 = (int)t0;
            r.next = -1;
            r.T = (int)T;
            tiles.push_back(r);
            chunks.push_back(i);
            chunks.push_back((int)t0);
        }
        h.uinfo[i] = make_int4((int)(ro & 0xffffffff), (int)(ro >> 32), (int)T, 0);
        pl->max_frames = std::max<int>(pl->max_frames, (int)T);
        ro += T;
    }
    h.uts[n_utt] = (int)tiles.size();
    pl->row_off[n_utt] = ro;
    pl->ext.total_frames = ro;
    pl->ext.n_tiles = (int)tiles.size();
    h.tiles = std::move(tiles);
    h.chunks = std::move(chunks);
    return CTU_OK;
}

// Front-end workgroups the chip holds at once: two per CU when the instantiation keeps to 128 VGPRs (four waves per SIMD) and 80 KB of LDS; the
// synthesis and the 512-point detector instantiations take 256 VGPRs.  What plan_chains and a stream set's pushes build their chains for.
int fe_max_wg(const ctu_engine *e) {
    const FeSel &k = e->sel;
    return e->n_cu * ((fe_waves_per_simd(k.mode, k.vf, k.ss, k.sy) >= 4 && e->lds_bytes <= (size_t)LDS_2WG) ? 2 : 1);
}

// Step 2, host only, for plans over samples: the chains the front end walks and the grid they are built for.  (A plan over rows has
// no chains: rows_ingest_kernel strides over the tile list.)
// Each workgroup walks a chain of tiles.  Stateless chains stride over the tile list; with a
// per-utterance recurrence (exten) a workgroup takes whole utterances, tile after tile.
void plan_chains(const ctu_engine *e, ctu_plan *pl, PlanHost &h) {
    std::vector<TileRec> &tiles = h.tiles;
    const std::vector<int> &uts = h.uts;
    std::vector<int> &wg_first = h.wg_first;
    const int n_utt = pl->n_utt;
    const int max_wg = fe_max_wg(e);
    if (e->per_wave) {
        // chains per wave: whole utterances, longest first onto the least loaded chain (LPT), tile after tile
        std::vector<int> live;  // utterances that have at least one frame
        for (int i = 0; i < n_utt; i++)
            if (uts[i + 1] > uts[i]) live.push_back(i);
        std::stable_sort(live.begin(), live.end(), [&](int a, int b) { return pl->frames[a] > pl->frames[b]; });
        // (bigfft_kernel walks a chain with a whole workgroup of 256 threads: eight of them fit a CU at once)
        const int slots = (e->big && e->path != BIG_WAVE1K) ? e->n_cu * 8 : max_wg * NWAVE;
        const ChainDeal deal = chain_deal((int)live.size(), slots);  // (stream_plan.h: where chain c sits among the heads)
        const int C = deal.C, G = deal.G;
        wg_first.assign((size_t)deal.heads(), -1);
        std::vector<int> tail(C, -1);  // last tile of each chain so far
        std::priority_queue<std::pair<int64_t, int>, std::vector<std::pair<int64_t, int>>, std::greater<std::pair<int64_t, int>>> load;
        // (the chains of one workgroup are spread over the length ranks)
        for (int c = 0; c < C; c++) load.push({0, c});
        for (int u : live) {
            const auto top = load.top();
            load.pop();
            const int c = top.second, slot = deal.slot(c);
            for (int t = uts[u]; t + 1 < uts[u + 1]; t++) tiles[t].next = t + 1;
            tiles[uts[u + 1] - 1].next = -1;
            if (tail[c] < 0) wg_first[slot] = uts[u];
            else tiles[tail[c]].next = uts[u];
            tail[c] = uts[u + 1] - 1;
            load.push({top.first + pl->frames[u], c});
        }
        pl->ext.grid = G;
    } else {
        const int G = std::max(1, std::min(pl->ext.n_tiles, max_wg));
        wg_first.assign(G, -1);
        for (int t = 0; t < pl->ext.n_tiles; t++) tiles[t].next = (t + G < pl->ext.n_tiles) ? t + G : -1;
        for (int g = 0; g < G && g < pl->ext.n_tiles; g++) wg_first[g] = g;
        pl->ext.grid = G;
    }
}

// Step 3, the device side: the uploads and the scratch of every stage the engine's runs have.  Throws (ctu_plan_create's frame).
void plan_alloc(ctu_engine *e, ctu_plan *pl, const PlanHost &h) {
    const ctu::Design &d = *e->design;
    const int n_utt = pl->n_utt;
    const int64_t ro = pl->ext.total_frames;
    HIP_TRY(hipSetDevice(e->device));
    pl->tiles.upload(h.tiles);
    // the passes that run a workgroup per 64-frame chunk (TRAP, delta / stacking, CMS, CMVN); a plan over rows has the list in any case
    const bool chunked = e->rows_in || d.kind == ctu::FeaKind::TrapDct || d.post_order > 0 || d.cms || d.o.stat_cmvn || d.o.apply_cmvn;
    const bool per_utt = !e->rows_in && (d.signal_out || d.o.remove_dc1);  // the overlap-add and the -remove_dc1 recurrence go by utterance
    if (chunked || per_utt) pl->utt_info.upload(h.uinfo);
    if (chunked) {
        pl->trap_chunks.upload(h.chunks);
        pl->n_trap_chunks = (int)h.chunks.size() / 2;
    }
    if (d.post_order > 0 || d.cms) pl->base_rows.alloc((size_t)ro * d.Dbase);
    if (e->rows_in) return;  // what follows serves the front end and the stages that read its scratch
    pl->wg_first.upload(h.wg_first);
    pl->ext.heads = pl->wg_first.p;
    if (per_utt) pl->d_sample_off.upload(std::vector<long long>(pl->sample_off.begin(), pl->sample_off.end()));
    if (e->do_vad || (e->ss && e->big && !e->ss_file)) pl->d_row_off.upload(pl->row_off);
    if (e->ss) {
        std::vector<int> tu(h.tiles.size());
        for (int i = 0; i < n_utt; i++)
            for (int t = h.uts[i]; t < h.uts[i + 1]; t++) tu[t] = i;
        pl->tile_utt.upload(tu);
        pl->ss_seed.alloc((size_t)std::max(n_utt, 1) * d.K);
        pl->ss_last.alloc((size_t)std::max(n_utt, 1) * d.K);
        pl->ss_dirty.alloc((size_t)std::max(n_utt, 1));
        pl->ss_vbits.alloc((size_t)std::max<int64_t>(ro, 1));
        if (e->big) {  // bigss_kernel.h: the exported spectra, the detector's cepstra, on the speech path the subtracted magnitudes
            pl->xri.alloc((size_t)std::max<int64_t>(ro, 1) * d.K);
            pl->pnr.alloc((size_t)std::max<int64_t>(ro, 1) * d.K);
            if (synth_reads_pss(e)) pl->pss.alloc((size_t)std::max<int64_t>(ro, 1) * d.K);
            if (!e->ss_file) pl->vad_ci.alloc((size_t)std::max<int64_t>(ro, 1) * d.o.fea_ncepcoefs);
        }
    }
    if (e->do_vad) {
        if (e->vp.cri == 1) {
            if (!e->vf) {
                pl->xri.alloc((size_t)ro * d.K);
                pl->pnr.alloc((size_t)ro * d.K);
            }
            if (!e->vf) pl->vad_ci.alloc((size_t)ro * e->vp.ncoef);
            else {
                pl->vad_cf.alloc((size_t)std::max<int64_t>(ro, 1) * VFC_STRIDE);
                std::vector<int> ord;
                for (int i = 0; i < n_utt; i++)
                    if (pl->frames[i] > 0) ord.push_back(i);
                std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return pl->frames[a] > pl->frames[b]; });
                pl->n_live = (int)ord.size();
                if (ord.empty()) ord.push_back(0);
                pl->vf_order.upload(ord);
            }
        } else if (e->vp.cri == 0) pl->pnr.alloc((size_t)ro);
    }
    if (d.signal_out) {
        if (!e->sy && !synth_reads_pss(e)) {  // (with pss the *ss block above has allocated the exported spectra)
            pl->xri.alloc((size_t)ro * d.K);
            pl->pnr.alloc((size_t)ro * d.K);
        }
        pl->out_samples.resize(n_utt);
        for (int i = 0; i < n_utt; i++) pl->out_samples[i] = pl->frames[i] * d.wshift + (d.window - d.wshift);
        pl->ybuf.alloc((size_t)ro * d.window);
    }
    if (d.o.remove_dc1) {
        pl->dc1m.alloc((size_t)std::max<int64_t>(ro, 1));
        pl->dc1.alloc((size_t)std::max<int64_t>(ro, 1));
    }
    if (chunked) {  // the 128-frame chunks (trapdct_split16_kernel): every other 64-frame one
        std::vector<int> c128;
        for (size_t k = 0; k + 1 < h.chunks.size(); k += 2)
            if (!(h.chunks[k + 1] & 64)) {
                c128.push_back(h.chunks[k]);
                c128.push_back(h.chunks[k + 1]);
            }
        pl->n_trap_chunks128 = (int)c128.size() / 2;
        if (c128.empty()) c128.assign(2, 0);
        pl->trap_chunks128.upload(c128);
    }
    if (d.kind == ctu::FeaKind::TrapDct || e->dctw) pl->logmel.alloc((size_t)ro * d.B);
    if (lp_tail_runs(e)) pl->lp_r.alloc(((size_t)std::max<int64_t>(ro, 1) * (d.o.fea_lporder + 1) * (lags_double(e) ? 8 : 4) + 7) / 8);
}
}  // namespace

// The plan of an engine that starts from rows (-format_in htk) takes row counts as lengths and lays its arena out by
// ctu_rows_arena_layout; its tiles are what rows_ingest_kernel strides over, four (one per wave) to a workgroup pass.
int ctu_plan_create(ctu_engine *e, const int64_t *utt_nsamples, int32_t n_utt, ctu_plan **out) {
    if (!e || !out || n_utt < 0 || (n_utt && !utt_nsamples)) return CTU_ERR_INPUT;
    *out = nullptr;
    std::unique_ptr<ctu_plan> pl(new ctu_plan);
    PlanHost h;
    if (const int rc = plan_layout(e, pl.get(), utt_nsamples, n_utt, h); rc != CTU_OK) return rc;
    if (e->rows_in) pl->ext.grid = std::max(1, std::min((pl->ext.n_tiles + 3) / 4, e->n_cu * ROWS_WG_PER_CU));
    else plan_chains(e, pl.get(), h);
    const int rc = guarded(e, [&]() -> int {
        plan_alloc(e, pl.get(), h);
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    *out = pl.release();
    return CTU_OK;
}

void ctu_plan_destroy(ctu_plan *p) { delete p; }
const int64_t *ctu_plan_sample_offsets(const ctu_plan *p) { return p->sample_off.data(); }
const int64_t *ctu_plan_row_offsets(const ctu_plan *p) { return p->row_off.data(); }
int64_t ctu_plan_total_samples(const ctu_plan *p) { return p->total_samples; }
int64_t ctu_plan_total_frames(const ctu_plan *p) { return p->ext.total_frames; }

void ctu_vad_ring_step(int32_t order, int64_t frames, int32_t *hidx, int32_t *hsize) {
    // medianFilter::push / flush_frame / cleanFilter as VAD::process_frame, BATCH::flush_vad and VAD::clean drive them over one file
    // (src/vad/vad.h:110-175, src/vad/vad.cc:692-699,705-708,742-745): cleanFilter resets neither historyIdx nor historySize
    if (order < 1 || !hidx || !hsize) return;
    const int delay = (order - 1) / 2;
    int hi = ((*hidx % order) + order) % order, hs = *hsize;
    bool ready = false;
    for (int64_t t = 0; t < frames; t++) {
        hi = (hi + 1) % order;
        if (hs < delay) hs++;
        else ready = true;
    }
    for (;;) {
        if (hs > 0) {
            hi = (hi + 1) % order;
            hs--;
        } else
            ready = false;
        if (!ready) break;
    }
    *hidx = hi;
    *hsize = hs;
}

int64_t ctu_vad_ring_rows(int32_t order, int64_t frames, int32_t hidx0, int32_t *src) {
    // the ring of one file: push t writes slot (hidx0 + t) % order; the k-th written row reads slot k % order - at push k + delay, or after
    // the last push for the rows of the flush (src/vad/vad.h:126-175 with `start` reset by cleanFilter, historyIdx not)
    if (order < 1 || frames < 0) return CTU_ERR_INPUT;
    const int delay = (order - 1) / 2;
    if (frames <= delay) return 0;  // the filter never gets ready: nothing is written
    if (!src) return frames;
    const int h0 = ((hidx0 % order) + order) % order;
    std::vector<int32_t> slot((size_t)order, -1);
    int64_t k = 0;
    for (int64_t t = 0; t < frames; t++) {
        slot[(size_t)((h0 + t) % order)] = (int32_t)t;
        if (t >= delay) {
            src[k] = slot[(size_t)(k % order)];
            k++;
        }
    }
    for (; k < frames; k++) src[k] = slot[(size_t)(k % order)];
    return frames;
}

int ctu_plan_set_vad_ring(ctu_plan *pl, const int32_t *hidx) {
    if (!pl) return CTU_ERR_INPUT;
    ctu_engine *e = pl->eng;
    const ctu::Design &d = *e->design;
    pl->ring_hidx.clear();
    if (!hidx || !e->do_vad || d.o.vad_filter_order <= 1) return CTU_OK;
    const int order = d.o.vad_filter_order, delay = (order - 1) / 2;
    bool any = false;
    for (int i = 0; i < pl->n_utt; i++) any = any || (hidx[i] % order) != 0;
    if (!any) return CTU_OK;
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        pl->ring_hidx.assign(hidx, hidx + pl->n_utt);
        std::vector<int> src((size_t)std::max<int64_t>(pl->ext.total_frames, 1), -1);
        std::vector<int32_t> rel;
        for (int i = 0; i < pl->n_utt; i++) {
            const int64_t T = pl->frames[i], r0 = pl->row_off[i];
            if (T <= delay) continue;  // nothing is written for it
            rel.assign((size_t)T, -1);
            ctu_vad_ring_rows(order, T, hidx[i], rel.data());
            for (int64_t k = 0; k < T; k++) src[(size_t)(r0 + k)] = rel[(size_t)k] < 0 ? -1 : (int)(r0 + rel[(size_t)k]);
        }
        pl->ring_src.upload(src);
        pl->ring_tmp.reserve((size_t)std::max<int64_t>(pl->ext.total_frames, 1) * d.D);
        return CTU_OK;
    });
    if (rc != CTU_OK) pl->ring_hidx.clear();  // a plan without its ring is in phase
    return rc;
}

// A run of a plan over the extent `x`: the plan's own, or the front of it a push of a stream set covers.  `row_stages` off stops ahead of
// stage_post and stage_cms with the base rows in the plan's scratch: a stream set with row state runs its own forms of the two
// (stream_rows_kernels.h) over them and its history.  `vad_stages` off likewise leaves the VAD's sequential stages out - the detector's
// replay, the short files' bytes, the ring - with the criterion's input of every frame in the plan's scratch (vad_cf / vad_ci / the
// energy): a stream set with detector state replays them from its own state (stream_vad_kernels.h) and needs no d_vad here.
static int run_chain(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, const int16_t *d_pcm, float *d_rows, uint8_t *d_vad, void *stream, bool row_stages,
                     bool vad_stages = true) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (e->rows_in) {
        set_error(e, "ENGINE: this configuration starts from feature files (-format_in htk): use ctu_engine_run_rows");
        return CTU_ERR_INPUT;
    }
    if (x.n_tiles == 0) return CTU_OK;
    const ctu::Design &d = *e->design;
    const bool signal = d.signal_out;
    if (signal && !e->in_signal_call) {
        set_error(e, "ENGINE: this configuration writes speech (-format_out raw|wave): use ctu_engine_run_signal");
        return CTU_ERR_INPUT;
    }
    if (!d_pcm || (!signal && !d_rows) || (e->do_vad && vad_stages && !d_vad)) {
        set_error(e, "ENGINE: null device buffer");
        return CTU_ERR_INPUT;
    }
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        KParams kp = run_kparams(e, pl, x, d_pcm, d_rows);
        const BigParams bp = e->big ? run_bigparams(e, pl, x, kp) : BigParams{};
        const int grid = x.grid;
#if CTU_STAMP
        e->stamps.reserve((size_t)grid * NWAVE * 16);
        HIP_TRY(hipMemsetAsync(e->stamps.p, 0, e->stamps.n * 8, s));
        kp.stamps = e->stamps.p;
#endif
        if (d.o.remove_dc1) stage_dc1(e, pl, s, d_pcm);
        HIP_TRY(hipEventRecord(e->ev0, s));
        // the front end; with hwss / fwss / 2fwss `pass` is one pass of the seed iteration, which launches it
        std::function<void()> pass = [&] { launch_frontend(e, dim3(grid), s, kp, x.xstate != nullptr); };
        switch (e->path) {
            case BIG_NONE: if (!e->ss) pass(); break;
            case BIG_WAVE1K: stage_wave1k(e, pl, x, s, bp); break;
            case BIG_SS: pass = stage_bigss_front(e, pl, x, s, bp); break;
            case BIG_FFT: launch_bigfft(e, x, s, bp); break;
        }
        if (e->ss) {
            const int rc = run_ss_chain(e, pl, x, s, kp, pass);
            if (rc != CTU_OK) return rc;
        }
        if (e->dctw) stage_dctw(e, pl, x, s, kp);  // (inside the timed span: the tail finishes what the front end of a narrower chain does itself)
        HIP_TRY(hipEventRecord(e->ev1, s));
        e->timed = true;
        e->host_timed = false;
        HIP_TRY(hipGetLastError());
#if CTU_STAMP
        if (const char *sf = getenv("CTU_STAMP_FILE")) dump_stamps(e, grid, s, sf);
#endif
        if (lp_tail_runs(e)) stage_lp_tail(e, pl, x, s, kp);
        if (e->do_vad) stage_burg_vad(e, pl, x, s);
        if (d.kind == ctu::FeaKind::TrapDct) stage_trap(e, pl, s, d_rows);
        if (d.post_order > 0 && row_stages) stage_post(e, pl, s, d_rows);
        if (d.cms && row_stages) stage_cms(e, pl, s, d_rows);
        if (e->do_vad && e->vf && pl->n_live > 0) stage_fused_vad(e, pl, x, s, d_vad, vad_stages);
        if (e->do_vad && !e->vf && vad_stages) stage_vad_decide(e, pl, s, d_rows, d_vad);
        if (e->do_vad && d.o.vad_filter_order > 1 && vad_stages) stage_short_files(e, pl, s, d_vad);
        if (e->do_vad && !pl->ring_hidx.empty() && x.total_frames > 0 && vad_stages) stage_ring_gather(e, pl, x, s, d_rows);
        return CTU_OK;
    });
}

int ctu_engine_run(ctu_engine *e, const ctu_plan *pl, const int16_t *d_pcm, float *d_rows, uint8_t *d_vad, void *stream) {
    if (!pl) return CTU_ERR_INPUT;
    return run_chain(e, pl, pl->ext, d_pcm, d_rows, d_vad, stream, true);
}

void *ctu_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void ctu_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

namespace {
bool is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// The utterance ranges of a host-buffer run (ctu_engine_run_host, ctu_engine_run_rows_host): `nparts` consecutive ranges of about equal
// input as plans of their own, and the two streams they alternate on.  Keyed on the count asked for: fewer ranges may come out (a long
// utterance spans several).  A part's arena is the slice of the caller's arena that starts where its first utterance does - PCM_HEAD
// samples ahead of it for PCM: both layout rules are translation invariant.  A failure leaves the plan without ranges.
int split_host_parts(ctu_engine *e, ctu_plan *pl, int nparts) {
    if (nparts <= 1 || pl->parts_for == nparts) return CTU_OK;
    pl->parts.clear();
    pl->parts_for = 0;
    pl->part_first.assign(1, 0);
    const int64_t per = (pl->sample_off[pl->n_utt] - pl->sample_off[0] + nparts - 1) / nparts;
    for (int k = 1; k < nparts; k++) {
        int u = pl->part_first.back();
        const int64_t goal = pl->sample_off[0] + per * k;
        while (u < pl->n_utt && pl->sample_off[u] < goal) u++;
        if (u > pl->part_first.back() && u < pl->n_utt) pl->part_first.push_back(u);
    }
    pl->part_first.push_back(pl->n_utt);
    for (size_t k = 0; k + 1 < pl->part_first.size(); k++) {
        ctu_plan *sub = nullptr;
        const int u0 = pl->part_first[k], u1 = pl->part_first[k + 1];
        const int rc = ctu_plan_create(e, pl->nsamples.data() + u0, u1 - u0, &sub);
        if (rc != CTU_OK) {
            pl->parts.clear();
            return rc;
        }
        pl->parts.emplace_back(sub);
    }
    for (hipStream_t &st : pl->part_stream)
        if (!st) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    pl->parts_for = nparts;
    return CTU_OK;
}
// How many utterance ranges a host-buffer run is cut into - the one home of the rule: CTU_HOST_CHUNKS if set (1 = one range), else 8
// for batches of at least 16 utterances and 32 MiB of input (16 Mi samples, 8 Mi words of feature files) with both buffers page-locked.
// Modes whose state crosses utterances (the *ss noise seed) stay in one range; an engine over rows (-format_in htk) refuses the NR
// options, so e->ss is 0 there.
int host_chunks(const ctu_engine *e, const ctu_plan *pl, int64_t input_bytes, bool pinned) {
    if (e->ss) return 1;
    // pageable buffers go through blocking staged copies: cutting those up only adds calls (measured 1.04e8 -> 0.96e8 frames/s)
    int k = (pinned && pl->n_utt >= 16 && input_bytes >= (int64_t)32 << 20) ? 8 : 1;
    if (const char *v = getenv("CTU_HOST_CHUNKS")) k = std::max(1, atoi(v));
    return std::min(k, std::max(1, pl->n_utt));
}

// What a host-buffer run feeds run_host_ranges: the caller's arena and how a (sub)plan stages and runs its share of it.
struct HostInput {
    const void *base;   // the caller's arena
    size_t elem;        // bytes per element of it: an int16 sample or a 32-bit word of a feature file
    int64_t head;       // elements ahead of the first utterance that belong to a plan's arena (PCM_HEAD; a plan over rows has none)
    std::function<void *(ctu_plan *)> stage;          // the device copy of a (sub)plan's arena, grown to hold it (with what else its run needs)
    std::function<int(ctu_plan *, hipStream_t)> run;  // the device run of a (sub)plan from its staged arena into its h_rows
    // with the VAD only (else empty): hands a range, which starts at utterance `first`, its share of the caller's majority-filter ring ...
    std::function<int(ctu_plan *sub, int first)> ring;
    std::function<void(const ctu_plan *, int64_t row0)> vad;  // ... and fetches a finished (sub)plan's bytes, which start at row `row0`
};

// (start, stop) of every range's front-end launch; destroyed on every way out of the run
struct RangeEvents {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    ~RangeEvents() {
        for (auto &pe : ev) {
            if (pe.first) (void)hipEventDestroy(pe.first);
            if (pe.second) (void)hipEventDestroy(pe.second);
        }
    }
    void take(ctu_engine *e) {  // the engine's pair is re-recorded by every range: keep the recorded pair, leave a fresh one
        ev.emplace_back(nullptr, nullptr);
        HIP_TRY(hipEventCreate(&ev.back().first));
        HIP_TRY(hipEventCreate(&ev.back().second));
        std::swap(ev.back().first, e->ev0);
        std::swap(ev.back().second, e->ev1);
    }
    float sum_ms() const {
        float sum = 0.f, ms = 0.f;
        for (auto &pe : ev)
            if (hipEventElapsedTime(&ms, pe.first, pe.second) == hipSuccess) sum += ms;
        return sum;
    }
};

// The host-buffer run (ctu_engine_run_host, ctu_engine_run_rows_host): upload, device run, download; in ranges on two streams when
// host_chunks says so, else the whole plan on the default stream - the same walk with one part.  Device buffers are allocated once
// per plan (per part).  Transfers: a caller buffer from ctu_host_alloc (pinned) is DMA-ed asynchronously at the link rate; pageable
// memory goes through the runtime's own staging (hipMemcpy).  Throws (the caller's frame); a refusal of `run` or `ring` is returned.
int run_host_ranges(ctu_engine *e, ctu_plan *pl, const HostInput &in, float *h_rows) {
    const int D = e->design->D;
    HIP_TRY(hipSetDevice(e->device));
    const bool pin_in = is_pinned(in.base), pin_out = is_pinned(h_rows);
    const int nparts = host_chunks(e, pl, pl->total_samples * (int64_t)in.elem, pin_in && pin_out);
    if (const int rc = split_host_parts(e, pl, nparts); rc != CTU_OK) return rc;
    const bool ranges = nparts > 1 && pl->parts.size() > 1;
    const int np = ranges ? (int)pl->parts.size() : 1;
    auto part = [&](int k) { return ranges ? pl->parts[k].get() : pl; };
    auto first = [&](int k) { return ranges ? pl->part_first[k] : 0; };
    const hipStream_t st[2] = {ranges ? pl->part_stream[0] : nullptr, ranges ? pl->part_stream[1] : nullptr};
    RangeEvents events;
    auto download = [&](int k) {
        ctu_plan *sp = part(k);
        if (sp->ext.total_frames == 0) return;
        float *dst = h_rows + pl->row_off[first(k)] * D;
        if (pin_out) HIP_TRY(hipMemcpyAsync(dst, sp->h_rows.p, (size_t)sp->ext.total_frames * D * 4, hipMemcpyDeviceToHost, st[k & 1]));
        else {
            HIP_TRY(hipStreamSynchronize(st[k & 1]));
            HIP_TRY(hipMemcpy(dst, sp->h_rows.p, (size_t)sp->ext.total_frames * D * 4, hipMemcpyDeviceToHost));
        }
    };
    for (int k = 0; k < np; k++) {
        ctu_plan *sp = part(k);
        if (ranges && in.ring) {  // a range is a plan of its own: it starts its utterances where the caller's plan does
            const int rc = in.ring(sp, first(k));
            if (rc != CTU_OK) return rc;
        }
        if (sp->ext.total_frames) {
            void *d_in = in.stage(sp);
            sp->h_rows.reserve((size_t)sp->ext.total_frames * D);
            // a part's arena is the slice of the caller's that starts `head` elements ahead of its first utterance (split_host_parts)
            const char *src = static_cast<const char *>(in.base) + (pl->sample_off[first(k)] - in.head) * (int64_t)in.elem;
            if (pin_in) HIP_TRY(hipMemcpyAsync(d_in, src, (size_t)sp->total_samples * in.elem, hipMemcpyHostToDevice, st[k & 1]));
            else HIP_TRY(hipMemcpy(d_in, src, (size_t)sp->total_samples * in.elem, hipMemcpyHostToDevice));
            const int rc = in.run(sp, st[k & 1]);
            if (rc != CTU_OK) {  // earlier ranges are still in flight on the two streams: drain them before the caller reuses its buffers
                if (ranges) {
                    (void)hipStreamSynchronize(st[0]);
                    (void)hipStreamSynchronize(st[1]);
                }
                return rc;
            }
            if (ranges) events.take(e);  // (one range: the engine's own pair is the time of the run)
        }
        if (k > 0) download(k - 1);  // behind the launch of part k: the copy engines and the kernels overlap
    }
    download(np - 1);
    if (ranges || pin_out) HIP_TRY(hipStreamSynchronize(st[0]));  // (one range into pageable rows has waited in download)
    if (ranges) {
        HIP_TRY(hipStreamSynchronize(st[1]));
        e->host_kernel_ms = events.sum_ms();  // ctu_engine_last_kernel_ms after a host run in ranges
        e->host_timed = true;
    }
    if (in.vad)
        for (int k = 0; k < np; k++)
            if (part(k)->ext.total_frames) in.vad(part(k), pl->row_off[first(k)]);
    return CTU_OK;
}
}  // namespace

int ctu_engine_run_host(ctu_engine *e, const ctu_plan *pl_, const int16_t *h_pcm, float *h_rows, uint8_t *h_vad,
                        int64_t *rows_per_utt) {
    if (!e || !pl_ || pl_->eng != e) return CTU_ERR_INPUT;
    if (e->rows_in) {
        set_error(e, "ENGINE: this configuration starts from feature files (-format_in htk): use ctu_engine_run_rows_host");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);  // the device copies live in the plan
    const ctu::Design &d = *e->design;
    if (rows_per_utt)
        for (int i = 0; i < pl->n_utt; i++) rows_per_utt[i] = pl->frames[i];
    if (pl->ext.total_frames == 0) return CTU_OK;
    if (!h_pcm || !h_rows) {
        set_error(e, "ENGINE: null host buffer");
        return CTU_ERR_INPUT;
    }
    return guarded(e, [&]() -> int {
        std::vector<uint8_t> v(e->do_vad ? (size_t)pl->ext.total_frames : 0);
        HostInput in{h_pcm, sizeof(int16_t), PCM_HEAD};
        in.stage = [&](ctu_plan *p) {
            p->h_pcm.reserve((size_t)p->total_samples);
            if (e->do_vad) p->h_vad.reserve((size_t)p->ext.total_frames);
            return p->h_pcm.p;
        };
        in.run = [&](ctu_plan *p, hipStream_t s) { return ctu_engine_run(e, p, p->h_pcm.p, p->h_rows.p, p->h_vad.p, s); };
        if (e->do_vad) {
            in.ring = [&](ctu_plan *sub, int first) { return ctu_plan_set_vad_ring(sub, pl->ring_hidx.empty() ? nullptr : pl->ring_hidx.data() + first); };
            in.vad = [&](const ctu_plan *p, int64_t row0) { HIP_TRY(hipMemcpy(v.data() + row0, p->h_vad.p, (size_t)p->ext.total_frames, hipMemcpyDeviceToHost)); };
        }
        if (const int rc = run_host_ranges(e, pl, in, h_rows); rc != CTU_OK) return rc;
        if (e->do_vad) {
            if (h_vad) std::memcpy(h_vad, v.data(), v.size());
            if (d.o.vad_apply_mode == "drop") {
                // rows of non-speech frames are dropped (src/io/batch.cc:237-238): compact each utterance in place
                for (int i = 0; i < pl->n_utt; i++) {
                    const int64_t r0 = pl->row_off[i], T = pl->frames[i];
                    int64_t keep = 0;
                    for (int64_t t = 0; t < T; t++)
                        if (v[r0 + t] == '1') {
                            if (keep != t) std::memmove(h_rows + (r0 + keep) * d.D, h_rows + (r0 + t) * d.D, (size_t)d.D * 4);
                            keep++;
                        }
                    if (rows_per_utt) rows_per_utt[i] = keep;
                }
            } else if (rows_per_utt) {
                // a file the majority filter never got ready on (no more frames than its delay) writes no row (ctu_engine_run)
                const int64_t delay = (d.o.vad_filter_order - 1) / 2;
                for (int i = 0; i < pl->n_utt; i++)
                    if (pl->frames[i] <= delay) rows_per_utt[i] = 0;
            }
        }
        return CTU_OK;
    });
}

// ---- runs that start from rows (-format_in htk) ------------------------------------------------------------------------------
// Stages: ingest (rows_in_kernels.h) -> 7 delta chain / stacking -> 8 CMS; CMVN is the caller's, over the resulting rows.
int ctu_engine_run_rows(ctu_engine *e, const ctu_plan *pl, const void *d_rows_in, float *d_rows, void *stream) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (!e->rows_in) {
        set_error(e, "ENGINE: this configuration starts from samples: use ctu_engine_run (ctu_engine_run_rows needs -format_in htk)");
        return CTU_ERR_INPUT;
    }
    if (pl->ext.n_tiles == 0) return CTU_OK;
    if (!d_rows_in || !d_rows) {
        set_error(e, "ENGINE: null device buffer");
        return CTU_ERR_INPUT;
    }
    const ctu::Design &d = *e->design;
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const bool staged = d.post_order > 0 || d.cms;  // the passes behind read the plan's base rows, else the ingest writes the caller's
        uint32_t *dst = reinterpret_cast<uint32_t *>(staged ? pl->base_rows.p : d_rows);
        HIP_TRY(hipEventRecord(e->ev0, s));
        lift<0, 1>(d.o.swap_in, [&](auto sw) {
            lift<0, 1>(d.post_stack, [&](auto rot) {
                hipLaunchKernelGGL((rows_ingest_kernel<decltype(sw)::value != 0, decltype(rot)::value != 0>), dim3(pl->ext.grid), dim3(256), 0, s,
                                   static_cast<const uint32_t *>(d_rows_in), dst, pl->tiles.p, pl->ext.n_tiles, d.Dbase);
            });
        });
        HIP_TRY(hipEventRecord(e->ev1, s));
        e->timed = true;
        e->host_timed = false;
        HIP_TRY(hipGetLastError());
        if (d.post_order > 0) stage_post(e, pl, s, d_rows);
        if (d.cms) stage_cms(e, pl, s, d_rows);
        return CTU_OK;
    });
}

int ctu_engine_run_rows_host(ctu_engine *e, const ctu_plan *pl_, const void *h_rows_in, float *h_rows) {
    if (!e || !pl_ || pl_->eng != e) return CTU_ERR_INPUT;
    if (!e->rows_in) {
        set_error(e, "ENGINE: this configuration starts from samples: use ctu_engine_run_host (ctu_engine_run_rows_host needs -format_in htk)");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);  // the device copies live in the plan
    if (pl->ext.total_frames == 0) return CTU_OK;
    if (!h_rows_in || !h_rows) {
        set_error(e, "ENGINE: null host buffer");
        return CTU_ERR_INPUT;
    }
    return guarded(e, [&]() -> int {
        HostInput in{h_rows_in, sizeof(uint32_t), 0};
        in.stage = [](ctu_plan *p) {
            p->h_words.reserve((size_t)p->total_samples);
            return p->h_words.p;
        };
        in.run = [&](ctu_plan *p, hipStream_t s) { return ctu_engine_run_rows(e, p, p->h_words.p, p->h_rows.p, s); };
        return run_host_ranges(e, pl, in, h_rows);
    });
}

static void cmvn_maps(ctu_engine *e) {
    if (!e->col_of_slot.empty()) return;
    const ctu::Design &d = *e->design;
    const int fc = d.o.fea_ncepcoefs + 1, X = fc * (d.post_order + 1);
    e->col_of_slot.assign(X, 0);
    e->slot_of_col.assign(d.D, -1);
    for (int k = 0; k < X; k++) {
        if (e->rows_in) {  // feature files: slot k is vector entry k, written to column k (src/fea/post_impl.cc:55-57, src/io/out.cc:177-179)
            e->col_of_slot[k] = k;
            e->slot_of_col[k] = k;
            continue;
        }
        const int i = (k + 1) % X;               // internal vector entry held by slot k (post_impl.cc:56-62)
        const int j = i / fc, ii = i % fc;       // block, entry within the block (0 = c0)
        const int col = fc * j + (ii == 0 ? fc - 1 : ii - 1);  // writer order: c1..cN, c0 (out.cc:188-201)
        e->col_of_slot[k] = col;
        e->slot_of_col[col] = k;
    }
    e->d_col_of_slot.upload(e->col_of_slot);
    e->d_slot_of_col.upload(e->slot_of_col);
}

static int cmvn_check(ctu_engine *e, const ctu_plan *pl, const int32_t *spk_of_utt, int32_t n_spk) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    const ctu::Design &d = *e->design;
    if (!(d.o.stat_cmvn || d.o.apply_cmvn)) {
        set_error(e, "ENGINE: engine was not created with -stat_cmvn / -apply_cmvn");
        return CTU_ERR_INPUT;
    }
    if (n_spk < 1 || (pl->n_utt && !spk_of_utt)) {
        set_error(e, "ENGINE: speaker table missing");
        return CTU_ERR_INPUT;
    }
    for (int i = 0; i < pl->n_utt; i++)
        if (spk_of_utt[i] < 0 || spk_of_utt[i] >= n_spk) {
            set_error(e, "ENGINE: speaker index out of range");
            return CTU_ERR_INPUT;
        }
    return CTU_OK;
}

int ctu_cmvn_cols(const ctu_engine *e) {
    if (!e) return -1;
    const ctu::Design &d = *e->design;
    return (d.o.fea_ncepcoefs + 1) * (d.post_order + 1);
}

int ctu_cmvn_accumulate(ctu_engine *e, const ctu_plan *pl, const float *d_rows, const int32_t *spk_of_utt, int32_t n_spk,
                        const double *mean, double *acc, void *stream) {
    int rc = cmvn_check(e, pl, spk_of_utt, n_spk);
    if (rc != CTU_OK) return rc;
    if (!acc || (pl->ext.total_frames && !d_rows)) return CTU_ERR_INPUT;
    if (pl->ext.total_frames == 0) return CTU_OK;
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        cmvn_maps(e);
        const int cols = ctu_cmvn_cols(e);
        std::vector<int> spk(spk_of_utt, spk_of_utt + pl->n_utt);
        e->d_spk.upload(spk);
        std::vector<double> zero((size_t)n_spk * (cols + 1), 0.0);
        e->d_stat_a.upload(zero);
        if (mean) e->d_stat_b.upload(std::vector<double>(mean, mean + (size_t)n_spk * cols));
        hipLaunchKernelGGL(cmvn_accumulate_kernel, dim3(pl->n_trap_chunks), dim3(256), 0, s, d_rows, pl->utt_info.p,
                           pl->trap_chunks.p, e->d_spk.p, e->d_col_of_slot.p, mean ? e->d_stat_b.p : nullptr, e->d_stat_a.p,
                           cols, e->design->D);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(zero.data(), e->d_stat_a.p, zero.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < zero.size(); i++) acc[i] += zero[i];
        return CTU_OK;
    });
}

int ctu_cmvn_apply(ctu_engine *e, const ctu_plan *pl, float *d_rows, const int32_t *spk_of_utt, int32_t n_spk,
                   const double *mean, const double *var, void *stream) {
    int rc = cmvn_check(e, pl, spk_of_utt, n_spk);
    if (rc != CTU_OK) return rc;
    if (!mean || !var || (pl->ext.total_frames && !d_rows)) return CTU_ERR_INPUT;
    if (pl->ext.total_frames == 0) return CTU_OK;
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        cmvn_maps(e);
        const int cols = ctu_cmvn_cols(e);
        std::vector<int> spk(spk_of_utt, spk_of_utt + pl->n_utt);
        e->d_spk.upload(spk);
        e->d_stat_a.upload(std::vector<double>(mean, mean + (size_t)n_spk * cols));
        e->d_stat_b.upload(std::vector<double>(var, var + (size_t)n_spk * cols));
        hipLaunchKernelGGL(cmvn_apply_kernel, dim3(pl->n_trap_chunks), dim3(256), 0, s, d_rows, pl->utt_info.p,
                           pl->trap_chunks.p, e->d_spk.p, e->d_slot_of_col.p, e->d_stat_a.p, e->d_stat_b.p, cols, e->design->D);
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
}

const int64_t *ctu_plan_out_samples(const ctu_plan *p) { return p->out_samples.empty() ? nullptr : p->out_samples.data(); }

int ctu_engine_run_signal(ctu_engine *e, const ctu_plan *pl, const int16_t *d_pcm, int16_t *d_out, void *stream) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    const ctu::Design &d = *e->design;
    if (!d.signal_out) {
        set_error(e, "ENGINE: ctu_engine_run_signal needs -format_out raw|wave");
        return CTU_ERR_INPUT;
    }
    if (pl->n_utt == 0) return CTU_OK;
    if (!d_pcm || !d_out) {
        set_error(e, "ENGINE: null device buffer");
        return CTU_ERR_INPUT;
    }
    hipStream_t s = (hipStream_t)stream;
    e->in_signal_call = true;
    const int rc = ctu_engine_run(e, pl, d_pcm, nullptr, nullptr, stream);  // spectra before / after NR into the plan's scratch
    e->in_signal_call = false;
    if (rc != CTU_OK) return rc;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        SynthParams sp;
        sp.K = d.K; sp.wfft = d.wfft; sp.window = d.window; sp.wshift = d.wshift;
        sp.inv_n = 1.0f / (float)d.wfft;
        sp.corr = d.ola_corr;
        if (pl->ext.total_frames > 0 && e->big) launch_bigsynth(e, pl, pl->ext, s, sp.inv_n);
        else if (pl->ext.total_frames > 0 && !e->sy) {
            const int g = (int)std::min<int64_t>((pl->ext.total_frames + 7) / 8, (int64_t)e->n_cu * 8);
            hipLaunchKernelGGL(synth_kernel, dim3(g), dim3(256), 0, s, pl->xri.p, pl->pnr.p, pl->ybuf.p, (long long)pl->ext.total_frames, sp);
            HIP_TRY(hipGetLastError());
        }
        int64_t longest = 0;
        for (int64_t n : pl->out_samples) longest = std::max(longest, n);
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((longest + 255) / 256, 64));
        hipLaunchKernelGGL(ola_kernel, dim3(gx, pl->n_utt), dim3(256), 0, s, pl->ybuf.p, d_out, pl->utt_info.p, pl->d_sample_off.p,
                           pl->n_utt, sp);
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
}

int ctu_engine_run_signal_host(ctu_engine *e, const ctu_plan *pl, const int16_t *h_pcm, int16_t *h_out) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        DevBuf<int16_t> pcm, out;
        pcm.alloc((size_t)pl->total_samples);
        out.alloc((size_t)pl->total_samples);
        HIP_TRY(hipMemcpy(pcm.p, h_pcm, (size_t)pl->total_samples * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(out.p, 0, (size_t)pl->total_samples * 2));
        const int rc = ctu_engine_run_signal(e, pl, pcm.p, out.p, nullptr);
        if (rc != CTU_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, out.p, (size_t)pl->total_samples * 2, hipMemcpyDeviceToHost));
        return CTU_OK;
    });
}

int ctu_cmvn_accumulate_host(ctu_engine *e, const ctu_plan *pl, const float *h_rows, const int32_t *spk_of_utt, int32_t n_spk,
                             const double *mean, double *acc) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (pl->ext.total_frames == 0) return CTU_OK;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        DevBuf<float> rows;
        rows.alloc((size_t)pl->ext.total_frames * e->design->D);
        HIP_TRY(hipMemcpy(rows.p, h_rows, rows.n * sizeof(float), hipMemcpyHostToDevice));
        return ctu_cmvn_accumulate(e, pl, rows.p, spk_of_utt, n_spk, mean, acc, nullptr);
    });
}

int ctu_cmvn_apply_host(ctu_engine *e, const ctu_plan *pl, float *h_rows, const int32_t *spk_of_utt, int32_t n_spk,
                        const double *mean, const double *var) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (pl->ext.total_frames == 0) return CTU_OK;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        DevBuf<float> rows;
        rows.alloc((size_t)pl->ext.total_frames * e->design->D);
        HIP_TRY(hipMemcpy(rows.p, h_rows, rows.n * sizeof(float), hipMemcpyHostToDevice));
        const int rc = ctu_cmvn_apply(e, pl, rows.p, spk_of_utt, n_spk, mean, var, nullptr);
        if (rc != CTU_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_rows, rows.p, rows.n * sizeof(float), hipMemcpyDeviceToHost));
        return CTU_OK;
    });
}

int ctu_decode_g711(ctu_engine *e, const uint8_t *d_codes, int64_t n, int alaw, int16_t *d_pcm, void *stream) {
    if (!e || n < 0 || (n && (!d_codes || !d_pcm))) return CTU_ERR_INPUT;
    if (n == 0) return CTU_OK;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const int grid = (int)std::min<int64_t>((n / 8 + 255) / 256, (int64_t)e->n_cu * 8);
        hipLaunchKernelGGL(g711_kernel, dim3(std::max(grid, 1)), dim3(256), 0, (hipStream_t)stream, d_codes, d_pcm, n, alaw);
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
}

int ctu_engine_reset_chain(ctu_engine *e) {
    if (!e) return CTU_ERR_INPUT;
    e->ss_stale.clear();
    e->vad_pos = 0;
    return CTU_OK;
}

int ctu_engine_set_vad_stream(ctu_engine *e, const unsigned char *bytes, int64_t n) {
    if (!e || n < 0 || (n && !bytes)) return CTU_ERR_INPUT;
    if (!e->ss_file) {
        set_error(e, "ENGINE: this configuration does not take its VAD decisions from a stream (-nr_mode hwss|fwss|2fwss -vad file=...)");
        return CTU_ERR_INPUT;
    }
    e->vad_stream.assign(bytes, bytes + n);
    e->vad_pos = 0;
    return CTU_OK;
}

const char *ctu_engine_kernel_name(const ctu_engine *e) {
    if (!e) return "";
    if (e->kname.empty()) {
        std::string n;
        switch (e->path) {
            case BIG_WAVE1K: n = "wave1k_kernel"; break;
            case BIG_SS: n = "bigss_kernel<" + std::to_string(big_nit(e)) + ">"; break;
            case BIG_FFT: n = "bigfft_kernel<" + std::to_string(big_nit(e)) + ">"; break;
            case BIG_NONE: n = fe_name(e->sel); break;
        }
        if (e->dctw) n = "dct_wide_kernel";  // the front end ahead of it is ctu_config_table(..., "frontend") / the FFT size
        const_cast<ctu_engine *>(e)->kname = n;
    }
    return e->kname.c_str();
}

int ctu_engine_phase2_walk(const ctu_engine *e) { return e ? e->walk_launched : -1; }

float ctu_engine_last_kernel_ms(ctu_engine *e) {
    if (!e || !e->timed) return -1.f;
    if (e->host_timed) return e->host_kernel_ms;
    float ms = -1.f;
    if (hipEventSynchronize(e->ev1) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, e->ev0, e->ev1) != hipSuccess) return -1.f;
    return ms;
}


// ---- streaming input: stream sets, pushes (planned by stream_plan.h), finishes
#include "streams_host.h"

}  // extern "C"
