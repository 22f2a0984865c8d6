// MI355X (gfx950) engine: host side of the C ABI (include/ctu_engine.h) - uploads of the tables and of the plans, launches.  What is
// accepted (accept.cc), which front-end instantiation runs and what the tables hold (tables.cc), and the plan of an offline run - batch
// layout, tile chains, the stages' lists, the size of every scratch buffer (plan.cc) - is decided in host-only units of their own; this
// unit uploads their EngineTables and HostPlan values, allocates by them and launches by them.  The kernels live in the headers included
// below, in one translation unit:
//   kernel_common.h    the kernel parameter block, DPP / LDS helpers (layout_constants.h: every constant host-only code shares, the tile record)
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
//   stream_trap_kernels.h  streaming input with trap state: TRAP-DCT over the rows a push completes, sixteen (stream, row) columns per MFMA
//   stream_signal_kernels.h  streaming input with signal state: the overlap-add of a push from the stream's tail, the flush at a file's end
//   stream_plan.h      streaming input, host only and HIP-free: the descriptors of a push and the planner that fills them (slots, chains, rows)
//   stream_set_shape.h streaming input, host only and HIP-free: what a stream set is - its kinds of state, halo, strides, the size of every buffer
//   streams_host.h     streaming input, host side: the stream set, create by the shape / one push body (check, plan, commit, launch) / finish
//   wire_in_kernels.h  offline wire input: a plan's utterances out of G.711 codes, swapped and strided PCM into its arena, dealt in pieces of the arena
//   wire_plan.h        offline wire input, host only and HIP-free: the bound check ahead of that launch, its pieces, the bytes a range uploads
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
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ctu_engine.h"
#include "accept.h"
#include "design.h"
#include "opts.h"
#include "plan_host.h"
#include "tables.h"

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
#include "stream_set_shape.h"
#include "wire_layout.h"
#include "wire_in_kernels.h"

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
    template <class U>
    void upload(const std::vector<U> &h) {  // U: T, or the words a host-only table states T's records in
        release();
        n = h.size() * sizeof(U) / sizeof(T);
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

using namespace ctu;  // accept.h, tables.h: what is accepted, FeSel and fe_compiled, EngineTables

}  // namespace

#include "post_kernels.h"
#include "stream_rows_kernels.h"
#include "stream_trap_kernels.h"
#include "stream_vad_kernels.h"
#include "signal_kernels.h"
#include "stream_signal_kernels.h"

struct ctu_engine {
    std::unique_ptr<ctu::Design> design;
    int device = 0;
    int n_cu = 256;
    ctu::Spread sp;             // kstride > 1: an FFT size below 256 carried by the 256-point mode; the configuration's own FFT size and bin count
    std::string err, kname;
    ctu::EngineTables tab;      // what create decided and laid out (tables.h); the buffers below are its images on the device
    DevBuf<float> lanec, ftab, trapG, dctw_tab;
    DevBuf<uint4> trapG16;      // TRAP on the bf16 matrix pipe: A fragments [8 phases][4 k-steps][3 terms][64 lanes] (trap_kernel.h)
    DevBuf<int> itab;
    // FFT sizes of 1024 to 4096 points (bigfft_kernel.h)
    DevBuf<float> big_win, big_fbw, big_coef, big_lifter;
    DevBuf<float2> big_tw;
    DevBuf<int> big_range, big_slot, big_seg;
    DevBuf<double> big_coef_d;
    DevBuf<double> big_han;     // hwss / fwss / 2fwss at 2048 / 4096 points: the detector's Hann window [window] (bigssdet_kernel)
    int walk_launched = -1;     // what the last front-end launch ran: tab.sel.walk, -1 before the first run (ctu_engine_phase2_walk)
    std::vector<float> ss_stale;  // the spectrum vector the last file of the previous run left behind (zeros at first)
    // -vad file=<f> (tab.ss_file): ONE byte stream for all files of the process, a byte per frame, never rewound (nr.cc:205-209, 273, 297-302)
    std::vector<unsigned char> vad_stream;
    int64_t vad_pos = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    bool host_timed = false;    // the last run was a host run cut into ranges: host_kernel_ms = sum over the ranges' front-end launches
    float host_kernel_ms = 0.f;
    bool in_signal_call = false;
    // CMVN (row N2): statistic slot <-> row column maps, and per-call scratch
    std::vector<int> col_of_slot, slot_of_col;
    DevBuf<int> d_col_of_slot, d_slot_of_col, d_spk;
    DevBuf<double> d_stat_a, d_stat_b;
    DevBuf<unsigned long long> stamps;
    std::set<const void *> attr_done;  // kernels whose dynamic-LDS limit has been raised on this engine's device
    ctu::PlanGeom geom;     // what a plan needs to know of this engine, and which lists and buffers its stages need (plan_host.h)
    VadParams vp;
    KParams kp0;    // the kernels' parameter blocks as far as design and tables fix them (ctu_engine_create); a run adds its buffers
    BigParams bp0;  // (`big` only)
};

// What a run covers of a plan's buffers: a plan's own extent is the whole of it (ctu_plan_create), a push of
// a stream set runs the front of its set's plan with the extent of the push (streams_host.h).  Every stage launches by the extent it is
// given; a plan is not written once it is created.
struct RunExtent {
    int n_tiles = 0;
    int grid = 0;                  // workgroups of the front-end launch (tile chains are built for it)
    int64_t total_frames = 0;
    const int *heads = nullptr;    // first tile of every chain: a plan's wg_first, or the heads a push was dealt onto (null: a plan over rows)
    int n_heads = 0;               // entries of `heads`: the chains wave1k_kernel / bigfft_kernel are launched for with exten
    void *xstate = nullptr;        // a stream set with noise state: exten's state of every stream (null: none, every file starts afresh)
};

struct ctu_plan {
    ctu_engine *eng = nullptr;
    ctu::HostPlan hp;           // the plan itself (plan_host.h); what follows are its images on the device, the scratch it sizes, and run state
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
    // wire input (ctu_plan_unpack_wire), made by the first call: the lengths, the arena offsets where the plan's stages keep none
    // (d_sample_off) and the pieces of wire_unpack_kernel on the device; the element offsets of a call and the page-locked staging they go
    // up from, which the next call reuses once the copy behind wire_free has read it; host-buffer runs: the device copy of the wire bytes
    DevBuf<long long> wire_n, wire_off, wire_elem;
    DevBuf<int> wire_piece;
    DevBuf<uint8_t> h_wire;
    long long *wire_stage = nullptr;
    hipEvent_t wire_free = nullptr;
    ~ctu_plan() {
        for (hipStream_t st : part_stream)
            if (st) (void)hipStreamDestroy(st);
        if (wire_free) (void)hipEventDestroy(wire_free);
        if (wire_stage) (void)hipHostFree(wire_stage);
    }
    DevBuf<int> tile_utt;            // utterance of every tile (SS); the stream of every tile (a stream set with noise state)
    DevBuf<float> ss_seed, ss_last;  // SS: noise seeds per utterance [n_utt][K] and the vectors the utterances leave behind
    DevBuf<unsigned char> ss_dirty;  // SS: utterances a pass of the seed iteration recomputes
    DevBuf<unsigned char> ss_vbits;  // SS: the detector's decision of every frame (first pass), reused by the later passes
    DevBuf<float2> xri;         // the exported spectra (PlanGeom::spectra)
    DevBuf<float> pnr;
    DevBuf<float> pss;          // hwss / fwss / 2fwss with speech output at 2048 / 4096 points: the subtracted magnitudes (pnr stays as exported)
    DevBuf<double> vad_ci;
    DevBuf<float> vad_cf;      // fused Burg-cepstral VAD: cepstra of every frame [total_frames][VFC_STRIDE] ahead of vad_lanes_kernel
    DevBuf<int> vf_order;      // utterances with at least one frame, longest first (a wave of vad_lanes_kernel takes 16 in a row)
    DevBuf<int64_t> d_row_off;
    DevBuf<double> dc1m;       // -remove_dc1: frame means, then
    DevBuf<float> dc1;         // the offsets the frames subtract (decode_kernels.h)
    // scratch between the kernels of one run; owned by the plan, so plans can run concurrently on different streams
    DevBuf<float> logmel;      // TRAP: log-mel rows [total_frames][B]
    DevBuf<double> lp_r;       // LP kinds: autocorrelation lags [total_frames][lporder + 1] (used as float rows by the fp32 path) ahead of lp_tail_kernel
    DevBuf<float> base_rows;   // front-end rows ahead of the delta / stacking / CMS passes [total_frames][Dbase]
    DevBuf<float> ybuf;        // signal output: time-domain frames ahead of the overlap-add [total_frames][window]
    DevBuf<long long> d_sample_off;
    DevBuf<int4> utt_info;
    DevBuf<int> trap_chunks, trap_chunks128;   // (utterance, first frame) of every 64- / 128-frame chunk
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

// The images of e->tab on the device.
void build_tables(ctu_engine *e) {
    const EngineTables &t = e->tab;
    e->lanec.upload(t.lanec);
    e->ftab.upload(t.p2.ft);
    e->itab.upload(t.p2.it);
    e->trapG.upload(t.trapG);
    e->trapG16.upload(t.trapG16);
    e->dctw_tab.upload(t.dctw_tab);
    e->big_win.upload(t.big_win);
    e->big_tw.upload(t.big_tw);
    e->big_fbw.upload(t.big_fbw);
    e->big_range.upload(t.big_range);
    e->big_seg.upload(t.big_seg);
    e->big_coef.upload(t.big_coef);
    e->big_coef_d.upload(t.big_coef_d);
    e->big_slot.upload(t.big_slot);
    e->big_lifter.upload(t.big_lifter);
    e->big_han.upload(t.big_han);
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
    hipLaunchKernelGGL(kern, grid, dim3(WG), e->tab.lds_bytes, s, kp);
}

// f(integral_constant<int, C>) for the C that v equals
template <int... C, class F>
void lift(int v, F &&f) {
    (void)((v == C && (f(std::integral_constant<int, C>{}), true)) || ...);
}
// The front-end launch of an engine: its FeSel lifted to template arguments, one at a time; fe_compiled decides which leaves exist.
// `xs`: the launch of a stream set with noise or subtraction state (frontend_kernel<..., XS>; the generic walk: the same rows bit for bit).
// (with detector state as well: the fused Burg-cepstral criterion behind exten, C4's front end - its cepstra go to the scratch by frame, nothing of it runs along a file)
// (with signal state: the one instantiation per (NZ, MODE) a speech-output design runs on - FEAT_BANDS, 16 coefficient rows, GEN_FULL,
// with SY.  VX stays out: the VAD's export is not carried behind exten's state, and streams_unsupported_reason refuses those configurations)
constexpr bool fe_streamed_signal(const FeSel &k) { return k.feat == FEAT_BANDS && k.nc == 16 && k.gen == GEN_FULL && !k.vf && !k.ss && k.sy && !k.vx; }
// (with subtraction state: the twin of every feature-path *ss instantiation - a set runs the engine's own instantiation plus the state traffic)
// (with signal state as well: the twin of the one speech-output *ss instantiation per mode, FEAT_BANDS, 16 coefficient rows, GEN_FULL)
constexpr bool fe_streamed_ss(const FeSel &k) { return k.ss && !k.vx && !k.vf && (!k.sy || (k.feat == FEAT_BANDS && k.nc == 16 && k.gen == GEN_FULL)); }
constexpr bool fe_streamed(const FeSel &k) { return fe_streamed_signal(k) || fe_streamed_ss(k) || (!k.vx && !k.ss && !k.sy && (k.gen == GEN_EXTEN || (k.gen == GEN_FULL && !k.vf))); }
void launch_frontend(ctu_engine *e, dim3 grid, hipStream_t s, const KParams &kp, bool xs = false) {
    const FeSel &k = e->tab.sel;
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

// NIT of the large-FFT kernels (samples per thread of a workgroup's 256): 4, 8 or 16
int big_nit(const ctu_engine *e) { return e->design->wfft / 256; }

// The parameter block of the 256 / 512-point front end as far as design and tables fix it (after build_tables and e->vp).
KParams engine_kparams(const ctu_engine *e) {
    const ctu::Design &d = *e->design;
    const Phase2Tables &t = e->tab.p2;  // the offsets of the table area, stated once
    const bool signal = d.signal_out;
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    kp.band_log = d.kind != ctu::FeaKind::Spec;
    kp.band_to_scratch = d.kind == ctu::FeaKind::TrapDct ? 1 : e->tab.dctw ? 2 : 0;  // 2: the bands to the scratch, the energy column (-fea_E) to its slot of the row
    kp.lp_is_lpa = d.kind == ctu::FeaKind::Lpa;
    kp.syn_scale = 1.0f / (float)d.wfft;
    kp.vad_export = (!e->geom.do_vad || e->tab.sel.vf || signal) ? 0 : (e->vp.cri == 1 ? 1 : (e->vp.cri == 0 ? 2 : 0));
    kp.vad_nc = e->vp.ncoef;
    kp.ss_mode = e->tab.ss; kp.ss_init = d.o.nr_initsegs; kp.ss_nc = d.o.fea_ncepcoefs; kp.han_off = t.han_off;
    kp.nr_b = (float)d.o.nr_b; kp.ss_q = d.o.nr_q;
    kp.skip_phase2 = signal ? 1 : 0;
    kp.lanec = e->lanec.p; kp.ftab = e->ftab.p; kp.itab = e->itab.p;
    kp.tab_floats = t.tab_floats; kp.ck_off = t.ck_off; kp.cf_off = t.cf_off; kp.cfd_off = t.cfd_off; kp.am_off = t.am_off;
    kp.NS = t.NS; kp.CW = t.CW; kp.ncoef_out = t.ncoef_out; kp.lift_off = t.lift_off;
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
    kp.remove_dc = d.o.remove_dc; kp.kstride = e->sp.kstride;
    kp.remove_dc1 = d.o.remove_dc1 ? 1 : 0; kp.dc1_J = d.window / d.wshift;
    kp.fb_power = d.o.fb_power; kp.fb_inld = d.o.fb_inld; kp.lifter_on = d.o.fea_lifter > 1;
    kp.nr_exten = d.o.nr_mode == "exten"; kp.nr_after_fb = d.o.nr_when_afterFB ? 1 : 0;
    kp.nr_p = (float)d.o.nr_p; kp.nr_p_d = d.o.nr_p; kp.nr_a = (float)d.o.nr_a;
    kp.per_wave = e->geom.per_wave ? 1 : 0;
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
    bp.ncoef_out = e->tab.p2.ncoef_out; bp.feat = e->tab.feat; bp.e_mode = kp.e_mode; bp.e_slot = kp.e_slot;
    bp.remove_dc = kp.remove_dc; bp.fb_power = kp.fb_power; bp.fb_inld = kp.fb_inld; bp.band_log = kp.band_log;
    bp.band_to_scratch = kp.band_to_scratch; bp.lp_is_lpa = kp.lp_is_lpa; bp.lporder = kp.lporder; bp.ncep = kp.ncep;
    bp.lifter_on = kp.lifter_on; bp.preem = kp.preem;
    bp.fb_total = e->tab.big_fb_total;
    bp.seg = e->big_seg.p;
    bp.nr_exten = kp.nr_exten; bp.nr_p = kp.nr_p; bp.nr_a = kp.nr_a;
    bp.dc1_J = kp.dc1_J;
    bp.xri_only = d.signal_out ? 1 : 0;
    if (e->tab.ss) {
        bp.ss_mode = e->tab.ss; bp.ss_init = d.o.nr_initsegs; bp.ss_a = d.o.nr_a; bp.ss_b = d.o.nr_b; bp.ss_p = d.o.nr_p;
    }
    return bp;
}
// A run's blocks: the engine's, with the caller's buffers and the plan's scratch.
KParams run_kparams(const ctu_engine *e, const ctu_plan *pl, const RunExtent &x, const int16_t *d_pcm, float *d_rows) {
    const ctu::Design &d = *e->design;
    KParams kp = e->kp0;
    kp.pcm = d_pcm;
    kp.rows = e->geom.staged ? pl->base_rows.p : d_rows;
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
    bp.chain_first = x.heads; bp.n_chains = x.n_heads;  // (the plan's own, or those of a push: a stream set with large-transform state)
    bp.xstate = static_cast<float *>(x.xstate);
    bp.vad_en = e->geom.vad_energy ? pl->pnr.p : nullptr;
    bp.dc1 = pl->dc1.p;
    // the spectra leave bigfft_kernel for bigsynth_kernel, bigburg_kernel (which reads them; the rows are projected as well) or bigss_kernel
    bp.xri = e->geom.spectra ? pl->xri.p : nullptr; bp.pnr = e->geom.spectra ? pl->pnr.p : nullptr;
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
    const int gx = std::max(1, std::min((pl->hp.max_frames + 3) / 4, 64));
    hipLaunchKernelGGL(dc1_means_kernel, dim3(gx, pl->hp.n_utt), dim3(256), 0, s, d_pcm, pl->utt_info.p, pl->d_sample_off.p, pl->dc1m.p, pl->hp.n_utt, d.window, d.wshift);
    hipLaunchKernelGGL(dc1_offsets_kernel, dim3((pl->hp.n_utt + 63) / 64), dim3(64), 0, s, pl->dc1m.p, pl->utt_info.p, pl->dc1.p, pl->hp.n_utt, d.window, d.wshift);
}

// bigfft_kernel: a workgroup per frame over the tile list, as many as fit the chip at once; with exten one workgroup per chain of utterances
void launch_bigfft(ctu_engine *e, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const LdsFit fit = bigfft_lds(*e->design, e->tab.feat, e->tab.p2.ncoef_out, e->tab.big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the large-FFT kernel");
    if (bp.nr_exten && !e->geom.per_wave) throw std::runtime_error("internal: exten without chains");
    const dim3 g((unsigned)std::max(1, bp.nr_exten ? bp.n_chains : std::min(x.n_tiles, e->n_cu * fit.per_cu)));
    lift<4, 8, 16>(big_nit(e), [&](auto nit) {
        constexpr int NIT = decltype(nit)::value;
        if (bp.nr_exten && x.xstate) launch_lds(e, &bigfft_kernel<NIT, true, true>, g, dim3(256), fit.bytes, s, bp);
        else if (bp.nr_exten) launch_lds(e, &bigfft_kernel<NIT, true>, g, dim3(256), fit.bytes, s, bp);
        else launch_lds(e, &bigfft_kernel<NIT>, g, dim3(256), fit.bytes, s, bp);
    });
}
// 1024 points: one wave per frame, the transform in registers (wave1k_kernel.h); tiles are dealt to waves
void stage_wave1k(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const ctu::Design &d = *e->design;
    const LdsFit fit = wave1k_lds(d, e->tab.feat, e->tab.p2.ncoef_out, e->tab.big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the 1024-point kernel");
    if (bp.nr_exten && !e->geom.per_wave) throw std::runtime_error("internal: exten without per-wave chains");
    // exten: one wave per chain of utterances, every chain gets its wave whatever fits the chip at once
    const int wg = bp.nr_exten ? std::max(1, (bp.n_chains + W1K_WAVES - 1) / W1K_WAVES)
                               : std::max(1, std::min((x.n_tiles + W1K_WAVES - 1) / W1K_WAVES, e->n_cu * fit.per_cu));
    if (bp.nr_exten && x.xstate) launch_lds(e, &wave1k_kernel<true, true>, dim3(wg), dim3(64 * W1K_WAVES), fit.bytes, s, bp, (void *)pl->lp_r.p, d.o.fea_lporder + 1);
    else
        lift<0, 1>(bp.nr_exten, [&](auto ex) {
            launch_lds(e, &wave1k_kernel<decltype(ex)::value != 0>, dim3(wg), dim3(64 * W1K_WAVES), fit.bytes, s, bp, (void *)pl->lp_r.p, d.o.fea_lporder + 1);
        });
}
// hwss / fwss / 2fwss at 2048 / 4096 points (bigss_kernel.h): the spectra once (bigfft_kernel with the export on and the projection off),
// the detector's cepstra and decisions once; returns the launch of bigss_kernel, one pass of the seed iteration (run_ss_chain).
// With the extent of a push of a stream set with subtraction state (x.xstate): the export and the detector's cepstra are per frame and run
// as they are over the push's frames; the decisions come from ss_decide_stream_kernel and the returned launch is bigss_kernel<NIT, true>,
// both along the push's chains from the streams' slots - run_chain launches it once.
std::function<void()> stage_bigss_front(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const BigParams &bp) {
    const ctu::Design &d = *e->design;
    if (d.wfft != 2048 && d.wfft != 4096) throw std::runtime_error("internal: SS engine without an SS instantiation");
    const bool streamed = x.xstate != nullptr;
    if (streamed && e->tab.ss_file) throw std::runtime_error("internal: -vad file= on a stream set");
    BigParams xp = bp;
    xp.xri_only = 1;
    launch_bigfft(e, x, s, xp);
    HIP_TRY(hipGetLastError());
    if (!e->tab.ss_file) {
        const LdsFit fit = bigburg_lds(d.wfft);
        const dim3 bg((unsigned)std::min<int64_t>(x.total_frames, (int64_t)e->n_cu * fit.per_cu));
        const int nc = d.o.fea_ncepcoefs, two = e->tab.ss == 3;
        lift<8, 16>(big_nit(e), [&](auto nit) {
            lift<16, 32>(nc <= 16 ? 16 : 32, [&](auto cap) {
                launch_lds(e, &bigssdet_kernel<decltype(nit)::value, decltype(cap)::value>, bg, dim3(256), fit.bytes, s, pl->xri.p, pl->pnr.p, pl->vad_ci.p, d.wfft,
                           d.window, nc, (int64_t)x.total_frames, e->big_tw.p, e->big_han.p, (float)d.o.nr_a, two);
            });
        });
        HIP_TRY(hipGetLastError());
        if (streamed) {  // the chains of the push, the detector's record in every stream's slot
            SsDecideStreamParams sp;
            sp.ci = pl->vad_ci.p; sp.tiles = pl->tiles.p; sp.tile_stream = pl->tile_utt.p; sp.heads = x.heads; sp.n_heads = x.n_heads;
            sp.xstate = static_cast<float *>(x.xstate); sp.slot_floats = xs_ss_big_floats(big_nit(e)); sp.det_doubles = xs_ss_big_doubles(big_nit(e));
            sp.nc = nc; sp.ninit = d.o.nr_initsegs; sp.pcoef = d.o.nr_p; sp.qcoef = d.o.nr_q; sp.vbits = pl->ss_vbits.p;
            hipLaunchKernelGGL(ss_decide_stream_kernel, dim3((unsigned)std::max(1, x.n_heads)), dim3(64), 0, s, sp);
        } else
            hipLaunchKernelGGL(ss_decide_kernel, dim3((unsigned)pl->hp.n_utt), dim3(64), 0, s, pl->vad_ci.p, pl->d_row_off.p, pl->hp.n_utt, nc, d.o.nr_initsegs,
                               (double)d.o.nr_p, (double)d.o.nr_q, pl->ss_vbits.p);
        HIP_TRY(hipGetLastError());
    }
    const LdsFit fit = bigss_lds(d, e->tab.feat, e->tab.p2.ncoef_out, e->tab.big_fb_total);
    if (fit.bytes > 160 * 1024) throw std::runtime_error("filter bank too wide for the LDS tables of the large-FFT kernel");
    if (!e->geom.per_wave) throw std::runtime_error("internal: hwss / fwss / 2fwss without chains");
    return [e, s, &bp, streamed, shm = fit.bytes] {
        lift<8, 16>(big_nit(e), [&](auto nit) {
            constexpr int NIT = decltype(nit)::value;
            if (streamed) launch_lds(e, &bigss_kernel<NIT, true>, dim3((unsigned)std::max(1, bp.n_chains)), dim3(256), shm, s, bp);
            else launch_lds(e, &bigss_kernel<NIT>, dim3((unsigned)std::max(1, bp.n_chains)), dim3(256), shm, s, bp);
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
    const size_t nk = (size_t)pl->hp.n_utt * d.K;
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
        for (int i = 0; i < pl->hp.n_utt; i++) {
            scaled(&dst[(size_t)i * d.K], prev >= 0 ? &last[(size_t)prev * d.K] : e->ss_stale.data(), skipped);
            if (pl->hp.frames[i] > 0) {
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
    std::vector<unsigned char> dirty(std::max(pl->hp.n_utt, 1), 1);
    if (e->tab.ss_file) {
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
        kp.ss_cached = e->tab.ss_file || iter > 0;
        HIP_TRY(hipMemcpyAsync(pl->ss_seed.p, seed.data(), nk * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(pl->ss_dirty.p, dirty.data(), dirty.size(), hipMemcpyHostToDevice, s));
        pass();
        HIP_TRY(hipMemcpyAsync(last.data(), pl->ss_last.p, nk * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        propagate(next);
        bool any = false;
        for (int i = 0; i < pl->hp.n_utt; i++) {
            dirty[i] = std::memcmp(&next[(size_t)i * d.K], &seed[(size_t)i * d.K], d.K * sizeof(float)) != 0;
            any = any || dirty[i];
        }
        if (!any) break;
        if (iter > pl->hp.n_utt) throw std::runtime_error("internal: noise seeds of the *ss chain did not settle");
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
    tp.lifter = e->tab.big ? e->big_lifter.p : e->ftab.p + e->tab.p2.lift_off;
    tp.row_slot = e->tab.big ? e->big_slot.p : e->itab.p + e->tab.p2.NS + 1;
    tp.stride = kp.lp_stride; tp.D = kp.D; tp.lporder = kp.lporder; tp.ncep = kp.ncep; tp.is_lpa = kp.lp_is_lpa;
    tp.lifter_on = kp.lifter_on; tp.e_mode = kp.e_mode; tp.e_slot = kp.e_slot;
    tp.inv_stride = (unsigned)((1ull << 32) / (unsigned)tp.stride) + 1u;
    tp.inv_D = (unsigned)((1ull << 32) / (unsigned)tp.D) + 1u;
    const LdsFit fit = lp_tail_lds(tp.stride, tp.D, e->geom.lags_double);
    const dim3 tg((unsigned)std::max<int64_t>(1, std::min<int64_t>((x.total_frames + 255) / 256, (int64_t)e->n_cu * fit.per_cu)));
    if (e->geom.lags_double) launch_lds(e, &lp_tail_kernel<double, 0>, tg, dim3(256), fit.bytes, s, tp);
    else if (kp.lporder == 12 && kp.ncep == 12 && !kp.lp_is_lpa) launch_lds(e, &lp_tail_kernel<float, 12>, tg, dim3(256), fit.bytes, s, tp);
    else launch_lds(e, &lp_tail_kernel<float, 0>, tg, dim3(256), fit.bytes, s, tp);
    HIP_TRY(hipGetLastError());
}

// The VAD's Burg-cepstral criterion outside the fused path, on the spectra the front end exported: bigburg_kernel at 1024 .. 4096 points
// (a workgroup per frame), vad_burg_kernel below (a wave per frame; Q samples per lane: windows of up to 256 samples, or longer)
void stage_burg_vad(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s) {
    const ctu::Design &d = *e->design;
    const int cap = e->vp.ncoef <= 16 ? 16 : 32;
    if (e->tab.big && x.total_frames > 0) {
        const LdsFit fit = bigburg_lds(d.wfft);
        const dim3 g((unsigned)std::min<int64_t>(x.total_frames, (int64_t)e->n_cu * fit.per_cu));
        lift<4, 8, 16>(big_nit(e), [&](auto nit) {
            lift<16, 32>(cap, [&](auto nc) {
                launch_lds(e, &bigburg_kernel<decltype(nit)::value, decltype(nc)::value>, g, dim3(256), fit.bytes, s, pl->xri.p, pl->pnr.p, pl->vad_ci.p, e->vp,
                           (int64_t)x.total_frames, e->big_tw.p);
            });
        });
    } else if (!e->tab.big) {
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
    const TrapPath tp = trap_path(d.B, tl, nd);  // layout_constants.h: which kernel, its instantiation and its dynamic LDS
    if (tp.split16 != (e->tab.trap_bf16 ? 1 : 0)) throw std::runtime_error("internal: the TRAP tables are not those of the kernel trap_path names");
    if (tp.split16) {
        launch_lds(e, &trapdct_split16_kernel, dim3(std::max(pl->hp.n_chunks128, 1)), dim3(512), (size_t)tp.lds_bytes, s, (const float *)pl->logmel.p, d_rows,
                   (const uint4 *)e->trapG16.p, (const int4 *)pl->utt_info.p, (const int *)pl->trap_chunks128.p, pl->hp.n_chunks128, d.B, tl, nd, d.D);
    } else {
        // 50 and 51 bands on contexts of 245 frames and more ask for up to 67 324 bytes (tile and mask): launch_lds raises the limit there
        lift<1, 2>(tp.nrb, [&](auto nrb) {
            lift<TRAP_COMP_STEPS, 64>(tp.nsm, [&](auto nsm) {
                launch_lds(e, &trapdct_mfma_kernel<decltype(nrb)::value, decltype(nsm)::value>, dim3(pl->hp.n_chunks), dim3(256), (size_t)tp.lds_bytes, s,
                           (const float *)pl->logmel.p, d_rows, (const float *)e->trapG.p, (const int4 *)pl->utt_info.p, (const int *)pl->trap_chunks.p, d.B, tl, nd,
                           d.D);
            });
        });
    }
    HIP_TRY(hipGetLastError());
}

// The wide DCT tail (dctw_kernel.h) over the band logarithms the front end left, into the rows the front end would have written
void stage_dctw(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, const KParams &kp) {
    DctwParams wp;
    wp.logmel = pl->logmel.p; wp.rows = kp.rows; wp.atab = e->dctw_tab.p; wp.total_frames = x.total_frames;
    wp.B = kp.B; wp.D = kp.D; wp.nout = e->tab.dctw_nout; wp.chunks = e->tab.dctw_chunks;
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
    const int pgrid = std::min(pl->hp.n_chunks, e->n_cu * 8);
    const bool std39 = !d.post_stack && d.post_order == 2 && pp.fea_c == 13 && d.Dbase == 13 && d.D == 39 && pp.w[0] == 2 && pp.w[1] == 2;
    lift<0, 1>(std39, [&](auto v) {
        hipLaunchKernelGGL(post_kernel<decltype(v)::value != 0>, dim3(pgrid), dim3(256), shm, s, pl->base_rows.p, d_rows, pl->utt_info.p, pl->trap_chunks.p, pl->hp.n_chunks, pp);
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
    if (d.cms == 1) hipLaunchKernelGGL(cms_exp_kernel, dim3((pl->hp.n_utt + 1) / 2), dim3(64), 0, s, pl->base_rows.p, d_rows, pl->utt_info.p, pl->hp.n_utt, cp);
    else
        hipLaunchKernelGGL(cms_block_kernel, dim3(pl->hp.n_chunks), dim3(256), (size_t)(64 + cp.L - 1) * cp.ncols * sizeof(float), s, pl->base_rows.p, d_rows,
                           pl->utt_info.p, pl->trap_chunks.p, cp);
    HIP_TRY(hipGetLastError());
}

// The fused path left the lattice's output of every frame behind: the coefficient recursion and a -> c one frame per lane,
// then the detector's recurrences, sixteen utterances per wave
void stage_fused_vad(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, hipStream_t s, uint8_t *d_vad, bool replay) {
    hipLaunchKernelGGL((vad_a2c_kernel<VF_NC>), dim3((unsigned)((x.total_frames + 255) / 256)), dim3(256), 0, s, pl->vad_cf.p, (int64_t)x.total_frames);
    if (replay) lift<0, 1, 2, 3>(e->vp.thr, [&](auto thr) {
        hipLaunchKernelGGL((vad_lanes_kernel<VF_NC, decltype(thr)::value>), dim3((pl->hp.n_live + 15) / 16), dim3(64), 0, s, pl->vad_cf.p, pl->vf_order.p, pl->hp.n_live,
                           pl->d_row_off.p, d_vad, e->vp);
    });
    HIP_TRY(hipGetLastError());
}

// After the post passes: the `fea` criterion reads the vector the writer sees (CMS applied), and the energy
// column is shifted in the finished rows.
void stage_vad_decide(ctu_engine *e, const ctu_plan *pl, hipStream_t s, float *d_rows, uint8_t *d_vad) {
    hipLaunchKernelGGL(vad_decide_kernel, dim3(pl->hp.n_utt), dim3(64), 0, s, pl->vad_ci.p, pl->pnr.p, d_rows, pl->d_row_off.p, pl->hp.n_utt, d_vad, e->vp);
    HIP_TRY(hipGetLastError());
}

// A file with no more frames than the majority filter delays never gets the filter `ready` (src/vad/vad.h:126-136), so
// BATCH::flush_vad's loop does not start (src/vad/vad.cc:742-745, src/io/batch.cc:243-249): the reference writes neither a
// row nor a decision for it.  Its decision bytes become NUL ("nothing written"); ctu_engine_run_host reports 0 rows.
void stage_short_files(ctu_engine *e, const ctu_plan *pl, hipStream_t s, uint8_t *d_vad) {
    hipLaunchKernelGGL(vad_short_files_kernel, dim3((unsigned)((pl->hp.n_utt + 255) / 256)), dim3(256), 0, s, d_vad, pl->d_row_off.p, pl->hp.n_utt,
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
        launch_lds(e, &bigsynth_kernel<decltype(nit)::value>, dim3(g), dim3(256), fit.bytes, s, pl->xri.p, e->geom.pss ? pl->pss.p : pl->pnr.p, pl->ybuf.p,
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
        else if (n == "trap_path") {  // the launch of offline TRAP-DCT (trap_path, layout_constants.h), then whether ctu_engine_create takes the configuration
            if (d.kind != ctu::FeaKind::TrapDct) {
                g_create_error = "trap_path: not a trapdct configuration";
                return CTU_ERR_INPUT;
            }
            spread_small_fft(d);
            std::string why;
            const TrapPath p = trap_path(d.B, d.o.fea_trapdct_traplen, d.o.fea_trapdct_ndct);
            v = {(double)p.split16, (double)p.nrb, (double)p.nsm, (double)p.lds_bytes, (double)p.big_lds, ctu::create_check(d, why) == CTU_OK ? 1.0 : 0.0};
        }
        else if (n == "host_tables") v = host_tables_report(d);  // EngineTables and VadParams as ctu_engine_create builds them (include/ctu_engine.h)
        else if (n == "tile_frames") v = {(double)TILE};  // frames per tile record of a plan (offline, and of a stream set's pushes)
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
        e->sp = spread_small_fft(d);
    } catch (const std::exception &ex) {
        g_create_error = ex.what();
        return CTU_ERR_OPTS;
    }
    if (const int rc = create_check(*e->design, g_create_error)) return rc;
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
        if (e->design->rows_in) e->kname = "rows_ingest_kernel";  // no front end: no tables, no parameter blocks
        else {
            e->tab = build_engine_tables(*e->design);
            build_tables(e.get());
        }
        e->geom = plan_geom(*e->design, e->tab, e->sp, e->n_cu);
        e->vp = vad_params(*e->design, e->sp);
        if (!e->geom.rows_in) e->kp0 = engine_kparams(e.get());
        if (e->tab.big) e->bp0 = engine_bigparams(e.get());
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
    out->wfft = e->sp.user_wfft;
    out->nbins = e->sp.user_K;
    return CTU_OK;
}

int64_t ctu_num_frames(const ctu_engine *e, int64_t n) { return plan_num_frames(e->geom, n); }
int64_t ctu_arena_layout(const int64_t *utt_nsamples, int32_t n_utt, int64_t *sample_off) { return arena_layout(utt_nsamples, n_utt, sample_off); }
int64_t ctu_rows_arena_layout(const int64_t *utt_rows, int32_t n_utt, int32_t width, int64_t *word_off) { return rows_arena_layout(utt_rows, n_utt, width, word_off); }

namespace {
// The device side of a plan: the images of the HostPlan's lists, and the scratch of every stage by its PlanScratch.  No arithmetic and
// no decision here: a list or a count that is empty or zero is not there (DevBuf).  Throws (ctu_plan_create's frame).
void plan_upload(ctu_engine *e, ctu_plan *pl) {
    static_assert(sizeof(UttInfo) == sizeof(int4), "the utterance info is read as int4 records");
    const HostPlan &h = pl->hp;
    const PlanScratch &n = h.scratch;
    HIP_TRY(hipSetDevice(e->device));
    pl->tiles.upload(h.tiles);
    pl->wg_first.upload(h.heads);
    pl->utt_info.upload(h.uinfo);
    pl->trap_chunks.upload(h.chunks);
    pl->trap_chunks128.upload(h.chunks128);
    pl->tile_utt.upload(h.tile_utt);
    pl->vf_order.upload(h.vf_order);
    if (n.d_sample_off) pl->d_sample_off.upload(h.sample_off);
    if (n.d_row_off) pl->d_row_off.upload(h.row_off);
    pl->base_rows.alloc((size_t)n.base_rows);
    pl->ss_seed.alloc((size_t)n.ss_seed);
    pl->ss_last.alloc((size_t)n.ss_last);
    pl->ss_dirty.alloc((size_t)n.ss_dirty);
    pl->ss_vbits.alloc((size_t)n.ss_vbits);
    pl->xri.alloc((size_t)n.xri);
    pl->pnr.alloc((size_t)n.pnr);
    pl->pss.alloc((size_t)n.pss);
    pl->vad_ci.alloc((size_t)n.vad_ci);
    pl->vad_cf.alloc((size_t)n.vad_cf);
    pl->ybuf.alloc((size_t)n.ybuf);
    pl->dc1m.alloc((size_t)n.dc1m);
    pl->dc1.alloc((size_t)n.dc1);
    pl->logmel.alloc((size_t)n.logmel);
    pl->lp_r.alloc((size_t)n.lp_r);
}
}  // namespace

// The plan of the engine's geometry (built at create) over the batch, on the host (plan.cc: layout, refusals, chains, lists, scratch
// sizes); then its images and its scratch on the device.
int ctu_plan_create(ctu_engine *e, const int64_t *utt_nsamples, int32_t n_utt, ctu_plan **out) {
    if (!e || !out || n_utt < 0 || (n_utt && !utt_nsamples)) return CTU_ERR_INPUT;
    *out = nullptr;
    std::unique_ptr<ctu_plan> pl(new ctu_plan);
    pl->eng = e;
    std::string why;
    if (const int rc = build_host_plan(e->geom, utt_nsamples, n_utt, pl->hp, why); rc != CTU_OK) {
        set_error(e, why);
        return rc;
    }
    const int rc = guarded(e, [&]() -> int {
        plan_upload(e, pl.get());
        return CTU_OK;
    });
    if (rc != CTU_OK) return rc;
    pl->ext.n_tiles = (int)pl->hp.tiles.size();
    pl->ext.grid = pl->hp.grid;
    pl->ext.total_frames = pl->hp.total_frames;
    pl->ext.heads = pl->wg_first.p;
    pl->ext.n_heads = (int)pl->wg_first.n;
    *out = pl.release();
    return CTU_OK;
}

void ctu_plan_destroy(ctu_plan *p) { delete p; }
const int64_t *ctu_plan_sample_offsets(const ctu_plan *p) { return p->hp.sample_off.data(); }
const int64_t *ctu_plan_row_offsets(const ctu_plan *p) { return p->hp.row_off.data(); }
int64_t ctu_plan_total_samples(const ctu_plan *p) { return p->hp.total_samples; }
int64_t ctu_plan_total_frames(const ctu_plan *p) { return p->hp.total_frames; }

void ctu_vad_ring_step(int32_t order, int64_t frames, int32_t *hidx, int32_t *hsize) { vad_ring_step(order, frames, hidx, hsize); }
int64_t ctu_vad_ring_rows(int32_t order, int64_t frames, int32_t hidx0, int32_t *src) { return vad_ring_rows(order, frames, hidx0, src); }

int ctu_plan_set_vad_ring(ctu_plan *pl, const int32_t *hidx) {
    if (!pl) return CTU_ERR_INPUT;
    ctu_engine *e = pl->eng;
    pl->ring_hidx.clear();
    if (!hidx || !e->geom.do_vad) return CTU_OK;
    const std::vector<int> src = plan_ring_src(pl->hp, e->design->o.vad_filter_order, hidx);
    if (src.empty()) return CTU_OK;  // every utterance is in phase
    const int rc = guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        pl->ring_hidx.assign(hidx, hidx + pl->hp.n_utt);
        pl->ring_src.upload(src);
        pl->ring_tmp.reserve(src.size() * e->design->D);
        return CTU_OK;
    });
    if (rc != CTU_OK) pl->ring_hidx.clear();  // a plan without its ring is in phase
    return rc;
}

// A run of a plan over the extent `x`: the plan's own, or the front of it a push of a stream set covers.  `row_stages` off stops ahead of
// stage_post and stage_cms with the base rows in the plan's scratch: a stream set with row state runs its own forms of the two
// (stream_rows_kernels.h) over them and its history.  It stops ahead of stage_trap likewise, with the log-mel rows in the plan's scratch: a
// stream set with trap state contracts them with its history (stream_trap_kernels.h); an offline run always has row_stages on.  `vad_stages` off likewise leaves the VAD's sequential stages out - the detector's
// replay, the short files' bytes, the ring - with the criterion's input of every frame in the plan's scratch (vad_cf / vad_ci / the
// energy): a stream set with detector state replays them from its own state (stream_vad_kernels.h) and needs no d_vad here.
static int run_chain(ctu_engine *e, const ctu_plan *pl, const RunExtent &x, const int16_t *d_pcm, float *d_rows, uint8_t *d_vad, void *stream, bool row_stages,
                     bool vad_stages = true) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (e->geom.rows_in) {
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
    if (!d_pcm || (!signal && !d_rows) || (e->geom.do_vad && vad_stages && !d_vad)) {
        set_error(e, "ENGINE: null device buffer");
        return CTU_ERR_INPUT;
    }
    hipStream_t s = (hipStream_t)stream;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        KParams kp = run_kparams(e, pl, x, d_pcm, d_rows);
        BigParams bp = e->tab.big ? run_bigparams(e, pl, x, kp) : BigParams{};
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
        // a stream set with subtraction state: every file of a stream is a first file, so the seed is zero and there is nothing to iterate -
        // one pass from the streams' own state, no read-back, and the engine's offline chain (ss_stale, vad_pos) is neither read nor written
        const bool ss_streamed = e->tab.ss && x.xstate != nullptr;
        if (ss_streamed) {
            if ((e->tab.path != BIG_NONE && e->tab.path != BIG_SS) || e->tab.ss_file) throw std::runtime_error("internal: a streamed *ss configuration outside the detector paths");
            kp.ss_cached = 0;
            kp.ss_dirty = nullptr;
            kp.ss_seed = nullptr;
            kp.ss_last = nullptr;
            bp.ss_dirty = nullptr;
            bp.ss_seed = nullptr;
            bp.ss_last = nullptr;
        }
        switch (e->tab.path) {
            case BIG_NONE: if (!e->tab.ss || ss_streamed) pass(); break;
            case BIG_WAVE1K: stage_wave1k(e, pl, x, s, bp); break;
            case BIG_SS:  // (streamed: export, detector, streamed decide, then bigss_kernel<NIT, true> once)
                pass = stage_bigss_front(e, pl, x, s, bp);
                if (ss_streamed) pass();
                break;
            case BIG_FFT: launch_bigfft(e, x, s, bp); break;
        }
        if (e->tab.ss && !ss_streamed) {
            const int rc = run_ss_chain(e, pl, x, s, kp, pass);
            if (rc != CTU_OK) return rc;
        }
        if (e->tab.dctw) stage_dctw(e, pl, x, s, kp);  // (inside the timed span: the tail finishes what the front end of a narrower chain does itself)
        HIP_TRY(hipEventRecord(e->ev1, s));
        e->timed = true;
        e->host_timed = false;
        HIP_TRY(hipGetLastError());
#if CTU_STAMP
        if (const char *sf = getenv("CTU_STAMP_FILE")) dump_stamps(e, grid, s, sf);
#endif
        if (e->geom.lp_tail) stage_lp_tail(e, pl, x, s, kp);
        if (e->geom.vad_burg) stage_burg_vad(e, pl, x, s);
        if (d.kind == ctu::FeaKind::TrapDct && row_stages) stage_trap(e, pl, s, d_rows);
        if (d.post_order > 0 && row_stages) stage_post(e, pl, s, d_rows);
        if (d.cms && row_stages) stage_cms(e, pl, s, d_rows);
        if (e->geom.vad_fused && pl->hp.n_live > 0) stage_fused_vad(e, pl, x, s, d_vad, vad_stages);
        if (e->geom.do_vad && !e->geom.vad_fused && vad_stages) stage_vad_decide(e, pl, s, d_rows, d_vad);
        if (e->geom.do_vad && d.o.vad_filter_order > 1 && vad_stages) stage_short_files(e, pl, s, d_vad);
        if (e->geom.do_vad && !pl->ring_hidx.empty() && x.total_frames > 0 && vad_stages) stage_ring_gather(e, pl, x, s, d_rows);
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
    pl->part_first = plan_part_first(pl->hp, nparts);
    for (size_t k = 0; k + 1 < pl->part_first.size(); k++) {
        ctu_plan *sub = nullptr;
        const int u0 = pl->part_first[k], u1 = pl->part_first[k + 1];
        const int rc = ctu_plan_create(e, pl->hp.nsamples.data() + u0, u1 - u0, &sub);
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
// options, so e->tab.ss is 0 there.
int host_chunks(const ctu_engine *e, const ctu_plan *pl, int64_t input_bytes, bool pinned) {
    if (e->tab.ss) return 1;
    // pageable buffers go through blocking staged copies: cutting those up only adds calls (measured 1.04e8 -> 0.96e8 frames/s)
    int k = (pinned && pl->hp.n_utt >= 16 && input_bytes >= (int64_t)32 << 20) ? 8 : 1;
    if (const char *v = getenv("CTU_HOST_CHUNKS")) k = std::max(1, atoi(v));
    return std::min(k, std::max(1, pl->hp.n_utt));
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
    // wire input only (else empty / negative): which bytes of the caller's buffer a (sub)plan that starts at utterance `first` uploads - the
    // covering range of its utterances, not a slice of an arena; called ahead of `stage` - and the bytes the 32 MiB rule judges the run by
    std::function<std::pair<const char *, size_t>(ctu_plan *sub, int first)> range;
    int64_t judged_bytes = -1;
    std::function<void(ctu_plan *)> prepare;  // what every (sub)plan needs on the device ahead of the walk, so that no range allocates inside it
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
    const int nparts = host_chunks(e, pl, in.judged_bytes >= 0 ? in.judged_bytes : pl->hp.total_samples * (int64_t)in.elem, pin_in && pin_out);
    if (const int rc = split_host_parts(e, pl, nparts); rc != CTU_OK) return rc;
    const bool ranges = nparts > 1 && pl->parts.size() > 1;
    const int np = ranges ? (int)pl->parts.size() : 1;
    auto part = [&](int k) { return ranges ? pl->parts[k].get() : pl; };
    auto first = [&](int k) { return ranges ? pl->part_first[k] : 0; };
    if (in.prepare)
        for (int k = 0; k < np; k++) in.prepare(part(k));
    const hipStream_t st[2] = {ranges ? pl->part_stream[0] : nullptr, ranges ? pl->part_stream[1] : nullptr};
    RangeEvents events;
    auto download = [&](int k) {
        ctu_plan *sp = part(k);
        if (sp->ext.total_frames == 0) return;
        float *dst = h_rows + pl->hp.row_off[first(k)] * D;
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
            // a part's arena is the slice of the caller's that starts `head` elements ahead of its first utterance (split_host_parts)
            const char *src = static_cast<const char *>(in.base) + (pl->hp.sample_off[first(k)] - in.head) * (int64_t)in.elem;
            size_t bytes = (size_t)sp->hp.total_samples * in.elem;
            if (in.range) std::tie(src, bytes) = in.range(sp, first(k));
            void *d_in = in.stage(sp);
            sp->h_rows.reserve((size_t)sp->ext.total_frames * D);
            if (pin_in) HIP_TRY(hipMemcpyAsync(d_in, src, bytes, hipMemcpyHostToDevice, st[k & 1]));
            else HIP_TRY(hipMemcpy(d_in, src, bytes, hipMemcpyHostToDevice));
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
            if (part(k)->ext.total_frames) in.vad(part(k), pl->hp.row_off[first(k)]);
    return CTU_OK;
}
}  // namespace

// The host-buffer run of a plan over samples behind its checks (ctu_engine_run_host, ctu_engine_run_wire_host): `in` says what goes up and
// how a range runs; the VAD's bytes, -vad_apply_mode drop and rows_per_utt are one statement for both.
static int run_host_samples(ctu_engine *e, ctu_plan *pl, HostInput &in, float *h_rows, uint8_t *h_vad, int64_t *rows_per_utt) {
    const ctu::Design &d = *e->design;
    return guarded(e, [&]() -> int {
        std::vector<uint8_t> v(e->geom.do_vad ? (size_t)pl->ext.total_frames : 0);
        if (e->geom.do_vad) {
            in.ring = [&](ctu_plan *sub, int first) { return ctu_plan_set_vad_ring(sub, pl->ring_hidx.empty() ? nullptr : pl->ring_hidx.data() + first); };
            in.vad = [&](const ctu_plan *p, int64_t row0) { HIP_TRY(hipMemcpy(v.data() + row0, p->h_vad.p, (size_t)p->ext.total_frames, hipMemcpyDeviceToHost)); };
        }
        if (const int rc = run_host_ranges(e, pl, in, h_rows); rc != CTU_OK) return rc;
        if (e->geom.do_vad) {
            if (h_vad) std::memcpy(h_vad, v.data(), v.size());
            if (d.o.vad_apply_mode == "drop") {
                // rows of non-speech frames are dropped (src/io/batch.cc:237-238): compact each utterance in place
                for (int i = 0; i < pl->hp.n_utt; i++) {
                    const int64_t r0 = pl->hp.row_off[i], T = pl->hp.frames[i];
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
                for (int i = 0; i < pl->hp.n_utt; i++)
                    if (pl->hp.frames[i] <= delay) rows_per_utt[i] = 0;
            }
        }
        return CTU_OK;
    });
}

int ctu_engine_run_host(ctu_engine *e, const ctu_plan *pl_, const int16_t *h_pcm, float *h_rows, uint8_t *h_vad,
                        int64_t *rows_per_utt) {
    if (!e || !pl_ || pl_->eng != e) return CTU_ERR_INPUT;
    if (e->geom.rows_in) {
        set_error(e, "ENGINE: this configuration starts from feature files (-format_in htk): use ctu_engine_run_rows_host");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);  // the device copies live in the plan
    if (rows_per_utt)
        for (int i = 0; i < pl->hp.n_utt; i++) rows_per_utt[i] = pl->hp.frames[i];
    if (pl->ext.total_frames == 0) return CTU_OK;
    if (!h_pcm || !h_rows) {
        set_error(e, "ENGINE: null host buffer");
        return CTU_ERR_INPUT;
    }
    HostInput in{h_pcm, sizeof(int16_t), PCM_HEAD};
    in.stage = [&](ctu_plan *p) {
        p->h_pcm.reserve((size_t)p->hp.total_samples);
        if (e->geom.do_vad) p->h_vad.reserve((size_t)p->ext.total_frames);
        return p->h_pcm.p;
    };
    in.run = [&](ctu_plan *p, hipStream_t s) { return ctu_engine_run(e, p, p->h_pcm.p, p->h_rows.p, p->h_vad.p, s); };
    return run_host_samples(e, pl, in, h_rows, h_vad, rows_per_utt);
}

// ---- runs that start from rows (-format_in htk) ------------------------------------------------------------------------------
// Stages: ingest (rows_in_kernels.h) -> 7 delta chain / stacking -> 8 CMS; CMVN is the caller's, over the resulting rows.
int ctu_engine_run_rows(ctu_engine *e, const ctu_plan *pl, const void *d_rows_in, float *d_rows, void *stream) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    if (!e->geom.rows_in) {
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
        // (staged: the passes behind read the plan's base rows, else the ingest writes the caller's)
        uint32_t *dst = reinterpret_cast<uint32_t *>(e->geom.staged ? pl->base_rows.p : d_rows);
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
    if (!e->geom.rows_in) {
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
            p->h_words.reserve((size_t)p->hp.total_samples);
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
        if (e->geom.rows_in) {  // feature files: slot k is vector entry k, written to column k (src/fea/post_impl.cc:55-57, src/io/out.cc:177-179)
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
    if (n_spk < 1 || (pl->hp.n_utt && !spk_of_utt)) {
        set_error(e, "ENGINE: speaker table missing");
        return CTU_ERR_INPUT;
    }
    for (int i = 0; i < pl->hp.n_utt; i++)
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
        std::vector<int> spk(spk_of_utt, spk_of_utt + pl->hp.n_utt);
        e->d_spk.upload(spk);
        std::vector<double> zero((size_t)n_spk * (cols + 1), 0.0);
        e->d_stat_a.upload(zero);
        if (mean) e->d_stat_b.upload(std::vector<double>(mean, mean + (size_t)n_spk * cols));
        hipLaunchKernelGGL(cmvn_accumulate_kernel, dim3(pl->hp.n_chunks), dim3(256), 0, s, d_rows, pl->utt_info.p,
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
        std::vector<int> spk(spk_of_utt, spk_of_utt + pl->hp.n_utt);
        e->d_spk.upload(spk);
        e->d_stat_a.upload(std::vector<double>(mean, mean + (size_t)n_spk * cols));
        e->d_stat_b.upload(std::vector<double>(var, var + (size_t)n_spk * cols));
        hipLaunchKernelGGL(cmvn_apply_kernel, dim3(pl->hp.n_chunks), dim3(256), 0, s, d_rows, pl->utt_info.p,
                           pl->trap_chunks.p, e->d_spk.p, e->d_slot_of_col.p, e->d_stat_a.p, e->d_stat_b.p, cols, e->design->D);
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
}

const int64_t *ctu_plan_out_samples(const ctu_plan *p) { return p->hp.out_samples.empty() ? nullptr : p->hp.out_samples.data(); }

int ctu_engine_run_signal(ctu_engine *e, const ctu_plan *pl, const int16_t *d_pcm, int16_t *d_out, void *stream) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    const ctu::Design &d = *e->design;
    if (!d.signal_out) {
        set_error(e, "ENGINE: ctu_engine_run_signal needs -format_out raw|wave");
        return CTU_ERR_INPUT;
    }
    if (pl->hp.n_utt == 0) return CTU_OK;
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
        if (pl->ext.total_frames > 0 && e->tab.big) launch_bigsynth(e, pl, pl->ext, s, sp.inv_n);  // (below 1024 points the front end's SY instantiations wrote the frames)
        int64_t longest = 0;
        for (int64_t n : pl->hp.out_samples) longest = std::max(longest, n);
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((longest + 255) / 256, 64));
        hipLaunchKernelGGL(ola_kernel, dim3(gx, pl->hp.n_utt), dim3(256), 0, s, pl->ybuf.p, d_out, pl->utt_info.p, pl->d_sample_off.p,
                           pl->hp.n_utt, sp);
        HIP_TRY(hipGetLastError());
        return CTU_OK;
    });
}

int ctu_engine_run_signal_host(ctu_engine *e, const ctu_plan *pl, const int16_t *h_pcm, int16_t *h_out) {
    if (!e || !pl || pl->eng != e) return CTU_ERR_INPUT;
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        DevBuf<int16_t> pcm, out;
        pcm.alloc((size_t)pl->hp.total_samples);
        out.alloc((size_t)pl->hp.total_samples);
        HIP_TRY(hipMemcpy(pcm.p, h_pcm, (size_t)pl->hp.total_samples * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(out.p, 0, (size_t)pl->hp.total_samples * 2));
        const int rc = ctu_engine_run_signal(e, pl, pcm.p, out.p, nullptr);
        if (rc != CTU_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, out.p, (size_t)pl->hp.total_samples * 2, hipMemcpyDeviceToHost));
        return CTU_OK;
    });
}

// ---- offline wire input: a plan's utterances out of G.711 codes, swapped and channel-interleaved PCM (wire_in_kernels.h, wire_plan.h)
namespace {
// What the three wire calls refuse before anything is launched, uploaded or written.  `rows_call`: the call to use on an engine over rows.
int wire_run_refusal(ctu_engine *e, const ctu_plan *pl, const void *buf, const int64_t *elem_off, const ctu_wire_layout *w, const char *rows_call) {
    if (pl->eng != e) {
        set_error(e, "wire: a plan of another engine");
        return CTU_ERR_INPUT;
    }
    if (e->geom.rows_in) {
        set_error(e, std::string("ENGINE: this configuration starts from feature files (-format_in htk): use ") + rows_call);
        return CTU_ERR_INPUT;
    }
    const std::string why = wire_unpack_fault(w, buf, pl->hp.n_utt, pl->hp.nsamples.data(), elem_off);
    if (!why.empty()) {
        set_error(e, why);
        return CTU_ERR_INPUT;
    }
    return CTU_OK;
}
bool plan_has_samples(const ctu_plan *pl) {
    for (int64_t n : pl->hp.nsamples)
        if (n > 0) return true;
    return false;
}
// What the plan keeps on the device for wire_unpack_kernel, made by the first call (throws)
void wire_prepare(ctu_plan *pl) {
    if (pl->wire_free) return;
    pl->wire_n.upload(pl->hp.nsamples);
    if (!pl->d_sample_off.p) pl->wire_off.upload(pl->hp.sample_off);
    pl->wire_piece.upload(wire_pieces(pl->hp.sample_off.data(), pl->hp.n_utt));
    pl->wire_elem.alloc((size_t)pl->hp.n_utt);
    if (!pl->wire_stage) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&pl->wire_stage), (size_t)pl->hp.n_utt * sizeof(long long), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&pl->wire_free, hipEventDisableTiming));
}
// The launch behind the checks (throws): element offsets up from the plan's staging, stream-ordered; wire_unpack_kernel by the layout
void wire_unpack(ctu_engine *e, ctu_plan *pl, const void *d_in, const int64_t *elem_off, const ctu_wire_layout &w, int16_t *d_pcm, hipStream_t s) {
    HIP_TRY(hipSetDevice(e->device));
    wire_prepare(pl);
    HIP_TRY(hipEventSynchronize(pl->wire_free));  // the copy of the previous call has read the staging
    for (int i = 0; i < pl->hp.n_utt; i++) pl->wire_stage[i] = pl->hp.nsamples[i] > 0 ? elem_off[i] : 0;
    HIP_TRY(hipMemcpyAsync(pl->wire_elem.p, pl->wire_stage, (size_t)pl->hp.n_utt * sizeof(long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(pl->wire_free, s));
    WireUnpack p;
    p.src = d_in;
    p.elem_off = pl->wire_elem.p;
    p.sample_off = pl->d_sample_off.p ? pl->d_sample_off.p : pl->wire_off.p;
    p.nsamples = pl->wire_n.p;
    p.piece_first = pl->wire_piece.p;
    p.pcm = d_pcm;
    p.stride = w.stride;
    const unsigned pieces = (unsigned)(pl->wire_piece.n - 1);
    lift<CTU_WIRE_S16, CTU_WIRE_S16_SWAPPED, CTU_WIRE_ALAW, CTU_WIRE_MULAW>(w.format, [&](auto fmt) {
        lift<0, 1>(w.stride != 1, [&](auto strided) {
            hipLaunchKernelGGL((wire_unpack_kernel<decltype(fmt)::value, decltype(strided)::value != 0>), dim3(pieces), dim3(256), 0, s, p);
        });
    });
    HIP_TRY(hipGetLastError());
}
}  // namespace

int ctu_plan_unpack_wire(ctu_engine *e, const ctu_plan *pl_, const void *d_in, const int64_t *elem_off, const ctu_wire_layout *w, int16_t *d_pcm,
                         void *stream) {
    if (!e || !pl_) return CTU_ERR_INPUT;
    if (const int rc = wire_run_refusal(e, pl_, d_in, elem_off, w, "ctu_engine_run_rows"); rc != CTU_OK) return rc;
    if (!plan_has_samples(pl_)) return CTU_OK;
    if (!d_pcm) {
        set_error(e, "ENGINE: null device buffer");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);  // the staging lives in the plan
    return guarded(e, [&]() -> int {
        wire_unpack(e, pl, d_in, elem_off, *w, d_pcm, (hipStream_t)stream);
        return CTU_OK;
    });
}

int ctu_engine_run_wire_host(ctu_engine *e, const ctu_plan *pl_, const void *h_in, const int64_t *elem_off, const ctu_wire_layout *w, float *h_rows,
                             uint8_t *h_vad, int64_t *rows_per_utt) {
    if (!e || !pl_) return CTU_ERR_INPUT;
    if (const int rc = wire_run_refusal(e, pl_, h_in, elem_off, w, "ctu_engine_run_rows_host"); rc != CTU_OK) return rc;
    if (e->design->signal_out) {
        set_error(e, "ENGINE: this configuration writes speech (-format_out raw|wave): use ctu_engine_run_signal_wire_host");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);  // the device copies live in the plan
    if (pl->ext.total_frames && !h_rows) {
        set_error(e, "ENGINE: null host buffer");
        return CTU_ERR_INPUT;
    }
    if (rows_per_utt)
        for (int i = 0; i < pl->hp.n_utt; i++) rows_per_utt[i] = pl->hp.frames[i];
    if (pl->ext.total_frames == 0) return CTU_OK;
    const size_t unit = (size_t)wire_elem_bytes(w->format);
    const int64_t *ns = pl->hp.nsamples.data();
    struct Part {
        std::vector<int64_t> rel;  // the utterances' offsets from the first element the part uploads
        size_t bytes = 0;
    };
    std::map<const ctu_plan *, Part> parts;
    HostInput in{h_in, unit, 0};
    in.judged_bytes = wire_part_range(w, 0, pl->hp.n_utt, ns, elem_off, nullptr, nullptr) * (int64_t)unit;
    in.range = [&](ctu_plan *p, int first) {
        Part &pt = parts[p];
        pt.rel.resize((size_t)p->hp.n_utt);
        int64_t lo = 0;
        pt.bytes = (size_t)wire_part_range(w, first, first + p->hp.n_utt, ns, elem_off, &lo, pt.rel.data()) * unit;
        return std::make_pair(static_cast<const char *>(h_in) + lo * (int64_t)unit, pt.bytes);
    };
    in.stage = [&](ctu_plan *p) {
        p->h_wire.reserve(parts[p].bytes);
        p->h_pcm.reserve((size_t)p->hp.total_samples);
        if (e->geom.do_vad) p->h_vad.reserve((size_t)p->ext.total_frames);
        return p->h_wire.p;
    };
    in.prepare = [&](ctu_plan *p) {
        if (p->ext.total_frames) wire_prepare(p);
    };
    in.run = [&](ctu_plan *p, hipStream_t s) {
        wire_unpack(e, p, p->h_wire.p, parts[p].rel.data(), *w, p->h_pcm.p, s);
        return ctu_engine_run(e, p, p->h_pcm.p, p->h_rows.p, p->h_vad.p, s);
    };
    return run_host_samples(e, pl, in, h_rows, h_vad, rows_per_utt);
}

int ctu_engine_run_signal_wire_host(ctu_engine *e, const ctu_plan *pl_, const void *h_in, const int64_t *elem_off, const ctu_wire_layout *w,
                                    int16_t *h_out) {
    if (!e || !pl_) return CTU_ERR_INPUT;
    if (const int rc = wire_run_refusal(e, pl_, h_in, elem_off, w, "ctu_engine_run_rows_host"); rc != CTU_OK) return rc;
    if (!e->design->signal_out) {
        set_error(e, "ENGINE: ctu_engine_run_signal_wire_host needs -format_out raw|wave");
        return CTU_ERR_INPUT;
    }
    ctu_plan *pl = const_cast<ctu_plan *>(pl_);
    if (pl->hp.n_utt == 0) return CTU_OK;
    if (!h_out) {
        set_error(e, "ENGINE: null host buffer");
        return CTU_ERR_INPUT;
    }
    return guarded(e, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        const size_t unit = (size_t)wire_elem_bytes(w->format), total = (size_t)pl->hp.total_samples;
        std::vector<int64_t> rel((size_t)pl->hp.n_utt);
        int64_t lo = 0;
        const size_t bytes = plan_has_samples(pl) ? (size_t)wire_part_range(w, 0, pl->hp.n_utt, pl->hp.nsamples.data(), elem_off, &lo, rel.data()) * unit : 0;
        DevBuf<uint8_t> wire;
        DevBuf<int16_t> pcm, out;
        wire.alloc(bytes);
        pcm.alloc(total);
        out.alloc(total);
        HIP_TRY(hipMemset(pcm.p, 0, total * 2));
        HIP_TRY(hipMemset(out.p, 0, total * 2));
        if (bytes) {
            HIP_TRY(hipMemcpy(wire.p, static_cast<const char *>(h_in) + lo * (int64_t)unit, bytes, hipMemcpyHostToDevice));
            wire_unpack(e, pl, wire.p, rel.data(), *w, pcm.p, nullptr);
        }
        const int rc = ctu_engine_run_signal(e, pl, pcm.p, out.p, nullptr);
        if (rc != CTU_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(h_out, out.p, total * 2, hipMemcpyDeviceToHost));
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
    if (!e->tab.ss_file) {
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
        switch (e->tab.path) {
            case BIG_WAVE1K: n = "wave1k_kernel"; break;
            case BIG_SS: n = "bigss_kernel<" + std::to_string(big_nit(e)) + ">"; break;
            case BIG_FFT: n = "bigfft_kernel<" + std::to_string(big_nit(e)) + ">"; break;
            case BIG_NONE: n = fe_name(e->tab.sel); break;
        }
        if (e->tab.dctw) n = "dct_wide_kernel";  // the front end ahead of it is ctu_config_table(..., "frontend") / the FFT size
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
