// Streaming input: what a stream set is, worked out on the host before anything is allocated.  Plain C++ (no HIP call, no HIP type), beside
// stream_plan.h: streams_host.h creates a set by it, tests/host/stream_set_shape_check.cc compiles it with g++ alone.
//
//   stream_set_halo    the halo and the largest window of a set, from the Design and the flags alone (ctu_streams_config_check_ex has no engine)
//   StreamSetFacts     what the shape reads of an engine (EngineTables, PlanGeom, the build)
//   stream_set_shape   the kinds of state, the PushGeom (but for what the plan fills in), strides, the size of every per-set buffer -
//                      or the sentence of an engine and a set that do not fit each other, which streams_unsupported_reason should have refused
//   stream_step_args_ok, stream_rows_step, stream_signal_step   the arithmetic of the exported ctu_streams_*_step calls
#pragma once

#include <algorithm>
#include <cstdint>

#include "../../include/ctu_engine.h"
#include "design.h"
#include "stream_plan.h"

namespace {

// Limits of the stream kernels, restated for host-only code (streams_host.h holds them to stream_signal_kernels.h / stream_rows_kernels.h)
constexpr int SHAPE_OLA_TAIL_MAX = 512, SHAPE_OLA_BIG_TAIL_MAX = 4096, SHAPE_STREAM_MEANS = 32;

// a chain or a stacking; with detector state on a configuration with the VAD module the majority filter's delay; with trap state on
// -fea_kind trapdct half a context (nothing else holds rows beside either: refused at create); with signal state on speech output nothing
// Detector state behind row state (CTU_STREAMS_VAD_ROW_STATE beside the two, the VAD module with a chain, a stacking or CMS behind it):
// the halos add up - H = delay + h, wmax the chain's - and *vh (may be null) receives h, the part that is the majority filter's
constexpr uint32_t SHAPE_VAD_ROW_FLAGS = CTU_STREAMS_ROW_STATE | CTU_STREAMS_VAD_STATE | CTU_STREAMS_VAD_ROW_STATE;
inline bool stream_set_vad_rows(const ctu::Design &d, uint32_t flags) {
    return (flags & SHAPE_VAD_ROW_FLAGS) == SHAPE_VAD_ROW_FLAGS && d.o.do_vad() && (d.post_order > 0 || d.cms);
}
inline void stream_set_halo(const ctu::Design &d, uint32_t flags, int *H, int *wmax, int *vh = nullptr) {
    stream_halo(d.post_order, d.post_w, d.post_stack, H, wmax);
    if (vh) *vh = 0;
    if (stream_set_vad_rows(d, flags)) {
        const int h = (d.o.vad_filter_order - 1) / 2;
        *H += h;
        if (vh) *vh = h;
    } else if ((flags & CTU_STREAMS_VAD_STATE) && d.o.do_vad()) stream_vad_halo(d.o.vad_filter_order, H, wmax);
    if ((flags & CTU_STREAMS_TRAP_STATE) && d.kind == ctu::FeaKind::TrapDct) stream_trap_halo(d.o.fea_trapdct_traplen, H, wmax);
    if ((flags & CTU_STREAMS_SIGNAL_STATE) && d.signal_out) *H = *wmax = 0;
}

inline bool stream_step_args_ok(int window, int wshift, int64_t total) { return window >= 1 && wshift >= 1 && wshift <= window && total >= 0; }
// rows that have gone out after `total` samples; pending: the frames' rows still held back
inline int64_t stream_rows_step(int window, int wshift, int H, int wmax, int64_t total, int64_t *pending) {
    const int64_t F = stream_frames(total, window, wshift), R = stream_rows_out(H, wmax, F);
    if (pending) *pending = F - R;
    return R;
}
// ... behind the VAD module's majority filter of delay h as well (detector state behind row state)
inline int64_t stream_vad_rows_step(int window, int wshift, int h, int H, int wmax, int64_t total, int64_t *pending) {
    const int64_t F = stream_frames(total, window, wshift), R = stream_vad_rows_out(H, wmax, h, F);
    if (pending) *pending = F - R;
    return R;
}
// samples that have gone out after `total` samples; pending: the overlap-add's tail a finish delivers, once there is a frame
inline int64_t stream_signal_step(int window, int wshift, int64_t total, int64_t *pending) {
    const int64_t F = stream_frames(total, window, wshift);
    if (pending) *pending = F > 0 ? window - wshift : 0;
    return F * wshift;
}

struct StreamSetFacts {
    int ss = 0;               // EngineTables::ss, big, ss_file; path == BIG_WAVE1K; sel.mode
    bool big = false, ss_file = false, wave1k = false;
    int mode = 0;
    bool per_wave = false;    // PlanGeom::per_wave, chain_slots, max_wg
    int chain_slots = 0, max_wg = 0;
};

struct StreamSetShape {
    const char *refusal = nullptr;  // set: nothing else of the shape holds
    // detector, trap, signal state in use; a tail beyond SHAPE_OLA_TAIL_MAX entries (stream_ola_big_kernel); chains of whole streams; subtraction state
    bool vad = false, trap = false, signal = false, ola_big = false, chained = false, ss = false;
    bool vad_rows = false;    // detector state behind row state: g.H, g.wmax are the chain's, g.vh the majority filter's delay
    int crec = 0;             // ... doubles of a stream's criterion record: one energy, or the Burg cepstra of a frame
    PushGeom g{};             // (arena_samples, tile_cap: the set's plan fills them in)
    int n_streams = 0, D = 0;
    int cstride = 0;          // samples of a stream's carry
    int hw = 0, C = 0;        // floats of a history row (Dbase, or B with trap state), rows of a history
    int tstride = 0;          // doubles of a stream's tail of the overlap-add
    int64_t xstate_floats = 0;  // per stream, by the kernel that runs
    int n_heads = 0;          // entries of the chain-head list of a push
    int64_t longest = 0;      // the slot the set's plan is made of, n_streams times

    // element counts of the per-set buffers; tf: the plan's total_frames (0: the set has no such buffer)
    // (a push that brings a stream's frame wmax + 2 delivers up to wmax + 1 more rows and bytes than it completes frames)
    int64_t vsink_n(int64_t tf) const { return vad ? std::max<int64_t>(tf + (int64_t)n_streams * (vad_rows ? std::max(g.H + g.vh, g.wmax + 1) : g.H), 1) : 0; }
    int64_t vbase_n(int64_t tf) const { return vad && g.held && !vad_rows ? std::max<int64_t>(tf, 1) * D : 0; }
    int64_t crec_n() const { return vad_rows ? (int64_t)n_streams * crec : 0; }
    int64_t hist_n() const { return g.held ? std::max<int64_t>((int64_t)2 * n_streams * C * hw, 1) : 0; }
    int64_t means_n() const { return g.held ? (int64_t)n_streams * SHAPE_STREAM_MEANS : 0; }
    int64_t otail_n() const { return signal ? (int64_t)n_streams * tstride : 0; }
    int64_t cols_n(int64_t tf) const { return trap ? std::max<int64_t>(tf, g.H) : 0; }  // a column per row that goes out: the frames of a push, or the half a finish delivers
    // what a stream has delivered after `total` samples - rows, or samples with signal state - and what its finish still delivers
    int64_t delivered(int64_t total, int64_t *pending = nullptr) const {
        return signal ? stream_signal_step(g.window, g.wshift, total, pending) : stream_vad_rows_step(g.window, g.wshift, g.vh, g.H, g.wmax, total, pending);
    }
};

// `d`: after spread_small_fft, accepted by streams_unsupported_reason(d, flags)
inline StreamSetShape stream_set_shape(const ctu::Design &d, uint32_t flags, const StreamSetFacts &f, int n_streams, int64_t max_push) {
    StreamSetShape s;
    const bool do_vad = d.o.do_vad();
    // (per-wave chains are exten's with the noise state, or those of hwss / fwss / 2fwss with the subtraction state, on the 256- / 512-point front end)
    // (with speech output the subtraction state and the signal state meet in one set: CTU_STREAMS_SS_SIGNAL_STATE beside the two)
    constexpr uint32_t ss_signal_flags = CTU_STREAMS_SS_STATE | CTU_STREAMS_SIGNAL_STATE | CTU_STREAMS_SS_SIGNAL_STATE;
    // (on 2048- / 4096-point frames the subtraction state reaches the feature path with CTU_STREAMS_SS_LARGE_STATE beside it: bigss_kernel<NIT, true>)
    s.ss = f.ss && (flags & CTU_STREAMS_SS_STATE) && !f.ss_file &&
           (f.big ? !d.signal_out && (flags & CTU_STREAMS_SS_LARGE_STATE) : !d.signal_out || (flags & ss_signal_flags) == ss_signal_flags);
    if ((f.per_wave && !f.ss && !(flags & CTU_STREAMS_NR_STATE)) || (do_vad && !(flags & CTU_STREAMS_VAD_STATE)) || (f.ss && !s.ss) ||
        (f.per_wave && f.big && !f.ss && !(flags & CTU_STREAMS_LARGE_STATE)) || (do_vad && f.big)) {
        s.refusal = "internal: a streamed configuration with chains of whole utterances";
        return s;
    }
    const int tail = d.window - d.wshift;
    s.n_streams = n_streams;
    s.D = d.D;
    s.cstride = (d.window + 7) / 8 * 8;
    s.vad = (flags & CTU_STREAMS_VAD_STATE) && do_vad;
    s.trap = (flags & CTU_STREAMS_TRAP_STATE) && d.kind == ctu::FeaKind::TrapDct;
    s.signal = (flags & CTU_STREAMS_SIGNAL_STATE) && d.signal_out;
    PushGeom &g = s.g;
    g.window = d.window;
    g.wshift = d.wshift;
    g.max_wg = f.max_wg;
    stream_set_halo(d, flags, &g.H, &g.wmax, &g.vh);
    s.vad_rows = s.vad && stream_set_vad_rows(d, flags);
    g.H -= g.vh;  // (the chain's own: the push plan counts calls by H, wmax and rows h behind them)
    if (s.vad_rows) s.crec = d.o.vad_cri_mode == "energy" ? 1 : d.o.vad_lpc_coefs;
    g.vad = s.vad;
    g.signal = s.signal;
    // rows are held by a chain, a stacking or CMS (only with CTU_STREAMS_ROW_STATE: refused without), by the filter's delay, by half a
    // context; speech output writes no rows
    g.held = s.signal ? false : s.trap ? true : s.vad && !s.vad_rows ? g.H > 0 : d.post_order > 0 || d.cms;
    if (s.signal) {
        s.tstride = (std::max(tail, 1) + 1) / 2 * 2;
        s.ola_big = tail > SHAPE_OLA_TAIL_MAX;
        if (((s.ola_big || f.big) && !(flags & CTU_STREAMS_LARGE_STATE)) || tail > SHAPE_OLA_BIG_TAIL_MAX) {
            s.refusal = "internal: a signal set beyond the 512-point front end";
            return s;
        }
    }
    s.chained = g.chained = f.per_wave;  // (exten with CTU_STREAMS_NR_STATE, hwss / fwss / 2fwss with CTU_STREAMS_SS_STATE - a signal set as well where s.signal)
    g.max_chains = f.chain_slots;        // (max_wg * NWAVE wave chains, or n_cu * 8 workgroup chains of bigfft_kernel)
    s.hw = s.trap ? d.B : d.Dbase;
    // (detector state: a row is copied h frames late, nothing more; trap state: the last 2 half log-mel rows)
    // (detector state behind row state: the rows held back are rebuilt from base rows, h more of them than the row state keeps)
    s.C = s.vad && !s.vad_rows ? g.H : s.trap ? 2 * g.H : g.held ? std::max(2 * g.H, g.H + (d.cms == 2 ? d.o.length_b : 1) - 1) + g.vh : 0;
    if (s.chained) {
        // [2][64 NJ] of xstate_t (frontend_kernel.h), [2][64 * 9] floats (wave1k_kernel.h), [2][256 NB] floats (bigfft_kernel.h); with
        // subtraction state the slot of layout_constants.h - both noise estimates and the detector's record, on large transforms in doubles
        const int nj = f.mode == 1 ? 3 : 5;
        s.xstate_floats = s.ss ? (f.big ? xs_ss_big_floats(d.wfft / 256) : xs_ss_floats(nj)) : !f.big ? 2 * 64 * nj : f.wave1k ? 2 * 64 * 9 : 2 * 256 * (d.wfft / 256 / 2 + 1);
    }
    s.n_heads = chain_deal(n_streams, g.max_chains).heads();
    // the lead, a full carry, a full push (and no shorter than the shortest file a delta chain is defined on: the plan of a set whose
    // pushes are shorter than that is still a plan of files that could be)
    s.longest = std::max((int64_t)STREAM_LEAD + d.window - 1 + max_push, (int64_t)d.window + (int64_t)(g.wmax + 1) * d.wshift);
    return s;
}

}  // namespace
