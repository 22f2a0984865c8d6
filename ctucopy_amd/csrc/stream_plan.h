// Streaming input: what a push is, worked out on the host before anything reaches the device.  Plain C++ (no HIP call, no HIP type):
// engine.hip includes it through stream_kernels.h / stream_rows_kernels.h, tests/host/stream_plan_check.cc compiles it with g++ alone.
//
//   StreamPush, RowPush   the descriptors the stream kernels read, one per pushed stream
//   stream_frames, stream_halo, stream_rows_out   frames of a file after so many samples, rows that have gone out after so many frames
//   chain_deal            where chain c of C sits among the chain heads of a launch (plan.cc deals the utterances of an offline run by it, a push streams)
//   stream_plan_push      a whole push from the set's geometry and mirrors: slots, prefix sums, chains, row descriptors, the launch's
//                         sizes, the mirrors' next values.  It writes its output only; ctu_streams_push commits and launches from it
//   stream_plan_finish    the same for ctu_streams_finish: the rows held back, the refusal of a file too short for its chain
//   SignalPush            signal state (CTU_STREAMS_SIGNAL_STATE, stream_signal_kernels.h): where the samples of a pushed stream go and which
//                         time-domain frames of the push they are made of; PushGeom::signal turns a push's counts into samples
//   stream_vad_halo       detector state (CTU_STREAMS_VAD_STATE): the majority filter's delay h as the halo of the row arithmetic, so that
//                         a frame's row and its decision leave together; PushGeom::vad then adds the list of the streams that run the replay
//   stream_vad_rows_out, VadCalls   detector state behind row state (CTU_STREAMS_VAD_ROW_STATE): the detector is called when a chain row is
//                         complete, C(F) = stream_rows_out(H, wmax, F) calls after F frames, and a row leaves h calls behind its own:
//                         R(F) = max(C(F) - h, 0).  PushGeom::vh is h; VadCalls says which calls a pushed stream makes
//   stream_trap_halo, stream_trap_columns   trap state (CTU_STREAMS_TRAP_STATE): half a context as the halo of the row arithmetic, and
//                         the stream of every output row of a push, which stream_trap_kernel takes sixteen at a time
#pragma once

#include <algorithm>
#include <cstdint>

#include "layout_constants.h"

#ifdef __HIPCC__
#define CTU_HOST_DEVICE __host__ __device__
#else
#define CTU_HOST_DEVICE
#endif

namespace {

constexpr int STREAM_LEAD = 8;       // samples of a slot ahead of the next frame's first one (= PCM_ALIGN: the frame starts 16-byte aligned)
constexpr int STREAM_SLICE = 2048;   // slot samples per workgroup of stream_stitch_kernel: 256 lanes x one b128 store

// Frames a file of `total` samples has produced: floor((total - (window - wshift)) / wshift), none while it is shorter than the
// window - wshift samples rawIN::new_file loads first (src/io/in.cc:277,314).  A trailing partial window never makes a frame.
CTU_HOST_DEVICE inline long long stream_frames(long long total, int window, int wshift) {
    const long long pre = window - wshift;
    return total < pre ? 0 : (total - pre) / wshift;
}

// The halo H and the largest window of a delta chain (`order` stages of half-widths w[]) or of a stacking (0, 0 without either)
inline void stream_halo(int order, const int *w, bool stack, int *H, int *wmax) {
    *H = *wmax = 0;
    for (int j = 0; j < order; j++) {
        if (!stack || j == 0) *H += w[j];
        *wmax = std::max(*wmax, w[j]);
    }
}
// Rows of a file that have gone out after F frames: all without a chain, else F - H once frame wmax + 2 exists
inline int64_t stream_rows_out(int H, int wmax, int64_t F) { return H == 0 ? F : (F >= wmax + 2 ? std::max<int64_t>(F - H, 0) : 0); }

// The VAD's majority filter of order `order` releases a decision h = (order - 1) / 2 frames late, and the reference's writer releases the
// row with it: R(F) = F - h once F > h, none before (a file of no more than h frames writes nothing).  That is stream_rows_out with
// H = h and wmax = h - 1; with h = 0 nothing is held back.
inline void stream_vad_halo(int order, int *H, int *wmax) {
    *H = (order - 1) / 2;
    *wmax = *H > 0 ? *H - 1 : 0;
}

// Detector state behind row state: the rows (and decisions) that have gone out after F frames of a file whose chain has halo H and
// largest window wmax and whose majority filter delays by h calls.  h = 0 is stream_rows_out.
inline int64_t stream_vad_rows_out(int H, int wmax, int h, int64_t F) { return std::max<int64_t>(stream_rows_out(H, wmax, F) - h, 0); }

// One stream of a push (host-built: the prefix sums over the push are the host's, which mirrors the counts)
struct StreamPush {
    long long src;    // where its new samples start in the caller's buffer: an element of it - a sample, or with a wire layout whatever
                      // the layout's format counts in; sample k is element src + k * stride of the layout (1 without)
    long long slot;   // where its slot starts in the push arena (samples, a multiple of PCM_ALIGN)
    long long row0;   // first row of the push it writes
    int id, n;        // stream, new samples
    int tile0, pad;   // first tile record it fills; pad: with noise state, the tile that follows its last one on its chain (-1: none)
};

// One stream of a push, or the stream that finishes (host-built from the mirrored counts)
struct RowPush {
    long long F0;    // frames of the file ahead of this push
    long long r0;    // rows of the file that have gone out ahead of it
    long long out0;  // first row of the caller's buffer it writes
    long long row0;  // first of its new base rows among the push's
    int id, Tn;      // stream; frames this push completes
    int nr;          // rows that go out now
    int hsel;        // which of the stream's two histories holds frames F0 - C .. F0 - 1
};

// One stream of a push on a set with detector state behind row state: the detector's calls c0 .. c0 + nc - 1 of the file, made now
// (call j reads the criterion of frame j + H, which is a frame of this push or - one push of a file at most - the one before it)
struct VadCalls {
    long long c0;  // calls of the file made ahead of this push: C(F0)
    int nc, pad;   // calls this push makes: C(F0 + Tn) - C(F0)
};

// One stream of a push on a set with signal state, or the stream that finishes (host-built): the overlap-add of stream_ola_kernel.
// The stream goes from F0 to F0 + T frames and delivers T * wshift samples, file samples F0 * wshift on; the sums its later frames
// still add to - window - wshift of them - stay in the stream's tail.  Samples of a push lie stream after stream, as rows do.
struct SignalPush {
    long long out0;  // first sample of the caller's buffer it writes
    long long row0;  // first of its time-domain frames among the push's
    long long F0;    // frames of the file ahead of this push
    int id, T;       // stream; frames this push completes
};

// Chains per wave: `live` files dealt onto C chains, at most `slots` of them, in G workgroups of NWAVE waves.  Chain c lives in wave
// c / G of workgroup c % G, so the chains of one workgroup are spread over the ranks of whatever order the files are dealt in.
struct ChainDeal {
    int C, G;
    int heads() const { return G * NWAVE; }  // entries of the chain-head list the launch reads (-1: a wave without a chain)
    int slot(int c) const { return (c % G) * NWAVE + c / G; }
};
inline ChainDeal chain_deal(int live, int slots) {
    const int C = std::max(1, std::min(live, slots));
    return {C, (C + NWAVE - 1) / NWAVE};
}

// What a stream set is, as far as the layout of a push goes
struct PushGeom {
    int window, wshift;
    int H, wmax;             // halo and largest window of the set's delta chain or stacking (0, 0: a frame's row goes out with it)
    bool held;               // row state: RowPush descriptors, the history flip
    int vh = 0;              // detector state behind row state: the majority filter's delay h, behind the chain's H (0: no such set)
    bool vad = false;        // detector state: RowPush descriptors (whether rows are held or not), the list of the streams that run the replay
    bool chained;            // noise state: chains of whole streams, a wave each
    bool signal = false;     // signal state: SignalPush descriptors; a push's counts, prefix sums and capacity are samples, wshift per frame
    int max_chains, max_wg;  // the most chains, and without chains the most workgroups, the front end is launched with
    int64_t arena_samples;   // the push arena, PCM_TAIL included
    int64_t tile_cap;        // tile records the set has room for
};

// A planned push.  The arrays are the caller's (a stream set keeps them from create on, so a push allocates nothing): n entries each,
// `heads` and `tail` chain_deal(n_streams, max_chains).heads() entries.  Entries past those a plan fills are left alone and never read.
struct PushLayout {
    StreamPush *push = nullptr;
    RowPush *rows = nullptr;         // (held or vad only)
    int *replay = nullptr;           // (vad only) positions in the push of the streams that complete a frame, in push order: the detector's
                                     // replay runs over these alone (16 to a wave); a stream that completes none is not touched
    int n_replay = 0;                // entries of `replay`
    VadCalls *calls = nullptr;       // (vh > 0 or a chain behind the detector: PushGeom::vad with H of a chain) the calls of every pushed stream;
                                     // null on every other set
    SignalPush *sig = nullptr;       // (signal only)
    int64_t capacity = -1;           // (signal only) what the caller's buffer holds; -1: not checked
    bool over_capacity = false;      // (signal only) the push delivers more than that: the plan fails and nothing of L may be used
    int *heads = nullptr;            // (chained only) first tile of every chain, by ChainDeal::slot
    int *tail = nullptr;             // (chained only) scratch: the stream at the end of every chain so far
    int64_t *row_counts = nullptr;   // rows every pushed stream delivers now
    int64_t *consumed = nullptr;     // the mirrors' next values, by position in the push
    uint8_t *hsel = nullptr;
    int n_heads = 0;                 // entries of `heads` the launch reads (0 without chains: the plan's own heads serve)
    int tiles = 0, slices = 1, grid = 1;
    int64_t base_rows = 0, rows_out = 0, most = 0;  // frames of the push, rows that go out (the same without row state), the most of one stream
};

// Plans the push of n_samples[i] new samples to stream ids[i], i < n (ids in range and distinct, counts >= 0: the caller has checked).
// false, with nothing the caller may use in L, when the push does not fit the arena or the tile list - or, on a set with signal state,
// delivers more samples than L.capacity (L.over_capacity says which).  src_base: the element of the caller's layout that the buffer the
// kernels read starts at - the first of the covering range a host wire form has uploaded, 0 everywhere else.
inline bool stream_plan_push(const PushGeom &g, const int64_t *consumed, const uint8_t *hsel, int n, const int32_t *ids, const int64_t *n_samples,
                             const int64_t *sample_off, PushLayout &L, const int64_t src_base = 0) {
    int live = 0;
    if (g.chained)  // the streams that complete a frame, dealt in turn onto at most max_chains chains
        for (int i = 0; i < n; i++) {
            const int64_t c = consumed[ids[i]];
            live += stream_frames(c + n_samples[i], g.window, g.wshift) > stream_frames(c, g.window, g.wshift);
        }
    const ChainDeal deal = chain_deal(live, g.max_chains);
    L.n_heads = g.chained ? deal.heads() : 0;
    if (g.chained) {
        std::fill(L.heads, L.heads + L.n_heads, -1);
        std::fill(L.tail, L.tail + deal.C, -1);
    }
    int64_t so = PCM_HEAD, ro = 0, oo = 0, most = 0;
    int tiles = 0, slices = 1, n_replay = 0;
    live = 0;
    for (int i = 0; i < n; i++) {
        const int64_t c = consumed[ids[i]];
        const int64_t F = stream_frames(c, g.window, g.wshift), T = stream_frames(c + n_samples[i], g.window, g.wshift) - F;
        const int64_t len = STREAM_LEAD + (c - F * g.wshift) + n_samples[i];  // the stitched utterance: an utterance of the arena (pcm_slot)
        StreamPush &p = L.push[i];
        p.src = n_samples[i] ? sample_off[i] - src_base : 0;
        p.slot = so;
        p.row0 = ro;
        p.id = ids[i];
        p.n = (int)n_samples[i];
        p.tile0 = tiles;
        p.pad = -1;
        if (g.chained && T > 0) {
            const int ch = live++ % deal.C;
            int &tail = L.tail[ch];
            if (tail < 0) L.heads[deal.slot(ch)] = tiles;
            else L.push[tail].pad = tiles;
            tail = i;
        }
        so += pcm_slot(len);
        ro += T;
        tiles += (int)((T + TILE - 1) / TILE);
        slices = std::max(slices, (int)((len + STREAM_SLICE - 1) / STREAM_SLICE));
        // what goes out now: rows - or, with signal state, the samples no later frame adds to: wshift for every frame
        const int64_t r0 = stream_vad_rows_out(g.H, g.wmax, g.vh, F), nr = g.signal ? T * g.wshift : stream_vad_rows_out(g.H, g.wmax, g.vh, F + T) - r0;
        if (L.calls) {
            const int64_t c0 = stream_rows_out(g.H, g.wmax, F);
            L.calls[i].c0 = c0; L.calls[i].nc = (int)(stream_rows_out(g.H, g.wmax, F + T) - c0); L.calls[i].pad = 0;
        }
        if (g.vad && T > 0) L.replay[n_replay++] = i;
        if (g.held || g.vad) {  // (vad: decision byte k of the push belongs to row k, so out0 serves both; F0 is the replay's absolute frame index)
            RowPush &r = L.rows[i];
            r.F0 = F; r.r0 = r0; r.out0 = oo; r.row0 = p.row0;
            r.id = ids[i]; r.Tn = (int)T; r.nr = (int)nr;
            r.hsel = hsel[ids[i]];
        }
        if (g.signal) {
            SignalPush &q = L.sig[i];
            q.out0 = oo; q.row0 = p.row0; q.F0 = F;
            q.id = ids[i]; q.T = (int)T;
        }
        oo += nr;
        most = std::max(most, nr);
        L.row_counts[i] = nr;
        L.consumed[i] = c + n_samples[i];
        L.hsel[i] = (uint8_t)(hsel[ids[i]] ^ (g.held && T > 0 ? 1 : 0));  // stream_rows_carry_kernel writes the other history
    }
    L.over_capacity = g.signal && L.capacity >= 0 && oo > L.capacity;
    if (so + PCM_TAIL > g.arena_samples || tiles > g.tile_cap || L.over_capacity) return false;
    L.tiles = tiles;
    L.slices = slices;
    L.grid = g.chained ? deal.G : std::max(1, std::min(tiles, g.max_wg));
    L.n_replay = n_replay;
    L.base_rows = ro;
    L.rows_out = oo;
    L.most = most;
    return true;
}

// Trap state (CTU_STREAMS_TRAP_STATE, stream_trap_kernels.h): the halo of trapdct's context.  Row t reads log-mel frames t - half ..
// t + half, half = (traplen - 1) / 2 (traplen is odd, at least 3), so R(F) = F - half once F >= half + 1 and none before - a file of
// 1 .. half frames is the offline plan's refusal (plan.cc: trap_min = (traplen + 1) / 2).  That is stream_rows_out with H = half and
// wmax = half - 1.
inline void stream_trap_halo(int traplen, int *H, int *wmax) {
    *H = (traplen - 1) / 2;
    *wmax = *H - 1;
}
// The columns of stream_trap_kernel: the rows that go out with a push are its columns, in the order of the caller's buffer (RowPush::out0
// is the prefix sum of nr over the push), sixteen to a wave whatever streams they belong to.  col[c] = the position in the push of the
// stream column c belongs to, c < sum of nr; `col` has room for that many.  Returns the sum.
inline int64_t stream_trap_columns(const RowPush *rows, int n, int *col) {
    int64_t c = 0;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < rows[i].nr; k++) col[c++] = i;
    return c;
}

// A stream that finishes after `consumed` samples: the rows held back for it, which go out now (RowPush `row`, meaningful while
// pending > 0), or none from a file too short for its chain (the plan's refusal: such a file has no defined rows).
// vad: H, wmax are stream_vad_halo's; a file of 1 .. h frames is no refusal there - the reference writes nothing for it - and the
// pending min(F, h) rows come with as many decisions, which the majority filter's flush makes (row.F0 = the file's frames).
// signal: H = wmax = 0; pending counts samples - the window - wshift sums of the stream's tail, which the reference's close() writes,
// once the file has a frame - and `sig` says whose tail (T = 0: no frame is added).
// vh (detector state behind row state; vad is false there and H, wmax are the chain's): the rows leave h calls behind theirs, so
// pending = F - max(C(F) - h, 0) - none from a file of no more than h frames, which writes nothing - and `calls` are those the finish
// still makes, C(F) .. F - 1, each on the criterion of the file's last frame; a file too short for its chain is refused as ever.
struct FinishLayout {
    int64_t frames, pending;
    bool too_short;
    VadCalls calls;
    RowPush row;
    SignalPush sig;
};
inline FinishLayout stream_plan_finish(int window, int wshift, int H, int wmax, int64_t consumed, int id, int hsel, bool vad = false, bool signal = false,
                                       int vh = 0) {
    FinishLayout f;
    f.sig.out0 = 0; f.sig.row0 = 0; f.sig.F0 = 0; f.sig.id = id; f.sig.T = 0;
    f.frames = stream_frames(consumed, window, wshift);
    const int64_t r0 = stream_vad_rows_out(H, wmax, vh, f.frames);
    f.too_short = H > 0 && f.frames > 0 && f.frames < wmax + 2;
    f.pending = f.too_short || f.frames <= vh ? 0 : f.frames - r0;
    f.calls.c0 = stream_rows_out(H, wmax, f.frames); f.calls.nc = f.pending ? (int)(f.frames - f.calls.c0) : 0; f.calls.pad = 0;
    if (vad) f.too_short = false;  // (pending stays 0: neither rows nor decisions)
    f.row.F0 = f.frames; f.row.r0 = r0; f.row.out0 = 0; f.row.row0 = 0;  // rows r0 .. F - 1 with the file's length known
    f.row.id = id; f.row.Tn = 0; f.row.nr = (int)f.pending;
    f.row.hsel = hsel;
    if (signal) {
        f.too_short = false;
        f.pending = f.frames > 0 ? window - wshift : 0;
        f.sig.F0 = f.frames;
    }
    return f;
}

}  // namespace
