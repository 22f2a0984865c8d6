// The plan of an offline run (plan.cc): host only, HIP-free.
// The boundary, as tables.h draws it for create: plan.cc decides and lays out - one plain value, HostPlan, from the engine's PlanGeom
// and the lengths of a batch - and engine.hip uploads that value's lists and allocates by its PlanScratch.  tests/host/plan_check.cc
// compiles the unit without the engine and pins every field to the commit it was moved out of engine.hip at.
//
//   PlanGeom          what a plan needs to know of an engine, and which lists and buffers the configuration's stages need: each
//                     predicate is stated once, here, and read by the planner, the parameter blocks of a run and the run itself
//   HostPlan          offsets, tiles and their chains, the lists the stages read, the element count of every scratch buffer
//   build_host_plan   the builder; the refusals of a batch are its return code and text
//   arena_layout, rows_arena_layout, vad_ring_step, vad_ring_rows   what the exported ctu_... functions of these names forward to
//   plan_ring_src, plan_part_first   the lists of ctu_plan_set_vad_ring and of the ranges of a host-buffer run
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "design.h"
#include "layout_constants.h"
#include "tables.h"

namespace ctu {

struct PlanGeom {
    // ---- the engine
    bool rows_in = false;     // -format_in htk: lengths are row counts, the arena holds the files' words, no front end
    int window = 0, wshift = 0, Dbase = 0, D = 0, K = 0, B = 0;
    int post_order = 0;       // stages of the delta chain / stacking, and
    int post_wmax = 0;        // the largest window among them: a file with frames has at least post_wmax + 2
    int trap_min = 0;         // trapdct: the fewest frames a file with frames may have, (traplen + 1) / 2 (0: no trapdct)
    bool per_wave = false;    // state along an utterance (exten, the *ss modes): chains of whole utterances, a wave - or, on the large-FFT
                              // workgroup kernels, a workgroup - per chain
    int max_wg = 0;           // front-end workgroups the chip holds at once: what the stateless chains, and a stream set's pushes, are built for
    int chain_slots = 0;      // per_wave: the most chains
    int rows_grid_cap = 0;    // rows_ingest_kernel: the most workgroups
    // ---- which lists and buffers the configuration's stages need (all off, but the first two, for an engine over rows)
    bool chunked = false;     // the passes that run a workgroup per 64-frame chunk (TRAP, delta / stacking, CMS, CMVN; an engine over rows in any case)
    bool staged = false;      // delta / stacking or CMS: the front end (the ingest) writes the plan's base rows, the passes behind write the caller's
    bool per_utt = false;     // the overlap-add and the -remove_dc1 recurrence go by utterance: utterance info, sample offsets on the device
    bool do_vad = false;      // the VAD module
    bool vad_energy = false, vad_burg = false, vad_fused = false;  // its criterion: frame energy; Burg-cepstral on exported spectra; the same fused into the front end
    int vad_ncoef = 0;        // coefficients per frame of the Burg-cepstral criterion
    bool ss = false;          // hwss / fwss / 2fwss: the utterance of every tile, seeds and decisions per utterance / frame
    bool ss_big = false;      // ... on 2048 / 4096-point frames (bigss_kernel.h), where an empty plan still has a row of every scratch
    bool ss_detector = false; // ... with the detector's cepstra of every frame (no -vad file=)
    int ss_ncep = 0;          // ... of which there are -fea_ncepcoefs
    bool row_off_dev = false; // the detectors' kernels walk an utterance's rows: row offsets on the device
    bool signal_out = false;  // speech output: samples written per utterance, the time-domain frames ahead of the overlap-add
    bool spectra = false;     // the spectra before and after NR leave the front end (xri, pnr [frames][K]): for the synthesis outside the
                              // front end, for the Burg-cepstral criterion outside it, for bigss_kernel
    bool pss = false;         // *ss with speech output on large frames: the synthesis reads the subtracted magnitudes (pss), pnr stays as exported
    bool dc1 = false;         // -remove_dc1: frame means and offsets
    bool logmel = false;      // band logarithms between the front end and TRAP / dct_wide_kernel
    bool lp_tail = false;     // the LP kinds' recursions run in lp_tail_kernel, on the lags the front end or wave1k_kernel left (bigfft_kernel and
                              // bigss_kernel finish the LP analysis themselves; nothing is projected with speech output)
    bool lags_double = false; // ... and its lags are double: LP analysis on uncompressed band energies, and wave1k_kernel's lags
    int lporder = 0;
};
// `d`: after spread_small_fft; `tab`: build_engine_tables(d), or the default value for an engine over rows (it has no tables)
PlanGeom plan_geom(const Design &d, const EngineTables &tab, const Spread &sp, int n_cu);

// (first row: low, high word; frames; 0) of an utterance: the int4 records the per-utterance and per-chunk kernels read
struct UttInfo {
    int row_lo, row_hi, frames, pad;
};

// Element counts of the device buffers a plan owns (ctu_plan's DevBufs of these names); 0: not allocated.
struct PlanScratch {
    int64_t base_rows = 0;                  // float [frames][Dbase]
    int64_t d_sample_off = 0, d_row_off = 0;  // the images of sample_off / row_off: n_utt + 1 entries
    int64_t ss_seed = 0, ss_last = 0;       // float [n_utt][K]
    int64_t ss_dirty = 0, ss_vbits = 0;     // bytes per utterance, per frame
    int64_t xri = 0, pnr = 0, pss = 0;      // float2 / float [frames][K]; pnr with the energy criterion: float [frames]
    int64_t vad_ci = 0;                     // double [frames][coefficients]
    int64_t vad_cf = 0;                     // float [frames][VFC_STRIDE]
    int64_t ybuf = 0;                       // float [frames][window]
    int64_t dc1m = 0, dc1 = 0;              // double, float [frames]
    int64_t logmel = 0;                     // float [frames][B]
    int64_t lp_r = 0;                       // double words holding [frames][lporder + 1] lags, float or double
};

struct HostPlan {
    int n_utt = 0;
    std::vector<int64_t> nsamples, frames;     // the lengths as given; frames of every utterance
    std::vector<int64_t> sample_off, row_off;  // n_utt + 1 entries: where every utterance starts in the arena and in the rows, the totals at the end
    int64_t total_samples = 0;                 // arena elements, padding included
    int64_t total_frames = 0;
    int max_frames = 0;                        // longest utterance
    std::vector<TileRec> tiles;                // with their `next` links
    std::vector<int> uts;                      // first tile of every utterance, the tile count at the end
    std::vector<int> heads;                    // first tile of every chain (-1: none); empty for a plan over rows
    int grid = 0;                              // workgroups of the front-end (ingest) launch the chains are built for
    std::vector<UttInfo> uinfo;                // (chunked or per_utt)
    std::vector<int> chunks, chunks128;        // (chunked) (utterance, first frame) of every 64-frame chunk and, over samples, of every other one
    int n_chunks = 0, n_chunks128 = 0;         //           (trapdct_split16_kernel); chunks128 is never empty there: one pair of zeros stands for none
    std::vector<int> tile_utt;                 // (ss) utterance of every tile
    std::vector<int> vf_order;                 // (vad_fused) utterances with at least one frame, longest first; never empty: a zero stands for none
    int n_live = 0;                            //             how many there are
    std::vector<int64_t> out_samples;          // (signal_out) samples written per utterance
    PlanScratch scratch;
};

// Frames of a file of n samples - or, over rows, of n rows; -1: shorter than one frame's worth (ctu_num_frames)
int64_t plan_num_frames(const PlanGeom &g, int64_t n);
// The plan of utterances of `lengths`: CTU_OK and the plan in `out`, or the refusal's code with its text in `err` and `out` untouched.
int build_host_plan(const PlanGeom &g, const int64_t *lengths, int32_t n_utt, HostPlan &out, std::string &err);

// ctu_arena_layout, ctu_rows_arena_layout, ctu_vad_ring_step, ctu_vad_ring_rows (include/ctu_engine.h)
int64_t arena_layout(const int64_t *utt_nsamples, int32_t n_utt, int64_t *sample_off);
int64_t rows_arena_layout(const int64_t *utt_rows, int32_t n_utt, int32_t width, int64_t *word_off);
void vad_ring_step(int32_t order, int64_t frames, int32_t *hidx, int32_t *hsize);
int64_t vad_ring_rows(int32_t order, int64_t frames, int32_t hidx0, int32_t *src);

// ctu_plan_set_vad_ring: which frame's vector every row of the plan carries when the majority filter of `order` starts utterance i at
// ring index hidx[i] (-1: an untouched ring slot = zeros; absolute row numbers; at least one entry).  Empty: every utterance is in
// phase, the rows are the frames' own.
std::vector<int> plan_ring_src(const HostPlan &p, int order, const int32_t *hidx);
// The first utterance of each of up to `nparts` consecutive ranges of about equal input, n_utt at the end (a long utterance spans
// several goals, so fewer ranges may come out)
std::vector<int> plan_part_first(const HostPlan &p, int nparts);

}  // namespace ctu
