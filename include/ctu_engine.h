/*
 * ctu_engine.h -- C ABI of the MI355X (gfx950) framewise feature engine.
 *
 * This is the drop-in boundary for CtuCopy's per-frame hot path.  The reference has no FFI; its
 * "operator API" is the set of per-stage objects BATCH wires together by pointer and drives once per
 * frame (src/io/batch.cc:24-69 wiring, :205-228 per-frame dispatch, :326-421 list loop).  The calls
 * below replace, for a whole list of files at once:
 *
 *   new opts(argc,argv) + new BATCH(o)        -> ctu_engine_create        (src/io/opts.cc:27-194, src/io/batch.cc:24-69)
 *   scanning the -S list / IN::new_file       -> ctu_plan_create          (src/io/batch.cc:349-371, src/io/in.cc:264-279)
 *   while(in->get_frame()) process_frame();   -> ctu_engine_run[_host]    (src/io/batch.cc:402-407 incl. flush_fea)
 *     rawIN::get_frame after loadframe           (src/io/in.cc:343-417)
 *     NR::process_frame                          (src/nr/nr.cc:95-140)
 *     FB::project_frame                          (src/fea/fb.cc:72-86)
 *     FEA::process_frame / flush_frame           (src/fea/fea_impl.cc:104-131,163-284, src/fea/fea_trap.cc:53-127)
 *     VAD::process_frame .. flush                (src/vad/vad.cc:692-745, src/io/batch.cc:230-249)
 *     htkOUT::save_frame reorder + (float)       (src/io/out.cc:174-203; the fwrite stays with the caller)
 *   throw "literal" caught in main()          -> negative return + ctu_last_error (src/main.cpp:54-60)
 *
 * File decoding (rawIN::loadframe, a-law/mu-law, WAVE headers) and the HTK/pfile/ark writers stay on
 * the caller's side of this ABI ("src/io left as-is"); the bundled `ctucopy` executable provides them.
 *
 * Plain pointers and sizes only.  Device pointers are HIP device addresses on the engine's device.
 * There is no CPU fallback: every entry point that computes fails with CTU_ERR_DEVICE when no gfx950
 * device is usable.
 */
#ifndef CTU_ENGINE_H
#define CTU_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctu_engine ctu_engine;
typedef struct ctu_plan ctu_plan;
typedef struct ctu_streams ctu_streams;

enum {
    CTU_OK = 0,
    CTU_ERR_OPTS = -1,        /* command line rejected (message = the reference's text) */
    CTU_ERR_UNSUPPORTED = -2, /* valid ctucopy configuration outside the accelerated path */
    CTU_ERR_DEVICE = -3,      /* no usable HIP device / HIP runtime error */
    CTU_ERR_INPUT = -4,       /* bad argument, or "IO: Signal shorter than one frame!" */
};

/* Geometry of a configured chain (all derived as in the reference, see each field). */
typedef struct {
    int32_t fs;
    int32_t window;     /* src/io/opts.cc:259 */
    int32_t wshift;     /* src/io/opts.cc:260 */
    int32_t wfft;       /* src/io/opts.cc:277-280 */
    int32_t nbins;      /* wfft/2+1, src/io/opts.cc:283 */
    int32_t nbands;     /* src/fea/fb.cc:183,289-302 */
    int32_t row_floats; /* floats per output row incl. c0/E, src/io/out.cc:95-113 */
    int32_t htk_kind;   /* src/io/out.cc:147-159 */
    uint32_t htk_period;/* src/io/out.cc:146 */
    int32_t has_vad;    /* a VAD byte per frame is produced, src/io/batch.cc:34-38 */
    int32_t swap_out;   /* caller must byte-swap on write (-endian_out big), src/io/opts.cc:287 */
    int32_t pcm_align;  /* utterance starts inside the packed PCM arena are multiples of this many samples */
    int32_t signal_out; /* -format_out raw|wave: the engine writes enhanced speech (ctu_engine_run_signal), no rows */
    int32_t rows_in;    /* -format_in htk: runs start from rows of row_floats_in floats (ctu_engine_run_rows), src/io/batch.cc:57-60 */
    int32_t row_floats_in; /* -nfeacoefs, src/io/in.cc:623-627 (0 unless rows_in) */
    int32_t swap_in;    /* the input's byte order is not the host's (-endian_in big), src/io/opts.cc:286 */
} ctu_dims;

/* argv = the ctucopy command line without argv[0] (flags of src/io/opts.cc:644-846, incl. -C <file>).
 * device = HIP ordinal.  On failure *out is NULL and ctu_create_error() holds the message. */
int ctu_engine_create(int argc, const char *const *argv, int device, ctu_engine **out);
void ctu_engine_destroy(ctu_engine *);
const char *ctu_create_error(void);
const char *ctu_last_error(const ctu_engine *);
int ctu_engine_dims(const ctu_engine *, ctu_dims *out);

/* Parse + design only (no device needed): used by host-side tools and CPU tests. */
int ctu_config_dims(int argc, const char *const *argv, ctu_dims *out);

/* Host-designed tables in double precision (no device needed), for inspection and tests:
 * name = "hamming" [window] | "fbank" [nbands*nbins] | "fb_first" | "fb_last" [nbands] |
 *        "dct" [(ncep+1)*nbands] | "idft" [(p+1)*nbands] | "trap" [ndct*traplen] | "lifter" [ncep] |
 *        "phase2_check" [3: table error, chunks, slots] | "phase2_walk" [slots + 1: the filter-bank walk's chunks per slot, then the
 *        index of the compiled walk signature that this configuration's bank and frame shape match, or -1; whether a run uses it
 *        depends on the instantiation too: ctu_engine_phase2_walk] |
 *        "frontend" [12: the frontend_kernel instantiation ctu_engine_create selects for the configuration, as its template arguments
 *        NZ, FEAT, MODE, VX, NC, GEN, LPO, MD, VF, SS, SY and last the index of its straight-line walk or -1 (CTU_PHASE2_GENERIC is
 *        honoured); eleven zeros and -1 for the large-FFT kernels (1024 points and above), which the FFT size alone selects] |
 *        "host_tables" [everything ctu_engine_create decides and lays out for the kernels before it touches the device, in this order:
 *          36 scalars: the twelve values of "frontend"; feat, big, path, ss, ss_file, dctw, trap_bf16, lds_bytes, dctw_nout,
 *            dctw_chunks, big_fb_total; lift_off, tab_floats, ck_off, cf_off, cfd_off, am_off, han_off, NS, CW, ncoef_out; kstride
 *            and the configuration's own FFT size and bin count;
 *          16 table images, each as its length in 32-bit words followed by the words' unsigned values (never as floats: the tables
 *            carry ints whose bit patterns are NaNs; a double is two words, low then high): lanec, ftab, itab, trapG, trapG16,
 *            dctw_tab, big_win, big_tw, big_fbw, big_range, big_seg, big_coef, big_coef_d, big_slot, big_lifter, big_han;
 *          the 32 fields of the kernels' VAD parameter block (VadParams, layout_constants.h) in declaration order, as values.
 *        Not for HTK feature input, which has no tables.  tests/golden/host_tables.json pins it] |
 *        "tile_frames" [1: frames per tile record of a plan - an offline run's and a stream set's alike: a push that completes more
 *        frames of a stream than this spans two tiles] |
 *        "trap_path" [6: the launch of offline TRAP-DCT for a -fea_kind trapdct configuration: 1 for the fp16-split kernel
 *        (trapdct_split16_kernel) or 0 for the fp32 one (trapdct_mfma_kernel<NRB, NSM>), NRB, NSM (zeros for the split kernel), the
 *        dynamic LDS bytes of the launch, whether the launch raises the kernel's LDS limit first (more than 64 KiB), and whether
 *        ctu_engine_create takes the configuration; CTU_ERR_INPUT for another feature kind].
 * Returns the number of values (written up to cap), or a negative error code. */
int64_t ctu_config_table(int argc, const char *const *argv, const char *name, double *out, int64_t cap);

/* floor((n - (window-wshift)) / wshift); -1 when n < window-wshift (src/io/in.cc:277,314). */
int64_t ctu_num_frames(const ctu_engine *, int64_t nsamples);

/* A plan fixes the batch layout: utterance i has utt_nsamples[i] samples and lives in the packed
 * int16 arena at sample offset ctu_plan_sample_offsets()[i] (offsets are multiples of pcm_align; the
 * arena has 8 samples of padding ahead of the first utterance and 512 behind the last one, and frames DO read past the
 * end of their window - into the gap, the next utterance or that padding - under zero weights: every byte of
 * ctu_plan_total_samples() must be readable, its contents between utterances do not matter).  Its output rows start at row ctu_plan_row_offsets()[i].  Both offset arrays
 * have n_utt+1 entries and stay valid until ctu_plan_destroy. */
int ctu_plan_create(ctu_engine *, const int64_t *utt_nsamples, int32_t n_utt, ctu_plan **out);
/* The arena layout rule of ctu_plan_create on its own (no engine, no device): writes the n_utt+1 sample offsets a plan over
 * these lengths will report (sample_off may be NULL) and returns its ctu_plan_total_samples(), or a negative error code.  A host
 * loop that reads files straight into a page-locked arena (the counterpart of rawIN::loadframe, src/io/in.cc:434-460) lays the
 * next batch out with it while the engine is busy with the current one. */
int64_t ctu_arena_layout(const int64_t *utt_nsamples, int32_t n_utt, int64_t *sample_off);
void ctu_plan_destroy(ctu_plan *);
const int64_t *ctu_plan_sample_offsets(const ctu_plan *);
const int64_t *ctu_plan_row_offsets(const ctu_plan *);
int64_t ctu_plan_total_samples(const ctu_plan *);
int64_t ctu_plan_total_frames(const ctu_plan *);

/* Device-resident run: d_pcm = packed arena (int16, total_samples), d_rows = total_frames*row_floats
 * floats in writer order (c1..cN,c0[,E]), d_vad = total_frames bytes '0'/'1' or NULL.
 * stream = hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing. */
int ctu_engine_run(ctu_engine *, const ctu_plan *, const int16_t *d_pcm, float *d_rows, uint8_t *d_vad, void *stream);

/* Page-locked host memory for the host-buffer calls below: buffers from ctu_host_alloc are DMA-ed asynchronously at the
 * link rate; any other (pageable) pointer is accepted too and goes through the runtime's staging. */
void *ctu_host_alloc(size_t bytes);
void ctu_host_free(void *);

/* Host-buffer convenience: H2D, run, D2H, synchronised on return.  The device copies are kept in the plan.  The 32 MiB rule:
 * a batch of at least 16 utterances and 32 MiB of input (the arena's bytes), with input and output in page-locked buffers,
 * goes in eight utterance ranges on two streams, so the upload of a range overlaps the kernels and the download of the
 * previous one (environment CTU_HOST_CHUNKS=<n> overrides, 1 = one range; the hwss / fwss / 2fwss chain always runs in one).
 * A null h_pcm or h_rows on a plan that has frames is CTU_ERR_INPUT.  rows_per_utt (optional, n_utt entries) receives the number
 * of rows actually produced per utterance: < frames with -vad_apply_mode drop, and 0 for an utterance with no more frames than the VAD's
 * majority filter delays ((vad_filter_order-1)/2: the filter never gets ready, src/vad/vad.h:126-136, and the reference writes neither a
 * row nor a decision; the utterance's bytes in h_vad / d_vad are NUL then, '0' / '1' otherwise). */
int ctu_engine_run_host(ctu_engine *, const ctu_plan *, const int16_t *h_pcm, float *h_rows, uint8_t *h_vad,
                        int64_t *rows_per_utt);

/* ---- feature files in (-format_in htk): delta / stacking, CMS and CMVN on rows that already exist ---------------
 * Replaces htkIN::get_frame (src/io/in.cc:691-709) and, behind it, what BATCH wires to in->_fvec (src/io/batch.cc:57-60,
 * 217-220): the delta chain, cms_POST and the writers' copy (src/io/out.cc:177-179).  An engine created with -format_in htk
 * starts its runs from rows: ctu_engine_run[_host] refuse it, and ctu_engine_run_rows[_host] refuse every other engine.
 * -nfeacoefs is the width of the files' rows (htkIN's vector, in.cc:623-627); reading the 12-byte headers, checking
 * sampSize / 4 against it and counting the whole rows a file really holds stay with the caller (bin/ctucopy does).
 *
 * Such an engine's plan takes ROW counts where ctu_plan_create says samples (ctu_num_frames is the identity) and its
 * ctu_plan_sample_offsets() / ctu_plan_total_samples() are in 32-bit words of the input arena.  The arena holds every file's
 * payload as it stands in the file - rows of `width` words in the file's byte order, -endian_in tells the engine which -
 * at the offsets this pure function computes (no engine, no device; word_off may be NULL): multiples of four words
 * (16 bytes), no padding around the arena.  Returns the arena's size in words, or a negative error code. */
int64_t ctu_rows_arena_layout(const int64_t *utt_rows, int32_t n_utt, int32_t width, int64_t *word_off);
/* Device-resident run: d_rows_in = the arena, d_rows = total_frames*row_floats floats.  Asynchronous on `stream`.  The rows
 * come out in file order - the reference's writers do not rotate c0 in this mode - and ctu_cmvn_* work on them as ever,
 * with statistic slot k = column k (src/fea/post_impl.cc:55-57). */
int ctu_engine_run_rows(ctu_engine *, const ctu_plan *, const void *d_rows_in, float *d_rows, void *stream);
/* Host-buffer convenience, the same pipeline as ctu_engine_run_host: its 32 MiB rule decides on the ranges (the arena's bytes:
 * four per word; CTU_HOST_CHUNKS overrides), pageable buffers go through the runtime's staging.  Synchronised on return. */
int ctu_engine_run_rows_host(ctu_engine *, const ctu_plan *, const void *h_rows_in, float *h_rows);

/* ---- streaming input: PCM pushed in chunks per stream, the rows of the offline run ---------------------------------
 * Replaces the reference's online mode (-online_in: rawIN::new_file on stdin, src/io/in.cc:268, and the same get_frame loop) for
 * many live channels at once: a stream is a file whose samples arrive in pushes, and a push computes every frame that its
 * samples complete - frame t of a stream comes out with the push that brings sample t * wshift + window - 1.  The rows are those
 * ctu_engine_run_host writes for the whole file: bit for bit when every push ends a multiple of eight frames into the file (the
 * front ends step through a tile in groups of eight frames), else to rounding.  They do not depend on
 * what else is in the push.
 *
 * Per stream the device keeps the samples the next frame still reads - the last window - wshift .. window - 1 samples and the
 * one ahead of them that pre-emphasis reaches back to (src/io/in.cc:365,384) - and the count of samples taken; nothing but the
 * row counts, which the host derives from the lengths, comes back between pushes.
 *
 * Streamed are the chains whose frames share nothing but samples: every feature kind, filter bank, FFT size and energy
 * column ctu_engine_create accepts, without -nr_mode, -remove_dc1, the VAD module, -fea_delta / -fea_trap / trapdct, CMS,
 * CMVN, speech output or HTK feature input (the flags of ctu_streams_create_ex below add the delta chains, stacking, CMS,
 * -nr_mode exten, the VAD module, speech output and trapdct).  ctu_streams_create refuses those with CTU_ERR_UNSUPPORTED and the option's name in
 * ctu_last_error; ctu_streams_config_check says the same from the command line alone (no device; `reason` receives the text).
 *
 * A push names n different streams (a repeat, an id outside the set, more than max_push_samples for one stream or more rows
 * than rows_capacity: CTU_ERR_INPUT before anything is launched or changed; the set stays usable).  Stream stream_ids[i] takes
 * n_samples[i] >= 0 samples from d_pcm + sample_off[i] (2-byte aligned is enough).  The rows of the push are written to d_rows one
 * stream after the other in the order of stream_ids, row_counts[i] of them for stream i (row_counts is host memory and is
 * filled on return; it may be NULL).  Asynchronous on `stream`; d_pcm may be reused once the work enqueued has run.  The calls on
 * one set must be ordered: one hipStream_t, or the caller's own synchronisation.  One set per engine runs at a time.
 * A push that returns CTU_ERR_DEVICE may have failed after the set had taken the push's sample counts for its own, so what the host
 * and the device hold for the set may differ, and nothing is rolled back.  Discard the rows of that push and call ctu_streams_finish
 * for every stream of the set (discarding those rows too) before pushing again: finish resets host and device state of a stream alike.
 *
 * Row state (ctu_streams_create_ex with CTU_STREAMS_ROW_STATE): the set also keeps, per stream, the last base rows of the file and
 * the running cepstral means, and so takes -fea_delta, -fea_trap, -fea_Z_exp and -fea_Z_block as well (the other refusals stand, and
 * so does every size limit ctu_engine_create puts on those chains).  Row t of a file is what the offline run writes for any file of
 * more than t + H frames (H, the halo: the sum of the chain's delta windows, or the stacking window; 0 with CMS alone), so after F
 * frames a stream has delivered R(F) = F - H rows - none while F < wmax + 2 (wmax: the largest window), since no row may go out of a
 * file that could still end where the offline plan refuses it - and holds F - R(F) back.  A push delivers the rows R(F) of its
 * streams advance by (row_counts, and the capacity check, count those; up to wmax + 1 more than the frames it completes), and
 * ctu_streams_finish delivers the rest with the file's end known.  On a chain without such state the flag changes nothing.
 *
 * Noise state (CTU_STREAMS_NR_STATE; the two flags combine): the set also keeps, per stream, the noise estimate of extended spectral
 * subtraction - Navg and Yavg of every bin (src/nr/nr.cc:86-140) - and so takes -nr_mode exten on the spectrum (-nr_when beforeFB) of the
 * 256- and 512-point front end, FFT sizes below 256 included: the plain cepstral chain, band outputs, -fea_E, -fb_inld / PLP and the LP
 * kinds, and with row state the delta chains, stacking and CMS behind them.  Exten is causal - frame t reads frames 0 .. t - so a row
 * still goes out with the push that completes its frame, R(F) is unchanged and ctu_streams_finish has nothing to add; a stream's next
 * file starts from the reference's initial estimate.  Still refused, by name, whatever the flags: -nr_when afterFB, exten on 1024 ..
 * 4096 points (without CTU_STREAMS_LARGE_STATE, below), hwss / fwss / 2fwss (without CTU_STREAMS_SS_STATE, below), the VAD module (without the flag below), -remove_dc1, trapdct (without CTU_STREAMS_TRAP_STATE, below), CMVN, speech output (without its
 * flag, below), HTK feature input.  On a chain without -nr_mode exten the flag changes nothing.
 *
 * Detector state (CTU_STREAMS_VAD_STATE; combines with the other two): the set also keeps, per stream, the state of the VAD module's
 * sequential part - the threshold recurrences, the background cepstrum, the majority filter's ring (src/vad/vad.cc:220-625,
 * src/vad/vad.h:126-175) - and so takes the VAD module on the 256- and 512-point front end, FFT sizes below 256 included: the energy
 * criterion and the Burg-cepstral one (-vad_cepdist_mode lpc), all four threshold modes, filter orders 1 .. 31, -vad_apply_mode none
 * (or silence, which is none on the feature path); with CTU_STREAMS_NR_STATE as well, -nr_mode exten ahead of the fused detector (25 ms
 * frames at 8 or 16 kHz, 14 coefficients: C4).  A frame's row and its decision leave together, as the reference's writer releases a
 * row when the majority filter releases its decision: with h = (vad_filter_order - 1) / 2, after F frames a stream has delivered
 * R(F) = F - h rows and decisions if F > h, else none (a file of no more than h frames writes nothing in the reference), and holds
 * F - R(F) back; ctu_streams_finish pushes h zeros through the filter and delivers the last min(F, h) of both - nothing, with CTU_OK,
 * for a file of 1 .. h frames.  The decisions are those of ctu_engine_run on the whole file, byte for byte, however it is cut into
 * pushes; every file of a stream is treated as the first file of a process (the rule above for the majority filter's ring: in phase).
 * The calls that deliver decisions are the *_vad forms below: d_vad / h_vad holds rows_capacity bytes, byte i is the decision of row
 * i of the same call ('0' / '1', as ctu_engine_run writes them); ctu_streams_push and ctu_streams_finish work on such a set and
 * deliver the rows only.  On a set without detector state a non-NULL vad buffer is CTU_ERR_INPUT before anything changes.  Refused by
 * name whatever the flags: -vad_apply_mode drop, -vad_cepdist_mode fea, the VAD module with -fea_delta / -fea_trap / -fea_Z_exp /
 * -fea_Z_block, -fea_E where the offline run shifts the energy column (filter orders above 2), the VAD on 1024-point and larger
 * frames, -nr_mode exten with a criterion outside the fused shapes.  On a configuration without the VAD module the flag changes nothing.
 *
 * Signal state (CTU_STREAMS_SIGNAL_STATE): the set streams the speech-enhancement output (-format_out raw | wave, row N3; what the
 * reference's -online_in / -online_out pair is for).  It also keeps, per stream, the tail of the overlap-add: the window - wshift
 * partial sums of the samples that later frames still add to (src/io/out.cc:436-451), in double.  A sample is final once frame
 * floor(n / wshift) is in, so after F frames a stream has delivered F * wshift samples, and ctu_streams_finish_signal delivers the
 * window - wshift behind them - what close() writes - once the file has a frame.  The samples are those of ctu_engine_run_signal on
 * the whole file: the partial sum of a sample is continued in frame order, the offline run's own sequence of additions, so the two
 * differ only where the front end's frames do (bit-equal when every push ends a multiple of eight frames into the file, else within
 * 1 LSB).  Taken: the configurations ctu_engine_create accepts for speech output on the 256- and 512-point front end (even windows
 * of 32 samples or more) - the plain chain, and with CTU_STREAMS_NR_STATE as well -nr_mode exten, whose noise estimate then travels
 * with the stream as above.  Still refused by name: hwss / fwss / 2fwss, -remove_dc1, speech output on 1024 .. 4096-point frames
 * (without CTU_STREAMS_LARGE_STATE, below).
 * Without the flag speech output is refused as before; on a configuration without speech output the flag changes nothing, and the
 * row and detector flags change nothing on one with it.  A set with signal state takes the *_signal calls below and refuses the row
 * calls (ctu_streams_push*, ctu_streams_finish*) with CTU_ERR_INPUT before anything changes; a set without it refuses the *_signal
 * calls likewise.  A stream delivers samples: wave headers are the caller's.
 *
 * Large-transform state (CTU_STREAMS_LARGE_STATE; combines with all of the above): the noise state and the signal state reach the
 * configurations whose FFT size is 1024, 2048 or 4096 points - 25 ms at 44.1 or 48 kHz, 40 ms at 16 kHz.  The flag keeps nothing of its
 * own, so it is a flag only beside CTU_STREAMS_NR_STATE or CTU_STREAMS_SIGNAL_STATE: without either, 64 is refused as an unknown flag,
 * as it always was.  Kept per stream: with
 * CTU_STREAMS_NR_STATE, Navg and Yavg of every bin as the large-transform kernels hold them in registers (floats, stored and reloaded
 * as they stand); with CTU_STREAMS_SIGNAL_STATE, an overlap-add tail of window - wshift doubles, up to 4095 of them.  Taken with the
 * noise state: -nr_mode exten on the spectrum (-nr_when beforeFB) with every feature tail ctu_engine_create accepts at these sizes,
 * and with row state the delta chains, stacking and CMS behind it.  Taken with the signal state: speech output of the plain chain,
 * and with the noise state as well behind exten; windows of odd length are fine here, as offline.  Rows and samples relate to the
 * offline run as above (bit-equal when every push ends a multiple of eight frames into the file).  Still
 * refused by name, whatever the flags: -nr_when afterFB, hwss / fwss / 2fwss on 2048- / 4096-point frames, -remove_dc1, the VAD module on 1024-point and larger
 * frames, trapdct (without CTU_STREAMS_TRAP_STATE, below), CMVN, HTK feature input.  On a configuration of 512 points or fewer the flag changes nothing, and without it
 * every answer - exten and speech output on 1024 .. 4096-point frames refused by name - is the one it was.
 *
 * Trap state (CTU_STREAMS_TRAP_STATE = 256; 128 is no flag; combines with the noise and large-transform flags): the set also keeps, per
 * stream, the last traplen - 1 log-mel rows of the file ([bands] floats each), and so takes -fea_kind trapdct,<traplen>,<ndct>: C5.
 * TRAP-DCT is a pure function of a window of log-mel rows - out[t][b * ndct + k] = sum_j G[k][j] logmel[clamp(t - half + j, 0, T - 1)][b],
 * half = (traplen - 1) / 2 - so row t is final once frame t + half exists: with H = half and wmax = half - 1 in the arithmetic of the
 * row state, after F frames a stream has delivered R(F) = F - half rows once F >= half + 1, none before (a push delivers at most as
 * many rows as it completes frames), and ctu_streams_finish delivers the last half with the file's length known.  A file that ends with
 * 1 .. half frames is the offline plan's "trapdct on fewer than (traplen+1)/2 frames": CTU_ERR_INPUT and no rows at finish, and the stream
 * starts over clean; a file without a frame finishes with nothing.  ctu_streams_config_check_ex reports halo = half, and the counting
 * function is ctu_streams_rows_step(window, wshift, half, half - 1, total, &pending): no entry point is new.  The contraction is the
 * offline fp32 one (v_mfma_f32_16x16x4_f32 over the operand minus the column's own centre value), so a row depends on nothing but its
 * own traplen log-mel rows - not on the cut into pushes, not on the other streams - and is the row of ctu_engine_run bit for bit
 * wherever the log-mel rows are (every push a multiple of eight frames into the file) and the offline run launches its fp32 kernel
 * (more than 24 bands, more than 16 coefficients or a context of more than 113 frames; elsewhere offline splits into fp16 terms and the two agree to rounding),
 * at every context length.  Contexts of more than 104 frames (traplen 105 .. 255) are summed in compensated runs of 8 taps, by the
 * offline fp32 kernel and by a stream set alike (one device helper): a single fp32 chain over them leaves the engine's parity bound
 * (1.9e-4 of the reference at 255 taps, against 1e-4).  The independence of pushes and streams holds at every size.  Taken: the plain chain at every FFT size ctu_engine_create takes trapdct at, 1024 .. 4096 points included; with
 * CTU_STREAMS_NR_STATE as well -nr_mode exten on the spectrum, and with CTU_STREAMS_LARGE_STATE beside that on 1024 .. 4096-point
 * frames.  Still refused by name with the flag: the VAD module beside trapdct (whatever the detector flag), -remove_dc1,
 * -nr_when afterFB behind exten, -s above -w; hwss / fwss / 2fwss and CMVN on trapdct are outside ctu_engine_create.  Without the flag
 * every answer is the one it was, and on a configuration of another feature kind the flag changes no answer and no row.
 *
 * Subtraction state (CTU_STREAMS_SS_STATE = 1024; 512 is no flag; combines with the row state): the set also keeps, per stream, what
 * -nr_mode hwss | fwss | 2fwss carry along a file (src/nr/nr.cc:181-442, src/vdet/CepstralDet.h:140-194) - the noise estimate Navg of
 * every bin (and Nravg in 2fwss), the Burg-cepstral detector's record (background cepstrum, dMean, dMean2, threshold, segment count) -
 * while the file's frame index, which -nr_initsegs counts, is the stream's own.  Taken: what ctu_engine_create accepts of these modes on
 * the feature path of the 256- and 512-point front end with -vad burg - cepstra, band outputs, -fea_E, -fb_inld and the LP kinds - and
 * with row state the delta chains, stacking and CMS behind them.  All of it is causal, so a row leaves with the push that completes its
 * frame, R(F) is the chain's, and ctu_streams_finish has nothing of the subtraction to add.  Every file of a stream is the first file
 * of a process: its noise estimate starts from zero and its detector afresh, so a file's rows are those of a fresh engine's
 * ctu_engine_run on that file alone - bit for bit when every push ends a multiple of eight frames into the file, else to the rounding
 * of the front end's steps - and a push neither reads nor writes what the engine's offline runs carry from
 * list to list (ctu_engine_reset_chain).  Refused by name with the flag: -vad file=... beside these modes (one byte stream per
 * process), the modes with speech output (without CTU_STREAMS_SS_SIGNAL_STATE, below), the modes on 2048- / 4096-point frames (without CTU_STREAMS_SS_LARGE_STATE, below), and what stands for every
 * set (-remove_dc1, -s above -w, ...).  Without the flag every answer is the one it was, and on a configuration without one of the
 * three modes the flag changes no answer and no row.
 *
 * Subtraction state with signal state (CTU_STREAMS_SS_SIGNAL_STATE = 2048): like CTU_STREAMS_LARGE_STATE the flag keeps nothing of its
 * own - it says that the subtraction state and the signal state meet in one set, so it is a flag only beside both
 * CTU_STREAMS_SS_STATE and CTU_STREAMS_SIGNAL_STATE: without either, 2048 is refused as an unknown flag, as it always was.  With the three
 * flags the set streams the speech-enhancement output behind -nr_mode hwss | fwss | 2fwss with -vad burg on the 256- and 512-point
 * front end (frontend_kernel<..., SS, SY, ..., XS>): windows of 129 .. 208 samples on 256 points and 257 .. 400 on 512, detectors of 2
 * to 16 coefficients, any -nr_a / -nr_b / -nr_p / -nr_q / -nr_initsegs.  Per stream the set keeps the slot of the subtraction state
 * and the overlap-add's tail of the signal state; ctu_streams_push_signal delivers wshift samples per frame a push completes,
 * ctu_streams_finish_signal the window - wshift behind them.  Every file of a stream is the first file of a process (zero seed,
 * detector afresh, tail zero), so its samples are those of a fresh engine's ctu_engine_run_signal on that file alone - bit for bit when
 * every push ends a multiple of eight frames into the file, else to the rounding of the front end's steps -
 * and a push neither reads nor writes what the engine's offline runs carry from list to list.  Refused by name with the flags:
 * -vad file=... (one byte stream per process), the modes on 2048- / 4096-point frames, -s above -w; what ctu_engine_create refuses
 * (-remove_dc1, the VAD module with speech output, longer windows) keeps the engine's words.  Without the flag every answer is the one
 * it was, and beside a configuration that is not one of the three modes with speech output the flag changes no answer and no sample.
 *
 * Subtraction state on large transforms (CTU_STREAMS_SS_LARGE_STATE = 8192; 4096 is no flag): a flag only beside CTU_STREAMS_SS_STATE -
 * without it 8192 is refused as an unknown flag, as it always was - and it does not involve CTU_STREAMS_LARGE_STATE.  With the two flags
 * the set runs -nr_mode hwss | fwss | 2fwss with -vad burg on the feature path of 2048- and 4096-point frames (44.1 / 48 kHz audio at
 * the presets' 25 ms, or long windows): whatever ctu_engine_create takes of these modes there - detectors of 2 to 32 coefficients,
 * cepstra, band outputs, the LP kinds, -fea_E, any -nr_a / -nr_b / -nr_p / -nr_q / -nr_initsegs - and with row state the delta chains,
 * stacking and CMS behind them.  Per stream the set keeps, as the large transforms' kernels hold them, Navg and Nravg of every bin and the
 * detector's record, all as doubles (bigss_kernel<NIT, true>, ss_decide_stream_kernel).  Every file of a stream is the first file of a
 * process, and none of these kernels works in steps of several frames: a file's rows are those of a fresh engine's ctu_engine_run on
 * that file alone bit for bit, however the file is cut into pushes.  A push neither reads nor writes what the
 * engine's offline runs carry from list to list.  Still refused by name with the flag: -vad file=..., the speech output of these modes
 * on 2048- / 4096-point frames (whatever other flags come with it), -s above -w, and what stands for every set; 1024-point frames,
 * more than 32 detector coefficients, trapdct, -nr_when afterFB and the VAD module beside these modes are outside ctu_engine_create.
 * Without the flag every answer is the one it was, and beside another configuration the flag changes no answer and no row.
 *
 * Detector state behind row state (CTU_STREAMS_VAD_ROW_STATE = 16384): like CTU_STREAMS_SS_SIGNAL_STATE the flag says that two kinds
 * of state meet in one set, so it is a flag only beside both CTU_STREAMS_ROW_STATE and CTU_STREAMS_VAD_STATE: alone, or beside one of
 * them, 16384 is refused as an unknown flag, as it always was.  With the three flags the set runs the VAD module with -fea_delta
 * d | d_a | d_a_t, -fea_trap, -fea_Z_exp or -fea_Z_block behind it - MFCC_0_D_A with CMS and a speech / non-speech byte per row - on
 * everything a set with detector state takes.  The reference calls the detector when a vector reaches the writer (src/io/batch.cc:172-192,
 * 230-241,251-291): call j, with the absolute index j in every branch of the recurrences, reads the criterion of input frame
 * min(j + delay, T - 1), delay the chain's halo (the sum of its windows, or the stacking window; 0 with CMS alone).  With
 * C(F) = F - delay once F >= wmax + 2 (none before: the R(F) of the row state), after F frames a stream has made C(F) calls and
 * delivered R(F) = max(C(F) - h, 0) rows and decisions, h = (vad_filter_order - 1) / 2; ctu_streams_finish makes the calls that are left
 * on the criterion of the file's last frame, pushes h zeros through the filter and delivers the rest: T rows and bytes in all for a
 * file of T > h frames the chain is defined on, nothing (CTU_OK) for one of no more than h frames, and the offline plan's "fewer than
 * window+2 frames" (CTU_ERR_INPUT) for one the chain is not defined on.  ctu_streams_config_check_ex reports halo = delay + h; the
 * counting function is ctu_streams_vad_rows_step below.  Per stream the set keeps the detector's record, the criterion input of the
 * newest frame (one energy, or up to 32 Burg cepstra, as doubles) and h more base rows than the row state alone, from which the rows
 * held back are rebuilt.  Decisions are those of ctu_engine_run on the whole file byte for byte however it is cut; rows relate to it
 * as those of the row state do.  With CTU_STREAMS_NR_STATE as well: -nr_mode exten ahead of the fused detector with CMS behind it
 * (C4 + -fea_Z_exp; delay 0).  Still refused by name with the flag: -vad_apply_mode drop, -vad_cepdist_mode fea, -fea_kind trapdct,
 * -remove_dc1, the VAD on 1024-point and larger frames, -fea_E with a filter order above 2, -nr_mode exten with a criterion outside the
 * fused shapes (so behind every delta chain or stacking).  Without the flag every answer is the one it was. */
enum { CTU_STREAMS_ROW_STATE = 1, CTU_STREAMS_NR_STATE = 4, CTU_STREAMS_VAD_STATE = 8, CTU_STREAMS_SIGNAL_STATE = 32, CTU_STREAMS_LARGE_STATE = 64, CTU_STREAMS_TRAP_STATE = 256,
       CTU_STREAMS_SS_STATE = 1024, CTU_STREAMS_SS_SIGNAL_STATE = 2048, CTU_STREAMS_SS_LARGE_STATE = 8192, CTU_STREAMS_VAD_ROW_STATE = 16384 };   /* (2, 16, 128, 512 and 4096 are no flags: sets refuse them as unknown, and callers may rely on that) */
int ctu_streams_create(ctu_engine *, int32_t n_streams, int64_t max_push_samples, ctu_streams **out);
void ctu_streams_destroy(ctu_streams *);   /* ahead of ctu_engine_destroy of its engine: a set reads its engine to the end */
int ctu_streams_config_check(int argc, const char *const *argv, char *reason, int64_t cap);
/* The two calls above are these with flags 0.  *halo (may be NULL) receives H of an accepted configuration. */
int ctu_streams_create_ex(ctu_engine *, int32_t n_streams, int64_t max_push_samples, uint32_t flags, ctu_streams **out);
int ctu_streams_config_check_ex(int argc, const char *const *argv, uint32_t flags, char *reason, int64_t cap, int32_t *halo);
/* The flag set a configuration needs (no device): the union of the kinds of state its options call for - row state for -fea_delta /
 * -fea_trap / -fea_Z_exp / -fea_Z_block, noise state for -nr_mode exten, detector state for the VAD module (and CTU_STREAMS_VAD_ROW_STATE
 * where it meets the row state), signal state for -format_out raw | wave, large-transform state beside the noise or the signal state on
 * 1024 .. 4096-point frames, trap state for trapdct, subtraction state for hwss / fwss / 2fwss (with CTU_STREAMS_SS_SIGNAL_STATE ahead of
 * speech output and CTU_STREAMS_SS_LARGE_STATE on 2048- / 4096-point frames).  No bit is set that the configuration does not need: an
 * accepted configuration is refused with any one of them cleared.  *flags (may be NULL) is written in both outcomes; the return code,
 * `reason` and *halo are those of ctu_streams_config_check_ex for that flag set - so a configuration no set takes comes back with the
 * refusal of the set that came closest, and a bad command line with the parser's text and flags 0.  A host that drives one stream per
 * input (the pipe mode of bin/ctucopy) creates its set with these flags. */
int ctu_streams_flags_for(int argc, const char *const *argv, uint32_t *flags, char *reason, int64_t cap, int32_t *halo);
int ctu_streams_push(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *d_pcm, const int64_t *sample_off,
                     const int64_t *n_samples, float *d_rows, int64_t rows_capacity, int64_t *row_counts, void *stream);
/* Host-buffer form: h_pcm[i] points at stream i's new samples, h_rows receives the rows; page-locked rows (ctu_host_alloc) are
 * DMA-ed, pageable ones go through the runtime's staging, as in ctu_engine_run_host.  Synchronised on return. */
int ctu_streams_push_host(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *const *h_pcm, const int64_t *n_samples,
                          float *h_rows, int64_t rows_capacity, int64_t *row_counts);
/* The end of a stream's file.  The reference's loop ends when fread comes up short (src/io/in.cc:314,438): a trailing partial
 * window makes no frame, so without row state every row of the file is out already and *row_count is 0.  A set with row state
 * writes the rows it held back (ctu_streams_pending of them) to d_rows, asynchronously on `stream`; room for fewer is CTU_ERR_INPUT
 * ahead of any launch, and the stream stays as it was.  A file of 1 .. window - wshift - 1 samples is the reference's "IO: Signal
 * shorter than one frame!", and a delta chain or stacking on a file of 1 .. wmax + 1 frames the offline plan's "fewer than window+2
 * frames", and trapdct (trap state) on a file of 1 .. (traplen - 1) / 2 frames its "fewer than (traplen+1)/2 frames": CTU_ERR_INPUT and no rows.  In every case but the lack of room the stream starts a new file with its next push. */
int ctu_streams_finish(ctu_streams *, int32_t stream_id, float *d_rows, int64_t rows_capacity, int64_t *row_count, void *stream);
/* Host-buffer form of the above.  Synchronised on return. */
int ctu_streams_finish_host(ctu_streams *, int32_t stream_id, float *h_rows, int64_t rows_capacity, int64_t *row_count);
/* The same four calls with the decisions of the rows they deliver (detector state): byte i of d_vad / h_vad belongs to row i of the call.
 * A NULL vad buffer makes them the calls above. */
int ctu_streams_push_vad(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *d_pcm, const int64_t *sample_off,
                         const int64_t *n_samples, float *d_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *d_vad, void *stream);
int ctu_streams_push_vad_host(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *const *h_pcm, const int64_t *n_samples,
                              float *h_rows, int64_t rows_capacity, int64_t *row_counts, uint8_t *h_vad);
int ctu_streams_finish_vad(ctu_streams *, int32_t stream_id, float *d_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *d_vad, void *stream);
int ctu_streams_finish_vad_host(ctu_streams *, int32_t stream_id, float *h_rows, int64_t rows_capacity, int64_t *row_count, uint8_t *h_vad);
/* The calls of a set with signal state.  They mirror the row calls: the samples of a push are written to d_out one stream after the
 * other in the order of stream_ids, out_counts[i] of them for stream i (host memory, filled on return; may be NULL); fewer than that
 * in out_capacity, a repeated or foreign id, or more than max_push_samples for one stream is CTU_ERR_INPUT before anything is launched
 * or changed.  Asynchronous on `stream`; the host forms are synchronised on return.  ctu_streams_finish_signal writes the window -
 * wshift samples of the stream's tail (none, with CTU_OK, for a file without a frame; 1 .. window - wshift - 1 samples are the
 * reference's "IO: Signal shorter than one frame!": CTU_ERR_INPUT and no samples), clears the tail, and the stream starts a new file -
 * with the reference's initial noise estimate - with its next push; room for fewer samples is CTU_ERR_INPUT and the stream stays as it was. */
int ctu_streams_push_signal(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *d_pcm, const int64_t *sample_off,
                            const int64_t *n_samples, int16_t *d_out, int64_t out_capacity, int64_t *out_counts, void *stream);
int ctu_streams_push_signal_host(ctu_streams *, int32_t n, const int32_t *stream_ids, const int16_t *const *h_pcm, const int64_t *n_samples,
                                 int16_t *h_out, int64_t out_capacity, int64_t *out_counts);
int ctu_streams_finish_signal(ctu_streams *, int32_t stream_id, int16_t *d_out, int64_t out_capacity, int64_t *out_count, void *stream);
int ctu_streams_finish_signal_host(ctu_streams *, int32_t stream_id, int16_t *h_out, int64_t out_capacity, int64_t *out_count);
/* The arithmetic of such a stream on its own (pure): the samples delivered after `total` input samples, F * wshift, and in *pending
 * (may be NULL) what a finish adds: window - wshift if F > 0, else 0. */
int64_t ctu_streams_signal_step(int32_t window, int32_t wshift, int64_t total, int64_t *pending);
/* Rows the stream's current file has produced so far (signal state: its frames). */
int64_t ctu_streams_frames(const ctu_streams *, int32_t stream_id);
/* Rows a finish would deliver now: the frames of the current file whose rows are held back (0 without row state).  Signal state: the
 * samples ctu_streams_finish_signal would deliver now. */
int64_t ctu_streams_pending(const ctu_streams *, int32_t stream_id);
/* The arithmetic of a stream on its own (pure): the frames a file has produced after `total` samples - the frame count of
 * ctu_num_frames, 0 while it has none - and in *carry (may be NULL) the samples the next frame already has. */
int64_t ctu_streams_step(int32_t window, int32_t wshift, int64_t total, int64_t *carry);
/* The same for the rows (pure): R(F) of a file after `total` samples for a chain of halo H >= wmax >= 0 (0, 0: no chain), and in
 * *pending (may be NULL) F - R(F).  Trap state: halo = (traplen - 1) / 2, wmax = halo - 1 (0 for a context of three frames). */
int64_t ctu_streams_rows_step(int32_t window, int32_t wshift, int32_t halo, int32_t wmax, int64_t total, int64_t *pending);
/* The same for a set with detector state (pure): R(F) for the majority filter of order filter_order (1 .. 31), F - R(F) in *pending. */
int64_t ctu_streams_vad_step(int32_t window, int32_t wshift, int32_t filter_order, int64_t total, int64_t *pending);
/* The same for a set with detector state behind row state (pure): R(F) = max(C(F) - h, 0) with C the rows of a chain of halo
 * H >= wmax >= 0 (the arguments of ctu_streams_rows_step) and h the delay of the majority filter, F - R(F) in *pending. */
int64_t ctu_streams_vad_rows_step(int32_t window, int32_t wshift, int32_t filter_order, int32_t halo, int32_t wmax, int64_t total, int64_t *pending);
/* Times of the last push on the set, measured with HIP events on its stream: ms3[0] stream_stitch_kernel, ms3[1] the front end
 * and its tails (with row state: and the row kernels behind them; with detector state: and the replay), ms3[2] stream_carry_kernel (and stream_rows_carry_kernel; trap state: stream_trap_kernel is in ms3[1]).  Blocks until that push has finished. */
int ctu_streams_last_push_ms(ctu_streams *, float *ms3);

/* ---- wire input: G.711 codes, byte-swapped and channel-interleaved PCM pushed as the caller holds them ----------------------------
 * What a push accepts beside native-endian int16_t, contiguous per stream: telephony arrives as G.711 codes, a network or a file may
 * hand over the other byte order, and capture hardware - a TDM trunk, a multichannel sound card, a microphone array - delivers frames
 * of [sample][channel].  A ctu_wire_layout says how the new samples of every stream of a push lie in one buffer, and the four calls
 * below are ctu_streams_push_vad (ctu_streams_push with a NULL vad buffer) and ctu_streams_push_signal, device and host form, with the
 * samples expanded to int16_t on their way into the set: stream_stitch_wire_kernel reads the caller's buffer where stream_stitch_kernel
 * reads d_pcm, so the expansion costs no launch and no pass through memory of its own.
 *
 * Sample k of stream stream_ids[i] is element elem_off[i] + k * stride of the buffer, k < n_samples[i].  Offsets count elements of the
 * format - 2 bytes for the S16 formats, 1 byte for G.711 - from d_in / h_in.  stride = 1 is a contiguous run, stride = the number of
 * channels with elem_off = the channel an interleaved block.  The ranges of different streams may interleave or overlap; the buffer is
 * only read, and only at the elements named.  CTU_WIRE_S16 is the sample as it lies, CTU_WIRE_S16_SWAPPED exchanges the two bytes of an
 * element, CTU_WIRE_ALAW / CTU_WIRE_MULAW is the expansion of src/io/amulaw.h:20-53, which ctu_decode_g711 computes.
 *
 * Kept: everything.  Rows, decisions, samples and counts are bit for bit those the plain call delivers for the same expanded samples, and
 * so are ctu_streams_frames / ctu_streams_pending and every later push and finish, for every flag set a set can be created with - the
 * wire calls add no flag, and ctu_streams_flags_for and the config checks answer as before.  What a set keeps of a stream is int16_t
 * either way, so wire and plain pushes may alternate on one stream.  ctu_streams_last_push_ms reports stream_stitch_wire_kernel in ms3[0].
 *
 * Refused with CTU_ERR_INPUT before anything is launched or changed, in words that name the fault: a NULL layout, a format outside
 * CTU_WIRE_S16 .. CTU_WIRE_MULAW, a stride below 1, a negative offset of a stream with samples, a buffer of 16-bit elements that is not
 * 2-byte aligned - and everything the plain call refuses: repeats, foreign ids, more than max_push_samples, too little room, the wrong
 * family of call for the set, a vad buffer on a set without detector state.  CTU_ERR_DEVICE is what it is for the plain pushes.
 *
 * The host forms take one buffer, not one pointer per stream.  They upload the covering range of the push - from the lowest element any
 * of its streams reads to the highest, ctu_wire_extent - in one copy, a page-locked buffer (ctu_host_alloc) as it lies, a pageable one
 * through the set's page-locked staging, and run the device form on it; they are synchronised on return.  A covering range of more than
 * n_streams * max_push_samples elements is CTU_ERR_INPUT: that is the staging a set owns for the per-pointer host forms, so the wire
 * forms add no memory to a set.  A layout that sparse - a few channels out of a long interleaved block - belongs to the device form,
 * which reads nothing but the elements named, or to the per-pointer calls. */
enum { CTU_WIRE_S16 = 0, CTU_WIRE_S16_SWAPPED = 1, CTU_WIRE_ALAW = 2, CTU_WIRE_MULAW = 3 };
typedef struct {
    int32_t format;   /* CTU_WIRE_*: the element type; an element is 2 bytes for the S16 formats, 1 byte for G.711 */
    int32_t stride;   /* elements from one sample of a stream to its next: 1 = contiguous, n_channels = interleaved */
} ctu_wire_layout;
int ctu_streams_push_wire(ctu_streams *, int32_t n, const int32_t *stream_ids, const void *d_in, const int64_t *elem_off,
                          const int64_t *n_samples, const ctu_wire_layout *, float *d_rows, int64_t rows_capacity, int64_t *row_counts,
                          uint8_t *d_vad /* may be NULL */, void *stream);
int ctu_streams_push_wire_host(ctu_streams *, int32_t n, const int32_t *stream_ids, const void *h_in, const int64_t *elem_off,
                               const int64_t *n_samples, const ctu_wire_layout *, float *h_rows, int64_t rows_capacity, int64_t *row_counts,
                               uint8_t *h_vad /* may be NULL */);
int ctu_streams_push_signal_wire(ctu_streams *, int32_t n, const int32_t *stream_ids, const void *d_in, const int64_t *elem_off,
                                 const int64_t *n_samples, const ctu_wire_layout *, int16_t *d_out, int64_t out_capacity, int64_t *out_counts,
                                 void *stream);
int ctu_streams_push_signal_wire_host(ctu_streams *, int32_t n, const int32_t *stream_ids, const void *h_in, const int64_t *elem_off,
                                      const int64_t *n_samples, const ctu_wire_layout *, int16_t *h_out, int64_t out_capacity, int64_t *out_counts);
/* The covering range of a push (pure): its length in elements, 0 for a push without samples, and in *first (may be NULL) its first
 * element.  Streams without samples are not looked at.  CTU_ERR_INPUT for a bad layout, a negative count or a negative offset. */
int64_t ctu_wire_extent(const ctu_wire_layout *, int32_t n, const int64_t *elem_off, const int64_t *n_samples, int64_t *first);
/* The expansion on the host (pure): samples k < n_samples of a stream whose first is element elem_off of `in`, written to out[k].
 * Returns n_samples, or CTU_ERR_INPUT for a bad layout, a negative count or offset, or a NULL buffer with samples to expand. */
int64_t ctu_wire_expand(const ctu_wire_layout *, const void *in, int64_t elem_off, int64_t n_samples, int16_t *out);

/* ---- wire input, offline: a plan's utterances out of the same buffers -----------------------------------------------------------
 * The offline twin of the wire pushes, for corpora that lie on disk as telephony left them - headerless a-law / mu-law files, PCM of the
 * other byte order, stereo call recordings with one party per channel: the bytes go to the device as they lie (half the bytes of the
 * samples for G.711, one upload for all channels of a file) and are expanded there, wire_unpack_kernel, into the plan's PCM arena.
 *
 * Addressing is that of ctu_streams_push_wire: sample k of utterance i is element elem_off[i] + k * stride of the buffer,
 * k < utt_nsamples[i] of the plan; offsets count elements of the format; stride = n_channels with elem_off = base + channel is an
 * interleaved file; ranges may interleave or overlap; the buffer is only read, and only at the elements named - it may end with the last
 * of them.  elem_off is host memory (n_utt entries) and is read before the call returns.
 *
 * ctu_plan_unpack_wire writes exactly the utterances' samples - d_pcm[ctu_plan_sample_offsets()[i] + k] - and neither the gaps between
 * utterances nor the 8 samples ahead of the first and the 512 behind the last, whose contents change no bit of a run.  d_pcm is an arena
 * as ctu_engine_run takes it (2-byte aligned is enough; 16-byte aligned stores b128).  One launch, asynchronous on `stream`; then
 * ctu_engine_run / ctu_engine_run_signal as ever, on the same stream or behind the caller's own synchronisation.  Calls on one plan
 * are ordered by the caller, as its runs are.
 *
 * Kept: everything.  Rows, VAD bytes, samples and rows_per_utt are bit for bit those of the plain call on an arena that holds
 * ctu_wire_expand's samples, for every configuration ctu_engine_create accepts on PCM - the hwss / fwss / 2fwss chain and
 * ctu_engine_reset_chain, -vad file=, ctu_plan_set_vad_ring, drop, the large transforms, speech output - because the run behind the
 * unpack is the plain one.
 *
 * The host forms are ctu_engine_run_host and ctu_engine_run_signal_host with the wire bytes going up in place of the arena: the
 * covering range of the plan's utterances (ctu_wire_extent) - of each range's utterances where the 32 MiB rule, judged on the wire
 * bytes, cuts the run into ranges on two streams; the hwss / fwss / 2fwss chain stays in one - a page-locked buffer as it lies, a
 * pageable one through the runtime's staging.  A sparse layout - a few channels out of a long interleaved block - uploads its whole
 * covering range: it belongs to the device form, which reads nothing but the elements named.  Synchronised on return.
 *
 * Refused with CTU_ERR_INPUT before anything is launched, uploaded or written, in words that name the fault: a NULL layout, a format
 * outside CTU_WIRE_S16 .. CTU_WIRE_MULAW, a stride below 1, a negative elem_off of an utterance with samples (utterances without samples
 * are not looked at), elem_off + (n - 1) * stride past int64_t, a buffer of 16-bit elements that is not 2-byte aligned, a NULL buffer on
 * a plan with samples, a plan of another engine, an engine over feature files (use ctu_engine_run_rows...),
 * ctu_engine_run_signal_wire_host on an engine without speech output and ctu_engine_run_wire_host on one with it. */
int ctu_plan_unpack_wire(ctu_engine *, const ctu_plan *, const void *d_in, const int64_t *elem_off /* host, n_utt */,
                         const ctu_wire_layout *, int16_t *d_pcm /* ctu_plan_total_samples() */, void *stream);
int ctu_engine_run_wire_host(ctu_engine *, const ctu_plan *, const void *h_in, const int64_t *elem_off, const ctu_wire_layout *,
                             float *h_rows, uint8_t *h_vad, int64_t *rows_per_utt);
int ctu_engine_run_signal_wire_host(ctu_engine *, const ctu_plan *, const void *h_in, const int64_t *elem_off,
                                    const ctu_wire_layout *, int16_t *h_out);

/* -format_in alaw | mulaw on the device: n G.711 codes -> n int16 samples, the expansion of src/io/amulaw.h:20-53
 * (alaw2lin, called from src/io/in.cc:481-560) bit for bit.  The caller lays the codes of an utterance at the same offsets
 * as its samples (ctu_plan_sample_offsets) and may decode the whole arena at once.  Asynchronous on `stream`. */
int ctu_decode_g711(ctu_engine *, const uint8_t *d_codes, int64_t n, int alaw, int16_t *d_pcm, void *stream);

/* hwss / fwss / 2fwss (-nr_mode, with -vad burg): hwssNR::new_file seeds a file's noise estimate from the spectrum vector
 * as the previous file left it (src/nr/nr.cc:212-221), so the list is one chain.  A run processes its utterances in plan
 * order as that chain (synchronously: the seeds are iterated to their fixed point) and the engine keeps the last vector
 * for the next run, as the reference keeps it for the life of the process; this call forgets it (a new process). */
int ctu_engine_reset_chain(ctu_engine *);
/* -vad file=<f> with those modes (hwssNR::vad_get_frame, src/nr/nr.cc:297-302): the decisions come from ONE byte stream for all files
 * of the process, one byte per frame in list order - every byte but NUL is speech, a byte 0xFF ends the run like the end of the
 * stream does ("NR: Unexpected end of VAD file!").  ctu_engine_create reads <f> (src/nr/nr.cc:205-209); this call replaces the
 * stream and rewinds it, ctu_engine_reset_chain rewinds it. */
int ctu_engine_set_vad_stream(ctu_engine *, const unsigned char *bytes, int64_t n);

/* The VAD's majority filter belongs to the process, not to the file: VAD::clean() = medianFilter::cleanFilter() resets `start`, the ring
 * and the decisions at the end of a file but neither historyIdx nor historySize (src/vad/vad.h:110-121), so the vectors of the next file
 * land in ring slots out of phase with the slots its rows are read from - its rows come out shifted by a frame or two, with an all-zero
 * or a repeated row - depending on the frame counts of the files in front of it (decisions are not affected).  By default every
 * utterance of a plan is treated as the first file of its own process (in phase).  A host that wants the reference's list behaviour
 * walks its list with ctu_vad_ring_step (pure: the state after a file of `frames` frames; start from 0, 0) and hands each plan the
 * historyIdx its utterances start with; the run then delivers the rows the reference would write.  bin/ctucopy does.  Not reproduced:
 * a historySize left over by a file with no more frames than the delay, at filter orders of 5 and more. */
void ctu_vad_ring_step(int32_t order, int64_t frames, int32_t *hidx, int32_t *hsize);
int ctu_plan_set_vad_ring(ctu_plan *, const int32_t *hidx /* n_utt entries, or NULL: all in phase */);
/* The same mapping for one file on its own (pure; what ctu_plan_set_vad_ring applies on the device): the number of rows the file writes - its
 * frames, or 0 when it has no more frames than the filter delays - and, if src is not NULL, for each of them the frame whose vector it carries
 * (-1: an untouched ring slot, zeros).  For hosts that pass rows through stages of their own between the engine and the writer (CMVN). */
int64_t ctu_vad_ring_rows(int32_t order, int64_t frames, int32_t hidx0, int32_t *src);

/* Timing of the last ctu_engine_run on this engine, measured with HIP events on the run's stream
 * around the dominant (front-end) kernel; blocks until that run has finished.  Returns < 0 if none. */
float ctu_engine_last_kernel_ms(ctu_engine *);
/* Name of that kernel: the instantiation this engine's configuration runs its front end on (profiles and the bench's roofline
 * line are keyed by it).  Valid for the life of the engine. */
const char *ctu_engine_kernel_name(const ctu_engine *);
/* What the front-end launch of the last run walked the filter bank with: the index of the compiled walk signature whose
 * straight-line kernel was launched, or -1 for the generic walk (no run yet, no signature matches the bank and frame shape, the
 * configuration's instantiation has no straight-line form, or CTU_PHASE2_GENERIC=1 was set at create). */
int ctu_engine_phase2_walk(const ctu_engine *);

/* ---- per-speaker CMVN over rows that are resident on the device -----------------------------------------------
 * Replaces cmvn_POST::sum_fea / stat_cm / sum_cv / stat_cv / process_frame (src/fea/post_impl.cc:51-118) and the
 * three passes over the list that BATCH::process makes for them (src/io/batch.cc:331-419): with the corpus' rows
 * kept in HBM the passes run over rows, not over audio.  The caller owns the speaker table (add_spk,
 * post_impl.cc:120-142: list order of first appearance) and, with several GPUs, sums `acc` over ranks.
 *
 * Statistics are in the reference's own order (the order of the -stat_cmvn file, src/io/out.cc:591-613):
 * slot k holds internal vector entry k+1, the last slot holds entry 0 (c0 of the base block); the energy column is
 * not part of the vector.  ctu_cmvn_cols = number of slots. */
int ctu_cmvn_cols(const ctu_engine *);

/* acc[n_spk][cols+1] (host, double) += per-speaker sums over the plan's rows and, in the last slot, the frame count.
 * mean == NULL: sums of the values (pass 1);  mean != NULL ([n_spk][cols]): sums of (value - mean)^2 (pass 2).
 * Synchronises on `stream`. */
int ctu_cmvn_accumulate(ctu_engine *, const ctu_plan *, const float *d_rows, const int32_t *spk_of_utt, int32_t n_spk,
                        const double *mean, double *acc, void *stream);

/* rows = (rows - mean) / var in place - the reference divides by the variance, not by its root
 * (src/fea/post_impl.cc:104-118).  mean, var: [n_spk][cols] (host, double).  Asynchronous on `stream`. */
int ctu_cmvn_apply(ctu_engine *, const ctu_plan *, float *d_rows, const int32_t *spk_of_utt, int32_t n_spk,
                   const double *mean, const double *var, void *stream);

/* ---- speech enhancement output (-format_out raw|wave; e.g. -preset exten) ----------------------------------
 * Replaces `while(in->get_frame()) { nr->process_frame(); out->save_frame(); }` plus the writer's close() for every
 * file: src/io/batch.cc:223-227,402-407 with sigOUT::save_frame / fill_cache (src/io/out.cc:405-451) and
 * rawOUT::close (out.cc:487-491).  d_out is an int16 arena laid out like the PCM arena: utterance i's samples start
 * at ctu_plan_sample_offsets()[i] and ctu_plan_out_samples()[i] = frames*wshift + window - wshift of them are
 * written (host byte order; the RIFF header and -endian_out are the caller's).  Asynchronous on `stream`. */
const int64_t *ctu_plan_out_samples(const ctu_plan *);
int ctu_engine_run_signal(ctu_engine *, const ctu_plan *, const int16_t *d_pcm, int16_t *d_out, void *stream);
int ctu_engine_run_signal_host(ctu_engine *, const ctu_plan *, const int16_t *h_pcm, int16_t *h_out);

/* Host-buffer conveniences (H2D of the rows, the call above, D2H for apply; synchronised on return) for callers
 * that hold the rows in host memory, like the `ctucopy` executable. */
int ctu_cmvn_accumulate_host(ctu_engine *, const ctu_plan *, const float *h_rows, const int32_t *spk_of_utt, int32_t n_spk,
                             const double *mean, double *acc);
int ctu_cmvn_apply_host(ctu_engine *, const ctu_plan *, float *h_rows, const int32_t *spk_of_utt, int32_t n_spk,
                        const double *mean, const double *var);

#ifdef __cplusplus
}
#endif
#endif
