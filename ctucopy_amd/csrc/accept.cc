// What the engine accepts, and with which words: the reasons a valid ctucopy configuration is outside the accelerated path, the
// eligibility predicates of the specialised kernels, and the constructor checks of the reference's VAD.  Host only, HIP-free: index
// arithmetic over Design and the constants of layout_constants.h.  engine.hip and streams_host.h ask; tables.cc decides from the
// same predicates which instantiation runs.
#include "accept.h"

#include "layout_constants.h"

namespace ctu {

// dctc with more values per frame (cepstra and c0) than phase 2 of the front ends accumulates: dct_wide_kernel behind a band-valued front end
bool dct_wide(const Design &d) { return !d.rows_in && !d.signal_out && d.kind == FeaKind::Dctc && d.nfea > MAXC; }

// Entries of the vector the VAD's `fea` criterion measures: VADcri_cepdist sizes itself on the vector it is handed (src/vad/vad.cc:182),
// which is the one OUT sees (src/io/batch.cc:76,122-130) - behind a delta or stacking chain every block of the chain's output
// (fea_delta.cc:47), not the base vector alone.
int vad_fea_entries(const Design &d) {
    const int fea_c = d.o.fea_ncepcoefs + 1;
    if (d.post_order == 0) return d.nfea;
    return d.post_stack ? fea_c * (2 * d.post_w[0] + 1) : fea_c * (d.post_order + 1);
}

// the passes behind the front end - or behind the ingest of feature files: delta chain / stacking, CMVN, CMS
static std::string post_unsupported_reason(const Design &d) {
    const Opts &o = d.o;
    if (d.post_order > 0) {
        if (d.kind != FeaKind::Dctc && d.kind != FeaKind::Lpc) return "delta / stacking on non-cepstral kinds (the reference sizes the chain as fea_ncepcoefs+1, src/fea/fea_delta.cc:22-28)";
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
        if (d.kind != FeaKind::Dctc && d.kind != FeaKind::Lpc) return "CMVN on non-cepstral kinds";
        if (!o.fea_c0) return "CMVN without -fea_c0 (c0 is part of the statistics but not of the written row)";
        if (d.post_stack) return "CMVN on stacked vectors";
        if (d.cms) return "CMVN together with CMS (the reference warns and lets CMVN win, src/io/opts.cc:262-264)";
        // the statistics are taken over every frame and the VAD runs on the normalised vectors of the last pass (src/io/batch.cc:193-204,230-241):
        // a criterion on those vectors would need the statistics first
        if (o.do_vad() && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "fea") return "the `fea` VAD criterion together with CMVN";
    }
    if (d.cms) {
        if (d.kind != FeaKind::Dctc && d.kind != FeaKind::Lpc) return "CMS on non-cepstral kinds (the reference walks fea_ncepcoefs+1 entries whatever the vector holds, src/fea/post_impl.cc:203-240)";
        if (d.post_stack) return "CMS on stacked vectors";
        if (d.cms == 2 && (o.length_b < 1 || o.length_b > 512)) return "block CMS window outside 1..512 frames";
        if (d.cms_cols > 32) return "more than 32 CMS columns";
        if (d.cms == 1 && d.post_order == 0 && d.Dbase > 32) return "exponential CMS on rows of more than 32 columns (cms_exp_kernel has a lane per column of a 32-lane half wave)";
        if (d.cms == 2 && (size_t)(64 + o.length_b - 1) * d.cms_cols * sizeof(float) > 64 * 1024) return "block CMS tile above 64 KiB of LDS";
    }
    return "";
}

// -format_in htk (src/io/batch.cc:57-60, src/io/in.cc:623-709): what DESIGN.md section 4.8 derives from the reference
static std::string rows_unsupported_reason(const Design &d) {
    const Opts &o = d.o;
    // no FEA object is built, so -fea_kind only picks the header's kind code and the writers' size rule (src/io/out.cc:95-113,148-153)
    if (d.kind == FeaKind::TrapDct) return "trapdct on input features (HTK feature input builds no FEA, src/io/batch.cc:57-60)";
    if (d.kind == FeaKind::None) return "fea_kind outside dctc | lpc | spec | logspec with HTK feature input";
    if (d.kind == FeaKind::Lpa) return "fea_kind lpa with HTK feature input (the writers drop the vector's last entry as if it held a0, src/io/out.cc:108,178)";
    if ((d.kind == FeaKind::Dctc || d.kind == FeaKind::Lpc) && !o.fea_c0)
        return "HTK feature input without -fea_c0 (the writers drop the vector's last entry, whatever it holds, src/io/out.cc:109-110,178)";
    // BATCH::init_out (src/io/batch.cc:98-119) picks the energy pointer OUT is built with: for dctc without -fea_rawenergy and with
    // -nr_when beforeFB it is nr->E (:101-108) - a load through the NR object that feature input never builds (:43,57-60; NR::E is a
    // member, src/nr/nr.h:59): the reference dies in its constructor.  The other branches pass in->E (:99,105,114) and are defined.
    if (d.kind == FeaKind::Dctc && !o.fea_rawenergy && !o.nr_when_afterFB)
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
    if (o.format_out == "pfile" && !d.post_stack && o.nfeacoefs != o.fea_ncepcoefs + 1 && (d.kind == FeaKind::Dctc || d.kind == FeaKind::Lpc))
        return "pfile output of feature files whose -nfeacoefs differs from fea_ncepcoefs+1 (pfileOUT rotates fea_ncepcoefs+1 entries and leaves the rest unwritten, src/io/out.cc:292-300)";
    return post_unsupported_reason(d);
}

namespace {
// -remove_dc1, with and without speech output
const char *dc1_unsupported_reason(const Design &d) {
    if (d.window / d.wshift > 8) return "-remove_dc1 with more than 8 frames over a sample (window / shift above 8)";
    if (d.o.fea_E && d.o.fea_rawenergy) return "-remove_dc1 together with -fea_rawenergy";
    return nullptr;
}
}  // namespace

// the constructor checks of src/vad/vad.cc:639-660, :149-195 and src/vad/vad.h:96-99, with the reference's texts; null: none fails
static const char *vad_ctor_error(const Opts &o) {
    if (!o.do_vad()) return nullptr;
    if (o.vad_cri_mode != "energy" && o.vad_cri_mode != "cepdist") return "VAD: unknown vad_cri_mode!";
    if (o.vad_thr_mode != "absolute" && o.vad_thr_mode != "perc" && o.vad_thr_mode != "adapt" && o.vad_thr_mode != "dyn") return "VAD: unknown vad_thr_mode!";
    if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode != "lpc" && o.vad_cepdist_mode != "fea" && o.vad_cepdist_mode != "in") return "VADcri_cepdist: unknown vad_cepdist_mode!";
    if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" && !o.phase_needed) return "VADcri_cepdist: cannot perform iFFT!";
    if (o.vad_filter_order < 1 || o.vad_filter_order % 2 == 0) return "medianFilter: filter order must be positive, odd number!";
    return nullptr;
}

// reasons a valid ctucopy configuration is outside the accelerated path
std::string unsupported_reason(const Design &d) {
    const Opts &o = d.o;
    if (d.signal_out) {  // row N3: IN -> NR -> sigOUT
        if (o.format_in == "htk") return "HTK feature input with signal output";
        if (o.fea_kind == "td-iir-mfcc") return "fea_kind outside the spectral path";
        if (o.dither != 0.) return "-dither != 0 makes outputs depend on file order (src/io/in.cc:205,454)";
        if (o.remove_dc1)
            if (const char *why = dc1_unsupported_reason(d)) return why;
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
        if (const char *why = dc1_unsupported_reason(d)) return why;
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
    if (o.fea_E && d.kind == FeaKind::TrapDct) return "-fea_E with trapdct (the energy lags the features by 50 frames in the reference)";
    if (o.do_vad()) {
        // trapdct delays the writer by half a context (src/fea/fea_trap.cc:53-127): the detector runs when a vector comes out, on the
        // newest input frame's criterion - the delta chains' mechanism (vp.delay); the `fea` criterion would read 368-entry vectors
        if (d.kind == FeaKind::TrapDct && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode != "lpc") return "the `fea` VAD criterion on TRAP vectors";
        if (o.vad_cri_mode != "energy" && o.vad_cri_mode != "cepdist") return "";  // rejected with the reference's text at create
        if (o.vad_cri_mode == "cepdist") {
            if (o.vad_cepdist_mode == "in") return "-vad_cepdist_mode in (HTK feature input)";
            if (o.vad_cepdist_mode == "fea" && d.kind != FeaKind::Dctc && d.kind != FeaKind::Lpc) return "-vad_cepdist_mode fea on non-cepstral features";
            const int nc = o.vad_cepdist_mode == "lpc" ? o.vad_lpc_coefs : d.nfea;
            if (nc > 32 || nc < 2) return "more than 32 (or fewer than 2) VAD cepstral coefficients";
            if (o.vad_cepdist_mode == "fea" && vad_fea_entries(d) > 64 * VAD_FEA_WIDE) return "the `fea` VAD criterion on stacked vectors of more than 512 entries";
        }
        if (o.vad_filter_order > 31) return "VAD filter order above 31";
        // behind a delayed chain the flush calls the detector again on the vector VAD::silence_frame zeroed (src/vad/vad.cc:727-736): the Burg
        // criterion divides by its energy and the reference aborts (src/vdet/Burg.h:72); the energy and `fea` criteria read the zeros unharmed
        if (o.vad_apply_mode == "silence" && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" && (d.post_order > 0 || d.kind == FeaKind::TrapDct))
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
    if (d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa) {
        if (o.fea_lporder >= d.B) return "LP order not below the number of bands: the normal equations are singular and the reference's output is rounding noise";
        if (o.fea_lporder > MAX_LP || o.fea_ncepcoefs > MAX_LP) return "LP order / cepstral order above 23 (the front end accumulates 24 lags per frame)";
    }
    if (d.B > 512) return "more than 512 filter bank channels";
    if (d.kind == FeaKind::TrapDct && o.fea_trapdct_ndct > TRAP_MAX_NDCT) return "more than 32 TRAP DCT coefficients";
    if (d.kind == FeaKind::TrapDct && o.fea_trapdct_traplen > TRAP_MAX_LEN) return "TRAP longer than 255 frames";
    // the launch shape (trap_path, layout_constants.h): the band limit is the tile's at the longest context; with the mask of non-finite
    // frames behind it the request of 50 and 51 bands passes 64 KiB from 245 frames on, and stage_trap raises the kernel's limit there
    if (d.kind == FeaKind::TrapDct && (!trap_bands_fit(d.B) || trap_path(d.B, o.fea_trapdct_traplen, o.fea_trapdct_ndct).lds_bytes > LDS_RAISED))
        return "too many bands for the TRAP tile";
    return "";
}

int create_check(const Design &d, std::string &err) {
    if (const char *bad = vad_ctor_error(d.o)) {
        err = bad;
        return CTU_ERR_OPTS;
    }
    if (const std::string why = unsupported_reason(d); !why.empty()) {
        err = "ENGINE: configuration not on the accelerated path: " + why;
        return CTU_ERR_UNSUPPORTED;
    }
    return CTU_OK;
}

int streams_check(const Design &d, uint32_t flags, std::string &err) {
    if (const std::string why = unsupported_reason(d); !why.empty()) {
        err = "ENGINE: configuration not on the accelerated path: " + why;
        return CTU_ERR_UNSUPPORTED;
    }
    if (streams_flags_unknown(flags)) {
        err = "ENGINE: unknown stream set flags";
        return CTU_ERR_INPUT;
    }
    if (const std::string why = streams_unsupported_reason(d, flags); !why.empty()) {
        err = "ENGINE: configuration cannot be streamed: " + why;
        return CTU_ERR_UNSUPPORTED;
    }
    return CTU_OK;
}

// Streaming input (ctu_streams_create): what an accepted configuration carries from one frame of a file to the next beyond the samples
// themselves.  A stream set keeps samples (stream_kernels.h), so every such chain is refused by the option that brings the state in.
// With CTU_STREAMS_ROW_STATE the set keeps base rows and running means as well (stream_rows_kernels.h): the delta chain, stacking and CMS pass.
// With CTU_STREAMS_NR_STATE it keeps the noise estimate of -nr_mode exten on the spectrum (256- and 512-point front end): that passes too.
// With CTU_STREAMS_SIGNAL_STATE it keeps the overlap-add's tail of speech output (stream_signal_kernels.h): -format_out raw | wave passes on
// the 256- and 512-point front end, the plain chain and - with the noise state as well - exten.  Without the flag every answer is the one it was.
// With CTU_STREAMS_LARGE_STATE the noise state and the signal state reach 1024 .. 4096-point frames (wave1k_kernel / bigfft_kernel<..., XS>,
// stream_ola_big_kernel): the two refusals by size below fall away, everything else stands.  Without the flag every answer is the one it was.
// With CTU_STREAMS_TRAP_STATE it keeps the last traplen - 1 log-mel rows of every stream (stream_trap_kernels.h): -fea_kind trapdct passes
// on the plain chain and behind exten's state; beside the VAD module it stays refused.  Without the flag every answer is the one it was.
// With CTU_STREAMS_SS_STATE it keeps what hwss / fwss / 2fwss carry along a file - the noise estimate(s) per bin and the Burg-cepstral detector's
// record (frontend_kernel<..., SS, ..., XS>): the modes pass on the feature path of the 256- and 512-point front end with -vad burg; -vad file=,
// speech output and 2048- / 4096-point frames are refused by name.  Without the flag every answer is the one it was.
// With CTU_STREAMS_SS_SIGNAL_STATE beside the subtraction state and the signal state the two meet in one set (frontend_kernel<..., SS, SY, ..., XS>
// ahead of stream_ola_kernel): the modes pass with speech output where ss_eligible holds; -vad file=, 2048- / 4096-point frames and -s above -w
// are refused by name.  Without the flag every answer is the one it was.
// With CTU_STREAMS_SS_LARGE_STATE beside the subtraction state the latter reaches 2048- / 4096-point frames (bigss_kernel<NIT, true> behind
// ss_decide_stream_kernel): the modes pass on the feature path where ss_big_eligible holds; -vad file=, speech output at these sizes and
// -s above -w are refused by name.  Without the flag every answer is the one it was.
// With CTU_STREAMS_VAD_ROW_STATE beside the row state and the detector state the VAD module passes with a delta chain, stacking or CMS behind
// it (the delayed calls of stream_vad_decide_kernel<true>, the criterion record, h more history rows); drop, the `fea` criterion, trapdct,
// -fea_E behind the majority filter, large frames and exten outside the fused shapes stay refused by name.  Without the flag every answer
// is the one it was.
std::string streams_unsupported_reason(const Design &d, uint32_t flags) {
    const Opts &o = d.o;
    if (d.rows_in) return "-format_in htk (HTK feature input: there are no samples to stream)";
    const bool ss_state = (flags & CTU_STREAMS_SS_STATE) != 0 && ss_mode_of(o) != 0;  // (beside another -nr_mode the flag changes no answer)
    const bool ss_large = ss_state && (flags & CTU_STREAMS_SS_LARGE_STATE) != 0;  // (the subtraction state reaches 2048- / 4096-point frames)
    // what no set with subtraction state carries, on the feature path or ahead of speech output
    auto ss_refused = [&]() -> std::string {
        if (o.vadmode == "file") return "-vad file=... with -nr_mode " + o.nr_mode + " (the decision bytes are one stream per process, read on from file to file: a stream set has no place in it)";
        if (!ss_eligible(d)) {  // (what ctu_engine_create takes beside ss_eligible: ss_big_eligible)
            if (!ss_large)
                return "-nr_mode " + o.nr_mode + " on " + std::to_string(d.wfft) + "-point frames (-w: the passes of the large transforms' subtraction are not streamed, a stream set carries the one of the 256- and 512-point front end)";
            // the large transforms' state travels with the stream (bigss_kernel<NIT, true>, ss_decide_stream_kernel): the feature path
            if (d.signal_out)
                return "-nr_mode " + o.nr_mode + " with -format_out raw | wave on " + std::to_string(d.wfft) + "-point frames (speech output behind the large transforms' subtraction is not streamed, whatever the other flags: CTU_STREAMS_SS_LARGE_STATE serves the feature path)";
        }
        return "";
    };
    // (CTU_STREAMS_SS_SIGNAL_STATE is a flag only beside the subtraction state and the signal state: streams_flags_unknown)
    constexpr uint32_t ss_signal_flags = CTU_STREAMS_SS_STATE | CTU_STREAMS_SIGNAL_STATE | CTU_STREAMS_SS_SIGNAL_STATE;
    if (d.signal_out && ss_state && (flags & ss_signal_flags) == ss_signal_flags) {
        // both kinds of state in one set (frontend_kernel<..., SS, SY, ..., XS> ahead of stream_ola_kernel): what neither carries alone is
        // refused in the words of the subtraction state and of the signal state
        if (const std::string why = ss_refused(); !why.empty()) return why;
        if (d.wshift > d.window) return "-s above -w (frames that leave samples out)";
        return "";  // (-remove_dc1, the VAD module, longer windows: unsupported_reason, ahead of anything a set is asked)
    }
    if (d.signal_out && ss_large)  // (on 2048- / 4096-point frames the refusal names the size, whatever other flags come with it)
        if (const std::string why = ss_refused(); !why.empty()) return why;
    if (d.signal_out && ss_state)
        return "-nr_mode " + o.nr_mode + " with -format_out raw | wave (speech output behind hwss / fwss / 2fwss is not streamed, whatever the signal flag: the subtraction state serves the feature path)";
    if (d.signal_out && !(flags & CTU_STREAMS_SIGNAL_STATE)) return "-format_out raw | wave (speech output: the overlap-add runs across a file's frames)";
    const bool nr_state = (flags & CTU_STREAMS_NR_STATE) != 0, large_state = (flags & CTU_STREAMS_LARGE_STATE) != 0;
    if (d.signal_out) {  // the overlap-add's tail travels with the stream (stream_signal_kernels.h), exten's state as on the feature path
        if (o.nr_mode != "none" && !(o.nr_mode == "exten" && nr_state)) return "-nr_mode " + o.nr_mode + " (the noise estimate runs from frame to frame of a file)";
        if (o.remove_dc1) return "-remove_dc1 (a frame's offset stays subtracted from the samples the later frames share with it)";
        if (d.wfft >= 1024 && !large_state)
            return "-format_out raw | wave on " + std::to_string(d.wfft) + "-point frames (-w: a stream set carries the overlap-add behind the 256- and 512-point front end; the large transforms' synthesis is not streamed)";
        if (d.wshift > d.window) return "-s above -w (frames that leave samples out)";
        return "";  // (nothing else of a speech-output configuration runs along a file: no rows, no detector - unsupported_reason)
    }
    if (o.nr_mode == "exten" && nr_state) {  // the state of exten on the spectrum travels with the stream (frontend_kernel<..., XS>)
        if (o.nr_when_afterFB) return "-nr_when afterFB (exten behind the filter bank keeps its noise estimate per band, inside the filter-bank walk: a stream set carries the estimate per bin)";
        if (d.wfft >= 1024 && !large_state) return "-nr_mode exten on " + std::to_string(d.wfft) + "-point frames (-w: the noise estimate of the large transforms lives in their own kernels, a stream set carries the one of the 256- and 512-point front end)";
    } else if (ss_state) {  // the noise estimate(s) and the detector's record travel with the stream (frontend_kernel<..., SS, ..., XS>)
        if (const std::string why = ss_refused(); !why.empty()) return why;
    } else if (o.nr_mode != "none") return "-nr_mode " + o.nr_mode + " (the noise estimate runs from frame to frame of a file)";
    if (o.remove_dc1) return "-remove_dc1 (a frame's offset stays subtracted from the samples the later frames share with it)";
    if (o.do_vad() && !(flags & CTU_STREAMS_VAD_STATE)) return "the VAD module (-vad_apply_mode / -vad_out_mode: thresholds and the majority filter run along the file)";
    if (o.do_vad()) {  // the detector's state travels with the stream (stream_vad_kernels.h); what it cannot carry is refused by name
        const bool burg = o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc";
        if (o.vad_apply_mode == "drop") return "-vad_apply_mode drop (the row count of a push would depend on the data)";
        if (o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "fea") return "-vad_cepdist_mode fea (the criterion reads finished rows)";
        if (d.kind == FeaKind::TrapDct) return "-fea_kind trapdct (a vector spans traplen frames)";
        // with CTU_STREAMS_VAD_ROW_STATE beside the row and the detector state the calls run behind the chain's delay (stream_vad_kernels.h:
        // stream_vad_decide_kernel<true>), and the rows leave h calls behind theirs
        const bool vad_rows = (flags & STREAMS_VAD_ROW_FLAGS) == STREAMS_VAD_ROW_FLAGS;
        if (d.post_order > 0 && !vad_rows)
            return std::string(d.post_stack ? "-fea_trap" : "-fea_delta") + " together with the VAD module (the detector is called when a vector reaches the writer, on frame min(t + H, T - 1))";
        if (d.cms && !vad_rows) return std::string(d.cms == 1 ? "-fea_Z_exp" : "-fea_Z_block") + " together with the VAD module (CMS behind the detector's delayed rows is not carried by a stream set)";
        if (o.fea_E && (o.vad_filter_order - 1) / 2 > 0) return "-fea_E with the VAD module's majority filter (the offline run shifts the energy column along the file)";
        if (d.wfft >= 1024) return "the VAD module on 1024-point and larger frames (-w: a stream set carries the detector behind the 256- and 512-point front end)";
        if (o.nr_mode == "exten" && !(burg && vf_eligible(d)))
            return "-nr_mode exten with a VAD criterion outside the fused shapes (25 ms frames at 8 or 16 kHz, the lpc criterion with 14 coefficients: the exported spectra are not carried behind exten's state)";
    }
    // with CTU_STREAMS_TRAP_STATE the last traplen - 1 log-mel rows travel with the stream (stream_trap_kernels.h)
    if (d.kind == FeaKind::TrapDct && !(flags & CTU_STREAMS_TRAP_STATE)) return "-fea_kind trapdct (a vector spans traplen frames)";
    const bool row_state = (flags & CTU_STREAMS_ROW_STATE) != 0;
    if (d.post_order > 0 && !row_state) return d.post_stack ? "-fea_trap (stacking spans 2 * trap_win + 1 frames)" : "-fea_delta (the delta chain spans the frames of its windows)";
    if (d.cms && !row_state) return d.cms == 1 ? "-fea_Z_exp (CMS: the running mean runs along the file)" : "-fea_Z_block (CMS: the block mean spans its window of frames)";
    if (o.stat_cmvn || o.apply_cmvn) return "-stat_cmvn / -apply_cmvn (CMVN: statistics over whole lists)";
    if (d.wshift > d.window) return "-s above -w (frames that leave samples out)";
    return "";
}

// The flag set a configuration needs on a stream set (ctu_streams_flags_for): the union of the kinds of state its options call for, each
// under the condition streams_unsupported_reason asks for it under - so every bit set is one whose absence is a refusal (or, for the flags
// that only say how far another reaches, an unknown flag set), and a configuration no set takes gets its refusal for this very set.
uint32_t streams_flags_for(const Design &d) {
    const Opts &o = d.o;
    const bool exten = o.nr_mode == "exten", ss = ss_mode_of(o) != 0;
    uint32_t f = 0;
    if (d.signal_out) {  // (the row and the detector flags change nothing beside speech output)
        f |= CTU_STREAMS_SIGNAL_STATE;
        if (exten) f |= CTU_STREAMS_NR_STATE;
        if (ss) f |= CTU_STREAMS_SS_STATE | CTU_STREAMS_SS_SIGNAL_STATE | (d.wfft >= 2048 ? CTU_STREAMS_SS_LARGE_STATE : 0);
        else if (d.wfft >= 1024) f |= CTU_STREAMS_LARGE_STATE;
        return f;
    }
    if (d.post_order > 0 || d.cms) f |= CTU_STREAMS_ROW_STATE;
    if (exten) f |= CTU_STREAMS_NR_STATE | (d.wfft >= 1024 ? CTU_STREAMS_LARGE_STATE : 0);
    if (o.do_vad()) f |= CTU_STREAMS_VAD_STATE | ((f & CTU_STREAMS_ROW_STATE) ? CTU_STREAMS_VAD_ROW_STATE : 0);
    if (d.kind == FeaKind::TrapDct) f |= CTU_STREAMS_TRAP_STATE;
    if (ss) f |= CTU_STREAMS_SS_STATE | (d.wfft >= 2048 ? CTU_STREAMS_SS_LARGE_STATE : 0);
    return f;
}

// the plain cepstral chain: what the specialised instantiations (GEN_PLAIN / GEN_EXTEN with MD) cover
static bool plain_cepstral(const Design &d) {
    const Opts &o = d.o;
    return !o.nr_when_afterFB && d.kind == FeaKind::Dctc && d.nfea <= 16 && !o.fea_E && o.fb_power && o.remove_dc && !o.remove_dc1 && !o.fb_inld && !d.signal_out;
}
// the frame shapes the fused detector paths are built for: 8 kHz / 25 ms (256-point mode, two frames per complex transform) and
// 16 kHz / 25 ms (512-point mode, 16 lanes x 25 samples) - vad_fused.h
static bool fused_frame_shape(const Design &d) {
    return (d.wfft == 256 && d.window == VF_WINDOW) || (d.wfft == 512 && d.window == VF0_WINDOW);
}
// the *ss modes' detector: any window its lanes' 13 / 25 samples cover in the two transform sizes (the run-time-flag instantiations look
// the window's end up at run time); the shapes above keep their straight-line instantiations on the plain chain
static bool ss_frame_shape(const Design &d) {
    return (d.wfft == 256 && d.window > 128 && d.window <= 16 * VF_SPL) || (d.wfft == 512 && d.window > 256 && d.window <= 16 * VF0_SPL);
}
// Burg-cepstral VAD criterion fused into the front end (vad_fused.h): 14 coefficients (the preset's detector)
bool vf_eligible(const Design &d) {
    const Opts &o = d.o;
    return plain_cepstral(d) && o.do_vad() && o.vad_cri_mode == "cepdist" && o.vad_cepdist_mode == "lpc" &&
           fused_frame_shape(d) && o.vad_lpc_coefs == VF_NC && d.post_order == 0;
}
// the compressed-band LP chain (PLP and friends: -fb_inld, at most 16 lags, no energy column, no NR, no VAD): its cosine iDFT
// (src/fea/fea_impl.cc:181-198) is the same contraction over the bands as the DCT and takes the same MFMA tail
static bool lp_md_eligible(const Design &d) {
    const Opts &o = d.o;
    return (d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa) && o.fb_inld && o.fea_lporder + 1 <= 16 && !o.nr_when_afterFB && !o.fea_E &&
           o.fb_power && o.remove_dc && !o.remove_dc1 && !d.signal_out && !o.do_vad() && o.nr_mode == "none";
}
bool md_eligible(const Design &d) {
    // (the *ss modes on another window than the presets' run the run-time-flag instantiation, which has no MFMA tail)
    return (plain_cepstral(d) && (!d.o.do_vad() || vf_eligible(d)) && !(ss_mode_of(d.o) && !fused_frame_shape(d))) || lp_md_eligible(d);
}
// hwss / fwss / 2fwss with the Burg cepstral detector (frontend_kernel<..., SS>): 25 ms frames at 8 or 16 kHz, the
// presets' 12 cepstral coefficients for the detector, the plain chain into cepstra or band energies
int ss_mode_of(const Opts &o) { return o.nr_mode == "hwss" ? 1 : o.nr_mode == "fwss" ? 2 : o.nr_mode == "2fwss" ? 3 : 0; }
// the same modes ahead of sigOUT (-format_out raw|wave): the NR object works on in->_Xsabs - magnitudes, -fb_power is forced off there -
// and the enhanced frames go back to the time domain inside the front end (frontend_kernel<..., SS, SY>)
static bool ss_signal_eligible(const Design &d) {
    const Opts &o = d.o;
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= SS_NC) || o.vadmode == "file";
    return d.signal_out && ss_mode_of(o) && det_ok && ss_frame_shape(d) && o.remove_dc && !o.remove_dc1 && !o.rasta && !o.do_vad();
}
bool ss_eligible(const Design &d) {
    const Opts &o = d.o;
    if (d.signal_out) return ss_signal_eligible(d);
    // cepstra / LP coefficients in the sixteen-row accumulators, or band energies; everything behind the front end (the LP tail, delta /
    // stacking, CMS, CMVN) runs on the rows of the last pass of the seed iteration
    const bool lp = d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa;
    const bool kind_ok = (d.kind == FeaKind::Dctc && d.nfea <= 16) || (lp && o.fea_lporder + 1 <= 16) || d.kind == FeaKind::Spec || d.kind == FeaKind::LogSpec;
    // -vad file=<f> (nr.cc:205-209, 297-302): the decisions come from a byte stream instead of the detector; same kernel, same frame shapes
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= SS_NC) || o.vadmode == "file";
    // CMVN is two passes over the list in the reference (statistics, then the rows): the second starts from the noise vector the first
    // left behind, and no oracle restates that - refused rather than guessed
    return ss_mode_of(o) && det_ok && !o.nr_when_afterFB && ss_frame_shape(d) && kind_ok && o.remove_dc && !o.remove_dc1 && !o.do_vad() && !d.signal_out && !o.rasta &&
           !o.stat_cmvn && !o.apply_cmvn;
}

// the same modes on 2048- and 4096-point frames (bigss_kernel.h): spectra exported once, a workgroup per frame for the detector's cepstra
// (2 to 32 coefficients: bigburg_kernel's two instantiations), a workgroup per chain of utterances for the subtraction.  What
// ss_eligible excludes for reasons that do not depend on the size stays excluded; 1024 points (wave1k_kernel's size) stay refused whole.
bool ss_big_eligible(const Design &d) {
    const Opts &o = d.o;
    if (!ss_mode_of(o) || (d.wfft != 2048 && d.wfft != 4096) || d.window <= d.wfft / 2) return false;
    const bool det_ok = (o.vadmode == "burg" && o.fea_ncepcoefs >= 2 && o.fea_ncepcoefs <= 32) || o.vadmode == "file";
    if (!det_ok || !o.remove_dc || o.remove_dc1 || o.rasta || o.do_vad()) return false;
    if (d.signal_out) return true;
    const bool kind_ok = d.kind == FeaKind::Dctc || d.kind == FeaKind::Lpc || d.kind == FeaKind::Lpa || d.kind == FeaKind::Spec ||
                         d.kind == FeaKind::LogSpec;
    return kind_ok && !o.nr_when_afterFB && !o.stat_cmvn && !o.apply_cmvn && d.B <= 64;
}

}  // namespace ctu
