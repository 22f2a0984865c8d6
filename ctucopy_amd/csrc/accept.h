// What the engine accepts (accept.cc): host only, HIP-free.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/ctu_engine.h"
#include "design.h"

namespace ctu {

// Reasons a valid ctucopy configuration is outside the accelerated path ("" = it runs): the whole configuration (the passes behind the
// front end and HTK feature input included), and what a stream set (ctu_streams_create, flags CTU_STREAMS_*) cannot carry from frame to frame.
std::string unsupported_reason(const Design &d);
std::string streams_unsupported_reason(const Design &d, uint32_t flags = 0);
// What ctu_engine_create answers before it looks at a device: CTU_OK, or the code to return with the text of ctu_create_error in `err`
// (the reference's VAD constructor checks with its texts, then unsupported_reason).
int create_check(const Design &d, std::string &err);
// ... and ctu_streams_config_check_ex, for a design after spread_small_fft
constexpr uint32_t STREAMS_FLAGS = CTU_STREAMS_ROW_STATE | CTU_STREAMS_NR_STATE | CTU_STREAMS_VAD_STATE | CTU_STREAMS_SIGNAL_STATE | CTU_STREAMS_LARGE_STATE |
                                   CTU_STREAMS_TRAP_STATE | CTU_STREAMS_SS_STATE | CTU_STREAMS_SS_SIGNAL_STATE | CTU_STREAMS_SS_LARGE_STATE |
                                   CTU_STREAMS_VAD_ROW_STATE;
// CTU_STREAMS_LARGE_STATE keeps nothing of its own: it says how far the noise state and the signal state reach.  Without either it names
// no state, and a set answers what it always answered to 64: unknown flags.  CTU_STREAMS_SS_SIGNAL_STATE likewise: it says that the
// subtraction state and the signal state meet in one set, and without both of them 2048 is the unknown flag it always was.
// CTU_STREAMS_SS_LARGE_STATE says how far the subtraction state reaches (2048- / 4096-point frames): without it 8192 is the unknown flag it always was.
// CTU_STREAMS_VAD_ROW_STATE says that the row state and the detector state meet in one set: without both of them 16384 is the unknown flag it always was.
constexpr uint32_t STREAMS_VAD_ROW_FLAGS = CTU_STREAMS_ROW_STATE | CTU_STREAMS_VAD_STATE | CTU_STREAMS_VAD_ROW_STATE;
inline bool streams_flags_unknown(uint32_t flags) {
    constexpr uint32_t both = CTU_STREAMS_SS_STATE | CTU_STREAMS_SIGNAL_STATE;
    if ((flags & CTU_STREAMS_VAD_ROW_STATE) && (flags & STREAMS_VAD_ROW_FLAGS) != STREAMS_VAD_ROW_FLAGS) return true;
    return (flags & ~STREAMS_FLAGS) || ((flags & CTU_STREAMS_LARGE_STATE) && !(flags & (CTU_STREAMS_NR_STATE | CTU_STREAMS_SIGNAL_STATE))) ||
           ((flags & CTU_STREAMS_SS_SIGNAL_STATE) && (flags & both) != both) || ((flags & CTU_STREAMS_SS_LARGE_STATE) && !(flags & CTU_STREAMS_SS_STATE));
}
int streams_check(const Design &d, uint32_t flags, std::string &err);
// ... and ctu_streams_flags_for: the flags a set needs for this design (after spread_small_fft), whether or not any set takes it
uint32_t streams_flags_for(const Design &d);

// dctc with more values per frame (cepstra and c0) than phase 2 of the front ends accumulates: dct_wide_kernel behind a band-valued front end
bool dct_wide(const Design &d);
int ss_mode_of(const Opts &o);          // hwss / fwss / 2fwss: 1 / 2 / 3, else 0
int vad_fea_entries(const Design &d);   // entries of the vector the VAD's `fea` criterion measures
// Which specialised kernels a configuration is shaped for (fe_select and build_phase2 follow these)
bool vf_eligible(const Design &d);      // Burg-cepstral VAD criterion fused into the front end
bool md_eligible(const Design &d);      // DCT / cosine-iDFT tail on the matrix cores
bool ss_eligible(const Design &d);      // hwss / fwss / 2fwss inside the 256- / 512-point front end
bool ss_big_eligible(const Design &d);  // the same modes on 2048- / 4096-point frames (bigss_kernel.h)

}  // namespace ctu
