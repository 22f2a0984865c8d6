// Wire input (include/ctu_engine.h: ctu_wire_layout, ctu_streams_push_wire*), host side: what a layout is worth before anything reaches the
// device.  Plain C++ (no HIP call, no HIP type): engine.hip includes it and exports wire_extent / wire_expand as ctu_wire_extent /
// ctu_wire_expand; the command-line host includes it through host/g711.h, which needs no engine library for it.
//
//   wire_g711            one G.711 code -> one sample: the host statement of src/io/amulaw.h:20-53 (the device's is g711_expand)
//   wire_layout_fault    why a layout cannot be used, in the words of the refusal (null: it can)
//   wire_extent          the covering range of a push: the elements from the lowest any stream reads to the highest
//   wire_expand          n samples of one stream out of a buffer, as int16_t
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/ctu_engine.h"

// G.711 expansion exactly as the reference computes it (src/io/amulaw.h:20-53): chord/step -> magnitude,
// then "2x amplification" in 16-bit wrap-around arithmetic.
inline int16_t wire_g711(uint8_t code, bool alaw) {
    const int a = (int)(int8_t)code;  // the reference works on a (signed) char
    const int sgn = (~(a >> 7)) & 1;
    int mag;
    if (!alaw) {
        const int chord = (~(a >> 4)) & 7, step = (~a) & 0xf;
        mag = (((2 * step) + 33) << chord) - 33;
    } else {
        int chord = ((a ^ 0x55) >> 4) & 7;
        const int step = (a ^ 0x55) & 0xf;
        mag = (step << 1) + 1;
        if (chord > 0) mag += 32;
        else chord = 1;
        mag <<= chord;
    }
    int out = ((1 - 2 * sgn) * mag) & 0xffff;
    out = (out << 2) & 0xffff;
    if (out & 0x8000) out -= 65536;
    return (int16_t)out;
}

inline bool wire_is_g711(int32_t format) { return format == CTU_WIRE_ALAW || format == CTU_WIRE_MULAW; }
inline int wire_elem_bytes(int32_t format) { return wire_is_g711(format) ? 1 : 2; }

// `buf`: the buffer the layout is read from (null: not looked at)
inline const char *wire_layout_fault(const ctu_wire_layout *w, const void *buf) {
    if (!w) return "wire: null layout";
    if (w->format < CTU_WIRE_S16 || w->format > CTU_WIRE_MULAW) return "wire: unknown format (CTU_WIRE_S16 .. CTU_WIRE_MULAW)";
    if (w->stride < 1) return "wire: a stride below 1";
    if (!wire_is_g711(w->format) && (reinterpret_cast<uintptr_t>(buf) & 1)) return "wire: a buffer of 16-bit elements that is not 2-byte aligned";
    return nullptr;
}

// Elements of the covering range of a push (0: no stream has samples), its first element in *first (may be null; 0 for an empty push).
// A stream without samples is not looked at.  CTU_ERR_INPUT for a bad layout, a negative count or offset.
inline int64_t wire_extent(const ctu_wire_layout *w, int32_t n, const int64_t *elem_off, const int64_t *n_samples, int64_t *first) {
    if (first) *first = 0;
    if (wire_layout_fault(w, nullptr) || n < 0 || (n && (!elem_off || !n_samples))) return CTU_ERR_INPUT;
    int64_t lo = INT64_MAX, hi = -1;
    for (int32_t i = 0; i < n; i++) {
        if (n_samples[i] < 0 || (n_samples[i] && elem_off[i] < 0)) return CTU_ERR_INPUT;
        if (!n_samples[i]) continue;
        lo = std::min(lo, elem_off[i]);
        hi = std::max(hi, elem_off[i] + (n_samples[i] - 1) * (int64_t)w->stride);
    }
    if (hi < 0) return 0;
    if (first) *first = lo;
    return hi - lo + 1;
}

// Samples k < n_samples of a stream whose first is element elem_off of `in`: out[k].  Returns n_samples, or CTU_ERR_INPUT.
inline int64_t wire_expand(const ctu_wire_layout *w, const void *in, int64_t elem_off, int64_t n_samples, int16_t *out) {
    if (wire_layout_fault(w, in) || n_samples < 0 || elem_off < 0 || (n_samples && (!in || !out))) return CTU_ERR_INPUT;
    const uint8_t *b = static_cast<const uint8_t *>(in);
    for (int64_t k = 0; k < n_samples; k++) {
        const int64_t e = elem_off + k * (int64_t)w->stride;
        if (wire_is_g711(w->format)) out[k] = wire_g711(b[e], w->format == CTU_WIRE_ALAW);
        else {
            uint16_t v;
            std::memcpy(&v, b + 2 * e, 2);
            out[k] = (int16_t)(w->format == CTU_WIRE_S16_SWAPPED ? (uint16_t)((v >> 8) | (v << 8)) : v);
        }
    }
    return n_samples;
}
