// Offline wire input (include/ctu_engine.h: ctu_plan_unpack_wire, ctu_engine_run_wire_host), host side: what is decided before
// wire_unpack_kernel is launched or a byte is uploaded.  Plain C++ (no HIP call, no HIP type): engine.hip includes it, and
// tests/host/wire_files_check.cc compiles it without the engine.
//
//   wire_unpack_fault   why a plan's utterances cannot be read through a layout, in the words of the refusal (empty: they can).  This is
//                       the bound check: the caller describes its buffer by the elements it names, so a name below element 0, or one
//                       whose number or byte address leaves int64_t, is outside any buffer and is refused, not launched
//   wire_pieces         the arena in pieces of WIRE_PIECE samples: the utterance a piece's first sample belongs to (or follows), which
//                       is where a lane of wire_unpack_kernel starts looking for its own
//   wire_part_range     the covering range of utterances [u0, u1) - what a range of a host-buffer run uploads - and the offsets of
//                       those utterances from its first element
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "wire_layout.h"

constexpr int WIRE_PIECE = 2048;  // arena samples per workgroup of wire_unpack_kernel: 256 lanes of 8

// `buf`: the buffer (null with samples to read is a fault); n[i] samples of utterance i start at element off[i]
inline std::string wire_unpack_fault(const ctu_wire_layout *w, const void *buf, int32_t n_utt, const int64_t *n, const int64_t *off) {
    if (const char *m = wire_layout_fault(w, buf)) return m;
    const int64_t unit = wire_elem_bytes(w->format);
    bool any = false;
    for (int32_t i = 0; i < n_utt; i++) {
        if (n[i] <= 0) continue;  // an utterance without samples is not looked at
        any = true;
        if (!off) return "wire: null element offsets";
        if (off[i] < 0) return "wire: a negative element offset (utterance " + std::to_string(i) + ")";
        int64_t span, last;
        if (__builtin_mul_overflow(n[i] - 1, (int64_t)w->stride, &span) || __builtin_add_overflow(off[i], span, &last) ||
            last >= INT64_MAX / unit)  // (the covering range counts last + 1 elements, (last + 1) * unit bytes: both stay inside int64_t)
            return "wire: the last element of utterance " + std::to_string(i) + " lies past int64_t";
    }
    if (any && !buf) return "wire: null buffer";
    return std::string();
}

// piece_first[b], b <= pieces: the last utterance that starts at or ahead of arena sample b * WIRE_PIECE (0 where none does); the
// pieces cover [0, sample_off[n_utt]).  sample_off: the plan's, n_utt + 1 ascending entries.
inline std::vector<int> wire_pieces(const int64_t *sample_off, int32_t n_utt) {
    std::vector<int> first;
    if (n_utt <= 0) return first;
    const int64_t pieces = (sample_off[n_utt] + WIRE_PIECE - 1) / WIRE_PIECE;
    first.resize((size_t)pieces + 1);
    int u = 0;
    for (int64_t b = 0; b <= pieces; b++) {
        while (u + 1 < n_utt && sample_off[u + 1] <= b * WIRE_PIECE) u++;
        first[(size_t)b] = u;
    }
    return first;
}

// Elements of the covering range of utterances [u0, u1) (0: none of them has samples), its first element in *first, and in rel[0 .. u1 - u0)
// every utterance's offset from it (0 for one without samples).  The arguments have passed wire_unpack_fault.
inline int64_t wire_part_range(const ctu_wire_layout *w, int32_t u0, int32_t u1, const int64_t *n, const int64_t *off, int64_t *first, int64_t *rel) {
    int64_t lo = 0;
    const int64_t extent = wire_extent(w, u1 - u0, off + u0, n + u0, &lo);
    if (first) *first = lo;
    if (rel)
        for (int32_t i = u0; i < u1; i++) rel[i - u0] = n[i] > 0 ? off[i] - lo : 0;
    return extent;
}
