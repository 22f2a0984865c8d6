// Offline wire input (include/ctu_engine.h: ctu_plan_unpack_wire): a plan's utterances out of the caller's buffer - G.711 codes, 16-bit
// elements as they lie or with their bytes exchanged, contiguous or `stride` elements apart - into the plan's PCM arena as int16_t.
// Included by engine.hip.
//
//   wire_unpack_kernel<FMT, STRIDED>   sample k of utterance i, element elem_off[i] + k * stride of the buffer, to pcm[sample_off[i] + k],
//                                      k < nsamples[i].  One launch per plan.
//
// The work is dealt in pieces of the arena, not by utterance: a workgroup takes WIRE_PIECE = 2048 consecutive arena samples, a lane
// eight of them, so a ten-hour file beside ten thousand short ones is 280 000 workgroups of the same size.  Utterances start at multiples
// of eight samples (PCM_ALIGN), so a lane's eight belong to one utterance; it finds which between the utterance its piece starts in and
// the one the next piece starts in (wire_pieces, wire_plan.h: a search over at most the utterances that begin inside the piece - none or
// one for utterances longer than a piece).  What lies between utterances, the 8 samples ahead of the first and the 512 behind the last are
// not written: a lane with none of an utterance's samples returns.
//
// Reads: only the elements named.  A lane with eight samples of a contiguous source reads the 16 (S16) or 8 (G.711) bytes they lie in as
// wide as their address allows - one b128, four dwords, or a short | three dwords | a short for 16-bit elements at 2 (mod 4); one b64, two
// dwords, or the aligned dword inside and the four bytes around it for codes (the loads of stream_stitch_wire_kernel, stream_kernels.h) -
// and never a byte outside them; the last lane of an utterance, and every lane of a strided source, goes element by element.  The
// expansion itself is wire_value / wire_pair / wire_codes of stream_kernels.h, g711_expand behind them.
// Writes: ordinary vector stores, one b128 per lane where pcm + 8 q is 16-byte aligned (a 2-byte aligned arena is taken as
// ctu_engine_run takes it: four dwords at 4 (mod 16), eight shorts else), shorts for an utterance's last 1 .. 7 samples.  No LDS, no atomics.
//
// gfx950, hipcc -O3, from the code object's metadata (VGPRs, SGPRs; no scratch, no spills, no LDS in any of them):
//   <S16, contiguous> 12, 26    <S16_SWAPPED, contiguous> 12, 26    <ALAW, contiguous> 12, 26    <MULAW, contiguous> 12, 26
//   <S16, strided>    26, 28    <S16_SWAPPED, strided>    26, 28    <ALAW, strided>    21, 28    <MULAW, strided>    17, 28
// The kernels that were there before are the code they were: all 308 functions of the build without this header are instruction for
// instruction and descriptor for descriptor those of the build with it (tools/asm_identity.py, profiles/wire_offline_asm_identity.txt).
#pragma once

#include "stream_kernels.h"  // wire_value, wire_pair, wire_codes, pack2
#include "wire_plan.h"       // WIRE_PIECE, wire_pieces: the host deals the pieces

namespace {

struct WireUnpack {
    const void *src;              // the caller's buffer, whatever its elements are
    const long long *elem_off;    // [n_utt] first element of every utterance (this call's)
    const long long *sample_off;  // [n_utt + 1] the plan's arena offsets
    const long long *nsamples;    // [n_utt]
    const int *piece_first;       // [pieces + 1] wire_pieces
    int16_t *pcm;                 // the arena
    long long stride;
};

// Eight 16-bit elements from a 2-byte aligned address, and not a byte more
__device__ __forceinline__ uint4 wire_load8_s16(const uint8_t *a) {
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(a) & 15);
    if (m == 0) return *reinterpret_cast<const uint4 *>(a);
    if ((m & 3) == 0) {
        const unsigned *u = reinterpret_cast<const unsigned *>(a);
        return make_uint4(u[0], u[1], u[2], u[3]);
    }
    const unsigned *u = reinterpret_cast<const unsigned *>(a + 2);
    const unsigned h = *reinterpret_cast<const unsigned short *>(a), t = *reinterpret_cast<const unsigned short *>(a + 14);
    const unsigned m0 = u[0], m1 = u[1], m2 = u[2];
    return make_uint4(h | (m0 << 16), (m0 >> 16) | (m1 << 16), (m1 >> 16) | (m2 << 16), (m2 >> 16) | (t << 16));
}
// Eight codes from any address, and not a byte more
__device__ __forceinline__ uint2 wire_load8_codes(const uint8_t *a) {
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(a) & 7);
    if (m == 0) return *reinterpret_cast<const uint2 *>(a);
    if (m == 4) return make_uint2(*reinterpret_cast<const unsigned *>(a), *reinterpret_cast<const unsigned *>(a + 4));
    const int h = 4 - (int)(m & 3);  // 1 .. 3 bytes ahead of the aligned dword, 4 - h behind it
    unsigned long long v = (unsigned long long)*reinterpret_cast<const unsigned *>(a + h) << (8 * h);
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (k < h) v |= (unsigned long long)a[k] << (8 * k);
#pragma unroll
    for (int k = 5; k < 8; k++)
        if (k >= h + 4) v |= (unsigned long long)a[k] << (8 * k);
    return make_uint2((unsigned)v, (unsigned)(v >> 32));
}

// grid (pieces of the arena), 256 lanes
template <int FMT, bool STRIDED>
__global__ __launch_bounds__(256) void wire_unpack_kernel(const WireUnpack p) {
    constexpr bool G711 = FMT == CTU_WIRE_ALAW || FMT == CTU_WIRE_MULAW;
    const long long a = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;  // the lane's first arena sample
    int lo = p.piece_first[blockIdx.x], hi = p.piece_first[blockIdx.x + 1];
    while (lo < hi) {  // the last utterance that starts at or ahead of a
        const int mid = (lo + hi + 1) >> 1;
        if (p.sample_off[mid] <= a) lo = mid;
        else hi = mid - 1;
    }
    const long long k0 = a - p.sample_off[lo], left = p.nsamples[lo] - k0;
    if (k0 < 0 || left <= 0) return;  // the arena's head, a gap, the tail
    const uint8_t *base = reinterpret_cast<const uint8_t *>(p.src);
    const long long step = STRIDED ? p.stride : 1, e0 = p.elem_off[lo] + k0 * step;
    int16_t *dst = p.pcm + a;
    if (left < 8) {
        for (int k = 0; k < (int)left; k++) dst[k] = (int16_t)wire_value<FMT>(base, e0 + k * step);
        return;
    }
    uint4 o;
    if constexpr (STRIDED) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = wire_value<FMT>(base, e0 + k * step);
        o = make_uint4(pack2((int16_t)v[0], (int16_t)v[1]), pack2((int16_t)v[2], (int16_t)v[3]), pack2((int16_t)v[4], (int16_t)v[5]),
                       pack2((int16_t)v[6], (int16_t)v[7]));
    } else if constexpr (G711) {
        const uint2 w = wire_load8_codes(base + e0);
        const uint2 l = wire_codes<FMT>(w.x), h = wire_codes<FMT>(w.y);
        o = make_uint4(l.x, l.y, h.x, h.y);
    } else {
        const uint4 w = wire_load8_s16(base + 2 * e0);
        o = make_uint4(wire_pair<FMT>(w.x), wire_pair<FMT>(w.y), wire_pair<FMT>(w.z), wire_pair<FMT>(w.w));
    }
    const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15);
    if (m == 0) *reinterpret_cast<uint4 *>(dst) = o;
    else if ((m & 3) == 0) {
        unsigned *u = reinterpret_cast<unsigned *>(dst);
        u[0] = o.x, u[1] = o.y, u[2] = o.z, u[3] = o.w;
    } else {
        const unsigned w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            dst[2 * k] = (int16_t)(w[k] & 0xffff);
            dst[2 * k + 1] = (int16_t)(w[k] >> 16);
        }
    }
}

}  // namespace
