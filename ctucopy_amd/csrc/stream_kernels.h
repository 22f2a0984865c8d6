// Streaming input (include/ctu_engine.h: ctu_streams_*): the kernels around the front end of a push.
// Included by engine.hip.
//
// A stream is a file whose samples arrive in pushes.  Frame t of a file reads samples [t wshift - 1, t wshift + window): its window and,
// with pre-emphasis, the sample ahead of it (src/io/in.cc:365,384: preemtmp; 0 ahead of frame 0).  DC removal (-remove_dc) takes the mean
// of the frame's own window (in.cc:375-382) and needs nothing more.  So after `total` samples, of which F = stream_frames() frames have
// come out, the next frame still needs the samples from F wshift - 1 on: the carry, at most `window` values
//   carry[0]      the sample ahead of the next frame (anything while F = 0: the kernels put 0 there at a file's start, TileRec::t0)
//   carry[1 + k]  sample F wshift + k of the file, k < total - F wshift <= window - 1
// kept per stream in HBM beside the count of samples taken.
//
//   stream_stitch_kernel  writes lead | carry | new samples of every pushed stream into its slot of the push arena - the slot
//                         ctu_arena_layout's rule gives an utterance of 8 + carry + new samples, the next frame's first sample 8 samples
//                         into it - and the tile records of the frames the stream now completes: what an offline plan holds for an
//                         utterance of that many frames, except that t0 counts from the file's start (only t0 + frame == 0 is ever
//                         asked of it on the chains a stream set accepts: the first sample of a file has no history)
//   stream_stitch_wire_kernel<FMT, STRIDED>   the same with the new samples read through a ctu_wire_layout (ctu_streams_push_wire*): G.711
//                         codes through g711_expand, 16-bit elements as they lie or with their bytes exchanged, contiguous or `stride`
//                         elements apart - expanded on their way into the slot, which is int16_t as ever
//   stream_carry_kernel   behind it: the new carry out of the slot, the new count
// Vector loads and stores only; sources are 2-byte aligned (as the front ends' pcm4 loads are), the slots and the carry rows 16-byte
// aligned, so every store is a b128.  A workgroup of 256 lanes per stream and slice of 2048 slot samples; no atomics: a stream id
// appears once in a push.
//
// Noise state (CTU_STREAMS_NR_STATE on a chain with -nr_mode exten): the front end walks chains of whole
// streams, one per wave, as it walks chains of whole utterances offline.  The host deals the streams that complete a frame onto the
// chains and sends the heads and, per stream, the tile behind its last one; stream_stitch_kernel links the records accordingly and
// notes every tile's stream, where the front end finds the slot of the state.
//
// gfx950, hipcc -O3: stream_stitch_kernel 15 VGPRs, 58 SGPRs; stream_carry_kernel 17 VGPRs, 45 SGPRs; no spills, no scratch, no LDS.
// stream_stitch_wire_kernel, all eight instantiations: 15 VGPRs, 58 SGPRs, no spills, no scratch, no LDS (the record loop is the widest
// part of each).  With the wire kernels beside them stream_stitch_kernel and stream_carry_kernel are the code they were: instruction for
// instruction (743 and 536) and kernel descriptor for kernel descriptor equal to the build before the wire kernels existed, compared on
// the assembly of both builds.
#pragma once

#include "decode_kernels.h"  // g711_expand
#include "stream_plan.h"  // StreamPush, stream_frames, STREAM_LEAD, STREAM_SLICE: the host plans a push by them

namespace {

struct StreamState {
    long long consumed;  // samples of the current file taken so far
};

struct StreamParams {
    const StreamPush *push;
    StreamState *state;
    int16_t *carry;         // [n_streams][cstride]
    int16_t *arena;         // the push arena
    const int16_t *src;     // the caller's new samples (stream_stitch_wire_kernel: the caller's buffer, whatever its elements are)
    TileRec *tiles;
    int cstride, window, wshift;
    int n_tiles, grid;      // tiles of the whole push and the workgroups of the front-end launch: tile i is followed by tile i + grid
    int *tile_stream;       // noise state (null without): the stream of every tile, and chains of whole streams - a stream's tiles follow
                            // each other, StreamPush::pad follows its last one
};

__device__ __forceinline__ unsigned pack2(const int16_t a, const int16_t b) { return (unsigned)(unsigned short)a | ((unsigned)(unsigned short)b << 16); }

// The tile records of the frames a pushed stream completes now, T of them behind the file's first F: the one statement of them, expanded
// in stream_stitch_kernel and stream_stitch_wire_kernel (slice 0 of the stream's workgroups writes them) with their p, d, F and T in scope.
// A macro and not a device function: the compiler simplifies a function ahead of inlining it, and stream_stitch_kernel then comes out as
// other instructions (738 for 743, 16 VGPRs for 15, 60 SGPRs for 58, measured) - the plain push is to run what it ran.
#define STREAM_TILE_RECORDS()                                                                                                               \
    do {                                                                                                                                    \
        const int t0 = (int)(F < 0x3fffffff ? F : 0x3fffffff); /* frames ahead of the push; only "none" matters (file start) */             \
        for (int t = threadIdx.x; 64 * t < T; t += 256) {                                                                                   \
            const int idx = d.tile0 + t;                                                                                                    \
            const long long sbase = d.slot + STREAM_LEAD + (long long)t * TILE * p.wshift, rbase = d.row0 + (long long)t * TILE;            \
            int4 *w = reinterpret_cast<int4 *>(p.tiles + idx);                                                                              \
            w[0] = make_int4((int)(sbase & 0xffffffff), (int)(sbase >> 32), (int)(rbase & 0xffffffff), (int)(rbase >> 32));                 \
            int next = idx + p.grid < p.n_tiles ? idx + p.grid : -1;                                                                        \
            if (p.tile_stream) {                                                                                                            \
                next = TILE * (t + 1) < T ? idx + 1 : d.pad;                                                                                \
                p.tile_stream[idx] = d.id;                                                                                                  \
            }                                                                                                                               \
            w[1] = make_int4(min(TILE, T - TILE * t), t0 + TILE * t, next, t0 + T);                                                         \
        }                                                                                                                                   \
    } while (0)

// grid (pushed streams, slices), 256 lanes
__global__ __launch_bounds__(256) void stream_stitch_kernel(const StreamParams p) {
    const StreamPush d = p.push[blockIdx.x];
    const long long total = p.state[d.id].consumed;
    const long long F = stream_frames(total, p.window, p.wshift);
    const int c = (int)(total - F * p.wshift);  // carried samples of the next frame, < window
    const int T = (int)(stream_frames(total + d.n, p.window, p.wshift) - F);
    const int len = STREAM_LEAD + c + d.n;
    const int16_t *cr = p.carry + (size_t)d.id * p.cstride;
    const int16_t *nw = p.src + d.src;
    const int q = blockIdx.y * 256 + threadIdx.x;  // which 8 samples of the slot
    if (8 * q < len) {
        int16_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int r = 8 * q + k - STREAM_LEAD;  // position from the next frame's first sample
            int16_t x = 0;
            if (r >= -1 && r < c) x = cr[r + 1];
            else if (r >= c && r < c + d.n) x = nw[r - c];
            v[k] = x;
        }
        *reinterpret_cast<uint4 *>(p.arena + d.slot + 8 * (long long)q) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    }
    if (blockIdx.y == 0) STREAM_TILE_RECORDS();
}

// ---- wire input (ctu_streams_push_wire: G.711 codes, swapped and channel-interleaved PCM as the caller holds them)
// One element of the caller's buffer as a sample: low 16 bits of the result.  G.711 is g711_expand, the one device statement of it.
template <int FMT>
__device__ __forceinline__ int wire_value(const uint8_t *base, const long long e) {
    if constexpr (FMT == CTU_WIRE_ALAW || FMT == CTU_WIRE_MULAW) return g711_expand(base[e], FMT == CTU_WIRE_ALAW);
    const unsigned v = *reinterpret_cast<const unsigned short *>(base + 2 * e);
    return FMT == CTU_WIRE_S16_SWAPPED ? (int)(((v >> 8) | (v << 8)) & 0xffff) : (int)v;
}
// Two 16-bit elements as loaded -> two samples: the swap is one byte permute per packed pair
template <int FMT>
__device__ __forceinline__ unsigned wire_pair(const unsigned w) {
    return FMT == CTU_WIRE_S16_SWAPPED ? __builtin_amdgcn_perm(w, w, 0x02030001u) : w;
}
// Four codes as loaded -> four samples in two packed pairs
template <int FMT>
__device__ __forceinline__ uint2 wire_codes(const unsigned c) {
    constexpr bool alaw = FMT == CTU_WIRE_ALAW;
    return make_uint2(g711_expand(c & 255, alaw) | (g711_expand((c >> 8) & 255, alaw) << 16),
                      g711_expand((c >> 16) & 255, alaw) | (g711_expand(c >> 24, alaw) << 16));
}

// stream_stitch_kernel with the new samples read through a ctu_wire_layout: p.src is the caller's buffer whatever its element type,
// StreamPush::src an element offset into it, sample k of the push element src + k * stride.  Same slots, same stores, same records.
// A lane whose eight samples are all new ones of a contiguous source reads the 16 (S16) or 8 (G.711) bytes they lie in, which start at
// any element: as wide as their address allows - one b128, four dwords, or a short | three dwords | a short for 16-bit elements at
// 2 (mod 4); one b64, two dwords, or the aligned dword inside and the four bytes around it for codes - and never a byte outside them.
// Every other lane (the carry's edge, the push's last samples) and every lane of a strided source goes element by element.
// grid (pushed streams, slices), 256 lanes
template <int FMT, bool STRIDED>
__global__ __launch_bounds__(256) void stream_stitch_wire_kernel(const StreamParams p, const long long stride) {
    constexpr bool G711 = FMT == CTU_WIRE_ALAW || FMT == CTU_WIRE_MULAW;
    const StreamPush d = p.push[blockIdx.x];
    const long long total = p.state[d.id].consumed;
    const long long F = stream_frames(total, p.window, p.wshift);
    const int c = (int)(total - F * p.wshift);  // carried samples of the next frame, < window
    const int T = (int)(stream_frames(total + d.n, p.window, p.wshift) - F);
    const int len = STREAM_LEAD + c + d.n;
    const int16_t *cr = p.carry + (size_t)d.id * p.cstride;
    const uint8_t *base = reinterpret_cast<const uint8_t *>(p.src);
    const int q = blockIdx.y * 256 + threadIdx.x;  // which 8 samples of the slot
    if (8 * q < len) {
        const int j0 = 8 * q - STREAM_LEAD - c;  // the new sample the lane's first one is
        uint4 o;
        if (!STRIDED && j0 >= 0 && j0 + 8 <= d.n) {
            if constexpr (G711) {
                const uint8_t *a = base + d.src + j0;
                const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(a) & 7);
                uint2 w;
                if (m == 0) w = *reinterpret_cast<const uint2 *>(a);
                else if (m == 4) w = make_uint2(*reinterpret_cast<const unsigned *>(a), *reinterpret_cast<const unsigned *>(a + 4));
                else {
                    const int h = 4 - (int)(m & 3);  // 1 .. 3 bytes ahead of the aligned dword, 4 - h behind it
                    unsigned long long v = (unsigned long long)*reinterpret_cast<const unsigned *>(a + h) << (8 * h);
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        if (k < h) v |= (unsigned long long)a[k] << (8 * k);
#pragma unroll
                    for (int k = 5; k < 8; k++)
                        if (k >= h + 4) v |= (unsigned long long)a[k] << (8 * k);
                    w = make_uint2((unsigned)v, (unsigned)(v >> 32));
                }
                const uint2 lo = wire_codes<FMT>(w.x), hi = wire_codes<FMT>(w.y);
                o = make_uint4(lo.x, lo.y, hi.x, hi.y);
            } else {
                const uint8_t *a = base + 2 * (d.src + j0);
                const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(a) & 15);
                uint4 w;
                if (m == 0) w = *reinterpret_cast<const uint4 *>(a);
                else if ((m & 3) == 0) {
                    const unsigned *u = reinterpret_cast<const unsigned *>(a);
                    w = make_uint4(u[0], u[1], u[2], u[3]);
                } else {
                    const unsigned *u = reinterpret_cast<const unsigned *>(a + 2);
                    const unsigned h = *reinterpret_cast<const unsigned short *>(a), t = *reinterpret_cast<const unsigned short *>(a + 14);
                    const unsigned m0 = u[0], m1 = u[1], m2 = u[2];
                    w = make_uint4(h | (m0 << 16), (m0 >> 16) | (m1 << 16), (m1 >> 16) | (m2 << 16), (m2 >> 16) | (t << 16));
                }
                o = make_uint4(wire_pair<FMT>(w.x), wire_pair<FMT>(w.y), wire_pair<FMT>(w.z), wire_pair<FMT>(w.w));
            }
        } else {
            int16_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int r = 8 * q + k - STREAM_LEAD;  // position from the next frame's first sample
                int16_t x = 0;
                if (r >= -1 && r < c) x = cr[r + 1];
                else if (r >= c && r < c + d.n) x = (int16_t)wire_value<FMT>(base, d.src + (r - c) * (STRIDED ? stride : 1));
                v[k] = x;
            }
            o = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        }
        *reinterpret_cast<uint4 *>(p.arena + d.slot + 8 * (long long)q) = o;
    }
    if (blockIdx.y == 0) STREAM_TILE_RECORDS();
}

// grid (pushed streams), 256 lanes: the slot's samples from T wshift - 1 frames on are the next carry
__global__ __launch_bounds__(256) void stream_carry_kernel(const StreamParams p) {
    const StreamPush d = p.push[blockIdx.x];
    const long long total = p.state[d.id].consumed;
    const long long F = stream_frames(total, p.window, p.wshift), F1 = stream_frames(total + d.n, p.window, p.wshift);
    const int c1 = (int)(total + d.n - F1 * p.wshift);
    const int16_t *from = p.arena + d.slot + (STREAM_LEAD - 1) + (F1 - F) * p.wshift;  // from[0]: the sample ahead of the next frame
    int16_t *cr = p.carry + (size_t)d.id * p.cstride;
    for (int q = threadIdx.x; 8 * q < p.cstride; q += 256) {
        int16_t v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = 8 * q + k <= c1 ? from[8 * q + k] : (int16_t)0;
        *reinterpret_cast<uint4 *>(cr + 8 * q) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    }
    __syncthreads();  // every lane has read the old count
    if (threadIdx.x == 0) p.state[d.id].consumed = total + d.n;
}

}  // namespace
