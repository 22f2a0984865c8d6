// Streaming input (include/ctu_engine.h: ctu_streams_*): the two kernels around the front end of a push.
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
#pragma once

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
    const int16_t *src;     // the caller's new samples
    TileRec *tiles;
    int cstride, window, wshift;
    int n_tiles, grid;      // tiles of the whole push and the workgroups of the front-end launch: tile i is followed by tile i + grid
    int *tile_stream;       // noise state (null without): the stream of every tile, and chains of whole streams - a stream's tiles follow
                            // each other, StreamPush::pad follows its last one
};

__device__ __forceinline__ unsigned pack2(const int16_t a, const int16_t b) { return (unsigned)(unsigned short)a | ((unsigned)(unsigned short)b << 16); }

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
    if (blockIdx.y == 0) {
        const int t0 = (int)(F < 0x3fffffff ? F : 0x3fffffff);  // frames ahead of the push; only "none" matters (file start)
        for (int t = threadIdx.x; 64 * t < T; t += 256) {
            const int idx = d.tile0 + t;
            const long long sbase = d.slot + STREAM_LEAD + (long long)t * TILE * p.wshift, rbase = d.row0 + (long long)t * TILE;
            int4 *w = reinterpret_cast<int4 *>(p.tiles + idx);
            w[0] = make_int4((int)(sbase & 0xffffffff), (int)(sbase >> 32), (int)(rbase & 0xffffffff), (int)(rbase >> 32));
            int next = idx + p.grid < p.n_tiles ? idx + p.grid : -1;
            if (p.tile_stream) {
                next = TILE * (t + 1) < T ? idx + 1 : d.pad;
                p.tile_stream[idx] = d.id;
            }
            w[1] = make_int4(min(TILE, T - TILE * t), t0 + TILE * t, next, t0 + T);
        }
    }
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
