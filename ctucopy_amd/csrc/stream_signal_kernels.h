// Streaming input with signal state (include/ctu_engine.h: CTU_STREAMS_SIGNAL_STATE, ctu_streams_push_signal): the overlap-add of a push.
// Included by engine.hip behind signal_kernels.h (ola_round, the rounding rule it shares with ola_kernel).
//
// Offline, sample n of a file is 0.0 + y_t0[n - t0 s] + y_t0+1[..] + .., the frames that cover it in ascending order, in double
// (ola_kernel); it is final once frame floor(n / s) is in.  A stream that has F frames has therefore delivered F s samples, and of the
// w - s samples behind them it keeps the partial sums: its tail, w - s doubles in HBM, zero at create and after a finish.
//
//   stream_ola_kernel        a stream goes from F0 to F0 + T frames: its time-domain frames are rows row0 .. row0 + T - 1 of the plan's
//                            ybuf (the front end's SY instantiations, or bigsynth_kernel, wrote them).  Output sample j < T s is the tail's
//                            entry j (0.0 past the tail) plus the push's frames over it in ascending order, then ola_round.  The new
//                            tail's entry j < w - s is the old entry j + T s (0.0 past it) plus the push's frames over sample T s + j.
//                            Continuing a partial sum in frame order is the offline run's sequence of additions, so given the same
//                            frames the samples are the offline run's bit for bit.
//   stream_ola_flush_kernel  the end of a file: the tail's entries rounded - what close() writes in the reference - and the tail cleared.
//
// The tail is read and written by one launch, and a new entry reads an old one further on (whenever T s < w - s: one frame at 25 / 10
// ms), which another lane may already have replaced.  One workgroup owns a stream's tail - slice 0 of the stream; w - s < 512 on the
// 256- and 512-point front end, so two entries per lane hold all of it - and reads every old entry it needs, for the samples and for
// the new tail, ahead of a barrier; the stores come behind it.  The other slices of a long push (2048 samples each) lie past the tail
// and touch only ybuf and their own samples.  A stream that completes no frame returns at once: tail and output stay as they are.
// Plain C++ stores throughout (global_store_short / _dwordx2); no atomics: a stream id appears once in a push.
//
//
//   stream_ola_big_kernel    the same overlap-add for tails of 513 .. 4096 entries (CTU_STREAMS_LARGE_STATE: windows of up to 4096 samples
//                            behind the large transforms).  There the tail can be longer than a slice, so a workgroup of slice >= 1 of
//                            the kernel above would read old entries that slice 0's workgroup replaces in the same launch: a race
//                            between workgroups, which no barrier closes.  Of the two forms that cannot race - the tail's owner
//                            produces everything below w - s, or two tails flipped per push - this is the first: it needs no second
//                            tail per stream (32 KiB at 4096 points), no flip bit mirrored on the host that a refused push would have
//                            to leave alone, and nothing new in the plan of a push or a finish; its price, one workgroup's walk over
//                            up to 4095 positions, is small beside the transforms of the same frames.
//                            Position x of a push, counted from the first sample it delivers, is the old entry x (0.0 past the tail)
//                            plus the push's frames over x in ascending order; it is output sample x while x < T s and the new tail's
//                            entry x - T s from there to T s + w - s.  So every old entry is read exactly once, by position x < w - s.
//                            Workgroup 0 of a stream, the owner, reads all of them into registers - sixteen per lane - ahead of a
//                            barrier, and behind it writes every position below w - s, output or tail, and every other entry of the
//                            new tail.  The workgroups y >= 1 take the output positions w - s + 2048 (y - 1) on: they touch ybuf and
//                            their own samples, never the tail.  No tail entry is read outside the owner, none is written outside
//                            it, and inside it the barrier stands between the last read and the first store: nothing can race.
//                            Sums are ola_cover's, rounding ola_round's: the samples of the small kernel, and of ola_kernel, bit for bit.
//
// gfx950, hipcc -O3: stream_ola_kernel 24 VGPRs, 54 SGPRs; stream_ola_flush_kernel 20 VGPRs, 22 SGPRs; stream_ola_big_kernel 74 VGPRs, 75 SGPRs;
// no spills, no scratch, no LDS.
#pragma once

#include "stream_plan.h"  // SignalPush: the host plans a push by it

namespace {

constexpr int OLA_SLICE = 2048;  // samples per workgroup of stream_ola_kernel: 256 lanes x 8
constexpr int OLA_TAIL_MAX = 512;  // the longest tail a workgroup's lanes hold two entries each of (stream_ola_kernel)
constexpr int OLA_BIG_Q = 16;      // stream_ola_big_kernel: old entries per lane of the owner
constexpr int OLA_BIG_TAIL_MAX = 256 * OLA_BIG_Q;  // ... and so the longest tail it holds: window - wshift <= 4095 at 4096 points

struct SignalParams {
    const SignalPush *push;
    const float *ybuf;   // [frames of the push][window]
    double *tail;        // [n_streams][tstride]
    int16_t *out;
    int tstride, window, wshift;
    double corr;
};

// acc plus the frames of the push over position x, counted from the first sample the push delivers, in ascending frame order
__device__ __forceinline__ double ola_cover(double acc, const float *__restrict__ y, long long x, int T, int w, int s) {
    const long long m0 = x - w + 1 <= 0 ? 0 : (x - w + s) / s;  // ceil((x - w + 1) / s)
    long long m1 = x / s;
    if (m1 > T - 1) m1 = T - 1;
    for (long long m = m0; m <= m1; m++) acc += (double)y[m * w + (x - m * s)];
    return acc;
}

// grid (pushed streams, slices of OLA_SLICE samples), 256 lanes
__global__ __launch_bounds__(256) void stream_ola_kernel(const SignalParams p) {
    const SignalPush d = p.push[blockIdx.x];
    const int w = p.window, s = p.wshift, L = w - s;
    const long long n = (long long)d.T * s;
    if ((long long)blockIdx.y * OLA_SLICE >= n) return;  // (T = 0 among them: the whole workgroup leaves ahead of the barrier)
    const float *y = p.ybuf + d.row0 * w;
    double lead[2] = {0.0, 0.0};
    if (blockIdx.y == 0) {
        double *tl = p.tail + (size_t)d.id * p.tstride;
        double keep[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int j = threadIdx.x + 256 * q;
            lead[q] = j < L ? tl[j] : 0.0;
            keep[q] = (j < L && j + n < L) ? tl[j + n] : 0.0;
        }
        __syncthreads();  // every old entry is in a register
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int j = threadIdx.x + 256 * q;
            if (j < L) tl[j] = ola_cover(keep[q], y, n + j, d.T, w, s);
        }
    }
    int16_t *o = p.out + d.out0;
#pragma unroll
    for (int i = 0; i < OLA_SLICE / 256; i++) {
        const long long x = (long long)blockIdx.y * OLA_SLICE + threadIdx.x + 256 * i;
        if (x < n) o[x] = ola_round(ola_cover(i < 2 ? lead[i] : 0.0, y, x, d.T, w, s), p.corr);
    }
}

// grid (pushed streams, 1 + slices of OLA_SLICE output samples past the tail), 256 lanes
__global__ __launch_bounds__(256) void stream_ola_big_kernel(const SignalParams p) {
    const SignalPush d = p.push[blockIdx.x];
    const int w = p.window, s = p.wshift, L = w - s;
    const long long n = (long long)d.T * s;
    if (n == 0) return;  // (no frame: tail and output stay as they are; the whole workgroup leaves ahead of the barrier)
    const float *y = p.ybuf + d.row0 * w;
    int16_t *o = p.out + d.out0;
    if (blockIdx.y > 0) {  // output past the tail: nothing old under it
        const long long x0 = L + (long long)(blockIdx.y - 1) * OLA_SLICE;
#pragma unroll
        for (int i = 0; i < OLA_SLICE / 256; i++) {
            const long long x = x0 + threadIdx.x + 256 * i;
            if (x < n) o[x] = ola_round(ola_cover(0.0, y, x, d.T, w, s), p.corr);
        }
        return;
    }
    double *tl = p.tail + (size_t)d.id * p.tstride;
    double old[OLA_BIG_Q];
#pragma unroll
    for (int q = 0; q < OLA_BIG_Q; q++) {
        const int x = threadIdx.x + 256 * q;
        old[q] = x < L ? tl[x] : 0.0;
    }
    __syncthreads();  // every old entry is in a register
#pragma unroll
    for (int q = 0; q < OLA_BIG_Q; q++) {
        const int x = threadIdx.x + 256 * q;
        if (x < L) {
            const double v = ola_cover(old[q], y, x, d.T, w, s);
            if (x < n) o[x] = ola_round(v, p.corr);
            else tl[x - n] = v;
        }
    }
    for (long long x = (n > L ? n : L) + threadIdx.x; x < n + L; x += 256) tl[x - n] = ola_cover(0.0, y, x, d.T, w, s);  // the new tail past the old one
}

// one workgroup of 256 lanes: the stream d.id finishes its file
__global__ __launch_bounds__(256) void stream_ola_flush_kernel(const SignalParams p, const SignalPush d) {
    double *tl = p.tail + (size_t)d.id * p.tstride;
    for (int j = threadIdx.x; j < p.window - p.wshift; j += 256) {
        p.out[d.out0 + j] = ola_round(tl[j], p.corr);
        tl[j] = 0.0;
    }
}

}  // namespace
