// Streaming input with signal state (include/ctu_engine.h: CTU_STREAMS_SIGNAL_STATE, ctu_streams_push_signal): the overlap-add of a push.
// Included by engine.hip behind signal_kernels.h (ola_round, the rounding rule it shares with ola_kernel).
//
// Offline, sample n of a file is 0.0 + y_t0[n - t0 s] + y_t0+1[..] + .., the frames that cover it in ascending order, in double
// (ola_kernel); it is final once frame floor(n / s) is in.  A stream that has F frames has therefore delivered F s samples, and of the
// w - s samples behind them it keeps the partial sums: its tail, w - s doubles in HBM, zero at create and after a finish.
//
//   stream_ola_kernel        a stream goes from F0 to F0 + T frames: its time-domain frames are rows row0 .. row0 + T - 1 of the plan's
//                            ybuf (the front end's SY instantiations, or synth_kernel, wrote them).  Output sample j < T s is the tail's
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
// gfx950, hipcc -O3: stream_ola_kernel 24 VGPRs, 54 SGPRs; stream_ola_flush_kernel 20 VGPRs, 22 SGPRs; no spills, no scratch, no LDS.
#pragma once

#include "stream_plan.h"  // SignalPush: the host plans a push by it

namespace {

constexpr int OLA_SLICE = 2048;  // samples per workgroup of stream_ola_kernel: 256 lanes x 8
constexpr int OLA_TAIL_MAX = 512;  // the longest tail a workgroup's lanes hold two entries each of

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

// one workgroup of 256 lanes: the stream d.id finishes its file
__global__ __launch_bounds__(256) void stream_ola_flush_kernel(const SignalParams p, const SignalPush d) {
    double *tl = p.tail + (size_t)d.id * p.tstride;
    for (int j = threadIdx.x; j < p.window - p.wshift; j += 256) {
        p.out[d.out0 + j] = ola_round(tl[j], p.corr);
        tl[j] = 0.0;
    }
}

}  // namespace
