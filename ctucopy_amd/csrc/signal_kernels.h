// Row N3: speech-enhancement output (inverse transform, overlap-add).
// Included by engine.hip (one translation unit: the kernels and their host launchers share types).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Row N3: sigOUT (src/io/out.cc:346-451) - enhanced speech from the post-NR magnitudes and the ORIGINAL phases.
//   (the inverse transform runs inside the front end - frontend_kernel's SY instantiations - or, at 1024 to 4096 points, in
//   bigsynth_kernel: X[k] = |Y[k]|/N * X0[k]/|X0[k]|, DC and Nyquist as positive reals, as the reference stores them before
//   its sign fix-up, out.cc:416-419; the first `window` samples of a frame go to a per-frame scratch row)
//   ola_kernel     one thread per output sample: sum of the frames that cover it, in frame order as the ring of the
//                  reference accumulates them, floor(x / correction), +-32767 clip (out.cc:436-451); an utterance of
//                  T frames yields T*wshift + (window - wshift) samples (the tail is what close() writes).
struct SynthParams {
    int K, wfft, window, wshift;
    float inv_n;
    double corr;
};

// The rounding rule of sigOUT (out.cc:436-451), stated once for ola_kernel and the stream kernels (stream_signal_kernels.h): the sum of
// the frames over a sample, divided by the window's overlap-add gain, floor, +-32767 clip.
__device__ __forceinline__ int16_t ola_round(double acc, double corr) {
    const int value = (int)floor(acc / corr);
    return fabsf((float)value) > 32767.f ? (int16_t)(value < 0 ? -32767 : 32767) : (int16_t)value;
}

__global__ __launch_bounds__(256) void ola_kernel(const float *__restrict__ ybuf, int16_t *__restrict__ out,
                                                  const int4 *__restrict__ utt_info, const long long *__restrict__ sample_off,
                                                  int n_utt, const SynthParams sp) {
    const int u = blockIdx.y;
    if (u >= n_utt) return;
    const int4 ui = utt_info[u];
    const long long ro = (long long)(unsigned)ui.x | ((long long)ui.y << 32);
    const int T = ui.z, w = sp.window, s = sp.wshift;
    const long long nout = (long long)T * s + (w - s);
    int16_t *o = out + sample_off[u];
    // four samples per thread and step: their loads are independent, which is what keeps enough bytes in flight
    const int stride = gridDim.x * 256;
    for (long long n0 = (long long)blockIdx.x * 256 + threadIdx.x; n0 < nout; n0 += 4LL * stride) {
        double acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int n = (int)(n0 + (long long)q * stride);  // an utterance stays far below 2^31 samples
            acc[q] = 0.0;
            if (n < nout) {
                int t0 = n - w + 1 <= 0 ? 0 : (n - w + s) / s;  // ceil((n - w + 1) / s)
                int t1 = n / s;
                if (t1 > T - 1) t1 = T - 1;
                for (int t = t0; t <= t1; t++) acc[q] += (double)ybuf[(ro + t) * w + (n - t * s)];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const long long n = n0 + (long long)q * stride;
            if (n < nout) o[n] = ola_round(acc[q], sp.corr);
        }
    }
}

}  // namespace
