// The VAD's Burg-cepstral criterion (src/vad/vad.cc:149-294, src/vdet/Burg.h) on 1024 .. 4096-point frames: windows of 513 to 4096
// samples.  vad_burg_kernel (vad_kernels.h) holds a frame in one wave, at most 8 samples per lane; here a workgroup of 256 threads
// takes a frame, persistent over the frame list:
//   * the halfcomplex vector Xa cos(phi), Xa sin(phi) from the spectra and post-NR magnitudes bigfft_kernel exported (burg_hc_bin);
//   * the unnormalised HC2R of wfft points through LDS in float (big_hc2r_lds, bigsynth_kernel's inverse);
//   * the Burg lattice over the first `window` samples in double.  Thread t keeps samples NIT t .. NIT t + NIT - 1 in registers,
//     so the lattice's eb[i - 1] is the neighbouring register, for a thread's first sample the previous lane's last one (one DPP
//     shift) and for a wave's first sample the previous wave's last one.  An order costs one barrier: every wave leaves its two
//     partial sums (DPP reduction) and its last sample's (ef, eb[i - 1]) in LDS; behind the barrier every thread adds the four
//     partial sums in the same order, so the reflection coefficient is the same everywhere, and lane 0 of waves 1 .. 3 applies the
//     order's update to the neighbouring wave's last sample itself (the same fma the owner executes).  The exchange area is
//     double-buffered by the order's parity: a wave can be one barrier ahead of the slowest, never two;
//   * the prediction coefficients one per lane, redundantly in each wave; a -> c (burg_a2c); wave 0 stores vad_ci.
// The sums run over 1103 or 3072 samples and the decisions downstream are states, so the lattice is double throughout: the kernel
// is bound by its chain of (at most 31) reduction-and-barrier steps, not by arithmetic.
// Resources (gfx950, -O3, the code object's metadata): VGPRs <4,16> 97, <8,16> 109, <16,16> 157, <4,32> 162, <8,32> 170, <16,32> 187;
// the *ss modes' detector bigssdet_kernel (below) <8,16> 117, <8,32> 178, <16,16> 175, <16,32> 195
// (one wave per SIMD and workgroup: up to 512 are free), 106 SGPRs, no scratch; LDS 3 wfft / 2 float2 + 32 + 384 bytes: 12.4 KiB at
// 1024 points, 24.4 KiB at 2048, 48.4 KiB at 4096 - under 64 KiB, three workgroups a CU at the largest size.
// Included by engine.hip after vad_kernels.h and bigfft_kernel.h.
#pragma once

namespace {

constexpr int BIGBURG_XCH = 3 * 4 * 4;  // doubles: [order parity | energy][wave][num, den, ef, eb[i - 1]]
// Host side, bigburg_frames' carve-up (bigburg_kernel and bigssdet_kernel): bigsynth_kernel's two buffers and twiddles, and the lattice's exchange area
LdsFit bigburg_lds(int wfft) { return lds_fit(((size_t)(wfft / 2) * 3 + 4) * sizeof(float2) + BIGBURG_XCH * sizeof(double), 8); }

// SSDET: the detector of hwss / fwss / 2fwss (src/nr/nr.cc:278-295, src/vdet/CepstralDet.h:133-146) instead of the VAD's criterion: the
// magnitudes are X^a of the exported vector (X itself in 2fwss) and the first `window` samples take the detector's Hann window
// (han[window], doubles) ahead of the lattice.  The cepstra's recurrences are ss_decide_kernel's (bigss_kernel.h).
template <int NIT, int NCMAX, bool SSDET>  // NIT = wfft / 256 samples per thread; cepstral coefficients: ncoef <= NCMAX
__device__ __forceinline__ void bigburg_frames(const float2 *__restrict__ xri, const float *__restrict__ pnr, double *__restrict__ ci_out, const int wfft,
                                               const int W, const int nc, const int64_t total_frames, const float2 *__restrict__ tw,
                                               const double *__restrict__ han, const float ss_a, const int ss_two) {
    extern __shared__ __align__(16) float smem[];
    const int Nc = wfft >> 1, K = Nc + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float2 *A = reinterpret_cast<float2 *>(smem);       // [Nc + 1]
    float2 *Bf = A + Nc + 4;                            // [Nc]
    float2 *ltw = Bf + Nc;                              // [Nc] (cos, -sin)(2 pi m / wfft)
    double *xch = reinterpret_cast<double *>(ltw + Nc);  // [BIGBURG_XCH]
    for (int i = tid; i < Nc; i += 256) ltw[i] = tw[i];
    lds_barrier();
    for (int64_t fr = blockIdx.x; fr < total_frames; fr += gridDim.x) {
        for (int k = tid; k <= Nc; k += 256) {
            float2 h;
            float xa = pnr[fr * K + k];
            if constexpr (SSDET) xa = ss_two ? xa : ss_pow(xa, ss_a);
            burg_hc_bin<float>(xri[fr * K + k], xa, k, K, h.x, h.y);
            A[k] = h;
        }
        const float2 *z = big_hc2r_lds(A, Bf, ltw, Nc, tid);
        double ef[NIT], eb[NIT];
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < NIT; q++) {
            const int j = tid * NIT + q;  // < wfft
            const float2 v = z[j >> 1];
            ef[q] = j < W ? (double)((j & 1) ? v.y : v.x) : 0.0;  // only the first `window` samples go to Burg (src/vad/vad.cc:233)
            if constexpr (SSDET) ef[q] = j < W ? han[j] * ef[q] : 0.0;
            eb[q] = ef[q];
            part = fma(ef[q], ef[q], part);
        }
        double edge = 0.0;  // lane 0 of waves 1 .. 3: eb of the sample ahead of the wave's first one (index 64 NIT wave - 1 >= 1)
        if (wave > 0 && tid * NIT - 1 < W) {
            const float2 v = z[(tid * NIT - 1) >> 1];
            edge = (double)v.y;  // an odd index
            if constexpr (SSDET) edge *= han[tid * NIT - 1];
        }
        // (the transform's buffers are rewritten by the next frame: the barriers below come first)
        part = wave_sum_fast(part);
        if (lane == 63) xch[32 + wave * 4] = part;
        lds_barrier();
        double alpha = ((xch[32] + xch[36]) + (xch[40] + xch[44])) / (double)W;
        double acoef = lane == 0 ? 1.0 : 0.0;  // a[lane]
        for (int ik = 1; ik < nc; ik++) {
            double ebm[NIT];  // eb[i - 1]
            {
                const double up = dpp_mov<0x138>(eb[NIT - 1]);  // wave_shr:1
                ebm[0] = lane == 0 ? edge : up;
            }
#pragma unroll
            for (int q = 1; q < NIT; q++) ebm[q] = eb[q - 1];
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int q = 0; q < NIT; q++) {
                const int i = tid * NIT + q;
                if (i >= ik && i < W) {
                    den += ef[q] * ef[q] + ebm[q] * ebm[q];
                    num += ef[q] * ebm[q];
                }
            }
            num = wave_sum_fast(num);
            den = wave_sum_fast(den);
            double *mine = xch + (ik & 1) * 16 + wave * 4;
            if (lane == 63) {
                mine[0] = num;
                mine[1] = den;
                mine[2] = ef[NIT - 1];
                mine[3] = ebm[NIT - 1];
            }
            lds_barrier();
            const double *all = xch + (ik & 1) * 16;
            num = (all[0] + all[4]) + (all[8] + all[12]);
            den = (all[1] + all[5]) + (all[9] + all[13]);
            const double rc = -(2.0 * num) / den;
            alpha *= 1.0 - rc * rc;
            if (wave > 0) {  // the previous wave's last sample, index 64 NIT wave - 1 >= 1, after this order
                const double *pw = all + (wave - 1) * 4;
                edge = (64 * NIT * wave - 1 < W) ? fma(rc, pw[2], pw[3]) : 0.0;
            }
#pragma unroll
            for (int q = 0; q < NIT; q++) {
                const int i = tid * NIT + q;
                if (i >= 1 && i < W) {  // both updates use the old values
                    const double nef = fma(rc, ebm[q], ef[q]), neb = fma(rc, ef[q], ebm[q]);
                    ef[q] = nef;
                    eb[q] = neb;
                }
            }
            const double other = __shfl(acoef, (ik - lane) & 63, 64);
            acoef = (lane >= 1 && lane < ik) ? acoef + rc * other : (lane == ik ? rc : acoef);
        }
        const double c_lane = burg_a2c<double, NCMAX>(acoef, alpha, lane);
        if (wave == 0 && lane < nc) ci_out[fr * nc + lane] = c_lane;
    }
}

template <int NIT, int NCMAX>
__global__ __launch_bounds__(256) void bigburg_kernel(const float2 *__restrict__ xri, const float *__restrict__ pnr, double *__restrict__ ci_out,
                                                      const VadParams vp, const int64_t total_frames, const float2 *__restrict__ tw) {
    bigburg_frames<NIT, NCMAX, false>(xri, pnr, ci_out, vp.wfft, vp.window, vp.ncoef, total_frames, tw, nullptr, 1.f, 0);
}

template <int NIT, int NCMAX>
__global__ __launch_bounds__(256) void bigssdet_kernel(const float2 *__restrict__ xri, const float *__restrict__ pnr, double *__restrict__ ci_out,
                                                       const int wfft, const int window, const int nc, const int64_t total_frames,
                                                       const float2 *__restrict__ tw, const double *__restrict__ han, const float ss_a, const int ss_two) {
    bigburg_frames<NIT, NCMAX, true>(xri, pnr, ci_out, wfft, window, nc, total_frames, tw, han, ss_a, ss_two);
}

}  // namespace
