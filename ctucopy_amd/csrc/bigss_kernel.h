// hwss / fwss / 2fwss (src/nr/nr.cc:181-442) on 2048- and 4096-point frames: 44.1 / 48 kHz audio at the presets' 25 ms, or long windows.
// The 256 / 512-point form sits inside frontend_kernel (SS), a wave per chain with the detector in the wave; here the work is cut
// into passes over the plan's scratch, because a frame no longer fits a wave:
//   1. bigfft_kernel<8|16> with the export on and the projection off writes every frame's complex spectrum (xri) and the vector
//      the NR sees (pnr: power or magnitude by -fb_power) once per run;
//   2. bigssdet_kernel (bigburg_kernel.h), a workgroup per frame: X^a with the original phase back to the time domain, the
//      detector's Hann window, the Burg lattice in double, -fea_ncepcoefs cepstra per frame.  Frames are independent;
//   3. ss_decide_kernel, a wave per utterance with a coefficient per lane: the detector's recurrences (src/vdet/CepstralDet.h:140-194,
//      cepdet_frame of vad_fused.h) over the file's cepstra, one decision byte per frame.  The detector never sees a subtracted
//      spectrum (nr.cc:278-295), so 1 - 3 do not depend on the noise seed and run once, whatever the number of passes
//      (with -vad file=<f> 2 and 3 are skipped: the bytes come from the stream);
//   4. bigss_kernel<NIT>, once per pass of the seed iteration (engine.hip): a workgroup walks one of the plan's chains of whole
//      utterances (chain_first / TileRec::next, as bigfft_kernel<NIT, true> does), skips utterances whose seed did not change, and
//      keeps Navg (and Nravg in 2fwss) of its bins k = tid + 256 r in registers, seeded from ss_seed[utt][K].  Per frame: the
//      exported row, power law, gated update, subtraction, rectification, root; the row goes to LDS and through big_project
//      (bigfft_kernel.h: the code the plain chain runs), or on the speech path to pss for bigsynth_kernel.  Behind an
//      utterance's last frame its vector goes to ss_last[utt][K].
// Navg, Nravg and both differences are double: the kernel is bound by its chain and by 4 bytes per bin of reads, not by
// arithmetic, and the two subtractions of nearly equal quantities are where float operands cost digits.
// LDS: P[K] + 64 band values + 64 logarithms + the bank's runs and the tail's coefficient rows (the tables bigfft_kernel stages, without
// its transform buffers, twiddles and window: 4 K + fb_total * 4 + a few KiB; the engine raises the limit past 64 KiB as for bigfft_kernel).
// Resources (gfx950, -O3, the code object's metadata): bigss_kernel<8> 147 VGPRs, <16> 218, 106 SGPRs, no spills; 784 bytes of scratch
// are big_project's LP arrays of one lane, as in bigfft_kernel.  Every store is a vector store.
// Included by engine.hip after bigfft_kernel.h and bigburg_kernel.h.
#pragma once

namespace {

// Host side, the carve-up below: the spectrum vector, the bands and their logarithms, and the projection's tables (none on the speech
// path).  The grid is the plan's chains, whose number ctu_plan_create caps at eight a CU.
LdsFit bigss_lds(const ctu::Design &d, int feat, int ncoef_out, int fb_total) {
    return lds_fit((size_t)((d.K + 3) & ~3) * 4 + 64 * 4 + 4 * 8 + 64 * 4 + (d.signal_out ? 0 : big_proj_lds(d, feat, ncoef_out, fb_total)), 8);
}

template <int NIT>  // NIT = wfft / 256: 8 or 16; K = 128 NIT + 1 bins, NIT / 2 + 1 of them per thread
__global__ __launch_bounds__(256) void bigss_kernel(const BigParams p) {
    extern __shared__ __align__(16) float smem[];
    const int K = p.K, tid = threadIdx.x;
    float *P = smem;                                   // [K] (+3 padding)
    float *Y = P + ((K + 3) & ~3);                     // [64] band values
    double *red = reinterpret_cast<double *>(Y + 64);  // [4]
    float *lfb = reinterpret_cast<float *>(red + 4);
    double *lcoef_d = reinterpret_cast<double *>(lfb + ((p.fb_total + 3) & ~3));
    const int ncd = (p.feat == FEAT_LP) ? (p.lporder + 1) * p.B : 0, ncf = (p.feat == FEAT_DCTC) ? p.ncoef_out * p.B : 0;
    float *lcoef = reinterpret_cast<float *>(lcoef_d + ncd);
    int *lrange = reinterpret_cast<int *>(lcoef + ((ncf + 3) & ~3));
    float *Ylog = reinterpret_cast<float *>(lrange + ((3 * p.B + 3) & ~3));
    const bool project = !p.xri_only;  // speech output: the subtracted magnitudes go to pss, nothing is projected (no tables in LDS)
    if (project) {
        for (int i = tid; i < p.fb_total; i += 256) lfb[i] = p.fbw[i];
        for (int i = tid; i < ncd; i += 256) lcoef_d[i] = p.coef_d[i];
        for (int i = tid; i < ncf; i += 256) lcoef[i] = p.coef[i];
        for (int i = tid; i < 3 * p.B; i += 256) lrange[i] = p.fb_range[i];
    }
    lds_barrier();
    BigParams q = p;
    if (q.e_mode == 4) q.e_mode = 0;  // -fea_rawenergy: the export pass wrote the column
    constexpr int NB = NIT / 2 + 1;
    const bool two = p.ss_mode == 3;
    const double aexp = p.ss_a, bsub = p.ss_b, pp = p.ss_p, qq = 1.0 - p.ss_p;
    auto pw = [&](double x) { return aexp == 1.0 ? x : (aexp == 2.0 ? x * x : pow(x, aexp)); };
    auto root = [&](double x) { return aexp == 1.0 ? x : (aexp == 2.0 ? sqrt(x) : pow(x, 1.0 / aexp)); };
    double navg[NB], nrav[NB];
#pragma unroll
    for (int r = 0; r < NB; r++) navg[r] = nrav[r] = 0.0;
    int tile = (int)blockIdx.x < p.n_chains ? p.chain_first[blockIdx.x] : -1;
    while (tile >= 0) {
        const TileRec rec = load_rec(p.tiles, tile);
        const int utt = p.tile_utt[tile];
        tile = rec.next;
        if (!p.ss_dirty[utt]) continue;  // its seed is the one of the pass before: rows and last vector stand
        if (rec.t0 == 0) {  // new_file (nr.cc:212-221, 402-409): the estimate starts from the previous file's last vector
#pragma unroll
            for (int r = 0; r < NB; r++) {
                const int k = tid + 256 * r;
                const double sd = k < K ? (double)p.ss_seed[(int64_t)utt * K + k] : 0.0;
                navg[r] = two ? sd : pw(sd);
                nrav[r] = 0.0;
            }
        }
        float cur[NB];  // a frame's values are fetched one frame ahead: the loads fly under the previous frame's projection
        auto fetch = [&](int f) {
            const float *x = p.pnr + (rec.rbase + f) * K;
#pragma unroll
            for (int r = 0; r < NB; r++) {
                const int k = tid + 256 * r;
                cur[r] = k < K ? x[k] : 0.f;
            }
        };
        fetch(0);
        for (int f = 0; f < rec.nvalid; f++) {
            const int t = rec.t0 + f;
            const int64_t row = rec.rbase + f;
            // hwss counts its initial segments down before the test, the others after it (nr.cc:225 vs :367, :440)
            const bool upd = !p.ss_vbits[row] || t < (p.ss_mode == 1 ? p.ss_init - 1 : p.ss_init);
            double X[NB];
#pragma unroll
            for (int r = 0; r < NB; r++) X[r] = (double)cur[r];
            if (f + 1 < rec.nvalid) fetch(f + 1);
#pragma unroll
            for (int r = 0; r < NB; r++) {
                const int k = tid + 256 * r;
                double x = X[r];
                if (two) {  // dfwssNR::process_frame, nr.cc:418-442: -nr_a is ignored
                    if (upd) navg[r] = pp * navg[r] + qq * x;
                    x = fabs(x - navg[r]);
                    if (upd) nrav[r] = pp * nrav[r] + qq * x;
                    x = fabs(x - nrav[r]);
                } else {  // hwssNR / fwssNR::process_frame, nr.cc:223-261, 331-369
                    x = pw(x);
                    if (upd) navg[r] = pp * navg[r] + qq * x;
                    x -= bsub * navg[r];
                    if (x < 0.0) x = p.ss_mode == 1 ? 0.0 : -x;
                    x = root(x);
                }
                if (k < K) {
                    const float xf = (float)x;
                    P[k] = xf;
                    if (p.pss) p.pss[row * K + k] = xf;
                    if (t == rec.T - 1) {
                        // what the next file's estimate starts from.  On the speech path sigOUT has flipped the Nyquist entry's sign by
                        // then if that bin's phase was pi (src/io/out.cc:419)
                        const bool flip = p.pss && k == K - 1 && p.xri[row * K + k].x < 0.f;
                        p.ss_last[(int64_t)utt * K + k] = flip ? -xf : xf;
                    }
                }
            }
            if (project) {
                lds_barrier();
                big_project(q, P, Y, Ylog, red, lfb, lcoef, lcoef_d, lrange, row, 0.0, tid);
                lds_barrier();  // P and Y are rewritten by the next frame
            }
        }
    }
}

// The detector's recurrences over a file's cepstra (src/vdet/CepstralDet.h:140-194; the detector is rebuilt per file, nr.cc:263-271):
// a wave per utterance, coefficient `lane` of the background cepstrum in lane `lane`, everything else wave-uniform, in double.
__global__ __launch_bounds__(64) void ss_decide_kernel(const double *__restrict__ ci, const int64_t *__restrict__ row_off, const int n_utt, const int nc,
                                                       const int ninit, const double pcoef, const double qcoef, unsigned char *__restrict__ vbits) {
    const int u = blockIdx.x, lane = threadIdx.x;
    if (u >= n_utt) return;
    const int64_t r0 = row_off[u], T = row_off[u + 1] - r0;
    CepDetRun det;
    cepdet_reset(det);
    double nxt = (T > 0 && lane < nc) ? ci[r0 * nc + lane] : 0.0;
    for (int64_t t = 0; t < T; t++) {
        const double cil = nxt;
        if (t + 1 < T && lane < nc) nxt = ci[(r0 + t + 1) * nc + lane];
        const int v = cepdet_frame(det, cil, lane, nc, ninit, pcoef, qcoef);
        if (lane == 0) vbits[r0 + t] = (unsigned char)v;
    }
}

}  // namespace
