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
// On a stream set with subtraction state on large transforms (CTU_STREAMS_SS_STATE | CTU_STREAMS_SS_LARGE_STATE) 1 and 2 run as they are
// over the frames of a push, ss_decide_stream_kernel replaces 3 and bigss_kernel<NIT, true> runs 4 once, both along the push's chains
// from the streams' slots (below).  Resources of the twins, same build: bigss_kernel<8, true> 150 VGPRs, <16, true> 228, 106 SGPRs, the
// same 784 bytes of scratch, no VGPR spills, dynamic LDS as the offline kernel's (bigss_lds); ss_decide_stream_kernel 36 VGPRs, 52
// SGPRs, no scratch, no LDS (ss_decide_kernel: 34 / 38).  The offline instantiations are instruction for instruction what they were
// before the twins existed (147 / 218 VGPRs): the frame's step moved into bigss_frame_step, which both call.
// Included by engine.hip after bigfft_kernel.h and bigburg_kernel.h.
#pragma once

namespace {

// Host side, the carve-up below: the spectrum vector, the bands and their logarithms, and the projection's tables (none on the speech
// path).  The grid is the plan's chains, whose number ctu_plan_create caps at eight a CU.
LdsFit bigss_lds(const ctu::Design &d, int feat, int ncoef_out, int fb_total) {
    return lds_fit((size_t)((d.K + 3) & ~3) * 4 + 64 * 4 + 4 * 8 + 64 * 4 + (d.signal_out ? 0 : big_proj_lds(d, feat, ncoef_out, fb_total)), 8);
}

// What a frame's step needs of the options, read once per launch
struct BigSsCoef {
    double aexp, bsub, pp, qq;
    int mode;  // 1 / 2 / 3 = hwss / fwss / 2fwss
};
__device__ __forceinline__ double bigss_pw(double x, double aexp) { return aexp == 1.0 ? x : (aexp == 2.0 ? x * x : pow(x, aexp)); }
__device__ __forceinline__ double bigss_root(double x, double aexp) { return aexp == 1.0 ? x : (aexp == 2.0 ? sqrt(x) : pow(x, 1.0 / aexp)); }
// A frame's step on one bin: power law, gated update of the estimate(s), subtraction, rectification, root.  x: the exported value,
// navg / nrav: the bin's estimates (updated where `upd`); returns what the projection sees.  The one statement of the arithmetic: the
// offline kernel and its streamed twin (XS) run a frame by calling it for their NB bins, so a file's rows do not depend on which of
// the two ran them.
__device__ __forceinline__ double bigss_frame_step(const BigSsCoef &c, double x, double &navg, double &nrav, const bool upd) {
    if (c.mode == 3) {  // dfwssNR::process_frame, nr.cc:418-442: -nr_a is ignored
        if (upd) navg = c.pp * navg + c.qq * x;
        x = fabs(x - navg);
        if (upd) nrav = c.pp * nrav + c.qq * x;
        x = fabs(x - nrav);
    } else {  // hwssNR / fwssNR::process_frame, nr.cc:223-261, 331-369
        x = bigss_pw(x, c.aexp);
        if (upd) navg = c.pp * navg + c.qq * x;
        x -= c.bsub * navg;
        if (x < 0.0) x = c.mode == 1 ? 0.0 : -x;
        x = bigss_root(x, c.aexp);
    }
    return x;
}

// XS: a stream set with subtraction state on large transforms (CTU_STREAMS_SS_STATE | CTU_STREAMS_SS_LARGE_STATE), bigfft_kernel<NIT, true, XS>'s
// walk with this kernel's state: the chains are those of a push (p.chain_first = the heads the push was dealt onto, p.tile_utt = the stream
// of every tile), and a stream's estimates live in its slot of p.xstate - xs_ss_big_floats(NIT) floats (layout_constants.h): Navg[NB][256] |
// Nravg[NB][256] as doubles, bin tid + 256 r at [r][tid], 2 KiB contiguous per row and workgroup.  At a tile: a file's first (rec.t0 == 0)
// zeroes both - every file of a stream is the first file of a process, whose seed is the zero vector; else, where the tile is the chain's
// first or another stream's than the one before, the slot is loaded.  Behind a stream's last tile of the chain (the next is another
// stream's, or none) the slot is stored; between the tiles of a stream the estimates stay in registers.  Doubles travel as they stand, so
// a store and reload is exact, and a stream is named once in a push, so no two workgroups touch one slot in a launch.  ss_seed, ss_dirty,
// ss_last and pss are null on this path and not read: one pass, no read-back, and the store behind a file's last frame is compiled out (a
// push does not know the file's end).  A switch at compile time: the offline instantiations keep their code, registers, scratch and LDS.
template <int NIT, bool XS = false>  // NIT = wfft / 256: 8 or 16; K = 128 NIT + 1 bins, NIT / 2 + 1 of them per thread
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
    const BigSsCoef co = {p.ss_a, p.ss_b, p.ss_p, 1.0 - p.ss_p, p.ss_mode};
    double navg[NB], nrav[NB];
#pragma unroll
    for (int r = 0; r < NB; r++) navg[r] = nrav[r] = 0.0;
    int tile = (int)blockIdx.x < p.n_chains ? p.chain_first[blockIdx.x] : -1;
    int xs_prev = -1;  // XS: the stream of the tile before on this chain
    while (tile >= 0) {
        const TileRec rec = load_rec(p.tiles, tile);
        const int utt = p.tile_utt[tile];
        tile = rec.next;
        double *const xs = XS ? reinterpret_cast<double *>(p.xstate + (size_t)utt * xs_ss_big_floats(NIT)) : nullptr;
        if constexpr (XS) {
            if (rec.t0 == 0) {  // a file's first tile: zero seed
#pragma unroll
                for (int r = 0; r < NB; r++) navg[r] = nrav[r] = 0.0;
            } else if (utt != xs_prev) {  // the file goes on: where the stream's last push left off
#pragma unroll
                for (int r = 0; r < NB; r++) {
                    navg[r] = xs[256 * r + tid];
                    nrav[r] = xs[256 * (NB + r) + tid];
                }
            }
            xs_prev = utt;
        } else {
            if (!p.ss_dirty[utt]) continue;  // its seed is the one of the pass before: rows and last vector stand
            if (rec.t0 == 0) {  // new_file (nr.cc:212-221, 402-409): the estimate starts from the previous file's last vector
#pragma unroll
                for (int r = 0; r < NB; r++) {
                    const int k = tid + 256 * r;
                    const double sd = k < K ? (double)p.ss_seed[(int64_t)utt * K + k] : 0.0;
                    navg[r] = two ? sd : bigss_pw(sd, co.aexp);
                    nrav[r] = 0.0;
                }
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
                const double x = bigss_frame_step(co, X[r], navg[r], nrav[r], upd);
                if (k < K) {
                    const float xf = (float)x;
                    P[k] = xf;
                    if constexpr (!XS) {
                        if (p.pss) p.pss[row * K + k] = xf;
                        if (t == rec.T - 1) {
                            // what the next file's estimate starts from.  On the speech path sigOUT has flipped the Nyquist entry's sign by
                            // then if that bin's phase was pi (src/io/out.cc:419)
                            const bool flip = p.pss && k == K - 1 && p.xri[row * K + k].x < 0.f;
                            p.ss_last[(int64_t)utt * K + k] = flip ? -xf : xf;
                        }
                    }
                }
            }
            if (project) {
                lds_barrier();
                big_project(q, P, Y, Ylog, red, lfb, lcoef, lcoef_d, lrange, row, 0.0, tid);
                lds_barrier();  // P and Y are rewritten by the next frame
            }
        }
        if constexpr (XS) {
            const int xs_next = tile >= 0 ? p.tile_utt[tile] : -1;
            if (xs_next != utt) {  // behind the stream's last tile of this chain
#pragma unroll
                for (int r = 0; r < NB; r++) {
                    xs[256 * r + tid] = navg[r];
                    xs[256 * (NB + r) + tid] = nrav[r];
                }
            }
        }
    }
}

// ss_decide_kernel's twin for a stream set with subtraction state on large transforms: a wave per chain head of the push (ss_decide_kernel
// lays its rows out by the plan's d_row_off, which a push does not), a coefficient per lane, bigss_kernel<NIT, true>'s walk and its rule at
// tile edges on the detector's part of the stream's slot - behind the xs_ss_big_doubles(nit) doubles of the estimates c0 of every lane
// [64], dMean, dMean2, threshold as doubles and nseg as a 64-bit integer.  cepdet_frame (vad_fused.h) is the one statement of the step.
struct SsDecideStreamParams {
    const double *ci;        // [total_frames][nc] the detector's cepstra (bigssdet_kernel)
    const TileRec *tiles;
    const int *tile_stream;  // stream of every tile
    const int *heads;        // first tile of every chain (-1: none)
    int n_heads;
    float *xstate;           // [n_streams][slot_floats]
    int slot_floats, det_doubles;  // xs_ss_big_floats(nit), xs_ss_big_doubles(nit)
    int nc, ninit;
    double pcoef, qcoef;
    unsigned char *vbits;    // [total_frames]
};
__global__ __launch_bounds__(64) void ss_decide_stream_kernel(const SsDecideStreamParams p) {
    const int lane = threadIdx.x;
    int tile = (int)blockIdx.x < p.n_heads ? p.heads[blockIdx.x] : -1;
    CepDetRun det;
    cepdet_reset(det);
    int prev = -1;
    while (tile >= 0) {
        const TileRec rec = load_rec(p.tiles, tile);
        const int stream = p.tile_stream[tile];
        tile = rec.next;
        double *const xd = reinterpret_cast<double *>(p.xstate + (size_t)stream * p.slot_floats) + p.det_doubles;
        if (rec.t0 == 0) cepdet_reset(det);  // the detector is rebuilt per file (nr.cc:263-271)
        else if (stream != prev) {           // the file goes on: where the stream's last push left off
            det.c0 = xd[lane];
            det.dMean = xd[64];
            det.dMean2 = xd[65];
            det.threshold = xd[66];
            det.nseg = (int)reinterpret_cast<const long long *>(xd)[67];
        }
        prev = stream;
        double nxt = (rec.nvalid > 0 && lane < p.nc) ? p.ci[rec.rbase * p.nc + lane] : 0.0;
        for (int f = 0; f < rec.nvalid; f++) {
            const double cil = nxt;
            if (f + 1 < rec.nvalid && lane < p.nc) nxt = p.ci[(rec.rbase + f + 1) * p.nc + lane];
            const int v = cepdet_frame(det, cil, lane, p.nc, p.ninit, p.pcoef, p.qcoef);
            if (lane == 0) p.vbits[rec.rbase + f] = (unsigned char)v;
        }
        const int next_stream = tile >= 0 ? p.tile_stream[tile] : -1;
        if (next_stream != stream) {  // behind the stream's last tile of this chain
            xd[lane] = det.c0;
            if (lane == 0) {  // the wave-uniform part of the record: one lane, ordinary stores
                xd[64] = det.dMean;
                xd[65] = det.dMean2;
                xd[66] = det.threshold;
                reinterpret_cast<long long *>(xd)[67] = (long long)det.nseg;
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
