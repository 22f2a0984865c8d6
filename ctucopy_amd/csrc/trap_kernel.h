// TRAP-DCT on the matrix cores.
// Included by engine.hip (one translation unit: the kernels and their host launchers share types).
#pragma once

namespace {

// TRAP-DCT (src/fea/fea_trap.cc:53-127): out[t][b*ndct+k] = sum_j G[k][j] * logmel[clamp(t-half+j)][b]
// with mean removal, Hamming and REDFT10 folded into G on the host.  Unlike the banded filter bank this IS a dense
// contraction (ndct x traplen per band and frame), so it runs on the matrix cores: v_mfma_f32_16x16x4_f32 (exact
// fp32 FMA chain), D[k][t] += G[k][4s..4s+3] * X[4s..4s+3][t] with the Toeplitz operand X[j][t] = x[t+j-half][b]
// read straight from an LDS tile of log-mel frames.  Rows of G sum to zero, so each column is offset by its centre
// value first (keeps the fp32 accumulation small).
// One workgroup = 64 output frames of one utterance (4 waves x 16 frames), all bands.

// Non-finite log-mel values (an all-zero frame is the logarithm of an empty band, -inf).  Both kernels pad the context with taps of
// weight zero that fetch real neighbouring frames (to a multiple of four taps and to NSM tap groups here, to K = 128 taps in the 16-bit
// kernel), and 0 x -inf = NaN would reach rows whose own traplen frames are finite; the 16-bit split holds no such value either (the low
// term of -inf is -inf - -inf = NaN).  So such a value enters the tile as 0 and sets its frame's bit in a per-band mask in LDS (TM_BADW /
// TB_BADW words a band over the tile's frames); a row whose own context - tile frames f0 .. f0 + traplen - 1 of the band - holds a marked
// frame is written as NaN, which is what the reference's mean removal over the context makes of it (fea_trap.cc), and every other row is
// the contraction of finite values.  A tile without such a value (speech: "never digitally silent") pays the test per element while
// loading and one uniform branch behind the last row store; the MFMA loops and the stores are as they were.
constexpr unsigned TRAP_NAN = 0xffc00000u;  // what -inf - -inf gives, here as in the reference's mean removal: the rows of a silent context stay what they were
// (TM_BADW, TB_BADW and the tiles' sizes: layout_constants.h, where trap_path states the launch)
__device__ __forceinline__ bool f32_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool trap_context_marked(const unsigned *m, int f0, int n) {
    bool bad = false;
    for (int w = f0 >> 5; w <= (f0 + n - 1) >> 5; w++) {
        const int lo = max(f0 - 32 * w, 0), hi = min(f0 + n - 32 * w, 32);  // bits lo .. hi - 1 of word w
        const unsigned bits = (hi - lo == 32 ? ~0u : ((1u << (hi - lo)) - 1u)) << lo;
        bad |= (m[w] & bits) != 0;
    }
    return bad;
}

// Long contexts (more than TRAP_COMP_STEPS = 26 tap groups, traplen 105 .. 255): one fp32 accumulator chain over the whole context does
// not hold the engine's parity bound - at 255 taps the partial sums reach the hundreds for results below one, and on speech the rows
// were 1.9e-4 of max(|oracle|, 1) from the oracle (bound 1e-4) where the same log-mel rows contracted in float64 are 4.6e-5 from it.
// So there the taps still ascend from a zero accumulator over the same centred operand, but the accumulator is closed every
// TRAP_COMP_RUN = 2 tap groups (8 taps) and behind the last group: it joins a sum kept as two floats by an error-free addition
// (two-sum: s = hi + a, the rounding error of that addition collected in lo) and starts over from zero; the row is hi + lo.
// trapdct_mfma_kernel<NRB, 64> and stream_trap_kernel<NRB, true> (stream_trap_kernels.h) both sum this way, through these two
// functions alone, so their rows are the same bit for bit when the log-mel rows are.  12 VALU operations per accumulator register and run.
// Why runs of 2: measured on an MI355X against the float64 contraction of the device's own log-mel rows (tests/test_trapdct_shapes.py),
// runs of 4 / 2 / 1 leave 3.5 - 5.8e-5 / 1.9 - 3.7e-5 / 1.4 - 2.3e-5 at 105 .. 255 taps, and that float64 contraction is itself 7e-5 (23
// bands) to 1.0e-4 (51 bands) from the oracle at 201 .. 255 taps (bound 1e-4): with runs of 4 the 51-band rows came out at 1.11e-4.
// gfx950, hipcc -O3: trapdct_mfma_kernel<1, 64> 194 VGPRs + 4 AGPRs, <2, 64> 247 + 8, two waves per SIMD, no scratch.
__device__ __forceinline__ bool trap_comp_closes(int s_, int nsteps) { return (s_ & (TRAP_COMP_RUN - 1)) == TRAP_COMP_RUN - 1 || s_ + 1 == nsteps; }
__device__ __forceinline__ void trap_comp_close(f32x4 &acc, f32x4 &sum_hi, f32x4 &sum_lo) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float h = sum_hi[r], v = acc[r];
        const float t = h + v, vv = t - h;
        sum_lo[r] += (h - (t - vv)) + (v - vv);
        sum_hi[r] = t;
        acc[r] = 0.f;
    }
}
__device__ __forceinline__ f32x4 trap_comp_row(const f32x4 &sum_hi, const f32x4 &sum_lo) { return sum_hi + sum_lo; }

template <int NRB, int NSM>  // row blocks of 16 DCT coefficients (ndct <= 16*NRB); NSM >= ceil(traplen/4) tap groups; NSM > 32: summed in compensated runs
__global__ __launch_bounds__(256) void trapdct_mfma_kernel(const float *__restrict__ logmel, float *__restrict__ rows,
                                                           const float *__restrict__ G, const int4 *__restrict__ utt_info,
                                                           const int *__restrict__ chunk_tab, int B, int traplen, int ndct, int D) {
    extern __shared__ float tile[];  // [64 + 4*nsteps][Bs], then bad[B][TM_BADW] + 1
    const int u = chunk_tab[blockIdx.x * 2], tc = chunk_tab[blockIdx.x * 2 + 1];
    const int4 ui = utt_info[u];
    const int64_t r0 = ((int64_t)ui.y << 32) | (uint32_t)ui.x;
    const int T = ui.z;
    const int half = (traplen - 1) / 2, nsteps = (traplen + 3) / 4;
    const int Bs = B | 1, nfr = 64 + 4 * (NSM <= 32 ? NSM : nsteps);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned *bad = reinterpret_cast<unsigned *>(tile + nfr * Bs);  // [B][TM_BADW], then the tile's flag
    for (int e = tid; e <= B * TM_BADW; e += 256) bad[e] = 0u;
    __syncthreads();
    // log-mel tile with the first / last frame replicated beyond the utterance (src/fea/fea_trap.cc:64-70,111-127)
    for (int e = tid; e < nfr * B; e += 256) {
        const int f = e / B, b = e - f * B;
        int t = tc - half + f;
        t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
        float v = logmel[(r0 + t) * B + b];
        if (f32_nonfinite(v)) {
            atomicOr(&bad[b * TM_BADW + (f >> 5)], 1u << (f & 31));
            bad[B * TM_BADW] = 1u;
            v = 0.f;
        }
        tile[f * Bs + b] = v;
    }
    // this lane's slice of G: A[i = lane&15][k = lane>>4] of every 16x4 block
    const int ai = lane & 15, ak = lane >> 4;
    float areg[NRB][NSM];
#pragma unroll
    for (int rb = 0; rb < NRB; rb++)
#pragma unroll
        for (int s_ = 0; s_ < NSM; s_++) {
            const int k = rb * 16 + ai, j = 4 * s_ + ak;
            areg[rb][s_] = (s_ < nsteps && k < ndct && j < traplen) ? G[k * traplen + j] : 0.f;
        }
    __syncthreads();
    const int tl = wave * 16 + (lane & 15);  // local output frame of this lane's column
    const int t_out = tc + tl;
    for (int b = 0; b < B; b++) {
        const float xc = tile[(tl + half) * Bs + b];
        f32x4 acc[NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; rb++) acc[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (NSM <= 32) {
#pragma unroll
            for (int s_ = 0; s_ < NSM; s_++) {  // exact instantiations run unguarded (A is zero beyond traplen)
                const float bv = tile[(tl + 4 * s_ + ak) * Bs + b] - xc;
#pragma unroll
                for (int rb = 0; rb < NRB; rb++) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rb][s_], bv, acc[rb], 0, 0, 0);
            }
        } else {
            // long contexts: the tap groups that exist (a uniform guard), closed in compensated runs (trap_comp_close above)
            f32x4 sum_hi[NRB], sum_lo[NRB];
#pragma unroll
            for (int rb = 0; rb < NRB; rb++) sum_hi[rb] = sum_lo[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s_ = 0; s_ < NSM; s_++) {
                if (s_ < nsteps) {
                    const float bv = tile[(tl + 4 * s_ + ak) * Bs + b] - xc;
#pragma unroll
                    for (int rb = 0; rb < NRB; rb++) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[rb][s_], bv, acc[rb], 0, 0, 0);
                    if (trap_comp_closes(s_, nsteps)) {
#pragma unroll
                        for (int rb = 0; rb < NRB; rb++) trap_comp_close(acc[rb], sum_hi[rb], sum_lo[rb]);
                    }
                }
            }
#pragma unroll
            for (int rb = 0; rb < NRB; rb++) acc[rb] = trap_comp_row(sum_hi[rb], sum_lo[rb]);
        }
        if (t_out < T && ndct == 16 && NRB == 1 && (D & 3) == 0) {
            // C/D layout: this lane holds coefficients 4*(lane>>4)..+3 of frame column lane&15: one 16-byte store
            *reinterpret_cast<f32x4 *>(rows + (r0 + t_out) * D + b * 16 + ak * 4) = acc[0];
        } else if (t_out < T) {
            float *o = rows + (r0 + t_out) * D + b * ndct;
#pragma unroll
            for (int rb = 0; rb < NRB; rb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int k = rb * 16 + ak * 4 + r;  // C/D layout: row = (lane>>4)*4 + reg, col = lane&15
                    if (k < ndct) o[k] = acc[rb][r];
                }
        }
    }
    // A tile with marked frames (uniform over the workgroup): the lanes write NaN over what they stored above wherever the row's own
    // context - tile frames tl .. tl + traplen - 1 of the band - holds one.  Behind the loop, so that the loop is as it was.
    if (bad[B * TM_BADW] != 0u && t_out < T) {
        const float nan = __uint_as_float(TRAP_NAN);
        for (int b = 0; b < B; b++)
            if (trap_context_marked(bad + b * TM_BADW, tl, traplen)) {
                float *o = rows + (r0 + t_out) * D + b * ndct;
                for (int rb = 0; rb < NRB; rb++)
                    for (int r = 0; r < 4; r++) {
                        const int k = rb * 16 + ak * 4 + r;
                        if (k < ndct) o[k] = nan;
                    }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same contraction on the 16-bit matrix pipe with fp32 accuracy.  Every operand is split into 16-bit terms and the
// significant cross products accumulate in fp32: two fp16 terms (x = h + l to 2^-22), hh, hl, lh - 3 MFMAs per 32 taps (ll, 2^-22, dropped).
// v_mfma_f32_16x16x32_f16 does 8x the multiply-adds of the fp32 form per cycle.  The kernel is bound by that pipe
// at the clock the chip holds under it (neither the barrier, nor occupancy, nor the stores, nor the dependency chain of
// the accumulator moved its time), so the fp16 split - half the MFMAs of three bf16 terms and six products - is the one that runs; the log-mel values are
// centred per band (|x| of a few units) and G is at most 1, far inside fp16's range, and an element's absolute error is
// max(2^-22 |x|, 3e-8) (fp16 subnormal spacing).
// The Toeplitz operand X[j][t] = x[t + j - half] wants 8 consecutive taps per lane (16-byte LDS reads), i.e. a start that
// is a multiple of 8 for every column: the 16 columns of an MFMA are therefore output frames 8 apart (t = tc + 8 n + c),
// and each of the 8 phases c has its own copy of G shifted by c taps (host table, zero-padded to K = 128):
//     D[k][n] = sum_j' Gc[k][j'] X[8 n + j'],   X[tau] = x(tc - OFF + tau) - x0(band),   j' = j + c + OFF - half
// (rows of G sum to zero, so the per-band constant x0 - the tile's centre value - drops out and keeps the split small).
// One workgroup (8 waves, at most 128 VGPRs: two workgroups = four waves per SIMD on a CU) = 128 output frames x all
// bands; wave w takes bands w, w+8, ...; A fragments of a phase (4 k-steps x NT terms) live in registers meanwhile.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// (TB_TT, the tile row in frames: layout_constants.h)

// Workgroup barrier for LDS hand-overs only: __syncthreads() also drains the vector-memory counter, which would put the
// latency of a phase's row stores in front of the next phase.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ unsigned f16_bits(_Float16 h) { return (unsigned)__builtin_bit_cast(unsigned short, h); }

// the two fp16 terms of a value, most significant first
__device__ __forceinline__ void split16(float v, unsigned (&t)[2]) {
    const _Float16 h = (_Float16)v;  // v_cvt_f16_f32, round to nearest even
    const _Float16 l = (_Float16)(v - (float)h);
    t[0] = f16_bits(h);
    t[1] = f16_bits(l);
}

#ifndef TB_WGS
#define TB_WGS 2
#endif
__global__ __launch_bounds__(512, TB_WGS) void trapdct_split16_kernel(const float *__restrict__ logmel, float *__restrict__ rows,
                                                                const uint4 *__restrict__ Gtab, const int4 *__restrict__ utt_info,
                                                                const int *__restrict__ chunk_tab, int n_chunks, int B, int traplen, int ndct, int D) {
    constexpr int NT = 2;                 // terms per operand
    constexpr int NA = 4 * NT * 64;       // uint4 fragments of a phase
    extern __shared__ __align__(16) unsigned short xt[];  // [NT][B][TB_TT] terms, then x0[B] floats, then the fragment buffers, then bad[B][TB_BADW] + 1
    if ((int)blockIdx.x >= n_chunks) return;
    const int u = chunk_tab[blockIdx.x * 2], tc = chunk_tab[blockIdx.x * 2 + 1];  // chunks of 128 frames
    const int4 ui = utt_info[u];
    const int64_t r0 = ((int64_t)ui.y << 32) | (uint32_t)ui.x;
    const int T = ui.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *x0 = reinterpret_cast<float *>(xt + NT * B * TB_TT);
    unsigned *bad = reinterpret_cast<unsigned *>(reinterpret_cast<uint4 *>(x0 + ((B + 3) & ~3)) + 2 * NA);  // [B][TB_BADW], then the tile's flag
    if (tid < B) {
        int t = tc + 64;
        t = t > T - 1 ? T - 1 : t;
        const float v = logmel[(r0 + t) * B + tid];
        x0[tid] = f32_nonfinite(v) ? 0.f : v;  // (any constant serves: rows of G sum to zero)
    }
    if (tid <= B * TB_BADW) bad[tid] = 0u;  // B <= 24: 193 words at the most
    __syncthreads();
    // log-mel tile with the first / last frame replicated beyond the utterance (src/fea/fea_trap.cc:64-70,111-127)
    unsigned *xt32 = reinterpret_cast<unsigned *>(xt);
    {
        // two frames per lane and step (one dword store per term); every load of the tile is issued before the first use
        constexpr int NF = 6;  // ceil(128 * 24 / 512): B <= 24 on this path
        float v0[NF], v1[NF];
#pragma unroll
        for (int it = 0; it < NF; it++) {
            const int e = min(tid + 512 * it, 128 * B - 1);  // unconditional loads (a branch per step would serialise them)
            const int pr = e / B, b = e - pr * B;
            int t0_ = tc - TB_OFF + 2 * pr, t1_ = t0_ + 1;
            t0_ = t0_ < 0 ? 0 : (t0_ > T - 1 ? T - 1 : t0_);
            t1_ = t1_ < 0 ? 0 : (t1_ > T - 1 ? T - 1 : t1_);
            v0[it] = logmel[(r0 + t0_) * B + b];
            v1[it] = logmel[(r0 + t1_) * B + b];
        }
#pragma unroll
        for (int it = 0; it < NF; it++) {
            const int e = tid + 512 * it;
            if (e < 128 * B) {
                const int pr = e / B, b = e - pr * B;
                unsigned ta[NT], tb[NT];
                float d0 = v0[it] - x0[b], d1 = v1[it] - x0[b];
                if (f32_nonfinite(d0) || f32_nonfinite(d1)) {  // tile frames 2 pr and 2 pr + 1 share a word of the mask
                    atomicOr(&bad[b * TB_BADW + (pr >> 4)], (f32_nonfinite(d0) ? 1u : 0u) << (2 * pr & 31) | (f32_nonfinite(d1) ? 2u : 0u) << (2 * pr & 31));
                    bad[B * TB_BADW] = 1u;
                    d0 = f32_nonfinite(d0) ? 0.f : d0;
                    d1 = f32_nonfinite(d1) ? 0.f : d1;
                }
                split16(d0, ta);
                split16(d1, tb);
#pragma unroll
                for (int sp = 0; sp < NT; sp++) xt32[((sp * B + b) * TB_TT >> 1) + pr] = ta[sp] | (tb[sp] << 16);
            }
        }
    }
    __syncthreads();
    const int n = lane & 15, q = lane >> 4;
    // A fragments of a phase: 4 x NT x 64 lanes x 16 bytes, fetched once per workgroup into LDS one phase ahead (every wave
    // needs all of them).  One LDS-only barrier per phase: nothing in the loop waits for the rows' stores.
    uint4 *abuf = reinterpret_cast<uint4 *>(x0 + ((B + 3) & ~3));  // [2][NA]
    abuf[tid] = Gtab[tid];
    if (tid + 512 < NA) abuf[tid + 512] = Gtab[tid + 512];
    for (int c = 0; c < 8; c++) {
        lds_barrier();  // phase c's fragments are in abuf[c & 1]; every wave is done with the other half
        // next phase's fragments: named registers, fetched unconditionally (the last phase re-reads its own; lanes beyond the
        // table's end re-read an earlier entry): an array defined under a condition went to scratch
        const uint4 *gn = Gtab + (c + 1 < 8 ? c + 1 : c) * NA;
        const uint4 pre0 = gn[tid], pre1 = gn[(tid + 512 < NA) ? tid + 512 : tid];
        uint4 a[4][NT];
        const uint4 *ab = abuf + (c & 1) * NA;
#pragma unroll
        for (int s_ = 0; s_ < 4; s_++)
#pragma unroll
            for (int sp = 0; sp < NT; sp++) a[s_][sp] = ab[(s_ * NT + sp) * 64 + lane];
        const int t_out = tc + 8 * n + c;
        // a band of the wave: 4 x NT tile fragments from LDS, 12 MFMAs, one row store; four waves per
        // SIMD cover each other's LDS round trips
        for (int b = wave; b < B; b += 8) {
            uint4 X[4][NT];
#pragma unroll
            for (int s_ = 0; s_ < 4; s_++) {
                const int tau = 8 * n + 32 * s_ + 8 * q;
#pragma unroll
                for (int sp = 0; sp < NT; sp++) X[s_][sp] = *reinterpret_cast<const uint4 *>(xt + (sp * B + b) * TB_TT + tau);
            }
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s_ = 0; s_ < 4; s_++) {
                // smallest terms first
#define MF(A_, X_) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, A_), __builtin_bit_cast(f16x8, X_), acc, 0, 0, 0)
                MF(a[s_][1], X[s_][0]);
                MF(a[s_][0], X[s_][1]);
                MF(a[s_][0], X[s_][0]);
#undef MF
            }
            if (t_out < T) {
                if (ndct == 16 && (D & 3) == 0) {
                    // C/D layout: this lane holds coefficients 4*(lane>>4)..+3 of frame column lane&15: one 16-byte store
                    *reinterpret_cast<f32x4 *>(rows + (r0 + t_out) * D + b * 16 + q * 4) = acc;
                } else {
                    float *o = rows + (r0 + t_out) * D + b * ndct;
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (q * 4 + r < ndct) o[q * 4 + r] = acc[r];
                }
            }
        }
        uint4 *an = abuf + ((c + 1) & 1) * NA;
        an[tid] = pre0;
        if (tid + 512 < NA) an[tid + 512] = pre1;
    }
    // A tile with marked frames (uniform over the workgroup): the lanes write NaN over what they stored above wherever the row's own
    // context - tile frames 8 n + c + TB_OFF - half .. + traplen - 1 of the band - holds one.  Behind the phases, so that they are as they were.
    if (bad[B * TB_BADW] != 0u) {
        const float nan = __uint_as_float(TRAP_NAN);
        const int half = (traplen - 1) / 2;
        for (int c = 0; c < 8; c++) {
            const int t_out = tc + 8 * n + c;
            if (t_out >= T) continue;
            for (int b = wave; b < B; b += 8)
                if (trap_context_marked(bad + b * TB_BADW, 8 * n + c + TB_OFF - half, traplen)) {
                    float *o = rows + (r0 + t_out) * D + b * ndct;
                    for (int r = 0; r < 4; r++)
                        if (q * 4 + r < ndct) o[q * 4 + r] = nan;
                }
        }
    }
}

}  // namespace
