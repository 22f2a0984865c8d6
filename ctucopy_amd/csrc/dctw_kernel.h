// Wide DCT-II tail: 25 to 64 values per frame (hi-res MFCC), behind a band-valued front end.
// Included by engine.hip (one translation unit: the kernels and their host launchers share types).
#pragma once

namespace {

// dctcFEA (src/fea/fea_impl.cc:104-131) for more coefficients than phase 2 of the front ends accumulates (MAXC): the front end leaves
// the frame's band logarithms in the plan's scratch (logmel [total_frames][B], as for TRAP-DCT) and this kernel contracts them with the
// DCT table: rows[t][m] = sum_b A[m][b] * logmel[t][b].  A is the table of design.cc (norm and lifter folded in in double, rounded to
// float once) with its rows in the writer's order (c1..cN, then c0 with -fea_c0; row N2 of VERDICT.md), so a row block of the
// accumulator is a run of consecutive row columns.  The energy column (-fea_E), where there is one, follows the coefficients at column
// nout: the front end has written it and this kernel leaves it alone.
//
// v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains): D[m][n] += sum_k A[m][k] B[k][n] with m = coefficient, n = frame, k = band.
//   A operand: lane l holds A[m = l & 15][k = l >> 4]; the host lays the table out per (chunk, row block, k-step, lane): one coalesced
//              load per step, kept in registers while the workgroup walks its tiles (one chunk: banks of up to DCTW_KC bands)
//   B operand: lane l holds B[k = l >> 4][n = l & 15] = band 4 s + k of frame n, read from the LDS tile; row stride DCTW_LD = 68 floats
//              puts the 64 lanes of a step on 64 different banks (4 n + k + 4 s mod 64)
//   C/D:       lane l holds coefficients 4 (l >> 4) .. + 3 of frame l & 15
// A coefficient is one chain over the bands in ascending order, whatever the frame's place in its tile or the tile's in the batch.
//
// A workgroup of four waves takes tiles of DCTW_TILE = 64 consecutive rows of the flat row space (wave w: rows 16 w .. 16 w + 15).  The
// contraction is per row, so a tile may span utterances and needs no tile record; the last tile is partial.  The 64 x B block of logmel a
// tile reads and the 64 x nout block of the rows it writes are each one contiguous run in HBM (rows: but for the energy column).
// Results go through the LDS tile so that a wave stores whole rows, one row per store instruction.
constexpr int DCTW_TILE = 64, DCTW_LD = 68;  // (DCTW_KC, DCTW_MAX: layout_constants.h)

struct DctwParams {
    const float *logmel;   // [total_frames][B]
    float *rows;           // [total_frames][D]
    const float *atab;     // A operands [chunks][NRB][DCTW_KC / 4][64]: zero for bands >= B and rows >= nout
    int64_t total_frames;
    int B, D, nout, chunks, n_tiles;
};

template <int NRB>  // row blocks of 16 coefficients: nout <= 16 NRB
__global__ __launch_bounds__(256) void dct_wide_kernel(const DctwParams p) {
    __shared__ __attribute__((aligned(16))) float tile[DCTW_TILE * DCTW_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, kq = lane >> 4;
    constexpr int KS = DCTW_KC / 4;
    float a[NRB][KS];
    auto load_a = [&](int c) {
#pragma unroll
        for (int rb = 0; rb < NRB; rb++)
#pragma unroll
            for (int s = 0; s < KS; s++) a[rb][s] = p.atab[((size_t)(c * NRB + rb) * KS + s) * 64 + lane];
    };
    if (p.chunks == 1) load_a(0);
    for (int t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
        const int64_t r0 = (int64_t)t * DCTW_TILE;
        const int nvalid = (int)min((int64_t)DCTW_TILE, p.total_frames - r0);
        f32x4 acc[NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; rb++) acc[rb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < p.chunks; c++) {
            if (p.chunks > 1) load_a(c);
            __syncthreads();  // the tile's previous readers (the last chunk's steps, the last tile's stores) are done
            for (int i = tid; i < DCTW_TILE * DCTW_KC; i += 256) {
                const int r = i / DCTW_KC, j = i % DCTW_KC, b = c * DCTW_KC + j;
                tile[r * DCTW_LD + j] = (r < nvalid && b < p.B) ? p.logmel[(r0 + r) * p.B + b] : 0.f;
            }
            __syncthreads();
            const float *x = tile + (wave * 16 + n) * DCTW_LD + kq;
#pragma unroll
            for (int s = 0; s < KS; s++) {
                const float bv = x[4 * s];
#pragma unroll
                for (int rb = 0; rb < NRB; rb++) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][s], bv, acc[rb], 0, 0, 0);
            }
        }
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < NRB; rb++) *reinterpret_cast<f32x4 *>(tile + (wave * 16 + n) * DCTW_LD + rb * 16 + kq * 4) = acc[rb];
        __syncthreads();
        for (int r = wave; r < nvalid; r += 4)
            if (lane < p.nout) p.rows[(r0 + r) * p.D + lane] = tile[r * DCTW_LD + lane];
    }
}

}  // namespace
