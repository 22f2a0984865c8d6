// HTK feature input on the device (-format_in htk: htkIN::get_frame, src/io/in.cc:691-709, ahead of the delta chain / CMS / CMVN).
// Included by engine.hip.
#pragma once

namespace {

// The host freads every file's payload as it stands - 32-bit words in the file's byte order - into a packed arena: utterance i's
// rows start at word ctu_rows_arena_layout()[i] (a multiple of four words) and lie row after row, `width` words each.  This kernel is
// the rest of get_frame: SwapFloat on every word with -endian_in against the host's order (in.cc:696-698), then the value into the slot
// of the plan's row arena [total_frames][width] that the post kernels read it from.  That slot is the file's own column - the
// reference passes the vector on in file order and its writers copy it in order (src/io/out.cc:177-179) - except ahead of the
// stacking pass (-fea_trap), which takes vector entry i from column i - 1 and entry 0 from the last column (post_kernels.h):
// ROT stores file column c to column c - 1, column 0 to the last one.
//
// A tile is at most 64 rows of one utterance; 64 rows of any width are a multiple of 16 bytes, so a tile's source is 16-byte
// aligned wherever its utterance's is.  A wave takes tiles wave, wave + waves of the grid, ...: the grid is sized from the CU
// count alone.  Straight copy: 16 bytes per lane, stores aligned on the destination (row offsets are sums of frame counts, so at
// odd widths a tile's rows start at any 4-byte phase), contiguous over the wave.  No LDS; the next tile's record is fetched ahead
// of the copy.
// (ROWS_WG_PER_CU, layout_constants.h: workgroups of four waves per CU, 32 waves, each with a tile of 64 rows in flight)

struct __attribute__((aligned(4))) RowsWord4 {
    uint32_t x, y, z, w;
};
__device__ __forceinline__ uint32_t rows_word(uint32_t w, bool swap) { return swap ? __builtin_bswap32(w) : w; }

template <bool SWAP, bool ROT>
__global__ __launch_bounds__(256) void rows_ingest_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, const TileRec *__restrict__ tiles,
                                                          const int n_tiles, const int width) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * (blockDim.x >> 6);
    int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    TileRec r = load_rec(tiles, tile);
    while (true) {
        const int nxt = tile + nw;
        const bool more = nxt < n_tiles;
        TileRec rn = r;
        if (more) rn = load_rec(tiles, nxt);
        const uint32_t *src = in + r.sbase;
        uint32_t *dst = out + r.rbase * width;
        const int n = r.nvalid * width;
        if (ROT) {
            int row = 0, c = lane;  // (row, column) of word e, carried along instead of divided out
            for (int e = lane; e < n; e += 64, c += 64) {
                while (c >= width) { c -= width; row++; }
                dst[row * width + (c == 0 ? width - 1 : c - 1)] = rows_word(src[e], SWAP);
            }
        } else {
            // the words ahead of the destination's next 16-byte boundary one per lane, then 16 bytes per lane: aligned stores, loads at
            // whatever 4-byte phase the source is left with (one global_load_dwordx4 either way), the last one to three words one per lane
            const int head = min(n, (int)((4 - (((uintptr_t)dst >> 2) & 3)) & 3));
            if (lane < head) dst[lane] = rows_word(src[lane], SWAP);
            const RowsWord4 *s4 = reinterpret_cast<const RowsWord4 *>(src + head);
            uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
            const int n4 = (n - head) >> 2;
#pragma unroll 4
            for (int i = lane; i < n4; i += 64) {
                const RowsWord4 v = s4[i];
                d4[i] = make_uint4(rows_word(v.x, SWAP), rows_word(v.y, SWAP), rows_word(v.z, SWAP), rows_word(v.w, SWAP));
            }
            const int e = head + 4 * n4 + lane;
            if (e < n) dst[e] = rows_word(src[e], SWAP);
        }
        if (!more) break;
        tile = nxt;
        r = rn;
    }
}

}  // namespace
