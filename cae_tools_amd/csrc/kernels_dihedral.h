// kernels_dihedral.h - the eight symmetries of the square applied to packed rows (include/cae_hip.h, cae_dihedral_rows;
// DESIGN.md section 9, "Dihedral augmentation").
//
// k_dihedral_rows: dst[i] = g(code[i]) applied to src[row[i]], every channel, as 32-bit words: no arithmetic touches a value.
// A code is three bits - 4: transpose, 2: reverse the rows, 1: reverse the columns - applied in that order, so the word
// of destination pixel (y, x) is the source's at (a, b) without bit 2 and at (b, a) with it, a = bit 1 ? h - 1 - y : y and
// b = bit 0 ? w - 1 - x : x.  A row index outside 0 .. n_src - 1 or a code outside 0 .. group - 1 is never turned into an
// address: the destination row gets quiet NaNs (k_normalise_pack_gather's rule).
//
// Work item: one DH_TILE x DH_TILE tile of one channel of one destination row; a workgroup of DH_WAVES waves takes items
// blockIdx.x, blockIdx.x + gridDim.x, ...  Row, code and tile are the same for the whole workgroup, so every branch on
// them is scalar.  Wave v owns the tile's lines v, v + DH_WAVES, ..., lane l the l-th word of a line.
//   codes 0-3: a line of dst is a line of src, forward or lane-reversed: the load walks the line downwards where bit 0 is
//              set, the store always upwards; both touch the same 256 bytes.  No LDS.
//   codes 4-7: (square planes) the tile is read along the source's lines into LDS, line j of the LDS tile holding what
//              becomes COLUMN j of the destination tile, and written along the destination's lines from the LDS tile's
//              columns.  The LDS tile is [64][65] words: the pad of one word puts the 32 lanes of a column read
//              (ds_read_b32 is served in halves of 32 lanes over 32 banks) on 32 different banks, where a pitch of 64 would
//              put them on one.
// No atomics, no scratch.
#pragma once

namespace cae {

constexpr int DH_TILE = 64;             // words a side: one line of a tile per wave instruction
constexpr int DH_WAVES = 4;             // waves per 256-thread workgroup

struct DhArgs {
    const unsigned* src;
    unsigned* dst;
    const int* row;                     // NULL: row i
    const int* code;
    long long n_src, items;
    long long tiles_x, tiles_plane;     // tiles across a plane, tiles of a plane
    int c, h, w, group;
};

template <int WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_dihedral_rows(const DhArgs s) {
    __shared__ unsigned tile[DH_TILE][DH_TILE + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long plane = (long long)s.h * s.w;
    for (long long item = blockIdx.x; item < s.items; item += gridDim.x) {
        const long long img = item / s.tiles_plane, t = item - img * s.tiles_plane;
        const long long d = img / s.c, ch = img - d * s.c;
        const long long ty = t / s.tiles_x, tx = t - ty * s.tiles_x;
        const long long y0 = ty * DH_TILE, x0 = tx * DH_TILE;
        const int rows = s.h - y0 < DH_TILE ? (int)(s.h - y0) : DH_TILE;
        const int cols = s.w - x0 < DH_TILE ? (int)(s.w - x0) : DH_TILE;
        const long long sr = s.row ? (long long)s.row[d] : d;
        const int g = s.code[d];
        unsigned* out = s.dst + (d * s.c + ch) * plane;
        if (sr < 0 || sr >= s.n_src || g < 0 || g >= s.group) {
            for (int j = wave; j < rows; j += WAVES)
                if (lane < cols) out[(y0 + j) * s.w + x0 + lane] = 0x7fc00000u;
            continue;
        }
        const unsigned* in = s.src + (sr * s.c + ch) * plane;
        if (!(g & 4)) {
            const long long x = x0 + lane, b = (g & 1) ? s.w - 1 - x : x;
#pragma unroll 4
            for (int j = wave; j < rows; j += WAVES) {
                const long long y = y0 + j, a = (g & 2) ? s.h - 1 - y : y;
                if (lane < cols) out[y * s.w + x] = in[a * s.w + b];
            }
        } else {        // h == w: the source's line b(x) holds, at a(y), the word of destination pixel (y, x)
            const long long y = y0 + lane, a = (g & 2) ? s.h - 1 - y : y;
#pragma unroll 4
            for (int j = wave; j < cols; j += WAVES) {
                const long long x = x0 + j, b = (g & 1) ? s.w - 1 - x : x;
                if (lane < rows) tile[j][lane] = in[b * s.w + a];
            }
            __syncthreads();
#pragma unroll 4
            for (int j = wave; j < rows; j += WAVES)
                if (lane < cols) out[(y0 + j) * s.w + x0 + lane] = tile[lane][j];
            __syncthreads();        // the next item's loads overwrite the tile
        }
    }
}

}  // namespace cae
