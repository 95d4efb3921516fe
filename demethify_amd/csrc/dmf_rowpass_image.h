// The byte images X8 / D8 of a problem's methylated read counts and counts, as the deferred-C row pass holds them in LDS
// (dmf_kernels_rowpass2.hip: the x ring's slot, the byte count tile) -- one index map for the kernel, the builder
// (dmf_tables.hip) and the host test.
//
// One image is the 16 rows x 64 samples of one 16-row block and one 64-sample column group as 1024 bytes = 256 dwords of
// four consecutive samples.  The 16 rows stand in the order (row & 3, row >> 2), and row r's 16 dwords are rotated by
// 4 (r & 3).  Then
//   - the rows R, R + 4, R + 8, R + 12 that one phase-C read touches (lane = (row, dword m16)) are 64 consecutive dwords,
//   - the 16 rows x 4 dwords of one phase-A strip read (lane = (row m16, dword 4 t + q)) fall into 64 different banks,
//   - the 16 samples 16 q .. 16 q + 15 of row m16 that a lane of the integer product reads are ONE aligned 16-byte piece, and
//     the 16 lanes a 16-byte LDS read serves together touch 16 different pieces modulo 256 bytes,
//   - lane L's 16-byte piece of the image, bytes 16 L .. 16 L + 15, is samples 16 c .. 16 c + 15 of row r with
//     r = 4 ((L >> 2) & 3) + (L >> 4), c = ((L & 3) - (r & 3)) & 3: what the builder gathers per lane.
// In memory the images of a block's SD / 64 column groups are consecutive and the blocks follow in row order: the arrays
// are [N16 / 16][SD / 64][1024] bytes, zero where D16 is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMF_IMAGE_FN __host__ __device__ constexpr
#else
#define DMF_IMAGE_FN constexpr
#endif

namespace dmf {

constexpr int kRowpassImageBytes = 16 * 64;

// dword index within an image of dword `dword` (samples 4 dword .. 4 dword + 3) of row `row`
DMF_IMAGE_FN int rowpass_image_dword(int row, int dword) {
    return (4 * (row & 3) + (row >> 2)) * 16 + ((dword + 4 * (row & 3)) & 15);
}
// byte offset within an image of (row, sample): the samples of a dword in little-endian order
DMF_IMAGE_FN int rowpass_image_byte(int row, int sample) { return 4 * rowpass_image_dword(row, sample >> 2) + (sample & 3); }
// the inverse for a 16-byte piece: the row of piece `piece`, and which of the row's four 16-sample pieces it is
DMF_IMAGE_FN int rowpass_image_piece_row(int piece) { return 4 * ((piece >> 2) & 3) + (piece >> 4); }
DMF_IMAGE_FN int rowpass_image_piece_col(int piece) { return ((piece & 3) - ((piece >> 4) & 3)) & 3; }

}  // namespace dmf
