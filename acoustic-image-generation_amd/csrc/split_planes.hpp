// The split-plane ("brick") activation layout, stated once: the chunk swizzle, the byte offset of an element inside a plane,
// the brick-order enumeration of a producer's work items, the plane size behind acimg_split_plane_bytes and the store of one
// item.  Written by the producers in batchnorm.hip, read by the trunk kernels (igemm_split3d_kernel.hpp and the headers built
// on it) and by gram.hip; the on-the-fly split kernels (igemm_split3_kernel.hpp) lay their LDS tiles out with the same swz().
// tests/split_format_ref.py restates this file in Python.
// Device / host-inline only (conv_host.hpp's rule for kernel headers): no kernel, no launch, no read of g_cfg, so any
// translation unit may include it.  The VALUE format of a plane - the SPLIT3_* scales, split4_scaled / unsplit4 - stays in
// common.hpp with the h16 vector types; this header is the LAYOUT.
#pragma once
#include "common.hpp"

namespace acimg {

// LDS chunk swizzle: a tile row is 64 bytes = four 16-byte chunks; logical chunk kc of row `row` is stored at
// chunk kc ^ swz(row).  ds_read_b128 is serviced in the hardware lane groups {0-3,12-15,20-27},
// {4-11,16-19,28-31}, ... (not in natural 16-lane groups): each group sees all 16 fragment rows once, rows
// 0-3/12-15 with one k-chunk g and rows 4-11 with g^1.  swz = (0,3,2,1)[(row>>2)&3] is the assignment that
// makes the 16 lanes of every such group hit 16 distinct 16-byte slots of the 256-byte bank window
// (the plain (row>>2)&3 pattern measured 35 % of LDS cycles as bank conflicts).
__device__ __forceinline__ int swz(int row) { return (0 - (row >> 2)) & 3; }

// ------------------------------------------------------------------------------------------
// producers of the split-fp16 activation format consumed by the trunk kernels (igemm_split3d_kernel.hpp, "bricks"): two
// fp16 planes, lo plane lo_off bytes after the hi plane, values carry the 2^-2 scale.  A plane of a [P pixels][C] tensor
// (C % 32 == 0) is ceil(P / 16) x C / 32 bricks of 1 KiB: brick (f >> 4, c >> 5) holds 16 rows (f & 15) of 64 bytes, the
// logical 16-byte chunk (c >> 3) & 3 of a row at physical chunk ((c >> 3) ^ swz(f)) & 3, swz(f) = -(f >> 2) & 3 - the LDS
// image of 16 tile rows, so the consumer's LDS-DMA request is one contiguous KiB.
// Work items (one float4 = 4 channels each) are enumerated in brick order: a wave covers 8 pixels x 32 channels, i.e. it
// reads eight whole 128-byte lines of the fp32 source and writes 512 contiguous bytes (four whole lines) of each plane.
// ------------------------------------------------------------------------------------------
// byte offset of logical chunk kc of pixel f's row in channel chunk 0; c32 = C * 32 = bytes of one pixel block (the
// consumers step through the channel chunks themselves)
__device__ __forceinline__ unsigned brick_a_off(unsigned f, unsigned c32, unsigned kc) {
    return (f >> 4) * c32 + ((f & 15u) << 6) + (((kc ^ (unsigned)swz((int)f)) & 3u) << 4);
}
// byte offset of channels c .. c+3 of pixel f (the producers; CQ = C / 32): brick_a_off(f, CQ * 1024, c >> 3) +
// (c >> 5) * 1024 + (c & 4) * 2, written out (the nested form changes the producers' instruction text)
__device__ __forceinline__ unsigned plane_off(unsigned f, unsigned c, unsigned CQ) {      // c % 4 == 0
    return ((f >> 4) * CQ + (c >> 5)) * 1024u + ((f & 15u) << 6) + ((((c >> 3) ^ (unsigned)swz((int)f)) & 3u) << 4) + ((c & 4u) << 1);
}
struct BrickItem {
    unsigned pix, c, off;      // pixel, first of its 4 channels, byte offset inside a plane
};
__device__ __forceinline__ BrickItem brick_item(unsigned u, unsigned CQ, bool pow2, int sh) {
    const unsigned l = u & 63u, hb = u >> 6;
    const unsigned ph = pow2 ? hb >> sh : hb / CQ;
    const unsigned cq = hb - ph * CQ;
    BrickItem it;
    it.pix = ph * 8u + (l >> 3);
    it.c = cq * 32u + (l & 7u) * 4u;
    it.off = plane_off(it.pix, it.c, CQ);
    return it;
}

// the tail of every producer: 4 channels, scaled by 2^-2 and split, to byte offset `off` of the hi and of the lo plane
__device__ __forceinline__ void store_split4(const float4 v, char* out, long lo_off, unsigned off) {
    uint2 hi, lo;
    split4_scaled(scale4(v, SPLIT3_ASCALE), hi, lo);
    *reinterpret_cast<uint2*>(out + off) = hi;
    *reinterpret_cast<uint2*>(out + lo_off + off) = lo;
}

// bytes of one plane of a [rows][C] tensor: whole 16-row bricks of fp16 (acimg_split_plane_bytes)
static inline size_t split_plane_bytes(long rows, int C) { return (size_t)((rows + 15) / 16) * 16 * (size_t)C * 2; }

// items of a [rows][C] tensor in brick order (8 pixels x 32 channels per wave), or 0 if it cannot be one
static inline unsigned split_items(long rows, int C) {
    if (rows <= 0 || C <= 0 || (C & 31)) return 0;
    const long items = (rows + 7) / 8 * 8 * (C / 4);
    return items < (1L << 30) ? (unsigned)items : 0u;
}

}  // namespace acimg
